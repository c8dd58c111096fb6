"""The prior family library on the device over a grid of shapes and from tail to tail, against mpmath
(tests/golden/g21_prior_family_terms.npz; tests/extfamilies.py has the grid, the reference and the tolerance), one term at
a time through tda_engine_evaluate; and chains over the shapes at which the density diverges at an edge of the support,
against the oracle with scipy's own logpdf as the prior."""
import math

import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extfamilies as xf
from . import extprior as xp
from .extengine import PRIOR_SOURCE, assert_rate, compare, run_forward
from .extmodel import np_forward, source
from .extprior import SIGMA2, family_source, level_of, make_engine, oracle_proposals_outside

pytestmark = pytest.mark.gpu


# ---- (a) every term of the grid, one at a time ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["all_128_rows", "one_row_per_shape"])
def test_terms_against_mpmath(golden, layout):
    """Point 0 has every parameter at its rest point (the component's median); point n is point 0 with exactly one parameter
    moved to one probe.  got[n] - got[0] is compared with ref(probe) - ref(rest) of that one component: the other terms are
    bit-identical in both points, so the comparison is as sensitive as one term alone, not diluted by the other 127.  Bar:
    the tolerances of the two points, plus 2 * 8 * 2^-53 * sum_j |term_j(rest)| for the rounding of two sums of depth at most
    7 (a lane adds its two parameters, the wave sum has six levels).  A probe outside its support must give -inf exactly, as
    log-prior and as log-posterior.  all_128_rows has every family in lanes 0-63 and in the second parameter of a lane;
    one_row_per_shape (d = 46 < 64) has no second parameter at all."""
    from tinyda_amd.engine import Engine

    g = golden(xf.GOLDEN_NAME)
    rows = xf.decode_rows(g)
    use = list(range(len(rows))) if layout == "all_128_rows" else xf.first_row_of_each_shape(rows)
    d = len(use)
    assert d == (128 if layout == "all_128_rows" else sum(len(v) for v in xf.SHAPES.values()) + 6)
    col = {i: j for j, i in enumerate(use)}
    probes = [(i, k) for i, k in xf.kept_probes(g) if i in col]
    ref, tol = g["ref"], xf.tolerance(g)
    rest = g["x"][use, xf.REST]
    pts = np.tile(rest, (1 + len(probes), 1))
    for n, (i, k) in enumerate(probes):
        pts[1 + n, col[i]] = g["x"][i, k]
    p, q, psrc = family_source([xf.component(rows[i]) for i in use])
    e = Engine(len(pts), d, seed=1)
    e.set_prior_joint(np.full(d, PRIOR_SOURCE), p, q)
    e.set_level_source(0, source() + "\n" + psrc, np.array([0.3]), 0, SIGMA2)
    got = e.evaluate(pts)
    e.close()
    # point 0: the sum of the rest terms
    want0, tol0, sum_abs = math.fsum(ref[use, xf.REST]), float(np.sum(tol[use, xf.REST])), float(np.sum(np.abs(ref[use, xf.REST])))
    print("%s: %d probes; all at rest: error / tolerance %.3e" % (layout, len(probes), abs(got[0, 0] - want0) / tol0))
    assert abs(got[0, 0] - want0) <= tol0
    pi, pk = np.array([i for i, _ in probes]), np.array([k for _, k in probes])
    want = ref[pi, pk] - ref[pi, xf.REST]
    outside = want == -np.inf
    assert outside.sum() >= 2 * 9 and np.all(np.isfinite(want[~outside]))
    mine = got[1:, 0] - got[0, 0]
    assert not np.any(np.isnan(got[:, 0])) and not np.any(got[:, 0] == np.inf)
    assert np.array_equal(got[1:, 0] == -np.inf, outside), [(rows[i], k, g["x"][i, k]) for (i, k), a, b in zip(probes, got[1:, 0] == -np.inf, outside) if a != b]
    assert np.all(got[1:, 2][outside] == -np.inf)
    bar = tol[pi, pk] + tol[pi, xf.REST] + 2 * 8 * 2.0 ** -53 * sum_abs
    ratio = np.where(outside, 0.0, np.abs(mine - np.where(outside, 0.0, want)) / bar)
    names = np.array([rows[i][0] for i in pi])
    for name in xf.FAMILY_NAMES:
        print("%-12s largest error / tolerance %.3e over %d probes, %d outside" % (name, ratio[names == name].max(), (names == name).sum() - outside[names == name].sum(),
                                                                                  outside[names == name].sum()))
    bad = [(rows[i], k, g["x"][i, k], r) for (i, k), r in zip(probes, ratio) if r > 1.0]
    assert not bad, bad


# ---- (b) chains where the density diverges at the edge ----------------------------------------------------------------------------------
EDGE_COMPONENTS = (("gamma", (0.5,)), ("beta", (0.6, 0.8)), ("weibull_min", (0.7,)), ("invgamma", (0.5,)), ("lognorm", (3.0,)), ("t", (1.0,)),
                   ("truncnorm", (6.0, 8.0)), ("expon", None), ("halfnorm", None), ("uniform", None), ("laplace", None), ("cauchy", None),
                   ("norm", None))
EDGE_SCALING = 0.01  # oracle alone, three seeds: acceptance 0.44-0.49, 0.32-0.34 of the proposals outside a support


def test_chains_at_shapes_whose_density_diverges_at_the_edge():
    """gamma, beta and weibull_min with a shape below 1 (the density grows without bound towards z = 0, so a chain is drawn to
    the edge that rejects), the heaviest tails, a truncnorm window in a tail; fixed-scaling random walk, masks exact, log-prior
    and log-posterior at the bars of test_gpu_prior_source.py.  The scaling was chosen with the oracle alone."""
    d, m, N, T = 13, 23, 13, 120
    comps = [xp.component(name, shapes) for name, shapes in EDGE_COMPONENTS]
    rng = np.random.default_rng(d * 1000 + m)
    truth, theta0 = xp.starts_near_lower_edges(comps, N, rng)
    y = np_forward(truth, m)[0] + np.sqrt(SIGMA2) * rng.standard_normal(m)
    prior = xp.FamilyPrior(comps)
    assert np.all(prior.inside(theta0))
    prop = dict(kind="grw", C=np.eye(d), scaling=EDGE_SCALING)
    params, stats, acc, _, _, z, u = run_forward(make_engine(comps, N, [(source(), y, 0, SIGMA2)], prop), theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level_of(comps, m, y), prop, theta0, zz, uu)
    assert_rate(ref["accepted"][:, 1:])
    share = oracle_proposals_outside(ref, prior, zz, prop).mean()
    print("oracle share of proposals outside a support %.3f" % share)
    assert share >= 0.1, share
    compare(params, stats, acc, ref, prior=prior)
    assert np.all(np.isfinite(stats)) and np.all(prior.inside(params.reshape(-1, d)))
