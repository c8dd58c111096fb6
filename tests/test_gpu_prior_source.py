"""Source-defined priors on the device (TDA_PRIOR_SOURCE: tda_logprior_term compiled into tda_user_steps): the reference's
chains replayed through set_replay (g19), Philox forward mode against the oracle with scipy's own logpdf as the prior
(single level, Delayed Acceptance / MLDA), chains started at the edges of the supports, an all-normal DevicePrior against
the engine's own diagonal Gaussian prior, tda_engine_evaluate, checkpoint resume, the engine's refusals and
sample(backend='hip').

Every case that is compared with the oracle is conditioned on the oracle's acceptance rate lying in [0.1, 0.9], so that
agreement of the accept masks is not vacuous; the scalings were chosen on the CPU with the oracle alone."""
import warnings

import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from . import extprior as xp
from .extengine import (NOISE_SOURCE, PRIOR_SOURCE, assert_levels_resume_bitwise, assert_rate, assert_resume_bitwise, compare, compare_levels,
                        compare_replay, oracle_uniforms, run_forward, run_levels_forward, set_proposal)
from .extmodel import np_forward, source
from .extprior import SIGMA2, family_source, level_of, make_engine, oracle_proposals_outside
from .test_prior_source import _g19_components, g19_oracle_proposal

pytestmark = pytest.mark.gpu

SEED, CHAIN_OFFSET = 93, 5  # (extprior.make_engine's defaults, for the engines that are set up by hand below)


def problem(d, m, N, seed, names=xp.FAMILY_NAMES, q0=0.15):
    """the 13 families cycled over the parameters, data from a point at low quantiles of the components, starts around it"""
    rng = np.random.default_rng(seed)
    comps = xp.components(d, names)
    truth, theta0 = xp.starts_near_lower_edges(comps, N, rng, q0)
    y = np_forward(truth, m)[0] + np.sqrt(SIGMA2) * rng.standard_normal(m)
    return comps, y, theta0


# ---- 1. the reference's chains ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g19_prior_families_grw", "g19_prior_families_am"])
def test_engine_replays_reference_chain(golden, name):
    g = golden(name)
    am = "C0" in g.files
    N, T1, d = g["theta"].shape
    comps = _g19_components(g)
    prop = g19_oracle_proposal(g)
    e = make_engine(comps, N, [(source(), g["data"], 0, float(g["sigma2"]))], prop, seed=1, chain_offset=0)
    e.init(g["theta0"])
    e.set_replay(np.swapaxes(g["z"], 0, 1), np.swapaxes(g["u"], 0, 1))
    params, stats, acc = e.run_host(T1 - 1)
    state = e.proposal_state(want_am=am)
    e.close()
    compare_replay(params, stats, acc, g, logprior=True, **(dict(C=state["C"]) if am else dict(scaling=state["scaling"])))
    assert_rate(g["accepted"][:, 1:])
    assert int(g["n_outside"]) >= 1


# ---- 2. Philox forward mode against the oracle -----------------------------------------------------------------------------------
# d, m, proposal (the oracle's description), block_steps, likelihood (None: isotropic Gaussian noise; "t": a DeviceLogLike)
CASES = {
    "d1_m1_grw": (1, 1, dict(kind="grw", C=np.eye(1), scaling=0.3), 0, None),
    "d5_m23_grw_adaptive_split": (5, 23, dict(kind="grw", C=4e-3 * np.eye(5), scaling=1.0, adaptive=True, gamma=1.01, period=20), 33, None),
    "d13_m300_am": (13, 300, dict(kind="am", C0=2e-4 * np.eye(13), t0=20, period=20), 0, None),
    "d96_m300_grw_adaptive_split": (96, 300, dict(kind="grw", C=1e-4 * np.eye(96), scaling=1.0, adaptive=True, gamma=1.01, period=20), 16, None),
    "d128_m23_am_adaptive_split": (128, 23, dict(kind="am", C0=5e-5 * np.eye(128), t0=40, period=20, adaptive=True, gamma=1.01), 33, None),
    "d13_m23_student_loglike_grw": (13, 23, dict(kind="grw", C=1e-3 * np.eye(13), scaling=1.0), 0, "t"),
}


def case_inputs(case, N=13):
    d, m, prop, bs, like = CASES[case]
    comps, y, theta0 = problem(d, m, N, seed=d * 1000 + m)
    if like is None:
        return comps, m, prop, bs, theta0, (source(), y, 0, SIGMA2), level_of(comps, m, y)
    par = 0.1 * (1.0 + 0.1 * np.arange(m) / m)
    level = xl.LogLikeLevel(lambda th: np_forward(th, m), y, par, xl.KINDS[like][1], xp.FamilyPrior(comps))
    return comps, m, prop, bs, theta0, (source() + xl.KINDS[like][0], y, NOISE_SOURCE, par), level


@pytest.mark.parametrize("case", list(CASES))
def test_philox_forward_matches_oracle(case):
    N, T = 13, 120
    comps, m, prop, bs, theta0, lvl, level = case_inputs(case, N)
    params, stats, acc, scal, C, z, u = run_forward(make_engine(comps, N, [lvl], prop, bs), theta0, T, prop)
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    # (above 64 parameters the 128-term proposal sum and the adapted factor put their relative error into every increment)
    compare(params, stats, acc, ref, scal, prior=level.prior, span_form=params.shape[-1] > 64)
    if C is not None:
        np.testing.assert_allclose(C, ref["C"], rtol=1e-9, atol=1e-14)


# ---- 3. hierarchies ---------------------------------------------------------------------------------------------------------------
# d, m, (shift, coup) per level (the finest is the model itself), subchain lengths, fine steps, proposal, block_steps
HIER = {
    "da_grw_adaptive": (5, 23, [(0.004, 0.4), (0.0, 0.5)], [3], 25, dict(kind="grw", C=4e-3 * np.eye(5), scaling=1.0, adaptive=True, gamma=1.02, period=15), 0),
    "mlda_am": (13, 23, [(0.03, 0.2), (0.015, 0.35), (0.0, 0.5)], [3, 2], 14, dict(kind="am", C0=1e-3 * np.eye(13), t0=20, period=10), 7),
}


def hier_inputs(case, N=16):
    d, m, lv, sl, n_fine, prop, bs = HIER[case]
    comps, y, theta0 = problem(d, m, N, seed=77 + d + m)
    levels = [level_of(comps, m, y, sh, cp) for sh, cp in lv]
    return comps, m, lv, sl, n_fine, prop, bs, y, theta0, levels


def hier_engine(case, N=16, seed=993):
    comps, m, lv, sl, n_fine, prop, bs, y, theta0, levels = hier_inputs(case, N)
    e = make_engine(comps, N, [(source(shift=sh, coup=cp), y, 0, SIGMA2) for sh, cp in lv], prop, bs, seed=seed, chain_offset=0, subchains=sl)
    e.init(theta0)
    return e, sl, n_fine, prop, theta0, levels


@pytest.mark.parametrize("case", list(HIER))
def test_hierarchy_matches_oracle(case):
    N, seed = 16, 993
    e, sl, n_fine, prop, theta0, levels = hier_engine(case, N, seed)
    rows, z, outs, scal = run_levels_forward(e, n_fine)
    us, ridx = oracle_uniforms(seed, N, rows, sl, None)
    res, pstate = orc.run_multilevel(levels, prop, sl, theta0, np.swapaxes(z, 0, 1), us, n_fine, ridx)
    assert_rate(res[-1]["accepted"][:, 1:])
    assert_rate(res[0]["accepted"])
    np.testing.assert_allclose(scal, pstate.scaling, rtol=1e-12)
    compare_levels(outs, res, logprior_of=[level.prior for level in levels])


# ---- 4. supports ------------------------------------------------------------------------------------------------------------------
BOUNDED = ("lognorm", "gamma", "beta", "uniform", "expon", "halfnorm", "invgamma", "truncnorm", "weibull_min")


def support_inputs(N=13):
    """starts within 1e-3 of an edge of every component's support, fixed-scaling random walk"""
    d, m = 9, 23
    rng = np.random.default_rng(909)
    comps = xp.components(d, BOUNDED)
    theta0 = np.empty((N, d))
    for j, c in enumerate(comps):
        lo, hi = xp.support(c)
        off = 1e-3 * (0.05 + 0.9 * rng.random(N))
        theta0[:, j] = np.where((np.arange(N) + j) % 2 == 0, lo + off, hi - off) if np.isfinite(hi) else lo + off
    y = np_forward(theta0[0], m)[0] + np.sqrt(SIGMA2) * rng.standard_normal(m)
    prop = dict(kind="grw", C=np.eye(d), scaling=3e-4)
    return comps, m, y, theta0, prop


def test_proposals_outside_the_supports_are_rejected():
    N, T = 13, 120
    comps, m, y, theta0, prop = support_inputs(N)
    prior = xp.FamilyPrior(comps)
    assert np.all(prior.inside(theta0))
    params, stats, acc, _, _, z, u = run_forward(make_engine(comps, N, [(source(), y, 0, SIGMA2)], prop), theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level_of(comps, m, y), prop, theta0, zz, uu)
    outside = oracle_proposals_outside(ref, prior, zz, prop)
    share = outside.mean()
    print("oracle share of proposals outside a support %.3f, acceptance %.3f" % (share, ref["accepted"][:, 1:].mean()))
    assert 0.1 <= share <= 0.9, share
    assert not np.any(ref["accepted"][:, 1:][outside])
    compare(params, stats, acc, ref, prior=prior)
    assert np.all(np.isfinite(stats)) and np.all(prior.inside(params.reshape(-1, len(comps))))


# ---- 5. an all-normal DevicePrior against the engine's own diagonal Gaussian prior ------------------------------------------------
@pytest.mark.parametrize("d,m,prop,bs", [(5, 23, dict(kind="grw", C=1e-3 * np.eye(5), scaling=1.0, adaptive=True, gamma=1.01, period=20), 0),
                                         (96, 300, dict(kind="am", C0=6e-5 * np.eye(96), t0=40, period=20), 16)])
def test_normal_device_prior_matches_diagonal_gaussian_prior(d, m, prop, bs):
    from tinyda_amd.engine import Engine

    from .test_gpu_loglike_source import problem as gauss_problem

    N, T = 13, 120
    y, var, theta0, pm, pv = gauss_problem(d, m, "gauss", N, seed=d * 1000 + m)
    runs = []
    for src_prior in (False, True):
        e = Engine(N, d, seed=SEED, chain_offset=CHAIN_OFFSET, block_steps=bs)
        if src_prior:
            e.set_prior_joint(np.full(d, PRIOR_SOURCE), pm, np.sqrt(pv))
        else:
            e.set_prior(pm, np.diag(pv))
        e.set_level_source(0, source() + (xp.NORMAL_SRC if src_prior else ""), y, 1, var)
        set_proposal(e, prop)
        e.init(theta0)
        runs.append(e.run_host(T) + (e.proposal_state_scaling(),))
        e.close()
    (p0, s0, a0, c0), (p1, s1, a1, c1) = runs
    assert np.array_equal(a0, a1) and 0.1 <= a0.mean() <= 0.9
    # (the two sums associate differently -- -1/2 (logconst + sum r^2 / var) against sum of whole terms -- so not bitwise)
    np.testing.assert_allclose(s1[:, :, 0], s0[:, :, 0], rtol=1e-11)
    np.testing.assert_allclose(s1[:, :, 2], s0[:, :, 2], rtol=1e-11)
    np.testing.assert_allclose(p1, p0, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(c1, c0, rtol=1e-12)


# ---- 6. tda_engine_evaluate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(13, 23), (128, 300)])
def test_evaluate_against_scipy(d, m):
    """points inside and outside the supports; the prior is set AFTER the level here, so the program is compiled again"""
    from tinyda_amd.engine import Engine

    N = 11
    comps, y, theta0 = problem(d, m, N, seed=d + m)
    p, q, psrc = family_source(comps)
    e = Engine(N, d, seed=SEED)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, source() + "\n" + psrc, y, 0, SIGMA2)
    e.set_prior_joint(np.full(d, PRIOR_SOURCE), p, q)
    pts = theta0 + 0.05 * np.random.default_rng(2).standard_normal((N, d))
    pts[0] = theta0[0]
    pts[1, 0], pts[2, 4], pts[3, 2] = -0.01, 0.9, 1.0  # below the lognormal's support, above the uniform's, on the beta's open edge
    got_before_init = e.evaluate(pts)
    e.set_proposal(0, 1e-3 * np.eye(d))
    e.init(theta0)
    got = e.evaluate(pts)
    e.close()
    lp, ll, _ = level_of(comps, m, y).evaluate(pts)
    assert np.isfinite(lp[0]) and np.any(lp == -np.inf)
    assert np.array_equal(np.isfinite(lp), np.isfinite(got[:, 0])) and np.all(got[~np.isfinite(lp), 0] == -np.inf)
    fin = np.isfinite(lp)
    # (no chain has run: rounding alone, measured against the sum of the terms' magnitudes because the terms may cancel)
    assert np.all(np.abs(got[fin, 0] - lp[fin]) <= 1e-11 * xp.FamilyPrior(comps).magnitude(pts[fin]))
    np.testing.assert_allclose(got[:, 1], ll, rtol=1e-11)
    assert np.array_equal(got, got_before_init)


def test_programs_are_built_again_when_the_prior_changes_form():
    """one engine, the linear source model with the lognormal term and its gradient: the step program goes from the source's
    prior to the engine's Gaussian code (evaluate under each), then the MALA program from the Gaussian code to the source's prior
    (init under each, one step).  MALA over a source-defined model takes a Gaussian prior through set_prior only, so the same
    normal components are set that way for it.  Log-prior and log-likelihood against the NumPy twins at every stage, with the
    bounds of test_evaluate_against_scipy."""
    import scipy.stats as st

    from tinyda_amd.engine import Engine

    from .extpriorgrad import LOGNORMAL_GRAD_SRC
    from .test_gpu_mala_source import _linear_source

    d, m, N = 3, 4, 2
    rng = np.random.default_rng(12)
    A = rng.standard_normal((m, d))
    theta0 = np.exp(0.2 * rng.standard_normal((N, d)))
    y = theta0[0] @ A.T + np.sqrt(SIGMA2) * rng.standard_normal(m)
    p, q = 0.1 * np.arange(d), 0.5 + 0.1 * np.arange(d)
    loc, scale = 1.0 + 0.1 * np.arange(d), 0.5 + 0.25 * np.arange(d)
    pts = theta0 * np.array([[1.1], [0.9]])

    def check(got, theta, source_prior):
        if source_prior:
            terms = xp.lognormal_terms(theta, p, q)
        else:
            terms = st.norm(loc, scale).logpdf(theta)
        level = orc.CallableGaussianLevel(lambda t: t @ A.T, y, "iso", SIGMA2, orc.MVNPrior(loc, np.diag(scale ** 2)))
        ll = level.evaluate(theta)[1]
        assert np.all(np.isfinite(terms)) and np.all(np.abs(got[:, 0] - terms.sum(axis=1)) <= 1e-11 * np.abs(terms).sum(axis=1)), (got[:, 0], terms.sum(axis=1))
        np.testing.assert_allclose(got[:, 1], ll, rtol=1e-11)

    e = Engine(N, d, seed=SEED)
    try:
        e.set_prior(np.zeros(d), np.eye(d))
        e.set_level_source(0, _linear_source(A) + xp.LOGNORMAL_SRC + LOGNORMAL_GRAD_SRC, y, 0, SIGMA2)
        e.set_prior_joint(np.full(d, PRIOR_SOURCE), p, q)
        check(e.evaluate(pts), pts, True)
        e.set_prior_joint(np.zeros(d, dtype=np.int32), loc, scale)  # the step program: the source's term -> the engine's own code
        check(e.evaluate(pts), pts, False)
        e.set_prior(loc, np.diag(scale ** 2))
        e.set_proposal(6, None, scaling=0.05)
        e.init(theta0)
        check(e.current()[1], theta0, False)
        e.set_prior_joint(np.full(d, PRIOR_SOURCE), p, q)  # the MALA program: the engine's own code -> the source's term and gradient
        e.init(theta0)
        check(e.current()[1], theta0, True)
        params, stats, _ = e.run_host(1)
        check(stats[0], params[0], True)
        assert np.array_equal(e.current()[0], params[0])
    finally:
        e.close()


def test_start_outside_a_support_keeps_minus_inf_until_a_move_inside():
    """a chain started outside a support has log-prior -inf (as the host protocol and the DeviceLogLike path keep a -inf
    likelihood): the first proposal inside every support is accepted, whatever its density"""
    N, T = 13, 60
    comps, y, theta0 = problem(5, 23, N, seed=31)
    theta0 = theta0.copy()
    theta0[::2, 0] = -1e-3  # lognorm component
    prop = dict(kind="grw", C=4e-3 * np.eye(5), scaling=1.0)
    e = make_engine(comps, N, [(source(), y, 0, SIGMA2)], prop)
    e.init(theta0)
    assert np.all(e.current()[1][::2, 0] == -np.inf) and np.all(np.isfinite(e.current()[1][1::2, 0]))
    z, u = e.set_export(T)
    params, stats, acc = e.run_host(T)
    e.close()
    ref = orc.run_mh(level_of(comps, 23, y), prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert np.all(ref["logprior"][::2, 0] == -np.inf) and np.all(np.isfinite(ref["logprior"][::2, -1]))
    assert np.array_equal(acc, np.swapaxes(ref["accepted"][:, 1:], 0, 1))
    got, want = stats[:, :, 0], np.swapaxes(ref["logprior"][:, 1:], 0, 1)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.all(got[~np.isfinite(want)] == -np.inf)
    np.testing.assert_allclose(got[np.isfinite(want)], want[np.isfinite(want)], rtol=1e-10)


# ---- 7. checkpoints -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d96_m300_grw_adaptive_split", "d13_m300_am"])
def test_checkpoint_resume_is_bitwise(case):
    """get_state mid period, set_state into a fresh engine (the blob format carries nothing new: the prior is set-up, not state)"""
    N = 11
    comps, m, prop, bs, theta0, lvl, _ = case_inputs(case, N)

    def make():
        e = make_engine(comps, N, [lvl], prop, bs)
        e.init(theta0)
        return e

    assert_resume_bitwise(make)


def test_hierarchy_checkpoint_resume_is_bitwise():
    assert_levels_resume_bitwise(hier_engine("da_grw_adaptive", 12, seed=77)[0])


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_engine_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine
    from tinyda_amd.proposals import OperatorWeightedCrankNicolson

    d, m, N = 2, 3, 4
    y = np.array([0.1, 0.2, 0.3])
    src = source() + xp.LOGNORMAL_SRC
    kinds, p, q = np.full(d, PRIOR_SOURCE), np.zeros(d), np.ones(d)
    th0 = np.ones((N, d))

    def refused(e, match, theta0=th0):
        with pytest.raises(_lib.EngineError, match=match):
            e.init(theta0)

    # one single-level engine, one compile: every proposal the prior is closed to, and the missing initial parameters
    e = Engine(N, d, seed=1)
    try:
        with pytest.raises(_lib.EngineError, match="all source-defined"):
            e.set_prior_joint(np.array([PRIOR_SOURCE, 0]), p, q)
        with pytest.raises(_lib.EngineError, match="finite"):
            e.set_prior_joint(kinds, p, np.array([1.0, np.inf]))
        e.set_prior_joint(kinds, p, -q)  # (no positivity check on q for this kind)
        e.set_prior_joint(kinds, p, q)
        with pytest.raises(_lib.EngineError, match=r"defines no __device__ double tda_logprior_term\(double x, double p, double q, int j\)"):
            e.set_level_source(0, source(), y, 0, SIGMA2)
        e.set_level_source(0, src, y, 0, SIGMA2)
        e.set_proposal(0, 0.01 * np.eye(d))
        refused(e, "explicit initial parameters", None)
        e.set_proposal(1, None, scaling=0.1)
        refused(e, "source-defined prior under pCN")
        ow = OperatorWeightedCrankNicolson(0.5 * np.eye(d), 0.5)._lowering()
        e.set_proposal(**ow)
        refused(e, "source-defined prior under pCN and operator-weighted pCN")
        e.set_proposal(6, None, scaling=0.1)
        refused(e, "source-defined prior under MALA")
        e.set_proposal(4, np.eye(d), q_mean=np.zeros(d))
        refused(e, "source-defined prior under the Independence")
        e.set_proposal(0, 0.01 * np.eye(d))
        e.init(th0)  # ... and the engine is still good for what is lowered
        assert np.all(np.isfinite(e.run_host(3)[1]))
        e.set_proposal_dreamz(M0=10)
        refused(e, "source-defined prior under DREAM")
    finally:
        e.close()
    # levels whose prior another kernel would evaluate
    for setup in (lambda e: e.set_level(0, np.ones((m, d)), y, 0, SIGMA2),
                  lambda e: e.set_level_callback(0, lambda th: np.zeros((len(th), m)), y, 0, SIGMA2),
                  lambda e: e.set_level_source(0, src, y, 2, SIGMA2 * np.eye(m))):
        e = Engine(N, d, seed=1)
        try:
            e.set_prior_joint(kinds, p, q)
            setup(e)
            e.set_proposal(0, 0.01 * np.eye(d))
            refused(e, "source-defined prior needs source-defined forward models")
            with pytest.raises(_lib.EngineError, match="source-defined prior is evaluated by the step program"):
                e.evaluate(th0)
        finally:
            e.close()
    # a level program compiled before the prior was set, from a source without the function: named at init
    e = Engine(N, d, seed=1)
    try:
        e.set_prior(np.zeros(d), np.eye(d))
        e.set_level_source(0, source(), y, 0, SIGMA2)
        e.set_prior_joint(kinds, p, q)
        e.set_proposal(0, 0.01 * np.eye(d))
        refused(e, "defines no __device__ double tda_logprior_term")
    finally:
        e.close()
    # hierarchies: randomised subchain lengths, error models
    e = Engine(N, d, seed=1, n_levels=2)
    try:
        e.set_prior_joint(kinds, p, q)
        e.set_level_source(0, src, y, 0, SIGMA2)
        e.set_level_source(1, src, y, 0, SIGMA2)
        e.set_proposal(0, 0.01 * np.eye(d))
        e.set_subchains([3], True)
        refused(e, "source-defined prior with randomised subchain")
        e.set_subchains([3], False)
        e.set_error_model("state-independent-diagonal")
        refused(e, "source-defined prior together with an error model")
    finally:
        e.close()


def test_engine_refuses_five_levels():
    """five and six levels run on the engine's generic level kernel, which evaluates the prior itself"""
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    d, N = 2, 4
    y = np.array([0.1, 0.2, 0.3])
    e = Engine(N, d, seed=1, n_levels=5)
    try:
        e.set_prior_joint(np.full(d, PRIOR_SOURCE), np.zeros(d), np.ones(d))
        for k in range(5):
            e.set_level_source(k, source() + xp.LOGNORMAL_SRC, y, 0, SIGMA2)
        e.set_proposal(0, 0.01 * np.eye(d))
        e.set_subchains([2, 2, 2, 2], False)
        with pytest.raises(_lib.EngineError, match="source-defined prior: hierarchies of at most 4 levels"):
            e.init(np.ones((N, d)))
    finally:
        e.close()


# ---- 9. sample() ------------------------------------------------------------------------------------------------------------------------
def _sample_posteriors(d, m, fidelities):
    import tinyda_amd as tda

    comps, y, _ = problem(d, m, 1, seed=12)
    prior = tda.JointPrior(comps)
    like = tda.GaussianLogLike(y, SIGMA2 * np.eye(m))
    return comps, [tda.Posterior(prior, like, tda.DeviceModel(source(shift=sh, coup=cp), m, reference=lambda th, sh=sh, cp=cp: np_forward(th, m, shift=sh, coup=cp)[0]))
                   for sh, cp in fidelities]


def test_sample_api_family_prior_single_level():
    """theta0 ~ prior drawn on the host from the components, keyed by the global chain id; 4096 chains on the device"""
    import tinyda_amd as tda
    from tinyda_amd import api

    d, m, N, T = 13, 23, 4096, 60
    comps, (post,) = _sample_posteriors(d, m, [(0.0, 0.5)])
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(post, tda.AdaptiveMetropolis(2e-4 * np.eye(d), t0=20, period=20), T, n_chains=N, seed=7, backend="hip", chain_offset=2)
    assert res["sampler"] == "MH" and res["backend"] == "hip" and res["n_chains"] == N
    prior = xp.FamilyPrior(comps)
    starts = api._source_prior_starts(post.prior, N, 2, 7)
    for c in (0, 1777, N - 1):
        ch = res["chain_%d" % c]
        assert np.array_equal(ch[0].parameters, starts[c])
        link = ch[-1]
        assert np.isclose(link.prior, prior.logpdf(link.parameters)[0], rtol=1e-10)
        assert np.isclose(link.posterior, post.create_link(link.parameters).posterior, rtol=1e-10)
    rate = np.mean([np.mean(res["chain_%d" % c].accepted[1:]) for c in range(0, N, 64)])
    assert 0.05 < rate < 0.95
    last = np.stack([res["chain_%d" % c][-1].parameters for c in range(0, N, 16)])
    assert np.all(prior.inside(last))


def test_sample_api_family_prior_delayed_acceptance():
    import tinyda_amd as tda

    d, m, N = 5, 23, 4096
    comps, posts = _sample_posteriors(d, m, [(0.004, 0.4), (0.0, 0.5)])
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(posts, tda.GaussianRandomWalk(4e-3 * np.eye(d), adaptive=True, period=20), 40, n_chains=N, subchain_length=3, seed=5,
                         backend="auto")
    assert res["sampler"] == "DA" and res["backend"] == "hip"
    for c in (0, 1777, N - 1):
        link = res["chain_fine_%d" % c][-1]
        assert np.isclose(link.posterior, posts[1].create_link(link.parameters).posterior, rtol=1e-10)
    rate = np.mean([np.mean(res["chain_fine_%d" % c].accepted[1:]) for c in range(0, N, 64)])
    assert 0.05 < rate < 0.95
