"""The prior family library (tinyda_amd/csrc/tda_prior_families.h) and the host-side constants of its tables over a grid of
shapes and from tail to tail, against mpmath at 80 digits (tests/extfamilies.py has the grid, the points, the reference and
the tolerance; tests/golden/g21_prior_family_terms.npz is their record): the fixture itself, the constants of
likelihoods._family_component on the grid and beyond it, the shipped library compiled for the host behind the prologue of
the 128 rows, and what lowers and what declines."""
import numpy as np
import pytest
import scipy.stats as st

from . import extfamilies as xf
from .extprior import host_library


@pytest.fixture(scope="module")
def g21(golden):
    return golden(xf.GOLDEN_NAME)


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_mpmath_gives(g21):
    """the rows are the grid's, every shape occurs and every family sits in both halves of the table; the reference, the
    magnitudes, cond and the dropped mask recomputed from the stored points are the stored ones bit for bit; the drop stays
    under its caps"""
    pytest.importorskip("mpmath")
    rows = xf.decode_rows(g21)
    assert rows == xf.grid_rows() and len(rows) == xf.N_ROWS
    for name, shapes in xf.SHAPES.items():
        assert {r[1] for r in rows if r[0] == name} == set(shapes), name
    for half in (rows[:64], rows[64:]):
        assert {r[0] for r in half} == set(xf.FAMILY_NAMES)
    assert [r[2:] for r in rows[:4]] == xf.LOC_SCALE
    x = g21["x"]
    assert x.shape == (xf.N_ROWS, xf.N_COLS) and np.array_equal(np.isnan(x[:, xf.OUT_LO:]), ~xf.probe_exists(rows)[:, xf.OUT_LO:])
    again = xf.reference(rows, x)
    for k, v in again.items():
        assert np.array_equal(v, g21[k], equal_nan=True), k
    xf.assert_drop_caps(g21)
    # the points outside are outside, the rest points inside
    assert np.all(g21["ref"][:, xf.OUT_LO:][~np.isnan(x[:, xf.OUT_LO:])] == -np.inf) and np.all(np.isfinite(g21["ref"][:, xf.REST]))


# ---- 2. the constants ---------------------------------------------------------------------------------------------------------------
def _constant_errors(cases):
    """[(case, error / bar)] of likelihoods._family_component(...)[3] against mpmath, the bar being 1e-11 max(1, |c|); a
    component that declines to lower is reported as inf: every case here is expected to lower"""
    from tinyda_amd import likelihoods as lk

    mp = xf._mp()
    out = []
    for name, shapes, loc, scale in cases:
        comp = lk._family_component(xf.component((name, shapes, loc, scale)))
        want = xf.mp_constant(name, shapes) - mp.log(mp.mpf(scale))
        ratio = np.inf if comp is None else float(abs(mp.mpf(comp[3]) - want) / (mp.mpf(10) ** -11 * max(1, abs(want))))
        out.append(((name, shapes, loc, scale), ratio))
    return out


def _assert_constants(cases):
    res = _constant_errors(cases)
    worst = {}
    for (name, *_), r in res:
        worst[name] = max(worst.get(name, 0.0), r)
    print("constants: largest error / bar per family", {k: "%.2e" % v for k, v in worst.items()})
    bad = [(c, r) for c, r in res if not r <= 1.0]
    assert not bad, bad


def test_constants_on_the_grid(g21):
    """every row, and every shape of the grid once more at loc 0, scale 1: a row's log(scale) adds to |c| and so to the bar"""
    pytest.importorskip("mpmath")
    rows = xf.decode_rows(g21)
    _assert_constants(rows + [rows[i][:2] + (0.0, 1.0) for i in xf.first_row_of_each_shape(rows)])


def test_constants_beyond_the_grid():
    """the t constant up to nu = 1e15 (a difference of two gammaln there is noise), truncnorm windows that are narrow, far
    out, or both, and Gamma / Beta functions of huge and tiny arguments"""
    pytest.importorskip("mpmath")
    _assert_constants([(name, shapes) + ls for name, shapes in xf.EXTREME for ls in ((0.0, 1.0), (0.1, 0.7))])


# ---- 3. the shipped library, compiled for the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_terms(g21, tmp_path_factory):
    """[128, 14] the library's term at every stored point (NaN where the point is not finite)"""
    rows = xf.decode_rows(g21)
    term, low = host_library(tmp_path_factory.mktemp("families"), [xf.component(r) for r in rows])
    got = np.full(g21["x"].shape, np.nan)
    for j in range(len(rows)):
        ok = np.isfinite(g21["x"][j])
        got[j, ok] = term(g21["x"][j, ok], j)
    return got, low


def test_host_library_over_the_grid(g21, host_terms):
    got, _ = host_terms
    rows = xf.decode_rows(g21)
    ref, tol = g21["ref"], xf.tolerance(g21)
    keep = ~np.isnan(ref)  # the rest points and every probe that is not dropped
    assert keep.sum() >= 1 + 128 * (1 + xf.KEEP_PER_ROW)
    assert not np.any(np.isnan(got[keep])) and not np.any(got[keep] == np.inf)
    assert np.array_equal(got[keep] == -np.inf, ref[keep] == -np.inf), [(rows[i], k, g21["x"][i, k]) for i, k in zip(*np.nonzero(keep & ((got == -np.inf) != (ref == -np.inf))))]
    fin = keep & np.isfinite(ref)
    ratio = np.zeros(ref.shape)
    ratio[fin] = np.abs(got[fin] - ref[fin]) / tol[fin]
    for name in xf.FAMILY_NAMES:
        mine = np.array([r[0] == name for r in rows])
        print("%-12s largest error / tolerance %.3e over %d points, %d outside" % (name, ratio[mine].max(), fin[mine].sum(), (keep & ~fin)[mine].sum()))
    bad = [(rows[i], k, g21["x"][i, k], ratio[i, k]) for i, k in zip(*np.nonzero(ratio > 1.0))]
    assert not bad, bad


def test_host_library_at_shape_exactly_one(g21, host_terms):
    """gamma(1), beta(1, b) and weibull_min(1): (shape - 1) log z must be an exact zero whatever log z is, so the term is held
    to 4 * 2^-53 of the magnitude (+ cond): c, the remaining piece, their sum and the library call behind the piece each round
    once.  At 1e-11 a `0 * log z` done badly (a shape off by an ulp, a power taken for the product) would pass."""
    got, _ = host_terms
    rows = xf.decode_rows(g21)
    ref, n = g21["ref"], 0
    for i, (name, shapes, _, _) in enumerate(rows):
        if name in ("gamma", "beta", "weibull_min") and shapes[0] == 1.0:
            fin = np.isfinite(ref[i])
            bar = 4 * 2.0 ** -53 * g21["mag"][i, fin] + g21["cond"][i, fin]
            err = np.abs(got[i, fin] - ref[i, fin])
            print(name, shapes, "largest error / bar %.3f over %d points" % (np.max(err / bar), fin.sum()))
            assert np.all(err <= bar), (name, shapes, g21["x"][i, fin][err > bar], (err / bar).max())
            n += 1
    assert n >= 3 * 2  # each of the three at two (loc, scale) at least


# ---- 4. what lowers and what declines ----------------------------------------------------------------------------------------------
def test_keyword_and_positional_arguments_lower_to_the_same_row():
    from tinyda_amd import likelihoods as lk

    for by_keyword, by_position in ((st.t(df=4), st.t(4)), (st.gamma(a=2, scale=3), st.gamma(2, 0, 3)),
                                    (st.truncnorm(a=-1, b=2, loc=.2, scale=.4), st.truncnorm(-1, 2, .2, .4))):
        row = lk._family_component(by_keyword)
        assert row is not None and row == lk._family_component(by_position)
    assert lk._family_component(st.gamma(a=2, scale=3))[1:3] == (2.0, 0.0) and lk._family_component(st.gamma(a=2, scale=3))[4:] == (0.0, 3.0)
    assert lk._family_component(st.truncnorm(a=-1, b=2, loc=.2, scale=.4))[1:3] == (-1.0, 2.0)


def test_components_the_tables_cannot_hold_decline_without_an_exception():
    import tinyda_amd as tda
    from tinyda_amd import likelihoods as lk

    hist = st.rv_histogram(np.histogram(np.random.default_rng(0).standard_normal(100)))
    for comp in (st.truncnorm(-np.inf, 1), st.truncnorm(-1, np.inf), st.gamma([1, 2]), st.beta([1, 2], 3), st.t(4, loc=[0, 1]), hist):
        assert lk._family_component(comp) is None
        assert tda.JointPrior([st.norm(0.0, 1.0), comp])._source_lowering() is None
