"""Warm-up adaptation of a dense mass of HMC / NUTS on the device (k_dense_mass_shift / accumulate / update,
include/tinyda_amd_dense_mass_adaptation.h): the three kernels over chosen inputs through tda_dense_mass_window, the factor after
every window of an engine against the twin of tests/extdensemass.py applied to the engine's own records, the steps before and
after the first update, independence of what is recorded and of how a run is split, checkpoint blobs, the entry points' refusals,
and sample() end to end.

The matrix instruction's sum of four products has no documented order and the device fuses the factorisation's multiply-adds, so
the device is held to the twin and to a two-pass covariance in np.longdouble within the bound of extdensemass.tolerance, not
bitwise; what must be bitwise (cuts, records, splits, resume) is compared device against device."""
import ctypes as C

import numpy as np
import pytest
import scipy.stats as st

from . import extdense as xd
from . import extdensemass as xdm
from . import exthmc as xh
from . import extnuts as xn
from .test_dense_mass_adaptation import END_TO_END, whitened_eigenvalues
from .test_gpu_dense_mass import BITWISE_STEP
from .test_gpu_mass_adaptation import PARENT_NUTS_BLOB_BYTES
from .test_gpu_mass_adaptation import SHAPES as DIAGONAL_SHAPES

pytestmark = pytest.mark.gpu

PERIOD, W = 20, 160
WINDOWS = [(20, 40), (40, 80), (80, 160)]
# d -> (outputs, noise, problem seed, step size): the problems of tests/test_gpu_mass_adaptation.py, and at 128 parameters the
# problem and the step of the bitwise test of tests/test_gpu_dense_mass.py
SHAPES = {5: DIAGONAL_SHAPES[5], 64: DIAGONAL_SHAPES[64], 96: DIAGONAL_SHAPES[96], 128: (23, "diag", 128 * 1000 + 23, BITWISE_STEP[128])}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def window(X, chol_in, cuts=(), shift=None):
    """tda_dense_mass_window over the states X [n, N, d] -> (the factor, refused)"""
    from tinyda_amd import _lib

    lib = _lib.load()
    n, N, d = X.shape
    X, chol_in = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(chol_in, dtype=np.float64)
    cuts = np.ascontiguousarray(cuts, dtype=np.int64)
    shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    out, refused = np.full((d, d), np.nan), np.full(1, -1, dtype=np.int64)
    _lib.check(lib.tda_dense_mass_window(0, d, N, n, _ptr(X), _ptr(cuts) if cuts.size else None, int(cuts.size), _ptr(shift), _ptr(chol_in), _ptr(out), _ptr(refused)), lib)
    return out, int(refused[0])


# ---- 1. the kernels over chosen inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20, 120])
@pytest.mark.parametrize("N", [1, 13, 16, 70, 300])
@pytest.mark.parametrize("d", [1, 5, 16, 17, 64, 65, 128])
def test_window_matches_twin_and_reference(d, N, n):
    """the inputs of tests/test_dense_mass_adaptation.py scaled to the width (one tile, a partial second tile, both ends of
    DP = 128; a partial group of four chains, a partial chunk, exactly one chunk, several chunks), the shift at the origin so that
    |delta| reaches 10 where d allows: L L^T within the bound of the twin's and of the two-pass covariance; the shift kernel gives
    the twin's shift (seen through the factor: within the bound again); the same states cut at (3, 4, n - 5) give the same
    factor bitwise"""
    X = xdm.inputs(n, N, d, seed=1000 * N + n + d)
    start, ref = np.eye(d), xdm.reference(X)
    got, refused = window(X, start, shift=np.zeros(d))
    assert refused == 0
    xdm.assert_window(X, got, start, np.zeros(d), "shift 0:", ref)
    cut, refused = window(X, start, cuts=(3, 4, n - 5), shift=np.zeros(d))
    assert refused == 0 and np.array_equal(cut, got)
    own, refused = window(X, start)  # the shift kernel over X[0]
    assert refused == 0
    xdm.assert_window(X, own, start, xdm.shift(X[0]), "the device's shift:", ref)
    cut, refused = window(X, start, cuts=(3, 4, n - 5))
    assert refused == 0 and np.array_equal(cut, own)


def test_window_refusals_and_edges():
    """a NaN state and an indefinite matrix (a shift so far away that the raw moments cancel to rounding noise: the twin refuses
    it in tests/test_dense_mass_adaptation.py) leave chol_out == chol_in bitwise with refused == 1; a constant parameter gets
    sqrt(1e-3 * 5 / (T + 5)) exactly with exact zeros in its row and column; fewer states than parameters give a finite factor;
    bad arguments are named"""
    from tinyda_amd import _lib

    rng = np.random.default_rng(8)
    for N in (1, 70):
        n, d = 20, 5
        before = np.linalg.cholesky(np.diag(np.arange(2.0, 2.0 + d)) + 0.5)
        X = rng.standard_normal((n, N, d))
        good, refused = window(X, before)
        assert refused == 0 and not np.array_equal(good, before)
        bad = X.copy()
        bad[7, N // 2, 1] = np.nan
        got, refused = window(bad, before)
        assert refused == 1 and np.array_equal(got, before)
        const = X.copy()
        const[:, :, 2] = 0.375
        L, refused = window(const, before)
        T = float(n * N)
        assert refused == 0 and L[2, 2] == np.sqrt(1e-3 * 5.0 / (T + 5.0))
        assert np.all(L[2, :2] == 0.0) and np.all(L[3:, 2] == 0.0) and np.all(np.isfinite(L)) and np.all(np.diag(L) > 0.0)
    far, refused = window(rng.standard_normal((20, 13, 8)), np.eye(8), shift=1e9 * np.ones(8))
    assert refused == 1 and np.array_equal(far, np.eye(8))
    for d, N, n in ((17, 1, 3), (128, 5, 20), (65, 16, 2)):  # n N < d
        L, refused = window(rng.standard_normal((n, N, d)), np.eye(d))
        assert refused == 0 and np.all(np.isfinite(L)) and np.all(np.diag(L) > 0.0) and np.array_equal(L, np.tril(L))
    for kw, word in ((dict(cuts=(5, 5)), "must ascend"), (dict(cuts=(0,)), "must ascend"), (dict(cuts=(20,)), "must ascend")):
        with pytest.raises(_lib.EngineError, match=word):
            window(rng.standard_normal((20, 3, 4)), np.eye(4), **kw)


# ---- 2. engines ----------------------------------------------------------------------------------------------------------------------
def _make(kind, d, N, adapt=W, adaptive=True, block_steps=0, seed=xh.SEED, scaling=None, inv_mass=None, dense=None, period=PERIOD):
    """-> (make() -> an engine, not initialised; the starts; the oracle level; the twin's proposal, diagonal)"""
    m, noise, pseed, eps = SHAPES[d]
    y, th0, pm, pv, nz, level = xh.gaussian_problem(d, m, noise, N, seed=pseed)
    eps = eps if scaling is None else scaling
    prop = xn.nuts(eps, 4, adaptive=adaptive, inv_mass=inv_mass, period=period) if kind == "nuts" else dict(xh.hmc(eps, 4, adaptive, inv_mass), period=period)

    def make():
        mk = xn.gaussian_engine if kind == "nuts" else xh.gaussian_engine
        e = mk(d, m, noise, N, y, pm, pv, nz, prop, block_steps, seed=seed)
        if dense is not None:
            e.set_dense_mass(dense)
        if adapt is not None:
            e.set_dense_mass_adaptation(adapt)
        return e

    return make, th0, level, prop


def _info(t):
    ends = [end for _, end in WINDOWS]
    later = [end for end in ends if end > t]
    return dict(updates=len(ends) - len(later), window_steps=next((t - a for a, b in WINDOWS if a < t < b), 0), next_update=later[0] if later else -1, refused=0)


@pytest.mark.parametrize("N", [1, 70])
@pytest.mark.parametrize("d", [5, 64, 96, 128])
@pytest.mark.parametrize("kind", ["nuts", "hmc"])
def test_factor_is_the_statistic_of_the_records(kind, d, N):
    """after each window get_dense_mass() is within the bound of the twin over that window's recorded states, with the shift
    taken from the state before the window (and within it of the two-pass covariance); the factor does not change anywhere else;
    the four counters say where the schedule stands"""
    make, theta0, _, _ = _make(kind, d, N, block_steps=16 if d == 128 else 0)
    e = make()
    try:
        e.init(theta0)
        L = e.get_dense_mass()
        assert np.array_equal(L, np.eye(d)) and e.get_dense_mass_adaptation() == dict(updates=0, window_steps=0, next_update=40, refused=0)
        states, t = np.empty((0, N, d)), 0
        for piece in (20, 20, 20, 20, 80, 20):
            states = np.concatenate([states, e.run_host(piece)[0]])
            t += piece
            now = e.get_dense_mass()
            ends = [end for _, end in WINDOWS]
            if t in ends:
                first = WINDOWS[ends.index(t)][0]
                xdm.assert_window(states[first:t], now, L, xdm.shift(states[first - 1]), "%s d = %d, window [%d, %d):" % (kind, d, first, t))
                assert not np.array_equal(now, L)
            else:
                assert np.array_equal(now, L), t
            L = now
            assert e.get_dense_mass_adaptation() == _info(t), (t, e.get_dense_mass_adaptation())
        assert np.all(np.isfinite(states)) and e.counters()[0] == 180
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["nuts", "hmc"])
def test_before_the_first_update_the_unit_start_is_the_unit_mass(kind):
    """with the unit start, steps 0 .. 39 are bitwise those of an engine that does not adapt and has the unit mass (the diagonal
    program: W = I gives its numbers bit for bit, tests/test_gpu_dense_mass.py), although the blocks end at period boundaries and
    the window [20, 40) is being folded; step 40 onwards differs"""
    d, N = 5, 13
    got = []
    for adapt in (W, None):
        make, theta0, _, _ = _make(kind, d, N, adapt=adapt)
        e = make()
        try:
            e.init(theta0)
            got.append(e.run_host(60))
        finally:
            e.close()
    (pa, sa, aa), (pb, sb, ab) = got
    assert np.array_equal(pa[:40], pb[:40]) and np.array_equal(sa[:40], sb[:40]) and np.array_equal(aa[:40], ab[:40])
    assert not np.array_equal(pa[40:], pb[40:]) and np.all(np.isfinite(sa))


SEEDS = (91, 92, 93, 94, 95)  # (the engine's seed: the first whose period the twin admits is compared; on the CPU: 91 for both)
AFTER_UPDATE = {"nuts": (0.25, 0.04), "hmc": (0.6, 0.0025)}  # kind -> (step size, the diagonal start)


@pytest.mark.parametrize("kind", ["nuts", "hmc"])
def test_steps_after_an_update_use_the_new_factor(kind):
    """a fixed step size from a diagonal start under which it suits the mass before and after the first update (NUTS: 0.25 from
    0.04, as tests/test_gpu_mass_adaptation.py has it; HMC: 0.6 from 0.0025, chosen on the CPU with the twins alone so that the
    acceptance after the update lies inside the admission rule's 0.1 .. 0.9): steps 40 .. 59, from the state at the boundary, on
    the exported normals and under the factor that get_dense_mass() reports, are the twin's of tests/extdense.py -- masks exact,
    log-posterior 1e-10, states 1e-9 (atol 1e-12).  They are not the twin's under the starting mass"""
    d, N = 5, 13
    eps, w0 = AFTER_UPDATE[kind]
    start_factor = np.diag(np.sqrt(w0 * np.ones(d)))
    tried = []
    for seed in SEEDS:
        make, theta0, level, prop = _make(kind, d, N, adaptive=False, seed=seed, scaling=eps, inv_mass=w0 * np.ones(d))
        e = make()
        try:
            e.init(theta0)
            assert np.array_equal(e.get_dense_mass(), start_factor)  # the start: diag(sqrt(inv_mass))
            z, u = e.set_export(60)
            head = e.run_host(40)
            L = e.get_dense_mass()
            assert e.get_dense_mass_adaptation()["updates"] == 1 and np.count_nonzero(np.tril(L, -1)) == d * (d - 1) // 2
            params, stats, acc = e.run_host(20)
        finally:
            e.close()
        start, zt, ut = head[0][-1], np.swapaxes(z[40:], 0, 1), np.swapaxes(u[40:], 0, 1)
        after = dict(prop, chol=L)
        draws = (lambda: xn.PhiloxDraws(seed, xh.CHAIN_OFFSET, N, step0=40)) if kind == "nuts" else (lambda: ut)
        try:
            ref = xd.assert_admissible(level, after, start, zt, draws())[0]
        except AssertionError as exc:
            tried.append((seed, str(exc)[:80]))
            continue
        print("seed %d admitted (not admitted: %s)" % (seed, tried))
        xd.compare("after_a_dense_mass_update/" + kind, params, stats, acc, ref)
        before = dict(prop, chol=start_factor)
        old = xd.run_nuts(level, before, start, zt, draws()) if kind == "nuts" else xd.run_hmc(level, before, start, zt, draws())
        assert not np.allclose(np.swapaxes(old["theta"][:, 1:], 0, 1), params, rtol=1e-6, atol=1e-9)
        return
    pytest.fail("no seed of %s gives a period that the twin admits: %s" % (SEEDS, tried))


def _end(e):
    return e.get_dense_mass(), e.get_dense_mass_adaptation(), e.proposal_state_scaling(), e.current()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


def test_records_do_not_matter():
    """all parameters recorded into host memory, into device memory, nothing recorded, and thin = 4: bitwise the same factor,
    counters, step sizes and final states"""
    import torch

    from tinyda_amd.engine import pinned_empty

    d, N = 5, 70
    make, theta0, _, _ = _make("nuts", d, N)
    ends = []
    for route in ("host", "device", "none", "thin"):
        e = make()
        try:
            e.init(theta0)
            if route == "host":
                e.run_host(W)
            elif route == "device":
                e.run(W, torch.empty((W, N, d), dtype=torch.float64, device="cuda"))
            elif route == "none":
                e.run(W)
            else:
                e.set_record_thinning(4)
                rec = pinned_empty((W // 4, N, d))
                e.run(W, rec)
                assert np.all(np.isfinite(rec))
            ends.append(_end(e))
        finally:
            e.close()
    assert ends[0][1] == dict(updates=3, window_steps=0, next_update=-1, refused=0) and not np.array_equal(ends[0][0], np.eye(d))
    for other in ends[1:]:
        assert _same(ends[0], other)


@pytest.mark.parametrize("kind,d", [("nuts", 5), ("nuts", 128), ("hmc", 5)])
def test_split_independence_and_resume(kind, d):
    """160 steps in one run(), as 50 + 110, and as 70 steps, get_state, set_state into a fresh engine, 90 steps (blocks of 16
    steps, so that the cuts fall inside blocks, periods and windows alike): records, factor, counters, step sizes and states
    bitwise"""
    N = 11
    make, theta0, _, _ = _make(kind, d, N, block_steps=16)

    def finish(e, recs):
        out = ([np.concatenate(x) for x in zip(*recs)], _end(e), e.counters())
        e.close()
        return out

    a = make()
    a.init(theta0)
    whole = finish(a, [a.run_host(160)])
    b = make()
    b.init(theta0)
    split = finish(b, [b.run_host(50), b.run_host(110)])
    c = make()
    c.init(theta0)
    head = c.run_host(70)
    blob = c.get_state()
    c.close()
    r = make()
    r.init(theta0)
    r.set_state(blob)
    resumed = finish(r, [head, r.run_host(90)])
    assert whole[1][1]["updates"] == 3 and whole[1][1]["refused"] == 0 and whole[2][0] == 160
    for other in (split, resumed):
        assert all(np.array_equal(x, y) for x, y in zip(whole[0], other[0]))
        assert _same(whole[1], other[1]) and whole[2] == other[2]


def test_checkpoint_blobs():
    """the blobs of a NUTS engine that does not adapt, of one with a fixed dense mass and of one that adapts a diagonal mass have
    the lengths they had; a dense-adapting engine's has exactly the items of the header more; it goes only into an engine with the
    same warm-up length, period and kind of adaptation"""
    from tinyda_amd import _lib

    d, N = 5, 11
    DP, NP, NC, PAIRS = 8, 16, 1, 1
    sizes = {}
    for name, kw in (("plain", dict(adapt=None)), ("fixed", dict(adapt=None, dense=np.linalg.cholesky(xd.DENSE(d)))), ("off", dict(adapt=0)), ("on", dict(adapt=W))):
        make, theta0, _, _ = _make("nuts", d, N, **kw)
        e = make()
        try:
            e.init(theta0)
            e.run(30)
            sizes[name] = e.get_state()
        finally:
            e.close()
    make, theta0, _, _ = _make("nuts", d, N, adapt=None)
    e = make()
    try:
        e.set_mass_adaptation(W)
        e.init(theta0)
        e.run(30)
        sizes["diagonal"] = e.get_state()
    finally:
        e.close()
    assert sizes["plain"].size == sizes["fixed"].size == sizes["off"].size == PARENT_NUTS_BLOB_BYTES
    # (the diagonal adaptation's items, as tests/test_gpu_mass_adaptation.py counts them)
    assert sizes["diagonal"].size == PARENT_NUTS_BLOB_BYTES + (8 + 8) + (8 + 4) + (8 + 8) + (8 + 8) + (8 + 8 * DP) + 2 * (8 + 8 * NP * DP) + (8 + 4)
    # W, period (int32), n, updates, the refused count, a [DP], the factor [2][DP][DP], S1 [NC][DP], S2 [NC][pairs][4][64]: each
    # behind its 8-byte length
    extra = (8 + 8) + (8 + 4) + (8 + 8) + (8 + 8) + (8 + 4) + (8 + 8 * DP) + (8 + 8 * 2 * DP * DP) + (8 + 8 * NC * DP) + (8 + 8 * NC * PAIRS * 256)
    assert sizes["on"].size == PARENT_NUTS_BLOB_BYTES + extra
    for adapt, period, dense_kind, match in ((W - PERIOD, PERIOD, True, "another mass adaptation"), (W, 40, True, "another mass adaptation"),
                                             (0, PERIOD, True, "does not match"), (W, PERIOD, False, "does not match|not a state blob")):
        make, theta0, _, _ = _make("nuts", d, N, adapt=adapt if dense_kind else None, period=period)
        e = make()
        try:
            if not dense_kind:
                e.set_mass_adaptation(adapt)
            e.init(theta0)
            with pytest.raises(_lib.EngineError, match=match):
                e.set_state(sizes["on"])
            assert e.counters()[0] == 0 and np.all(np.isfinite(e.run_host(3)[1]))  # (the refused blob left the engine as it was)
        finally:
            e.close()


# ---- 3. the entry points -----------------------------------------------------------------------------------------------------------
def test_entry_points():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    from .test_mala_source import ROSEN_SRC

    d, N = 3, 4
    L = np.linalg.cholesky(xd.DENSE(d))
    e = Engine(N, d, seed=1)
    try:
        e.set_prior(np.zeros(d), np.eye(d))
        e.set_level_source(0, ROSEN_SRC, np.zeros(1), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="TDA_PROP_HMC or TDA_PROP_NUTS must precede set_dense_mass_adaptation"):
            e.set_dense_mass_adaptation(40)
        e.set_proposal(6, None, scaling=0.1, period=20)  # MALA
        with pytest.raises(_lib.EngineError, match="must precede set_dense_mass_adaptation"):
            e.set_dense_mass_adaptation(40)
        for kind, kw in ((xh.PROP_HMC, dict(n_leapfrog=2)), (xn.PROP_NUTS, dict(max_depth=3))):
            e.set_proposal(kind, None, scaling=0.01, period=20, **kw)
            for bad in (30, 20, -40, 50):
                with pytest.raises(_lib.EngineError, match=r"warmup_steps = %d must be a multiple of the period \(20\) and at least two periods" % bad):
                    e.set_dense_mass_adaptation(bad)
            with pytest.raises(_lib.EngineError, match="get_dense_mass_adaptation applies to an initialised"):
                e.get_dense_mass_adaptation()
            # beside the diagonal adaptation, in both orders, each naming the other call
            e.set_mass_adaptation(40)
            with pytest.raises(_lib.EngineError, match="set_dense_mass_adaptation on an engine that adapts a diagonal mass.*tda_engine_set_mass_adaptation"):
                e.set_dense_mass_adaptation(40)
            e.set_mass_adaptation(0)
            e.set_dense_mass_adaptation(40)
            with pytest.raises(_lib.EngineError, match="set_mass_adaptation on an engine that adapts a dense mass.*tda_engine_set_dense_mass_adaptation"):
                e.set_mass_adaptation(40)
            with pytest.raises(_lib.EngineError, match="set_dense_mass on an engine that adapts a dense mass.*tda_engine_set_dense_mass_adaptation"):
                e.set_dense_mass(L)
            # switched off, the older refusals are what they were, word for word
            e.set_dense_mass_adaptation(0)
            e.set_dense_mass(L)
            with pytest.raises(_lib.EngineError, match="set_mass_adaptation on an engine with a dense mass.*tda_engine_set_dense_mass"):
                e.set_mass_adaptation(40)
            e.set_dense_mass(None)
            e.set_mass_adaptation(40)
            with pytest.raises(_lib.EngineError, match="set_dense_mass on an engine that adapts its mass.*tda_engine_set_mass_adaptation"):
                e.set_dense_mass(L)
            e.set_mass_adaptation(0)
            # a dense start, then the adaptation: the factor in force is the start, bit for bit; get_mass stays refused
            e.set_dense_mass(L)
            e.set_dense_mass_adaptation(40)
            e.init(np.zeros((N, d)))
            assert np.array_equal(e.get_dense_mass(), L)
            assert e.get_dense_mass_adaptation() == dict(updates=0, window_steps=0, next_update=40, refused=0)
            with pytest.raises(_lib.EngineError, match="get_mass reads a diagonal mass.*tda_engine_get_dense_mass"):
                e.get_mass()
            assert np.all(np.isfinite(e.run_host(45)[1]))
            info = e.get_dense_mass_adaptation()
            assert info["updates"] == 1 and info["next_update"] == -1 and info["window_steps"] == 0
            assert info["refused"] == 1 or not np.array_equal(e.get_dense_mass(), L)
            # switching it off keeps a start that set_dense_mass gave, and removes one that it made itself
            e.set_dense_mass_adaptation(0)
            e.init(np.zeros((N, d)))
            assert np.array_equal(e.get_dense_mass(), L) and e.get_dense_mass_adaptation() == dict(updates=0, window_steps=0, next_update=-1, refused=0)
            e.set_proposal(kind, None, scaling=0.01, period=20, inv_mass=np.array([4.0, 1.0, 0.25]), **kw)
            e.set_dense_mass_adaptation(40)
            e.init(np.zeros((N, d)))
            assert np.array_equal(e.get_dense_mass(), np.diag([2.0, 1.0, 0.5]))
            e.set_dense_mass_adaptation(0)
            e.init(np.zeros((N, d)))
            with pytest.raises(_lib.EngineError, match="get_dense_mass applies to an initialised"):
                e.get_dense_mass()
            assert np.array_equal(e.get_mass()[0], [4.0, 1.0, 0.25])
            # set_proposal clears it, and takes it as a keyword
            e.set_dense_mass_adaptation(40)
            e.set_proposal(kind, None, scaling=0.01, period=20, **kw)
            e.init(np.zeros((N, d)))
            assert e.get_mass()[1] == dict(updates=0, window_steps=0, next_update=-1, refused=0)
            e.set_proposal(kind, None, scaling=0.01, period=20, adapt_mass=40, adapt_dense=True, dense_mass=L, **kw)
            e.init(np.zeros((N, d)))
            assert np.array_equal(e.get_dense_mass(), L) and e.get_dense_mass_adaptation()["next_update"] == 40
            with pytest.raises(ValueError, match="adapt_dense=True needs adapt_mass > 0"):
                e.set_proposal(kind, None, scaling=0.01, period=20, adapt_dense=True, **kw)
    finally:
        e.close()


def test_lds_refusal_applies_at_init():
    """the source of tests/test_gpu_dense_mass.py under which the diagonal NUTS program holds exactly 64 KiB per chain: an engine
    that adapts a dense mass builds the dense program from the start, so init refuses it with the byte counts of the dense mass"""
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    from . import extwave as xw

    d, m, N = 5, 24, 4
    _, y, theta0 = xw.problem(d, m, N, seed=524, sigma=0.01)
    src = xw.source("wave", "wave")
    big = "#define TDA_WORKSPACE 7752\n" + "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("#define TDA_WORKSPACE"))
    e = Engine(N, d, seed=1)
    try:
        e.set_prior(np.zeros(d), np.eye(d))
        e.set_level_source(0, big, y, 0, [1e-4])
        e.set_proposal(xn.PROP_NUTS, None, scaling=0.05, max_depth=10, period=20, adapt_mass=40, adapt_dense=True)
        with pytest.raises(_lib.EngineError, match=r"NUTS over a source-defined model needs more than 64 KiB of LDS per chain: this source needs 65088 bytes "
                                                   r".*1024 bytes for the operand of the dense mass's products\).* = 66560 bytes"):
            e.init(theta0)
    finally:
        e.close()


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
def test_sample_learns_the_covariance():
    """sample(backend='hip') on N(0, R diag(sd^2) R^T), sd = logspace(-1.5, 1.5, 8), 256 chains started from the posterior, 400
    steps of NUTS(0.05, adaptive, period 20, adapt_mass=160, adapt_dense=True): every eigenvalue of the learnt W whitened by the
    true covariance in [0.5, 2], three updates, none refused, and the mean tree depth of the last 100 steps below that of the same
    call with adapt_dense=False (tests/test_dense_mass_adaptation.py holds the NumPy reference to the same conditions)"""
    import copy
    import pickle

    import tinyda_amd as tda

    from .test_gpu_mala_source import _linear_source

    cfg = END_TO_END
    sd, N, T = cfg["sd"], cfg["N"], cfg["T"]
    R, Sigma = xdm.rotated_problem(sd, cfg["rotation_seed"])
    d, pv = sd.shape[0], 1e4
    nv = 1.0 / (1.0 / sd ** 2 - 1.0 / pv)  # F = R^T theta under the prior N(0, pv I): the posterior is N(0, R diag(sd^2) R^T)
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), pv * np.eye(d)), tda.GaussianLogLike(np.zeros(d), np.diag(nv)), tda.DeviceModel(_linear_source(R.T.copy()), d))
    starts = list((sd[None, :] * np.random.default_rng(5).standard_normal((N, d))) @ R.T)
    depth = {}
    for dense in (True, False):
        prop = tda.NUTS(cfg["scaling"], adaptive=True, period=cfg["period"], adapt_mass=cfg["adapt_mass"], adapt_dense=dense)
        head = tda.sample(post, prop, T - 100, n_chains=N, initial_parameters=starts, seed=21, backend="hip")
        res = tda.sample(post, prop, T, n_chains=N, initial_parameters=starts, seed=21, backend="hip")
        assert res["backend"] == "hip"
        ps, ps_head = res["proposal_state"], head["proposal_state"]
        # (a run is the head of a longer one: the last 100 steps' depths are the difference of the two runs' sums)
        depth[dense] = float(np.mean(np.asarray(ps["mean_tree_depth"]) * T - np.asarray(ps_head["mean_tree_depth"]) * (T - 100)) / 100.0)
        if dense:
            assert list(ps)[6:10] == ["inv_mass", "chol_inv_mass", "mass_updates", "mass_refused"] and len(ps) == 14
            Wm, L = np.asarray(ps["inv_mass"]), np.asarray(ps["chol_inv_mass"])
            assert Wm.shape == (d, d) and L.shape == (d, d) and np.array_equal(L, np.tril(L)) and np.all(np.diag(L) > 0.0)
            np.testing.assert_allclose(Wm, L @ L.T, rtol=1e-13, atol=1e-300)
            ev = whitened_eigenvalues(0.5 * (Wm + Wm.T), Sigma)
            print("eigenvalues of the learnt W whitened by the covariance: %.3f .. %.3f" % (ev.min(), ev.max()))
            assert 0.5 <= ev.min() and ev.max() <= 2.0
            assert ps["mass_updates"] == 3 and ps["mass_refused"] == 0
            assert np.array_equal(ps["chol_inv_mass"], ps_head["chol_inv_mass"])  # frozen after step 160
            for other in (copy.deepcopy(ps), pickle.loads(pickle.dumps(ps))):
                assert list(other) == list(ps) and np.array_equal(other["inv_mass"], Wm) and np.array_equal(other["chol_inv_mass"], L)
                assert other["mass_updates"] == 3 and other["mass_refused"] == 0
        else:
            assert list(ps)[6:9] == ["inv_mass", "mass_updates", "mass_refused"] and len(ps) == 13 and ps["inv_mass"].shape == (d,)
        tail = tda.get_samples(res, burnin=T - 100)
        assert np.all(np.isfinite(np.stack([tail["chain_%d" % i] for i in range(N)])))
    print("mean tree depth of the last 100 steps: %.2f dense, %.2f diagonal" % (depth[True], depth[False]))
    assert depth[True] < depth[False]
