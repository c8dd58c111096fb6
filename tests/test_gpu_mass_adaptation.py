"""Warm-up adaptation of the diagonal mass of HMC / NUTS on the device (k_mass_accumulate / k_mass_update, include/tinyda_amd_mass.h):
the mass after every window against the twin of tests/extmass.py applied to the device's own records, the steps after an update
against the twins of tests/extnuts.py / tests/exthmc.py under the mass the device reports, independence of what is recorded and of
how a run is split, bitwise checkpoint resume, a constant parameter, the refusals of the two entry points, and sample() end to end.

Every engine here runs extmodel's source (the program the HMC / NUTS tests compile) with periods of 20 steps, at most 8 of them."""
import numpy as np
import pytest
import scipy.stats as st

from . import exthmc as xh
from . import extmass as xms
from . import extnuts as xn
from .test_mass_adaptation import END_TO_END

pytestmark = pytest.mark.gpu

PERIOD, W = 20, 160
WINDOWS = [(20, 40), (40, 80), (80, 160)]
# d -> (outputs, noise, problem seed, step size): the problems of exthmc.FORWARD_CASES / extnuts.FORWARD_CASES at these widths
SHAPES = {1: (1, "iso", 5, 0.1), 5: (23, "diag", 5023, 0.04), 64: (23, "diag", 64023, 0.02), 96: (23, "iso", 96023, 0.01)}


def _make(kind, d, N, adapt=W, adaptive=True, block_steps=0, seed=xh.SEED, scaling=None, inv_mass=None, theta0=None):
    """-> (make() -> an engine, not initialised; the starts; the oracle level; the twin's proposal)"""
    m, noise, pseed, eps = SHAPES[d]
    y, th0, pm, pv, nz, level = xh.gaussian_problem(d, m, noise, N, seed=pseed)
    eps = eps if scaling is None else scaling
    prop = xn.nuts(eps, 4, adaptive=adaptive, inv_mass=inv_mass, period=PERIOD) if kind == "nuts" else dict(xh.hmc(eps, 4, adaptive, inv_mass), period=PERIOD)

    def make():
        mk = xn.gaussian_engine if kind == "nuts" else xh.gaussian_engine
        e = mk(d, m, noise, N, y, pm, pv, nz, prop, block_steps, seed=seed)
        if adapt is not None:
            e.set_mass_adaptation(adapt)
        return e

    return make, (th0 if theta0 is None else theta0), level, prop


# ---- 6. the mass is the statistic of the device's own records ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,N", [("nuts", 5, 70), ("nuts", 1, 70), ("nuts", 64, 70), ("nuts", 96, 70), ("nuts", 5, 1), ("nuts", 5, 300), ("hmc", 5, 70)])
def test_mass_is_the_statistic_of_the_records(kind, d, N):
    """after each window get_mass() is the twin over the recorded states of that window, within the tolerance of
    tests/test_mass_adaptation.py for the window's shape (and within it of a two-pass variance in np.longdouble); before the first
    window's end, inside a window and after the warm-up the mass does not change; the counters say where the schedule stands"""
    make, theta0, _, _ = _make(kind, d, N)
    e = make()
    try:
        e.init(theta0)
        w, info = e.get_mass()
        assert np.array_equal(w, np.ones(d)) and info == dict(updates=0, window_steps=0, next_update=40, refused=0)
        states, t = np.empty((0, N, d)), 0
        for piece in (20, 20, 20, 20, 80, 20):
            states = np.concatenate([states, e.run_host(piece)[0]])
            t += piece
            now, info = e.get_mass()
            ends = [end for _, end in WINDOWS]
            if t in ends:
                first = WINDOWS[ends.index(t)][0]
                xms.assert_window(states[first:t], now, w, "%s d = %d, window [%d, %d):" % (kind, d, first, t))
                assert not np.array_equal(now, w)
            else:
                assert np.array_equal(now, w), t
            w = now
            later = [end for end in ends if end > t]
            in_window = next((t - a for a, b in WINDOWS if a < t < b), 0)
            assert info == dict(updates=len(ends) - len(later), window_steps=in_window, next_update=later[0] if later else -1, refused=0), (t, info)
        assert np.all(np.isfinite(states)) and np.all(w > 0.0)
        assert e.counters()[0] == 180
    finally:
        e.close()


# ---- 7. the steps after an update use the new mass ----------------------------------------------------------------------------------
SEEDS = (91, 92, 93, 94, 95)  # (the engine's seed: the first whose period the twin admits is compared; chosen on the CPU: 91 for both)


@pytest.mark.parametrize("kind", ["nuts", "hmc"])
def test_steps_after_an_update_use_the_new_mass(kind):
    """fixed step size 0.25 from the mass 0.04 (the scale the first window finds, so that the step size suits both): the period
    after the first update, steps 40 .. 59, from the state at the boundary, on the exported normals and under the inverse mass
    that get_mass() reports, is the twin's -- masks exact, log-posterior 1e-10, states 1e-9 (atol 1e-12), as the forward cases of
    test_gpu_nuts.py / test_gpu_hmc.py are held for this source.  Under the starting mass instead the twin leaves the records"""
    d, N = 5, 13
    tried = []
    for seed in SEEDS:
        make, theta0, level, prop = _make(kind, d, N, adaptive=False, seed=seed, scaling=0.25, inv_mass=0.04 * np.ones(d))
        e = make()
        try:
            e.init(theta0)
            z, u = e.set_export(60)
            head = e.run_host(40)
            w, info = e.get_mass()
            assert info["updates"] == 1 and not np.array_equal(w, prop["inv_mass"])
            params, stats, acc = e.run_host(20)
            totals = e.nuts_totals() if kind == "nuts" else None
        finally:
            e.close()
        start, zt, ut = head[0][-1], np.swapaxes(z[40:], 0, 1), np.swapaxes(u[40:], 0, 1)
        after = dict(prop, inv_mass=w)
        try:
            if kind == "nuts":
                draws = xn.PhiloxDraws(seed, xh.CHAIN_OFFSET, N, step0=40)
                ref, dpost, dstate = xn.assert_admissible(level, after, start, zt, draws)
                xn.assert_within_tolerance("after_a_mass_update", dpost, dstate)
                assert ref["depth"].mean() >= 1.0
            else:
                ref = xh.assert_admissible(level, after, start, zt, ut, state_share=0.1)
        except AssertionError as exc:
            tried.append((seed, str(exc)[:80]))
            continue
        print("seed %d admitted (not admitted: %s); inverse mass %s" % (seed, tried, w))
        xn.compare("after_a_mass_update", params, stats, acc, ref)
        # the twin under the starting mass does not give these records: the comparison above sees the mass
        old = (xn.run_nuts(level, prop, start, zt, xn.PhiloxDraws(seed, xh.CHAIN_OFFSET, N, step0=40)) if kind == "nuts"
               else xh.run_hmc(level, prop, start, zt, ut))
        assert not np.allclose(np.swapaxes(old["theta"][:, 1:], 0, 1), params, rtol=1e-6, atol=1e-9)
        if totals is not None:  # (the totals run since init: the head's trees are in them)
            assert np.all(totals[:, 0] >= ref["totals"][:, 0])
        return
    pytest.fail("no seed of %s gives a period that the twin admits: %s" % (SEEDS, tried))


# ---- 8. what is recorded does not matter --------------------------------------------------------------------------------------------
def test_records_do_not_matter():
    """all parameters recorded into host memory, into device memory, nothing recorded, and thin = 4: bitwise the same mass,
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
            ends.append((e.get_mass(), e.proposal_state_scaling(), e.current()))
        finally:
            e.close()
    (w0, info0), sc0, (th0, st0) = ends[0]
    assert info0["updates"] == 3 and not np.array_equal(w0, np.ones(d))
    for (w, info), sc, (th, stt) in ends[1:]:
        assert np.array_equal(w, w0) and info == info0 and np.array_equal(sc, sc0) and np.array_equal(th, th0) and np.array_equal(stt, st0)


# ---- 9. how a run is split does not matter; checkpoints --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [("nuts", 5), ("nuts", 96), ("hmc", 5)])
def test_split_independence_and_resume(kind, d):
    """160 steps in one run(), as 50 + 110, and as 70 steps, get_state, set_state into a fresh engine, 90 steps (blocks of 16
    steps, so that the cuts fall inside blocks, periods and windows alike): records, mass, step sizes and counters bitwise"""
    N = 11
    make, theta0, _, _ = _make(kind, d, N, block_steps=16)

    def finish(e, recs):
        out = ([np.concatenate(x) for x in zip(*recs)], e.get_mass(), e.proposal_state_scaling(), e.counters())
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
    assert whole[1][1]["updates"] == 3 and whole[3][0] == 160
    for other in (split, resumed):
        assert all(np.array_equal(x, y) for x, y in zip(whole[0], other[0]))
        assert np.array_equal(whole[1][0], other[1][0]) and whole[1][1] == other[1][1]
        assert np.array_equal(whole[2], other[2]) and whole[3] == other[3]


# the length of the checkpoint blob of the NUTS engine below (N = 11, d = 5, extmodel's source, 23 outputs) as the parent commit
# writes it: read from an engine of that commit's library
PARENT_NUTS_BLOB_BYTES = 3852


def test_checkpoint_blob_of_other_engines_is_unchanged():
    """a NUTS engine that does not adapt its mass -- never asked to, or asked with 0 -- has the blob length it had before this
    extension existed; an adapting one has exactly the items of include/tinyda_amd_mass.h more; a blob goes only into an engine
    with the same warm-up length and period"""
    from tinyda_amd import _lib

    d, N = 5, 11
    DP, NP = 8, 16
    sizes = {}
    for name, adapt in (("never", None), ("off", 0), ("on", W)):
        make, theta0, _, _ = _make("nuts", d, N, adapt=adapt)
        e = make()
        try:
            e.init(theta0)
            e.run(30)
            sizes[name] = e.get_state()
        finally:
            e.close()
    assert sizes["never"].size == sizes["off"].size == PARENT_NUTS_BLOB_BYTES
    # W, period (int32), n, updates, inv_mass [DP], mean and M2 [NP][DP], the refused count: each behind its 8-byte length
    extra = (8 + 8) + (8 + 4) + (8 + 8) + (8 + 8) + (8 + 8 * DP) + 2 * (8 + 8 * NP * DP) + (8 + 4)
    assert sizes["on"].size == sizes["never"].size + extra
    for adapt, period, match in ((W - PERIOD, PERIOD, "another mass adaptation"), (W, 40, "another mass adaptation"), (0, PERIOD, "does not match")):
        m, noise, pseed, eps = SHAPES[d]
        y, theta0, pm, pv, nz, _ = xh.gaussian_problem(d, m, noise, N, seed=pseed)
        e = xn.gaussian_engine(d, m, noise, N, y, pm, pv, nz, xn.nuts(eps, 4, adaptive=True, period=period))
        try:
            e.set_mass_adaptation(adapt)
            e.init(theta0)
            with pytest.raises(_lib.EngineError, match=match):
                e.set_state(sizes["on"])
            assert e.counters()[0] == 0 and np.all(np.isfinite(e.run_host(3)[1]))  # (the refused blob left the engine as it was)
        finally:
            e.close()


# ---- 10. a parameter that does not move ----------------------------------------------------------------------------------------------
def test_constant_parameter_gets_the_floor():
    """inverse mass 1e-300 for parameter 2, the same start in all chains: its momentum z / sqrt(w) is finite, its position step
    eps w p vanishes against the position, so the window's variance is exactly zero.  The entry gets the regulariser's floor
    1e-3 * 5 / (n N + 5) and is not refused; the run goes on, the parameter moves from then on, every record is finite"""
    d, N = 5, 70
    w0 = np.ones(d)
    w0[2] = 1e-300
    m, noise, pseed, _ = SHAPES[d]
    theta0 = xh.gaussian_problem(d, m, noise, N, seed=pseed)[1].copy()
    theta0[:, 2] = 0.25
    make, theta0, _, _ = _make("nuts", d, N, inv_mass=w0, theta0=theta0)
    e = make()
    try:
        e.init(theta0)
        params, stats, _ = e.run_host(40)
        w, info = e.get_mass()
        assert np.all(params[:, :, 2] == 0.25) and np.ptp(params[:, :, 0]) > 0.0
        assert info == dict(updates=1, window_steps=0, next_update=80, refused=0)
        assert w[2] == 1e-3 * 5.0 / (20.0 * N + 5.0) and np.all(np.isfinite(w)) and np.all(w > 0.0)
        xms.assert_window(params[20:40][:, :, [0, 1, 3, 4]], w[[0, 1, 3, 4]], w0[[0, 1, 3, 4]], "beside the constant parameter:")
        more, stats2, _ = e.run_host(140)
        assert np.all(np.isfinite(more)) and np.all(np.isfinite(stats)) and np.all(np.isfinite(stats2))
        assert np.ptp(more[:, :, 2]) > 0.0 and e.get_mass()[1] == dict(updates=3, window_steps=0, next_update=-1, refused=0)
    finally:
        e.close()


def test_entry_point_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    from .test_mala_source import ROSEN_SRC

    e = Engine(4, 2, seed=1)
    try:
        e.set_prior(np.zeros(2), np.eye(2))
        e.set_level_source(0, ROSEN_SRC, np.zeros(1), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="TDA_PROP_HMC or TDA_PROP_NUTS must precede set_mass_adaptation"):
            e.set_mass_adaptation(40)
        e.set_proposal(6, None, scaling=0.1, period=20)  # MALA
        with pytest.raises(_lib.EngineError, match="must precede set_mass_adaptation"):
            e.set_mass_adaptation(40)
        for kind, kw in ((xh.PROP_HMC, dict(n_leapfrog=2)), (xn.PROP_NUTS, dict(max_depth=3))):
            e.set_proposal(kind, None, scaling=0.1, period=20, **kw)
            for bad in (30, 20, -40, 50):
                with pytest.raises(_lib.EngineError, match=r"warmup_steps = %d must be a multiple of the period \(20\) and at least two periods" % bad):
                    e.set_mass_adaptation(bad)
            with pytest.raises(_lib.EngineError, match="applies to an initialised HMC or NUTS engine"):
                e.get_mass()
            e.set_mass_adaptation(40)
            e.set_mass_adaptation(0)
            with pytest.raises(_lib.EngineError, match="at least two periods"):
                e.set_proposal(kind, None, scaling=0.1, period=20, adapt_mass=20, **kw)
    finally:
        e.close()
    # an engine that does not adapt reports its mass all the same
    make, theta0, _, _ = _make("hmc", 5, 4, adapt=None, inv_mass=xh.MASS(5))
    e = make()
    try:
        e.init(theta0)
        e.run(25)
        w, info = e.get_mass()
        assert np.array_equal(w, xh.MASS(5)) and info == dict(updates=0, window_steps=0, next_update=-1, refused=0)
    finally:
        e.close()


# ---- 11. end to end ---------------------------------------------------------------------------------------------------------------------
def test_sample_learns_the_scales():
    """sample(backend='hip') on N(0, diag(sd^2)), sd = logspace(-1.5, 1.5, 8), 256 chains, 400 steps of NUTS(adapt_mass=160):
    inv_mass / variance in [0.5, 2] for every parameter (the raw variances span 10^6; the last window pools 80 * 256 states), three
    updates, none refused, and the mean tree depth of the last 100 steps below that of the same call with adapt_mass = 0
    (tests/test_mass_adaptation.py holds the NumPy reference to the same conditions)"""
    import tinyda_amd as tda

    from .test_gpu_mala_source import _linear_source

    cfg = END_TO_END
    sd, N, T = cfg["sd"], cfg["N"], cfg["T"]
    d, pv = sd.shape[0], 1e4
    nv = 1.0 / (1.0 / sd ** 2 - 1.0 / pv)  # under the prior N(0, pv I) the posterior is N(0, diag(sd^2))
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), pv * np.eye(d)), tda.GaussianLogLike(np.zeros(d), np.diag(nv)), tda.DeviceModel(_linear_source(np.eye(d)), d))
    starts = list(sd[None, :] * np.random.default_rng(5).standard_normal((N, d)))
    depth = {}
    for adapt in (cfg["adapt_mass"], 0):
        prop = tda.NUTS(scaling=cfg["scaling"], adaptive=True, period=cfg["period"], adapt_mass=adapt)
        head = tda.sample(post, prop, T - 100, n_chains=N, initial_parameters=starts, seed=21, backend="hip")
        res = tda.sample(post, prop, T, n_chains=N, initial_parameters=starts, seed=21, backend="hip")
        ps, ps_head = res["proposal_state"], head["proposal_state"]
        # (a run is the head of a longer one: the last 100 steps' depths are the difference of the two runs' sums)
        depth[adapt] = float(np.mean(np.asarray(ps["mean_tree_depth"]) * T - np.asarray(ps_head["mean_tree_depth"]) * (T - 100)) / 100.0)
        if adapt:
            assert list(ps)[6:9] == ["inv_mass", "mass_updates", "mass_refused"] and len(ps) == 13
            ratio = np.asarray(ps["inv_mass"]) / sd ** 2
            print("inv_mass / variance:", np.array2string(ratio, precision=3))
            assert ps["inv_mass"].shape == (d,) and np.all(ratio >= 0.5) and np.all(ratio <= 2.0)
            assert ps["mass_updates"] == 3 and ps["mass_refused"] == 0
            assert np.array_equal(ps["inv_mass"], ps_head["inv_mass"])  # frozen after step 160
            import copy
            import pickle

            for other in (copy.deepcopy(ps), pickle.loads(pickle.dumps(ps))):
                assert list(other) == list(ps) and np.array_equal(other["inv_mass"], ps["inv_mass"]) and other["mass_updates"] == 3
        else:
            assert "inv_mass" not in ps and len(ps) == 10
        tail = tda.get_samples(res, burnin=T - 100)
        assert np.all(np.isfinite(np.stack([tail["chain_%d" % i] for i in range(N)])))
    print("mean tree depth of the last 100 steps: %.2f adapted, %.2f unit mass" % (depth[cfg["adapt_mass"]], depth[0]))
    assert depth[cfg["adapt_mass"]] < depth[0]
