"""NUTS over source-defined models on the device (tda_user_nuts_steps): Philox forward mode against the NumPy twin of
tests/extnuts.py over every form of the contract, a model with a NaN region, max_depth = 1 against HMC's leapfrog step, checkpoint
resume, the engine's refusals, and sample(backend='hip') on a closed-form posterior and from the ends of tda.maximize.

The reference has no NUTS, so parity is against the twin, which tests/test_nuts.py ties to HMC's twin, checks against a brute
force and a closed form, and admits case by case (one ulp on every gradient, up or down, leaves every tree as it is) on the
variates the engine draws here: the normals are exported, the tree draws restated from Philox stream 8."""
import numpy as np
import pytest
import scipy.stats as st

from . import exthmc as xh
from . import extnuts as xn
from .extengine import assert_resume_bitwise
from .test_gpu_hmc import _ill_conditioned
from .test_gpu_mala_source import _linear_source

pytestmark = pytest.mark.gpu


def _forward(level, prop, theta0, T, make):
    """-> the engine's outputs and per-chain totals, the twin's trace on the engine's exported normals and its own tree draws"""
    e = make()
    e.init(theta0)
    z, _ = e.set_export(T)
    params, stats, acc = e.run_host(T)
    scal, totals = e.proposal_state_scaling(), e.nuts_totals()
    e.close()
    ref = xn.run_nuts(level, prop, theta0, np.swapaxes(z, 0, 1), xn.PhiloxDraws(xn.SEED, xn.CHAIN_OFFSET, theta0.shape[0]))
    print("trees:", xn.coverage(ref, prop["max_depth"]))
    return params, stats, acc, scal, totals, ref


@pytest.mark.parametrize("case", list(xn.FORWARD_CASES))
def test_philox_forward_matches_twin(case):
    """masks exact, log-posterior 1e-10, states 1e-9 (atol 1e-12), the per-chain totals exact, the final step size 1e-12.
    d96_m23_depth4_iso_adaptive: log-posterior 1.6e-10, ten times what one ulp on every gradient moves in the twin
    (extnuts.TOLERANCE; the log-posterior passes close to zero under that case's tight prior)"""
    level, prop, theta0, T, make = xn.forward_case(case)
    params, stats, acc, scal, totals, ref = _forward(level, prop, theta0, T, make)
    assert np.array_equal(totals, ref["totals"])
    xn.compare(case, params, stats, acc, ref, scal)
    assert np.all(np.isfinite(stats))


@pytest.mark.parametrize("case", list(xn.CONTRACT_STEP))
def test_contract_forms_match_twin(case):
    """the wave forms of the model and its gradient, a separable and a coupled DeviceLogLike, a separable DevicePrior at the edge
    of its support and a coupled one, at max_depth = 4: the same comparison"""
    level, prop, theta0, T, make = xn.contract_case(case)
    params, stats, acc, scal, totals, ref = _forward(level, prop, theta0, T, make)
    if case == "lognormal_prior_at_the_edge":  # trees left the support, and no state did
        assert np.sum(ref["left"]) >= 5 and np.all(params > 0.0)
    assert np.array_equal(totals, ref["totals"])
    xn.compare(case, params, stats, acc, ref, scal)
    assert np.all(np.isfinite(stats))


def test_nan_region_makes_divergent_trees():
    level, prop, theta0, T, thr, make = xn.nan_case()
    params, stats, acc, scal, totals, ref = _forward(level, prop, theta0, T, make)
    assert ref["totals"][:, 1].sum() >= 5 and np.sum(ref["left"]) >= 5
    assert np.array_equal(totals[:, 1], ref["totals"][:, 1]) and np.array_equal(totals, ref["totals"])
    assert np.all(np.isfinite(stats)) and np.all(params[:, :, 0] <= thr)
    xn.compare("nan_region", params, stats, acc, ref, scal)


@pytest.mark.parametrize("d,scaling", [(5, 0.08), (96, 0.03)])
def test_max_depth_one_is_one_leapfrog_step(d, scaling):
    """max_depth = 1 on the device: every state is the state before it, or the end of one leapfrog step of HMC's twin from it
    under the step's exported normals, forward or backward; all three happen"""
    m, noise, N, T = 23, "diag" if d == 5 else "iso", 13, 120
    y, theta0, pm, pv, nz, level = xh.gaussian_problem(d, m, noise, N, seed=d * 1000 + m)
    prop = xn.nuts(scaling, 1, inv_mass=xh.MASS(d))
    e = xn.gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop)
    e.init(theta0)
    z, _ = e.set_export(T)
    params, stats, acc = e.run_host(T)
    totals = e.nuts_totals()
    e.close()
    assert np.all(totals[:, 0] == T) and np.all(totals[:, 3] + totals[:, 1] == T)  # one leaf per step; depth 1 unless it diverged
    w, eps = prop["inv_mass"], np.full(N, scaling)
    kinds = np.zeros(3, dtype=int)
    cur = theta0
    for s in range(T):
        _, _, F = level.evaluate(cur)
        g = level.grad_logpost(cur, F)
        p0 = z[s] / np.sqrt(w)
        fw = xh.leapfrog(level, cur, p0, g, eps, w, 1)[0]
        bw = xh.leapfrog(level, cur, -p0, g, eps, w, 1)[0]
        nxt = params[s]
        close = lambda a: np.all(np.abs(nxt - a) <= 1e-12 + 1e-9 * np.abs(a), axis=1)  # noqa: E731
        stay, f, b = np.all(nxt == cur, axis=1), close(fw), close(bw)
        assert np.all(stay | f | b), (s, np.flatnonzero(~(stay | f | b)))
        assert np.array_equal(acc[s].astype(bool), ~stay)
        kinds += [stay.sum(), (f & ~stay).sum(), (b & ~stay).sum()]
        cur = nxt
    print("stayed %d, forward %d, backward %d" % tuple(kinds))
    assert np.all(kinds >= 10)


@pytest.mark.parametrize("d", [5, 96])
def test_checkpoint_resume_is_bitwise(d):
    """get_state in the middle of a period (step 37 of periods of 20), set_state into a fresh engine configured by the same
    set_nuts call: records bitwise, and with them the totals and the adapted step size, which the period's acceptance sum feeds"""
    m, noise, N = 23, "diag", 11
    y, theta0, pm, pv, nz, _ = xh.gaussian_problem(d, m, noise, N, seed=7 + d)
    prop = xn.nuts(0.02, 4, adaptive=True, inv_mass=xh.MASS(d))
    ends = []

    def make():
        e = xn.gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop, block_steps=16)
        e.init(theta0)
        close = e.close

        def close_and_keep():
            ends.append((e.nuts_totals(), e.proposal_state_scaling()))
            close()

        e.close = close_and_keep
        return e

    assert_resume_bitwise(make)
    (tot_full, sc_full), (tot_same, sc_same), (tot_resumed, sc_resumed) = ends
    assert np.array_equal(tot_full, tot_same) and np.array_equal(sc_full, sc_same)
    assert np.array_equal(tot_full, tot_resumed) and np.array_equal(sc_full, sc_resumed)
    assert np.all(tot_full[:, 0] >= 90) and not np.all(sc_full == 0.02)


def test_engine_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    from . import extwave as xw
    from .test_mala_source import FORWARD_ONLY_SRC, ROSEN_SRC

    e = Engine(4, 2, seed=1)
    try:
        e.set_prior(np.zeros(2), np.eye(2))
        e.set_level_source(0, ROSEN_SRC, np.zeros(1), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="TDA_PROP_NUTS must precede set_nuts"):
            e.set_nuts(4)
        e.set_proposal(xh.PROP_HMC, None, scaling=0.1)
        with pytest.raises(_lib.EngineError, match="TDA_PROP_NUTS must precede set_nuts"):
            e.set_nuts(4)
        e.set_proposal(xn.PROP_NUTS, None, scaling=0.1)
        with pytest.raises(_lib.EngineError, match="max_depth = 0 outside 1 .. 10"):
            e.set_nuts(0)
        with pytest.raises(_lib.EngineError, match="max_depth = 11 outside 1 .. 10"):
            e.set_nuts(11)
        with pytest.raises(_lib.EngineError, match="target_accept = 1 outside"):
            e.set_nuts(4, 1.0)
        with pytest.raises(_lib.EngineError, match=r"inv_mass\[1\] = -2"):
            e.set_nuts(4, 0.8, [1.0, -2.0])
        with pytest.raises(_lib.EngineError, match=r"inv_mass\[0\] = (inf|nan)"):
            e.set_nuts(4, 0.8, [np.inf, 1.0])
        with pytest.raises(_lib.EngineError, match="applies to an initialised NUTS engine"):
            e.nuts_totals()
        # a source without tda_gradient: the compile's own message, with the signature
        e.set_level_source(0, FORWARD_ONLY_SRC, np.zeros(1), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="NUTS needs what MALA needs -- .*defines no __device__ double tda_gradient"):
            e.init(np.zeros((4, 2)))
        # HMC's preconditions over a source-defined model, worded with NUTS
        e.set_level_source(0, ROSEN_SRC, np.zeros(2049), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="NUTS over a source-defined model: at most 2048 outputs"):
            e.init(np.zeros((4, 2)))
        e.set_level_source(0, ROSEN_SRC, np.zeros(2), 2, np.eye(2))
        with pytest.raises(_lib.EngineError, match="NUTS over a source-defined model: isotropic or diagonal noise"):
            e.init(np.zeros((4, 2)))
    finally:
        e.close()
    # the engine's own linear model has no NUTS
    e = Engine(4, 2, seed=1)
    try:
        e.set_prior(np.zeros(2), np.eye(2))
        e.set_level(0, np.eye(2), np.zeros(2), 0, 1.0)
        e.set_proposal(xn.PROP_NUTS, None, scaling=0.1)
        with pytest.raises(_lib.EngineError, match="NUTS is lowered for source-defined forward models"):
            e.init(np.zeros((4, 2)))
    finally:
        e.close()
    # a workspace that leaves no room for the checkpoints: refused with the byte counts (the ring alone fits, and runs under HMC)
    d, m, N = 5, 24, 4
    _, y, theta0 = xw.problem(d, m, N, seed=524, sigma=0.01)
    src = xw.source("wave", "wave")
    big = "#define TDA_WORKSPACE 7800\n" + "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("#define TDA_WORKSPACE"))
    assert "TDA_WORKSPACE" in src
    for proposal, refused in ((lambda e: e.set_proposal(xh.PROP_HMC, None, scaling=0.05, n_leapfrog=2), False),
                              (lambda e: e.set_proposal(xn.PROP_NUTS, None, scaling=0.05, max_depth=10), True),
                              (lambda e: e.set_proposal(xn.PROP_NUTS, None, scaling=0.05, max_depth=1), False)):
        e = Engine(N, d, seed=1)
        try:
            e.set_prior(np.zeros(d), np.eye(d))
            e.set_level_source(0, big, y, 0, [1e-4])
            proposal(e)
            if refused:  # 5 parameters are padded to 8: 2 * 10 * 8 doubles of checkpoints
                with pytest.raises(_lib.EngineError, match=r"NUTS over a source-defined model holds at most 64 KiB of LDS per chain: this source needs \d+ bytes "
                                                           r".* \+ 192 bytes for its 24 outputs \+ 1280 bytes for the checkpoints of max_depth = 10 over 8 padded parameters"):
                    e.init(theta0)
            else:
                e.init(theta0)
                assert np.all(np.isfinite(e.run_host(3)[1]))
        finally:
            e.close()


def test_sample_api_ill_conditioned_gaussian_posterior():
    """sample(backend='hip') over a linear DeviceModel with condition number 100, 4096 chains, adaptive: pooled mean and covariance
    after burn-in within the bounds of test_gpu_hmc's test of the same posterior; the trees neither all trivial nor all at the
    cap, none divergent, and the last period's mean acceptance statistic within 0.1 of the target 0.8"""
    import tinyda_amd as tda

    d, m, N, T, burn = 8, 16, 4096, 400, 200
    A, y, nv, mean, cov = _ill_conditioned(d, m, seed=13)
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(y, nv * np.eye(m)), tda.DeviceModel(_linear_source(A), m))
    nuts = tda.NUTS(scaling=0.1, adaptive=True, period=50)
    res = tda.sample(post, nuts, T, n_chains=N, initial_parameters=None, seed=12, backend="hip")
    assert res["sampler"] == "MH" and res["n_chains"] == N and res["backend"] == "hip"
    ps = res["proposal_state"]
    assert {"scaling", "n_leapfrog", "n_divergent", "n_max_depth", "mean_tree_depth"} <= set(ps)
    depth, scal = np.asarray(ps["mean_tree_depth"]), np.asarray(ps["scaling"])
    print("mean tree depth %.2f, leapfrog steps per step %.1f, trees at max_depth %d, step size of chain 0 %.4f"
          % (depth.mean(), np.mean(ps["n_leapfrog"]) / T, np.sum(ps["n_max_depth"]), scal[0]))
    assert depth.shape == (N,) and np.all(depth > 1.0) and np.all(depth < nuts.max_depth)
    assert np.sum(ps["n_divergent"]) == 0
    # the adaptation's own arithmetic gives the last period's mean statistic back: the last update was the k = T / period - 1 th,
    # log(scaling after / before) = gamma^-k (rate - 0.8).  `before` is what a run one period shorter ends with; chains do not
    # interact and draw by their global id, so the first 256 of them stand for themselves
    n0 = 256
    res0 = tda.sample(post, tda.NUTS(scaling=0.1, adaptive=True, period=50), T - 50, n_chains=n0, initial_parameters=None, seed=12, backend="hip")
    before = np.asarray(res0["proposal_state"]["scaling"])
    rate = 0.8 + np.log(scal[:n0] / before) * 1.01 ** (T // 50 - 1)
    assert np.all(rate > 0.0) and np.all(rate <= 1.0 + 1e-9)  # (a statistic: the shorter run is the head of the longer one)
    print("mean acceptance statistic of the last period %.3f" % rate.mean())
    assert abs(rate.mean() - 0.8) < 0.1
    s = tda.get_samples(res, burnin=burn)
    X = np.stack([s["chain_%d" % i] for i in range(N)])
    cm = X.mean(axis=1)
    se = cm.std(axis=0, ddof=1) / np.sqrt(N)
    pooled = X.reshape(-1, d)
    assert np.all(np.abs(pooled.mean(axis=0) - mean) < 5 * se + 1e-12), (pooled.mean(axis=0), mean, se)
    C = np.cov(pooled.T)
    np.testing.assert_allclose(C, cov, atol=0.05 * np.sqrt(np.outer(np.diag(cov), np.diag(cov))).max())


def test_sample_from_the_ends_of_maximize():
    """maximize -> sample(initial_parameters=res.x) under NUTS, thinned records and the lazy proposal state included"""
    import tinyda_amd as tda

    from . import extmodel as xm

    d, m, N = 5, 23, 64
    y, _, pm, pv, nz, _ = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, np.diag(nz)), tda.DeviceModel(xm.source(), m))
    starts = list(tda.maximize(post, n_starts=N, seed=1).x)
    res = tda.sample(post, tda.NUTS(0.04, max_depth=5, inv_mass=xh.MASS(d), adaptive=True, period=20), 100, n_chains=N,
                     initial_parameters=starts, seed=3, backend="hip", thin=2)
    assert res["backend"] == "hip" and res["n_chains"] == N and res["iterations"] == 51
    s = tda.get_samples(res)
    X = np.stack([s["chain_%d" % i] for i in range(N)])
    assert X.shape == (N, 51, d) and np.all(np.isfinite(X))
    np.testing.assert_array_equal(X[:, 0], np.stack(starts))
    ps = res["proposal_state"]
    assert list(ps)[-4:] == ["n_leapfrog", "n_divergent", "n_max_depth", "mean_tree_depth"] and len(ps) == 10
    scal = np.asarray(ps["scaling"])
    assert scal.shape == (N,) and np.all(np.isfinite(scal)) and np.all(scal > 0.0) and not np.all(scal == 0.04)
    for key in ("n_leapfrog", "n_divergent", "n_max_depth", "mean_tree_depth"):
        assert np.asarray(ps[key]).shape == (N,)
    assert np.all(ps["n_leapfrog"] >= 100) and np.all(ps["mean_tree_depth"] >= 1.0) and np.all(ps["mean_tree_depth"] <= 5.0)
    assert np.all(ps["n_leapfrog"] <= 100 * 31) and np.all(ps["n_max_depth"] + ps["n_divergent"] <= 100)
    assert len({tuple(r) for r in X[0]}) > 25  # (the chain moved)
