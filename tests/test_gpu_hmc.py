"""HMC over source-defined models on the device (tda_user_hmc_steps): Philox forward mode against the NumPy twin of
tests/exthmc.py over every form of the contract, one leapfrog step against MALA on the device, a model with a NaN region,
checkpoint resume, and sample(backend='hip') on a closed-form posterior and from the ends of tda.maximize.

The reference has no HMC, so parity is against the twin, which tests/test_hmc.py ties to the oracle's MALA and admits case by
case (one ulp on every gradient moves no mask; acceptance in [0.1, 0.9]) on the variates the engine draws here."""
import numpy as np
import pytest
import scipy.stats as st

from . import exthmc as xh
from .extengine import assert_rate, assert_resume_bitwise, compare, run_forward
from .test_gpu_mala_source import _linear_source

pytestmark = pytest.mark.gpu


def _forward(level, prop, theta0, T, make):
    """-> the engine's outputs, the twin's trace on the engine's exported variates"""
    params, stats, acc, scal, _, z, u = run_forward(make(), theta0, T, prop)
    ref = xh.run_hmc(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    return params, stats, acc, scal, ref


@pytest.mark.parametrize("case", list(xh.FORWARD_CASES))
def test_philox_forward_matches_twin(case):
    """masks exact, log-posterior 1e-10, states 1e-9 (atol 1e-12), final step size 1e-12"""
    level, prop, theta0, T, make = xh.forward_case(case)
    params, stats, acc, scal, ref = _forward(level, prop, theta0, T, make)
    compare(params, stats, acc, ref, scal)
    assert np.all(np.isfinite(stats))


@pytest.mark.parametrize("case", list(xh.CONTRACT_CASES))
def test_contract_forms_match_twin(case):
    """the wave forms of the model and its gradient, a separable and a coupled DeviceLogLike, a separable DevicePrior with a
    support and a coupled one: the same comparison"""
    level, prop, theta0, T, make = xh.contract_case(case)
    params, stats, acc, scal, ref = _forward(level, prop, theta0, T, make)
    if case == "lognormal_prior_at_the_edge":  # trajectories left the support at an interior leapfrog step, and were rejected
        inside = (ref["ended"] > 0) & (ref["ended"] < prop["n_leapfrog"])
        print("trajectories that left the support at an interior leapfrog step: %d" % inside.sum())
        assert inside.sum() >= 10 and not np.any(ref["accepted"][:, 1:][ref["ended"] > 0])
        assert np.all(params > 0.0)
    compare(params, stats, acc, ref, scal)
    assert np.all(np.isfinite(stats))


@pytest.mark.parametrize("d,scaling", [(5, 0.06), (96, 0.02)])
def test_one_leapfrog_step_is_mala_on_the_device(d, scaling):
    """the same engine under TDA_PROP_MALA and under HMC with n_leapfrog = 1, same seed: masks equal, log-posterior 1e-9"""
    m, noise, N, T = 23, "diag" if d == 5 else "iso", 13, 120
    y, theta0, pm, pv, nz, _ = xh.gaussian_problem(d, m, noise, N, seed=d * 1000 + m)
    out = []
    for prop in (dict(kind="mala", scaling=scaling), xh.hmc(scaling, 1)):
        e = xh.gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop)
        e.init(theta0)
        out.append(e.run_host(T))
        e.close()
    (_, stats_m, acc_m), (_, stats_h, acc_h) = out
    assert 0.1 <= acc_m.mean() <= 0.9
    assert np.array_equal(acc_m, acc_h)
    np.testing.assert_allclose(stats_h[:, :, 2], stats_m[:, :, 2], rtol=1e-9)


def test_nan_region_ends_the_trajectory():
    level, free, prop, theta0, T, thr, make = xh.nan_case()
    params, stats, acc, _, _, z, u = run_forward(make(), theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = xh.run_hmc(level, prop, theta0, zz, uu)
    print("trajectories that entered the NaN region: %d of %d" % (np.count_nonzero(ref["ended"]), ref["ended"].size))
    assert np.array_equal(acc, np.swapaxes(ref["accepted"][:, 1:], 0, 1))
    np.testing.assert_allclose(stats[:, :, 2], np.swapaxes(ref["logpost"][:, 1:], 0, 1), rtol=1e-10)
    assert np.all(np.isfinite(stats)) and np.all(params[:, :, 0] <= thr)
    # trajectories into the NaN region happened (and were rejected): without it the same variates give another trace
    assert np.count_nonzero(ref["ended"]) >= 1
    assert not np.array_equal(xh.run_hmc(free, prop, theta0, zz, uu)["accepted"], ref["accepted"])


@pytest.mark.parametrize("d", [5, 96])
def test_checkpoint_resume_is_bitwise(d):
    """get_state mid period (the chain state is MALA's: the gradient at the current states travels in the blob), set_state into a
    fresh engine configured by the same set_hmc call"""
    m, noise, N = 23, "diag", 11
    y, theta0, pm, pv, nz, _ = xh.gaussian_problem(d, m, noise, N, seed=7 + d)
    prop = xh.hmc(0.02, 3, adaptive=True, inv_mass=xh.MASS(d))

    def make():
        e = xh.gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop, block_steps=16)
        e.init(theta0)
        return e

    assert_resume_bitwise(make)


def test_engine_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    from .test_mala_source import FORWARD_ONLY_SRC, ROSEN_SRC

    e = Engine(4, 2, seed=1)
    try:
        e.set_prior(np.zeros(2), np.eye(2))
        e.set_level_source(0, ROSEN_SRC, np.zeros(1), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="TDA_PROP_HMC must precede set_hmc"):
            e.set_hmc(4)
        e.set_proposal(6, None, scaling=0.1)
        with pytest.raises(_lib.EngineError, match="TDA_PROP_HMC must precede set_hmc"):
            e.set_hmc(4)
        e.set_proposal(xh.PROP_HMC, None, scaling=0.1)
        with pytest.raises(_lib.EngineError, match="n_leapfrog = 0"):
            e.set_hmc(0)
        with pytest.raises(_lib.EngineError, match="n_leapfrog = 1025"):
            e.set_hmc(1025)
        with pytest.raises(_lib.EngineError, match=r"inv_mass\[1\] = -2"):
            e.set_hmc(4, [1.0, -2.0])
        with pytest.raises(_lib.EngineError, match=r"inv_mass\[0\] = (inf|nan)"):
            e.set_hmc(4, [np.inf, 1.0])
        # a source without tda_gradient: the compile's own message, with the signature
        e.set_level_source(0, FORWARD_ONLY_SRC, np.zeros(1), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="HMC needs what MALA needs -- .*defines no __device__ double tda_gradient"):
            e.init(np.zeros((4, 2)))
        # MALA's preconditions over a source-defined model, worded with HMC
        e.set_level_source(0, ROSEN_SRC, np.zeros(2049), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="HMC over a source-defined model: at most 2048 outputs"):
            e.init(np.zeros((4, 2)))
        e.set_level_source(0, ROSEN_SRC, np.zeros(2), 2, np.eye(2))
        with pytest.raises(_lib.EngineError, match="HMC over a source-defined model: isotropic or diagonal noise"):
            e.init(np.zeros((4, 2)))
    finally:
        e.close()
    # the engine's own linear model has no HMC
    e = Engine(4, 2, seed=1)
    try:
        e.set_prior(np.zeros(2), np.eye(2))
        e.set_level(0, np.eye(2), np.zeros(2), 0, 1.0)
        e.set_proposal(xh.PROP_HMC, None, scaling=0.1)
        with pytest.raises(_lib.EngineError, match="HMC is lowered for source-defined forward models"):
            e.init(np.zeros((4, 2)))
    finally:
        e.close()


def _ill_conditioned(d, m, seed):
    """a linear-Gaussian posterior whose precision has the eigenvalues 1 .. 100 (N(0, I) prior): A, the data, the noise variance,
    the posterior's mean and covariance"""
    rng = np.random.default_rng(seed)
    V = np.linalg.qr(rng.standard_normal((d, d)))[0]
    U = np.linalg.qr(rng.standard_normal((m, d)))[0]
    lam, nv = np.logspace(0.0, 2.0, d), 0.25
    A = U @ np.diag(np.sqrt(nv * (lam - 1.0))) @ V.T
    y = A @ rng.standard_normal(d) + np.sqrt(nv) * rng.standard_normal(m)
    cov = np.linalg.inv(np.eye(d) + A.T @ A / nv)
    return A, y, nv, cov @ (A.T @ y / nv), cov


def test_sample_api_ill_conditioned_gaussian_posterior():
    """sample(backend='hip') over a linear DeviceModel, 4096 chains: pooled mean and covariance after burn-in against the
    closed-form posterior (condition number 100), to the tolerances of test_gpu_mala_source's test of the same kind"""
    import tinyda_amd as tda

    d, m, N, T, burn = 8, 16, 4096, 400, 200
    A, y, nv, mean, cov = _ill_conditioned(d, m, seed=13)
    assert 99.0 < np.linalg.cond(cov) < 101.0
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(y, nv * np.eye(m)), tda.DeviceModel(_linear_source(A), m))
    res = tda.sample(post, tda.HMC(scaling=0.1, n_leapfrog=8, adaptive=True, period=50), T, n_chains=N, initial_parameters=None, seed=12, backend="hip")
    assert res["sampler"] == "MH" and res["n_chains"] == N and res["backend"] == "hip"
    s = tda.get_samples(res, burnin=burn)
    X = np.stack([s["chain_%d" % i] for i in range(N)])  # [N, T - burn + 1, d]
    acc = np.mean([np.mean(res["chain_%d" % i].accepted[burn:]) for i in range(0, N, 64)])
    print("acceptance after burn-in %.3f, step size of chain 0 %.4f" % (acc, res["proposal_state"]["scaling"][0]))
    assert 0.3 < acc < 0.95
    # Monte Carlo error of the pooled moments from the spread of per-chain means (autocorrelation included)
    cm = X.mean(axis=1)
    se = cm.std(axis=0, ddof=1) / np.sqrt(N)
    pooled = X.reshape(-1, d)
    assert np.all(np.abs(pooled.mean(axis=0) - mean) < 5 * se + 1e-12), (pooled.mean(axis=0), mean, se)
    C = np.cov(pooled.T)
    np.testing.assert_allclose(C, cov, atol=0.05 * np.sqrt(np.outer(np.diag(cov), np.diag(cov))).max())


def test_sample_from_the_ends_of_maximize():
    """maximize -> sample(initial_parameters=res.x) under HMC, thinned records and the lazy proposal state included"""
    import tinyda_amd as tda

    from . import extmodel as xm

    d, m, N = 5, 23, 64
    y, _, pm, pv, nz, _ = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, np.diag(nz)), tda.DeviceModel(xm.source(), m))
    starts = list(tda.maximize(post, n_starts=N, seed=1).x)
    res = tda.sample(post, tda.HMC(0.04, n_leapfrog=4, inv_mass=xh.MASS(d), adaptive=True, period=20), 100, n_chains=N,
                     initial_parameters=starts, seed=3, backend="hip", thin=2)
    assert res["backend"] == "hip" and res["n_chains"] == N and res["iterations"] == 51
    s = tda.get_samples(res)
    X = np.stack([s["chain_%d" % i] for i in range(N)])
    assert X.shape == (N, 51, d) and np.all(np.isfinite(X))
    np.testing.assert_array_equal(X[:, 0], np.stack(starts))
    scal = np.asarray(res["proposal_state"]["scaling"])
    assert scal.shape == (N,) and np.all(np.isfinite(scal)) and np.all(scal > 0.0) and not np.all(scal == 0.04)
    assert len({tuple(r) for r in X[0]}) > 5  # (the chain moved)
