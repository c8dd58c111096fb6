"""MALA over source-defined forward models on the device (tda_user_mala_steps): the reference's chain replayed through
set_replay (g17, the MALA Rosenbrock example), Philox forward mode against the oracle with the same model and gradient
as NumPy callables, checkpoint resume, a model with a NaN region, and sample(backend='hip' / 'auto')."""
import warnings

import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from .extengine import assert_resume_bitwise, compare, compare_replay, run_forward
from .extmodel import GradLevel, np_forward, source  # the model, its NumPy twin and MALA gradient (tests/extmodel.py)
from .test_mala_source import FORWARD_ONLY_SRC, ROSEN_SRC

pytestmark = pytest.mark.gpu


def _src(nan_above=None):
    return source(nan_above)


def test_engine_replays_reference_chain(golden):
    from tinyda_amd.engine import Engine

    g = golden("g17_mala_rosenbrock")
    N, T1, d = g["theta"].shape
    e = Engine(N, d, seed=1)
    e.set_prior(g["prior_mean"], g["prior_cov"])
    e.set_level_source(0, ROSEN_SRC, g["data"], 0, [float(g["noise_var"])])
    e.set_proposal(6, None, scaling=float(g["scaling0"]), adaptive=bool(g["adaptive"]), gamma=float(g["gamma"]), period=int(g["period"]))
    e.init(g["theta0"])
    e.set_replay(np.swapaxes(g["z"], 0, 1), np.swapaxes(g["u"], 0, 1))
    params, stats, acc = e.run_host(T1 - 1)
    scal = e.proposal_state_scaling()
    e.close()
    compare_replay(params, stats, acc, g, scaling=scal, params_rtol=1e-10)


# (the scalings keep the drift theta -> theta + s^2/2 grad contractive: with s^2/2 times the posterior's curvature above 1
# it amplifies the last-bit differences of two correct implementations step by step, and no tolerance holds)
CASES = {  # d, m, noise, adaptive, scaling, block_steps
    "d1_m1_iso_fixed": (1, 1, "iso", False, 0.25, 0),
    "d5_m23_diag_fixed_split": (5, 23, "diag", False, 0.06, 33),
    "d5_m300_iso_adaptive": (5, 300, "iso", True, 0.01, 0),
    "d96_m300_diag_adaptive_split": (96, 300, "diag", True, 0.006, 16),
    "d96_m23_iso_fixed": (96, 23, "iso", False, 0.02, 0),
}


def _problem(d, m, noise, N, seed, nan_above=None):
    rng = np.random.default_rng(seed)
    truth = 0.3 * rng.standard_normal(d)
    sd = 0.05 if (d, m) == (5, 23) else 0.1
    y = np_forward(truth, m)[0] + sd * rng.standard_normal(m)
    theta0 = truth + 0.01 * rng.standard_normal((N, d))
    pm, pv = 0.1 * np.ones(d), 0.5 + 0.01 * np.arange(d)
    nz = sd ** 2 if noise == "iso" else sd ** 2 * (1.0 + 0.1 * np.arange(m) / m)
    level = GradLevel(lambda t: np_forward(t, m, nan_above), y, noise, nz, orc.MVNPrior(pm, np.diag(pv)))
    return y, theta0, pm, pv, nz, level


def _engine(d, m, noise, N, y, pm, pv, nz, scaling, adaptive, block_steps, seed=91, nan_above=None):
    from tinyda_amd.engine import Engine

    e = Engine(N, d, seed=seed, chain_offset=3, block_steps=block_steps)
    e.set_prior(pm, np.diag(pv))
    e.set_level_source(0, _src(nan_above), y, 0 if noise == "iso" else 1, np.atleast_1d(nz))
    e.set_proposal(6, None, scaling=scaling, adaptive=adaptive, gamma=1.01, period=20)
    return e


@pytest.mark.parametrize("case", list(CASES))
def test_philox_forward_matches_oracle(case):
    d, m, noise, adaptive, scaling, bs = CASES[case]
    N, T = 13, 120
    y, theta0, pm, pv, nz, level = _problem(d, m, noise, N, seed=d * 1000 + m)
    prop = dict(kind="mala", scaling=scaling, adaptive=adaptive, gamma=1.01, period=20)
    params, stats, acc, scal, _, z, u = run_forward(_engine(d, m, noise, N, y, pm, pv, nz, scaling, adaptive, bs), theta0, T, prop)
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    compare(params, stats, acc, ref, scal)
    assert 0.05 < acc.mean() < 0.98


@pytest.mark.parametrize("d", [5, 96])
def test_checkpoint_resume_is_bitwise(d):
    """get_state mid period (the gradient at the current states travels in the blob), set_state into a fresh engine"""
    m, noise, N = 23, "diag", 11
    y, theta0, pm, pv, nz, _ = _problem(d, m, noise, N, seed=7 + d)

    def make():
        e = _engine(d, m, noise, N, y, pm, pv, nz, 0.02, True, 16)
        e.init(theta0)
        return e

    assert_resume_bitwise(make)


def test_nan_region_is_rejected():
    d, m, noise, N, T = 5, 23, "diag", 13, 120
    y, theta0, pm, pv, nz, free = _problem(d, m, noise, N, seed=5023)
    thr = float(np.max(theta0[:, 0])) + 0.005
    level = GradLevel(lambda t: np_forward(t, m, thr), y, noise, nz, orc.MVNPrior(pm, np.diag(pv)))
    e = _engine(d, m, noise, N, y, pm, pv, nz, 0.02, True, 0, nan_above=thr)
    e.init(theta0)
    z, u = e.set_export(T)
    params, stats, acc = e.run_host(T)
    e.close()
    ref = orc.run_mh(level, dict(kind="mala", scaling=0.02, adaptive=True, gamma=1.01, period=20), theta0,
                     np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert np.array_equal(acc, np.swapaxes(ref["accepted"][:, 1:], 0, 1))
    np.testing.assert_allclose(stats[:, :, 2], np.swapaxes(ref["logpost"][:, 1:], 0, 1), rtol=1e-10)
    assert np.all(np.isfinite(stats)) and np.all(params[:, :, 0] <= thr)
    # proposals into the NaN region were made (and rejected): without it the same variates give another trace
    ref_free = orc.run_mh(free, dict(kind="mala", scaling=0.02, adaptive=True, gamma=1.01, period=20), theta0,
                          np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert not np.array_equal(ref_free["accepted"], ref["accepted"])


def _linear_source(A):
    m, d = A.shape
    vals = ", ".join("%.17g" % v for v in A.ravel())
    return r"""
__device__ const double A_[%d] = {%s};
__device__ double tda_forward(const double* theta, int dim, int o) {
  double s = 0.0;
  for (int j = 0; j < dim; ++j) s += A_[o * dim + j] * theta[j];
  return s;
}
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int m, int j) {
  double g = 0.0;
  for (int o = 0; o < m; ++o) g += A_[o * dim + j] * sens[o];
  return g;
}
""" % (m * d, vals)


def test_sample_api_linear_gaussian_posterior():
    """sample(backend='hip') over a linear DeviceModel, 4096 chains: pooled mean and covariance after burn-in against the
    closed-form posterior"""
    import tinyda_amd as tda

    d, m, N, T, burn = 3, 8, 4096, 600, 200
    rng = np.random.default_rng(11)
    A = rng.standard_normal((m, d)) / np.sqrt(d)
    pm, pv = np.array([0.2, -0.1, 0.0]), np.array([1.0, 0.5, 2.0])
    nv = 0.3 ** 2 * (1.0 + 0.2 * np.arange(m))
    y = A @ rng.standard_normal(d) + np.sqrt(nv) * rng.standard_normal(m)
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, np.diag(nv)),
                         tda.DeviceModel(_linear_source(A), m))
    P = np.linalg.inv(np.diag(pv)) + A.T @ np.diag(1.0 / nv) @ A
    cov = np.linalg.inv(P)
    mean = cov @ (pm / pv + A.T @ (y / nv))
    res = tda.sample(post, tda.MALA(scaling=0.3, adaptive=True, period=50), T, n_chains=N, initial_parameters=None, seed=12,
                     backend="hip")
    assert res["sampler"] == "MH" and res["n_chains"] == N
    s = tda.get_samples(res, burnin=burn)
    X = np.stack([s["chain_%d" % i] for i in range(N)])  # [N, T - burn + 1, d]
    acc = np.mean([np.mean(res["chain_%d" % i].accepted[burn:]) for i in range(0, N, 64)])
    assert 0.3 < acc < 0.9
    # Monte Carlo error of the pooled moments from the spread of per-chain means (autocorrelation included)
    cm = X.mean(axis=1)
    se = cm.std(axis=0, ddof=1) / np.sqrt(N)
    pooled = X.reshape(-1, d)
    assert np.all(np.abs(pooled.mean(axis=0) - mean) < 5 * se + 1e-12), (pooled.mean(axis=0), mean, se)
    C = np.cov(pooled.T)
    np.testing.assert_allclose(C, cov, atol=0.05 * np.sqrt(np.outer(np.diag(cov), np.diag(cov))).max())


def test_source_without_gradient():
    import tinyda_amd as tda
    from tinyda_amd.api import HostFallbackWarning

    post = tda.Posterior(st.multivariate_normal(np.zeros(2), np.eye(2)), tda.GaussianLogLike(np.zeros(1), np.eye(1)),
                         tda.DeviceModel(FORWARD_ONLY_SRC, 1, reference=lambda t: np.array([t[0]])))
    with pytest.raises(Exception, match="tda_gradient"):
        tda.sample(post, tda.MALA(0.1), 20, n_chains=2, seed=1, backend="hip")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.MALA(0.1), 20, n_chains=2, seed=1, backend="auto", force_sequential=True)
    fb = [x for x in w if issubclass(x.category, HostFallbackWarning)]
    assert len(fb) == 1 and "tda_gradient" in str(fb[0].message)
    assert res["n_chains"] == 2 and len(res["chain_0"]) == 21
    # the engine itself refuses such a source for MALA with a message naming the missing function
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    e = Engine(4, 2, seed=1)
    e.set_prior(np.zeros(2), np.eye(2))
    e.set_level_source(0, FORWARD_ONLY_SRC, np.zeros(1), 0, [1.0])
    e.set_proposal(6, None, scaling=0.1)
    with pytest.raises(_lib.EngineError, match="defines no __device__ double tda_gradient"):
        e.init(np.zeros((4, 2)))
    e.close()


def test_engine_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    def attempt(setup):
        e = Engine(4, 2, seed=1)
        try:
            setup(e)
            e.set_proposal(6, None, scaling=0.1)
            with pytest.raises(_lib.EngineError):
                e.init(np.zeros((4, 2)))
        finally:
            e.close()

    attempt(lambda e: (e.set_prior_joint(np.array([0, 0]), np.zeros(2), np.ones(2)), e.set_level_source(0, ROSEN_SRC, np.zeros(1), 0, [1.0])))
    attempt(lambda e: (e.set_prior(np.zeros(2), np.eye(2)), e.set_level_source(0, ROSEN_SRC, np.zeros(2), 2, np.eye(2))))
    attempt(lambda e: (e.set_prior(np.zeros(2), np.eye(2)), e.set_level_source(0, ROSEN_SRC, np.zeros(2049), 0, [1.0])))
