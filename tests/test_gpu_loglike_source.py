"""Source-defined log-likelihoods on the device (TDA_NOISE_SOURCE: tda_loglike_term compiled into tda_user_steps,
tda_user_level_action and the MALA kernels): the reference's chains replayed through set_replay (g18), Philox forward mode
against the oracle with the same terms in NumPy (single level, MALA, Delayed Acceptance / MLDA), the Gaussian term against
the engine's own diagonal noise, tda_engine_evaluate, checkpoint resume, a term with NaN / -inf regions, the engine's
refusals and sample(backend='hip').

Every case that is compared with the oracle is conditioned on the oracle's acceptance rate lying in [0.1, 0.9], so that
agreement of the accept masks is not vacuous; the scalings were chosen on the CPU with the oracle alone."""
import warnings

import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from .extengine import (NOISE_SOURCE, assert_levels_resume_bitwise, assert_rate, assert_resume_bitwise, compare, compare_levels, compare_replay,
                        oracle_uniforms, run_forward, run_levels_forward, set_proposal)
from .extmodel import np_forward, source

pytestmark = pytest.mark.gpu

SEED, CHAIN_OFFSET = 91, 3


def problem(d, m, kind, N, seed, shift=0.0, coup=0.5):
    """model and prior as test_gpu_mala_source._problem; Student-t scale 0.1 (1 + 0.1 o / m), Poisson exposure 20 + o % 7"""
    rng = np.random.default_rng(seed)
    truth = 0.3 * rng.standard_normal(d)
    F = np_forward(truth, m)[0]
    if kind == "poisson":
        par = 20.0 + np.arange(m) % 7
        y = rng.poisson(par * np.exp(F)).astype(float)
    else:  # "t", and "gauss" with the variances par
        par = 0.1 * (1.0 + 0.1 * np.arange(m) / m)
        y = F + par * rng.standard_t(4, m)
        if kind == "gauss":
            par = par ** 2
    theta0 = truth + 0.01 * rng.standard_normal((N, d))
    pm, pv = 0.1 * np.ones(d), 0.5 + 0.01 * np.arange(d)
    return y, par, theta0, pm, pv


def level_of(kind, m, y, par, pm, pv, shift=0.0, coup=0.5, terms=None):
    _, t, g = xl.KINDS[kind]
    return xl.LogLikeLevel(lambda th: np_forward(th, m, shift=shift, coup=coup), y, par, terms or t, orc.MVNPrior(pm, np.diag(pv)), g, shift, coup)


def full_source(kind, shift=0.0, coup=0.5):
    return source(shift=shift, coup=coup) + xl.KINDS[kind][0]


# single level: d, m, likelihood, proposal (the oracle's description), block_steps
CASES = {
    "d1_m1_t_grw": (1, 1, "t", dict(kind="grw", C=np.eye(1), scaling=1.2), 0),
    "d5_m23_t_pcn": (5, 23, "t", dict(kind="pcn", scaling=0.05), 0),
    "d5_m23_poisson_grw_adaptive_split": (5, 23, "poisson", dict(kind="grw", C=1e-3 * np.eye(5), scaling=1.0, adaptive=True, gamma=1.01, period=20), 33),
    "d5_m300_poisson_am": (5, 300, "poisson", dict(kind="am", C0=1e-3 * np.eye(5), t0=20, period=20), 0),
    "d1_m300_poisson_am_split": (1, 300, "poisson", dict(kind="am", C0=1e-2 * np.eye(1), t0=20, period=20, adaptive=True, gamma=1.01), 16),
    "d96_m300_t_grw_adaptive_split": (96, 300, "t", dict(kind="grw", C=2e-5 * np.eye(96), scaling=1.0, adaptive=True, gamma=1.01, period=20), 16),
    "d96_m23_poisson_pcn": (96, 23, "poisson", dict(kind="pcn", scaling=0.03, adaptive=True, gamma=1.01, period=20), 0),
    "d96_m1_t_am_split": (96, 1, "t", dict(kind="am", C0=3e-2 * np.eye(96), t0=40, period=20), 33),
}

# (as in test_gpu_mala_source.py: scalings that keep the drift theta -> theta + s^2/2 grad contractive.  Checked on the oracle
# alone: a relative perturbation of theta0 by 1e-14 moves its log-posterior trace by less than 1e-14 at these scalings, while at
# 0.6 (d = 1) and 0.035 (d = 96, m = 23) it grows to 3e-3 and 4e-9 within the 120 steps)
MALA_CASES = {
    "d1_m1_poisson_mala": (1, 1, "poisson", dict(kind="mala", scaling=0.4), 0),
    "d5_m23_t_mala_split": (5, 23, "t", dict(kind="mala", scaling=0.08), 33),
    "d5_m300_t_mala_adaptive": (5, 300, "t", dict(kind="mala", scaling=0.01, adaptive=True, gamma=1.01, period=20), 0),
    "d96_m300_poisson_mala_adaptive_split": (96, 300, "poisson", dict(kind="mala", scaling=0.012, adaptive=True, gamma=1.01, period=20), 16),
    "d96_m23_t_mala": (96, 23, "t", dict(kind="mala", scaling=0.025), 0),
}

def case_inputs(case, N=13):
    d, m, kind, prop, bs = {**CASES, **MALA_CASES}[case]
    y, par, theta0, pm, pv = problem(d, m, kind, N, seed=d * 1000 + m)
    return d, m, kind, prop, bs, y, par, theta0, pm, pv


def make_engine(d, N, src, y, par, pm, pv, prop, bs, n_levels=1, seed=SEED, chain_offset=CHAIN_OFFSET):
    from tinyda_amd.engine import Engine

    e = Engine(N, d, seed=seed, chain_offset=chain_offset, block_steps=bs, n_levels=n_levels)
    e.set_prior(pm, np.diag(pv))
    if n_levels == 1:
        e.set_level_source(0, src, y, NOISE_SOURCE, par)
        set_proposal(e, prop)
    return e


# ---- 6. the reference's chains --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g18_loglike_student_grw", "g18_loglike_poisson_am"])
def test_engine_replays_reference_chain(golden, name):
    from tinyda_amd.engine import Engine

    g = golden(name)
    kind = str(g["kind"])
    N, T1, d = g["theta"].shape
    e = Engine(N, d, seed=1)
    e.set_prior(g["prior_mean"], g["prior_cov"])
    e.set_level_source(0, full_source(kind), g["data"], NOISE_SOURCE, g["par"])
    if kind == "t":
        e.set_proposal(0, g["C"], scaling=float(g["scaling0"]), adaptive=bool(g["adaptive"]), gamma=float(g["gamma"]), period=int(g["period"]))
    else:
        e.set_proposal(2, g["C0"], sd=float(g["sd"]), epsilon=float(g["epsilon"]), t0=int(g["t0"]), period=int(g["period"]))
    e.init(g["theta0"])
    e.set_replay(np.swapaxes(g["z"], 0, 1), np.swapaxes(g["u"], 0, 1))
    params, stats, acc = e.run_host(T1 - 1)
    state = e.proposal_state(want_am=kind != "t")
    e.close()
    compare_replay(params, stats, acc, g, loglike=True, **(dict(scaling=state["scaling"]) if kind == "t" else dict(C=state["C"])))
    assert_rate(g["accepted"][:, 1:])


# ---- 7. / 8. Philox forward mode against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES) + list(MALA_CASES))
def test_philox_forward_matches_oracle(case):
    N, T = 13, 120
    d, m, kind, prop, bs, y, par, theta0, pm, pv = case_inputs(case, N)
    params, stats, acc, scal, C, z, u = run_forward(make_engine(d, N, full_source(kind), y, par, pm, pv, prop, bs), theta0, T, prop)
    ref = orc.run_mh(level_of(kind, m, y, par, pm, pv), prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    compare(params, stats, acc, ref, scal)
    if C is not None:
        np.testing.assert_allclose(C, ref["C"], rtol=1e-9, atol=1e-14)


# ---- 9. hierarchies ----------------------------------------------------------------------------------------------------------
# levels: (likelihood or "lin" for a linear model with isotropic Gaussian noise, shift, coup); the finest level is the model itself
HIER = {
    "da_t_t_pcn": (5, 23, [("t", 0.004, 0.4), ("t", 0.0, 0.5)], [4], 25, dict(kind="pcn", scaling=0.08, adaptive=True, gamma=1.02, period=15), 0),
    "da_linear_coarse_t_fine_grw": (5, 23, [("lin", 0.0, 0.0), ("t", 0.0, 0.5)], [3], 25, dict(kind="grw", C=2e-3 * np.eye(5), scaling=1.0), 0),
    "mlda_am_mixed": (5, 23, [("gauss", 0.008, 0.3), ("t", 0.004, 0.4), ("t", 0.0, 0.5)], [3, 2], 14,
                      dict(kind="am", C0=2e-3 * np.eye(5), t0=20, period=10, adaptive=True, gamma=1.02), 7),
    "da_d96_poisson_grw": (96, 300, [("poisson", 0.002, 0.45), ("poisson", 0.0, 0.5)], [3], 20,
                           dict(kind="grw", C=2e-5 * np.eye(96), scaling=1.0, adaptive=True, gamma=1.01, period=12), 0),
}


def hier_inputs(case, N=16):
    d, m, lv, sl, n_fine, prop, bs = HIER[case]
    y, par, theta0, pm, pv = problem(d, m, lv[-1][0], N, seed=77 + d + m)
    Alin = 0.1 + 0.01 * ((np.arange(m)[:, None] * 7 + np.arange(d)[None, :] * 3) % 11)  # the model linearised at the origin
    levels = []
    for kind, shift, coup in lv:
        if kind == "lin":  # a crude surrogate with an inflated variance
            levels.append(orc.LinearGaussianLevel(Alin, y, "iso", 0.3 ** 2, orc.MVNPrior(pm, np.diag(pv))))
        elif kind == "gauss":
            levels.append(level_of("gauss", m, y, par ** 2 * 4.0, pm, pv, shift, coup))
        else:
            levels.append(level_of(kind, m, y, par, pm, pv, shift, coup))
    return d, m, lv, sl, n_fine, prop, bs, y, par, theta0, pm, pv, Alin, levels


def hier_engine(case, N=16, seed=991):
    d, m, lv, sl, n_fine, prop, bs, y, par, theta0, pm, pv, Alin, levels = hier_inputs(case, N)
    e = make_engine(d, N, None, y, par, pm, pv, prop, bs, n_levels=len(lv), seed=seed, chain_offset=0)
    for i, (kind, shift, coup) in enumerate(lv):
        if kind == "lin":
            e.set_level(i, Alin, y, 0, 0.3 ** 2)
        elif kind == "gauss":  # the engine's own diagonal Gaussian likelihood over a source-defined model
            e.set_level_source(i, source(shift=shift, coup=coup), y, 1, par ** 2 * 4.0)
        else:
            e.set_level_source(i, full_source(kind, shift, coup), y, NOISE_SOURCE, par)
    set_proposal(e, prop)
    e.set_subchains(sl, False)
    e.init(theta0)
    return e, sl, n_fine, prop, theta0, levels


@pytest.mark.parametrize("case", list(HIER))
def test_hierarchy_matches_oracle(case):
    N, seed = 16, 991
    e, sl, n_fine, prop, theta0, levels = hier_engine(case, N, seed)
    rows, z, outs, scal = run_levels_forward(e, n_fine)
    us, ridx = oracle_uniforms(seed, N, rows, sl, None)
    res, pstate = orc.run_multilevel(levels, prop, sl, theta0, np.swapaxes(z, 0, 1), us, n_fine, ridx)
    assert_rate(res[-1]["accepted"][:, 1:])  # (the finest level only: the scalings were chosen for it)
    np.testing.assert_allclose(scal, pstate.scaling, rtol=1e-12)
    compare_levels(outs, res)


# ---- 10. the Gaussian term against the engine's own diagonal noise -------------------------------------------------------------
@pytest.mark.parametrize("d,m,prop", [(5, 23, dict(kind="grw", C=1e-3 * np.eye(5), scaling=1.0, adaptive=True, gamma=1.01, period=20)),
                                      (96, 300, dict(kind="pcn", scaling=0.01)),
                                      (5, 300, dict(kind="mala", scaling=0.01, adaptive=True, gamma=1.01, period=20))])
def test_gaussian_term_matches_diagonal_noise(d, m, prop):
    from tinyda_amd.engine import Engine

    N, T = 13, 120
    y, var, theta0, pm, pv = problem(d, m, "gauss", N, seed=d * 1000 + m)
    runs = []
    for noise_kind, src in ((1, source()), (NOISE_SOURCE, full_source("gauss"))):
        e = Engine(N, d, seed=SEED, chain_offset=CHAIN_OFFSET)
        e.set_prior(pm, np.diag(pv))
        e.set_level_source(0, src, y, noise_kind, var)
        set_proposal(e, prop)
        e.init(theta0)
        runs.append(e.run_host(T) + (e.proposal_state_scaling(),))
        e.close()
    (p0, s0, a0, c0), (p1, s1, a1, c1) = runs
    assert np.array_equal(a0, a1) and 0.1 <= a0.mean() <= 0.9
    # (the two sums associate differently -- -1/2 sum r^2 w against sum -1/2 r^2 / p -- so not bitwise)
    np.testing.assert_allclose(s1[:, :, 2], s0[:, :, 2], rtol=1e-11)
    np.testing.assert_allclose(p1, p0, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(c1, c0, rtol=1e-12)


# ---- 11. tda_engine_evaluate -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,kind", [(1, 1, "t"), (5, 23, "poisson"), (96, 300, "t"), (128, 300, "poisson")])
def test_evaluate_against_numpy(d, m, kind):
    N = 11
    y, par, theta0, pm, pv = problem(d, m, kind, N, seed=d + m)
    e = make_engine(d, N, full_source(kind), y, par, pm, pv, dict(kind="grw", C=1e-3 * np.eye(d), scaling=1.0), 0)
    e.init(theta0)
    pts = theta0 + 0.05 * np.random.default_rng(2).standard_normal((N, d))
    got = e.evaluate(pts)
    e.close()
    lp, ll, _ = level_of(kind, m, y, par, pm, pv).evaluate(pts)
    np.testing.assert_allclose(got[:, 0], lp, rtol=1e-11)
    np.testing.assert_allclose(got[:, 1], ll, rtol=1e-11)


# ---- 12. checkpoints ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d96_m300_t_grw_adaptive_split", "d5_m23_t_mala_split", "d96_m300_poisson_mala_adaptive_split"])
def test_checkpoint_resume_is_bitwise(case):
    """get_state mid period, set_state into a fresh engine (the format carries nothing new: the parameters are set-up, not state)"""
    N = 11
    d, m, kind, prop, bs, y, par, theta0, pm, pv = case_inputs(case, N)

    def make():
        e = make_engine(d, N, full_source(kind), y, par, pm, pv, prop, bs)
        e.init(theta0)
        return e

    assert_resume_bitwise(make)


def test_hierarchy_checkpoint_resume_is_bitwise():
    assert_levels_resume_bitwise(hier_engine("da_t_t_pcn", 12, seed=77)[0])


# ---- 13. NaN and -inf terms --------------------------------------------------------------------------------------------------
def restricted_inputs(N=13):
    d, m = 5, 23
    y, par, theta0, pm, pv = problem(d, m, "t", N, seed=5023)
    F0 = np_forward(theta0, m)
    nan_f, inf_f = float(F0[:, 0].max()) + 0.004, float(F0[:, 1].min()) - 0.004
    prop = dict(kind="grw", C=1e-3 * np.eye(d), scaling=1.0, adaptive=True, gamma=1.01, period=20)
    return d, m, y, par, theta0, pm, pv, nan_f, inf_f, prop


def test_nan_and_minus_inf_terms_are_rejected():
    N, T = 13, 120
    d, m, y, par, theta0, pm, pv, nan_f, inf_f, prop = restricted_inputs(N)
    e = make_engine(d, N, source() + xl.restricted_t_source(nan_f, inf_f), y, par, pm, pv, prop, 0)
    params, stats, acc, _, _, z, u = run_forward(e, theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level_of("t", m, y, par, pm, pv, terms=xl.restricted_t_terms(nan_f, inf_f)), prop, theta0, zz, uu)
    assert_rate(ref["accepted"][:, 1:])
    compare(params, stats, acc, ref)
    F = np_forward(params.reshape(-1, d), m)
    assert np.all(np.isfinite(stats)) and np.all(F[:, 0] <= nan_f) and np.all(F[:, 1] >= inf_f)
    # proposals into both regions were made (and rejected): each restriction alone changes the unrestricted trace
    free = orc.run_mh(level_of("t", m, y, par, pm, pv), prop, theta0, zz, uu)
    only_nan = orc.run_mh(level_of("t", m, y, par, pm, pv, terms=xl.restricted_t_terms(nan_f, -np.inf)), prop, theta0, zz, uu)
    only_inf = orc.run_mh(level_of("t", m, y, par, pm, pv, terms=xl.restricted_t_terms(np.inf, inf_f)), prop, theta0, zz, uu)
    assert not np.array_equal(free["accepted"], only_nan["accepted"])
    assert not np.array_equal(free["accepted"], only_inf["accepted"])


# ---- 14. refusals ------------------------------------------------------------------------------------------------------------
def test_engine_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    d, m, N = 2, 3, 4
    y, par = np.array([0.1, 0.2, 0.3]), np.ones(m)
    src = full_source("t")

    def attempt(setup, match, n_levels=1, at_init=True):
        e = Engine(N, d, seed=1, n_levels=n_levels)
        try:
            e.set_prior(np.zeros(d), np.eye(d))
            if at_init:
                setup(e)
                with pytest.raises(_lib.EngineError, match=match):
                    e.init(np.zeros((N, d)))
            else:
                with pytest.raises(_lib.EngineError, match=match):
                    setup(e)
        finally:
            e.close()

    # the kind belongs to set_level_source
    attempt(lambda e: e.set_level(0, np.ones((m, d)), y, NOISE_SOURCE, par), "source-defined likelihood", at_init=False)
    attempt(lambda e: e.set_level_callback(0, lambda th: np.zeros((len(th), m)), y, NOISE_SOURCE, par), "source-defined likelihood", at_init=False)
    # missing functions: named with their signatures
    attempt(lambda e: e.set_level_source(0, source(), y, NOISE_SOURCE, par),
            r"defines no __device__ double tda_loglike_term\(double f, double y, double p, int o\)", at_init=False)
    attempt(lambda e: (e.set_level_source(0, source() + xl.TERM_ONLY_SRC, y, NOISE_SOURCE, par), e.set_proposal(6, None, scaling=0.1)),
            r"defines no __device__ double tda_loglike_term_grad\(double f, double y, double p, int o\)")
    # routes that would evaluate the likelihood outside the level's program
    attempt(lambda e: (e.set_level_source(0, src, y, NOISE_SOURCE, par), e.set_proposal_dreamz(M0=10)), "DREAM")
    attempt(lambda e: (e.set_level_source(0, src, y, NOISE_SOURCE, par), e.set_proposal(4, np.eye(d), q_mean=np.zeros(d))), "Independence")
    from tinyda_amd.proposals import OperatorWeightedCrankNicolson

    ow = OperatorWeightedCrankNicolson(0.5 * np.eye(d), 0.5)._lowering()
    attempt(lambda e: (e.set_level_source(0, src, y, NOISE_SOURCE, par), e.set_proposal(**ow)), "operator-weighted")

    def two_levels(e):
        e.set_level_source(0, src, y, NOISE_SOURCE, par)
        e.set_level_source(1, src, y, NOISE_SOURCE, par)
        e.set_proposal(0, 0.01 * np.eye(d))

    attempt(lambda e: (two_levels(e), e.set_subchains([3], True)), "randomised subchain", n_levels=2)
    attempt(lambda e: (two_levels(e), e.set_subchains([3], False), e.set_error_model("state-independent")), "error model", n_levels=2)
    attempt(lambda e: (two_levels(e), e.set_subchains([3], False), e.set_error_model("state-independent-diagonal")), "error model", n_levels=2)
    attempt(lambda e: (two_levels(e), e.set_subchains([3], False), e.set_proposal_dreamz(M0=10)), "DREAM", n_levels=2)
    with pytest.raises(ValueError, match="one parameter per model output"):
        e = Engine(N, d, seed=1)
        try:
            e.set_level_source(0, src, y, NOISE_SOURCE, [1.0])
        finally:
            e.close()


# ---- 15. sample() -------------------------------------------------------------------------------------------------------------
def test_sample_api_linear_gaussian_posterior():
    """sample(backend='hip') over a linear DeviceModel with the Gaussian term, 4096 chains: pooled mean and covariance after
    burn-in against the closed-form posterior (the error estimate of test_gpu_mala_source's test of the same name)"""
    import tinyda_amd as tda

    from .test_gpu_mala_source import _linear_source

    d, m, N, T, burn = 3, 8, 4096, 600, 200
    rng = np.random.default_rng(11)
    A = rng.standard_normal((m, d)) / np.sqrt(d)
    pm, pv = np.array([0.2, -0.1, 0.0]), np.array([1.0, 0.5, 2.0])
    nv = 0.3 ** 2 * (1.0 + 0.2 * np.arange(m))
    y = A @ rng.standard_normal(d) + np.sqrt(nv) * rng.standard_normal(m)
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.DeviceLogLike(xl.GAUSS_SRC, y, nv), tda.DeviceModel(_linear_source(A), m))
    P = np.linalg.inv(np.diag(pv)) + A.T @ np.diag(1.0 / nv) @ A
    cov = np.linalg.inv(P)
    mean = cov @ (pm / pv + A.T @ (y / nv))
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(post, tda.MALA(scaling=0.3, adaptive=True, period=50), T, n_chains=N, initial_parameters=None, seed=12, backend="hip")
    assert res["sampler"] == "MH" and res["n_chains"] == N and res["backend"] == "hip"
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


def test_sample_api_poisson_delayed_acceptance():
    import tinyda_amd as tda

    d, m, N = 5, 23, 4096
    y, par, theta0, pm, pv = problem(d, m, "poisson", 1, seed=12)
    prior = st.multivariate_normal(pm, np.diag(pv))
    like = tda.DeviceLogLike(xl.POISSON_SRC, y, par, reference=xl.poisson_terms)
    posts = [tda.Posterior(prior, like, tda.DeviceModel(source(shift=sh, coup=cp), m, reference=lambda th, sh=sh, cp=cp: np_forward(th, m, shift=sh, coup=cp)[0]))
             for sh, cp in ((0.004, 0.4), (0.0, 0.5))]
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(posts, tda.GaussianRandomWalk(1e-3 * np.eye(d), adaptive=True, period=20), 40, n_chains=N,
                         initial_parameters=[theta0[0]] * N, subchain_length=3, seed=5, backend="auto")
    assert res["sampler"] == "DA" and res["backend"] == "hip"
    for c in (0, 1777, N - 1):
        link = res["chain_fine_%d" % c][-1]
        assert np.isclose(link.posterior, posts[1].create_link(link.parameters).posterior, rtol=1e-10)
    rate = np.mean([np.mean(res["chain_fine_%d" % c].accepted[1:]) for c in range(0, N, 64)])
    assert 0.05 < rate < 0.95
