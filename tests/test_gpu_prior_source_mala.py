"""MALA under source-defined priors on the device (tda_user_mala_steps with TDA_PRIOR_SOURCE: tda_logprior_term and
tda_logprior_term_grad of the level's source): Philox forward mode against the oracle with scipy's own logpdf and the exact
gradient of the 13 families, the prior's gradient alone at every point of the g22 fixture, an all-normal DevicePrior against
the engine's own diagonal Gaussian prior, checkpoint resume, sample(backend='hip') and the engine's refusals.

The reference has no MALA under a non-Gaussian prior to record (its grad_log_p differentiates a bound method), so parity is
against the oracle.  Every compared case is conditioned on the oracle's acceptance rate lying in [0.1, 0.9]; the scalings were
chosen on the CPU with the oracle alone, on the engine's own Philox variates (orc.PhiloxStream).  The chains start around the
components' low quantiles as in test_gpu_prior_source.py, inside the supports and not at their edges: the drift diverges
there, and chains started within 1e-3 of an edge reject every step."""
import warnings

import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extfamilies as xf
from . import extloglike as xl
from . import extmodel as xm
from . import extprior as xp
from . import extpriorgrad as xg
from . import extwave as xw
from .extengine import NOISE_SOURCE, PRIOR_SOURCE, assert_rate, assert_resume_bitwise, compare, run_forward, set_proposal
from .extprior import SIGMA2
from .test_gpu_prior_source import problem

pytestmark = pytest.mark.gpu

SEED, CHAIN_OFFSET = 93, 5  # (extpriorgrad.make_engine's defaults)


def mala(scaling, adaptive=False):
    return dict(kind="mala", scaling=scaling, adaptive=adaptive, gamma=1.01, period=20)


# ---- (e) Philox forward mode against the oracle ------------------------------------------------------------------------------------
# d, m, proposal, block_steps, model ("model": extmodel's, "wave": extwave's with tda_gradient_wave), likelihood (None: isotropic
# Gaussian noise; "t": the Student-t DeviceLogLike with its derivative).  Oracle acceptance / proposals outside the supports of
# the fixed-scaling cases (of 1560), on the engine's own variates: see the table in the test's docstring.
CASES = {
    "d1_m1": (1, 1, mala(0.25), 0, "model", None),
    "d5_m23_split": (5, 23, mala(0.08), 33, "model", None),
    "d13_m300_adaptive": (13, 300, mala(0.01, True), 0, "model", None),
    "d96_m300_adaptive_split": (96, 300, mala(0.004, True), 16, "model", None),
    "d128_m23": (128, 23, mala(0.012), 0, "model", None),
    "d13_m23_student_loglike": (13, 23, mala(0.045), 0, "model", "t"),
    "d13_m47_wave_model_wave_gradient": (13, 47, mala(0.06), 33, "wave", None),
}


def case_inputs(case, N=13):
    """-> comps, prop, block_steps, theta0, the engine's level tuple, the oracle level"""
    d, m, prop, bs, model, like = CASES[case]
    prior = None
    if model == "wave":
        rng = np.random.default_rng(d * 1000 + m)
        comps = xp.components(d)
        # (the starts of test_gpu_prior_source.problem: around the quantiles 0.15 - 0.35 with a spread of 0.01, inside the supports)
        truth, theta0 = xp.starts_near_lower_edges(comps, N, rng)
        y = xw.np_forward(truth, m)[0] + np.sqrt(SIGMA2) * rng.standard_normal(m)
        prior = xg.FamilyGradPrior(comps)
        level = orc.CallableGaussianLevel(lambda th: xw.np_forward(th, m), y, "iso", SIGMA2, prior)
        level.grad_logpost = lambda theta, F: prior.grad(theta) + xw.np_vjp(theta, level.loglike.grad(F))
        return comps, prop, bs, theta0, (xw.source("wave", "wave"), y, 0, SIGMA2), level
    comps, y, theta0 = problem(d, m, N, seed=d * 1000 + m)
    prior = xg.FamilyGradPrior(comps)
    if like is None:
        return comps, prop, bs, theta0, (xm.source(), y, 0, SIGMA2), xg.gaussian_grad_level(prior, m, y)
    par = 0.1 * (1.0 + 0.1 * np.arange(m) / m)
    return comps, prop, bs, theta0, (xm.source() + xl.KINDS[like][0], y, NOISE_SOURCE, par), xg.loglike_grad_level(prior, m, y, par, like)


def case_engine(case, N=13):
    comps, prop, bs, theta0, lvl, level = case_inputs(case, N)
    p, q, psrc = xg.family_source(comps)
    return xg.make_engine(psrc, p, q, N, lvl, prop, bs), comps, prop, theta0, level


@pytest.mark.parametrize("case", list(CASES))
def test_philox_forward_matches_oracle(case):
    """masks exact, log-posterior 1e-10, log-prior 1e-10 of its summed magnitudes, states 1e-9 / 1e-12 (above 64 parameters in
    the span form, for the reason the GRW prior tests give: the 128-term sums put their relative error into every increment),
    final scaling 1e-12.  On the CPU oracle with the engine's variates (N = 13, T = 120):

        case                                  acceptance   proposals outside a support
        d1_m1                                 0.43         -
        d5_m23_split                          0.57         210 of 1560
        d13_m300_adaptive                     0.67         (adaptive)
        d96_m300_adaptive_split               0.65         (adaptive)
        d128_m23                              0.65         468 of 1560
        d13_m23_student_loglike               0.64         374 of 1560
        d13_m47_wave_model_wave_gradient      0.69         328 of 1560

    and at these scalings a relative perturbation of theta0 by 1e-14 leaves every accept mask as it is and moves the log-posterior
    trace by 1e-11 of itself at most (d = 1; 8e-13 at d = 96, below 1e-13 elsewhere): the drift stays contractive.
    """
    N, T = 13, 120
    e, comps, prop, theta0, level = case_engine(case, N)
    params, stats, acc, scal, _, z, u = run_forward(e, theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level, prop, theta0, zz, uu)
    assert_rate(ref["accepted"][:, 1:])
    if not prop["adaptive"] and len(comps) > 1:
        outside = xg.mala_proposals_outside(ref, level.prior, level, zz, prop)
        print("proposals outside a support: %d of %d" % (outside.sum(), outside.size))
        assert outside.sum() >= 1 and not np.any(ref["accepted"][:, 1:][outside])
    compare(params, stats, acc, ref, scal, prior=level.prior, span_form=len(comps) > 64)
    assert np.all(np.isfinite(stats)) and np.all(level.prior.inside(params.reshape(-1, len(comps))))


# ---- (f) the prior's gradient alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 46])
def test_prior_gradient_alone_at_every_probe(golden, d):
    """A model with constant outputs and a zero tda_gradient, replayed with zero uniforms and the normals of
    extpriorgrad.probe_chains (zero in every compared parameter): the step of an accepted chain moves a compared parameter by
    exactly h grad log p, h = s^2 / 2, so (theta_1 - theta_0) / h is the device's tda_logprior_term_grad at theta_0.  One
    engine, one compile; a run of one step per step size (the scaling is one number per engine), of which the chains built
    for that size are read.  Every such chain must be accepted (on the CPU oracle all are).  Bound: that of the host comparison
    (8 eps gmag + gcond + gallow) plus eps |theta| / h for the rounding of the sum; it is vacuous for the points within a few
    ulps of an edge, which admit no step they could resolve: the share of points held to 1e-6 of the gradient or better is
    printed and must be above 80 %.  d = 46: the rows 0-45, no second parameter per lane."""
    from tinyda_amd.engine import Engine

    g21, g22 = golden(xf.GOLDEN_NAME), golden(xg.GOLDEN_NAME)
    rows = xf.decode_rows(g21)[:d]
    x, h, z, compared, ref, tol = xg.probe_chains(g21, g22, d)
    C = x.shape[0]
    p, q, psrc = xg.family_source([xf.component(r) for r in rows])
    got = np.full(x.shape, np.nan)
    e = Engine(C, d, seed=1)
    try:
        e.set_prior_joint(np.full(d, PRIOR_SOURCE), p, q)
        e.set_level_source(0, xg.ZERO_MODEL + "\n" + psrc, np.zeros(3), 0, 1.0)
        for hv in np.unique(h):
            sel = h == hv
            sg = float(np.sqrt(2.0 * hv))
            assert 0.5 * sg * sg == hv
            e.set_proposal(6, None, scaling=sg)
            e.init(x)
            e.set_replay(z[None, :, :], np.zeros((1, C)))
            params, stats, acc = e.run_host(1)
            assert acc[0][sel].all(), (hv, acc[0][sel])
            got[sel] = (params[0][sel] - x[sel]) / hv
    finally:
        e.close()
    bound = xg.probe_bound(x, h, ref, tol)
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(compared, np.where(bound > 0, err / bound, np.where(err == 0.0, 0.0, np.inf)), 0.0)
        sharp = (bound <= 1e-6 * np.abs(ref))[compared & (ref != 0.0)].mean()
    for name in xf.FAMILY_NAMES:
        mine = np.array([r[0] == name for r in rows])
        print("%-12s largest error / bound %.3e over %d points" % (name, ratio[:, mine].max(), compared[:, mine].sum()))
    print("share of points held to 1e-6 of the gradient or better: %.3f" % sharp)
    assert sharp > 0.8
    assert np.all(ratio <= 1.0), [(rows[j], x[c, j], ratio[c, j]) for c, j in zip(*np.nonzero(ratio > 1.0))]


# ---- (g) an all-normal DevicePrior against the engine's own diagonal Gaussian prior ------------------------------------------------
@pytest.mark.parametrize("d,m,prop,bs", [(5, 23, mala(0.08), 0), (96, 300, mala(0.004, True), 16)])
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
        e.set_level_source(0, xm.source() + (xp.NORMAL_SRC + xg.NORMAL_GRAD_SRC if src_prior else ""), y, 1, var)
        set_proposal(e, prop)
        e.init(theta0)
        runs.append(e.run_host(T) + (e.proposal_state_scaling(),))
        e.close()
    (p0, s0, a0, c0), (p1, s1, a1, c1) = runs
    assert np.array_equal(a0, a1) and 0.1 <= a0.mean() <= 0.9
    np.testing.assert_allclose(s1[:, :, 2], s0[:, :, 2], rtol=1e-10)
    np.testing.assert_allclose(p1, p0, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(c1, c0, rtol=1e-12)
    # the log-prior: 1e-10 of the summed magnitudes of its terms (the two sums associate differently)
    sd = np.sqrt(pv)
    mag = np.sum(np.abs(-0.5 * ((p0 - pm) / sd) ** 2) + np.abs(-np.log(sd) - 0.9189385332046727), axis=2)
    assert np.all(np.abs(s1[:, :, 0] - s0[:, :, 0]) <= 1e-10 * mag)


# ---- (h) checkpoints ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d5_m23_split", "d96_m300_adaptive_split"])
def test_checkpoint_resume_is_bitwise(case):
    """get_state mid period, set_state into a fresh engine: the blob carries what MALA's always carried (the gradient at the
    current state), nothing of the prior"""
    N = 11

    def make():
        e, _, _, theta0, _ = case_engine(case, N)
        e.init(theta0)
        return e

    assert_resume_bitwise(make)


# ---- (i) sample() ------------------------------------------------------------------------------------------------------------------
def test_sample_api_normal_components_reach_the_closed_form_posterior():
    """sample(backend='hip') over a linear DeviceModel under from_distributions of norm components, 4096 chains: the problem, the
    proposal and the error estimate of test_gpu_mala_source.test_sample_api_linear_gaussian_posterior, whose prior is the
    multivariate normal with the same moments; theta0 ~ prior comes from the components' quantile functions here"""
    import scipy.stats as st

    import tinyda_amd as tda

    from .test_gpu_mala_source import _linear_source

    d, m, N, T, burn = 3, 8, 4096, 600, 200
    rng = np.random.default_rng(11)
    A = rng.standard_normal((m, d)) / np.sqrt(d)
    pm, pv = np.array([0.2, -0.1, 0.0]), np.array([1.0, 0.5, 2.0])
    nv = 0.3 ** 2 * (1.0 + 0.2 * np.arange(m))
    y = A @ rng.standard_normal(d) + np.sqrt(nv) * rng.standard_normal(m)
    prior = tda.DevicePrior.from_distributions([st.norm(pm[j], np.sqrt(pv[j])) for j in range(d)])
    post = tda.Posterior(prior, tda.GaussianLogLike(y, np.diag(nv)), tda.DeviceModel(_linear_source(A), m))
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
    print("acceptance %.3f" % acc)
    assert 0.3 < acc < 0.9
    # Monte Carlo error of the pooled moments from the spread of per-chain means (autocorrelation included)
    cm = X.mean(axis=1)
    se = cm.std(axis=0, ddof=1) / np.sqrt(N)
    pooled = X.reshape(-1, d)
    assert np.all(np.abs(pooled.mean(axis=0) - mean) < 5 * se + 1e-12), (pooled.mean(axis=0), mean, se)
    C = np.cov(pooled.T)
    np.testing.assert_allclose(C, cov, atol=0.05 * np.sqrt(np.outer(np.diag(cov), np.diag(cov))).max())


def test_sample_api_bounded_components_stay_inside_their_supports():
    import scipy.stats as st

    import tinyda_amd as tda

    d, m, N, T = 6, 23, 512, 200
    comps = [st.gamma(2.5, scale=0.15), st.lognorm(0.7, scale=0.3), st.beta(2.0, 3.5), st.gamma(4.0, scale=0.1), st.lognorm(0.4, scale=0.5),
             st.beta(3.0, 2.0)]
    truth = np.array([c.ppf(0.5) for c in comps])
    y = xm.np_forward(truth, m)[0] + np.sqrt(SIGMA2) * np.random.default_rng(8).standard_normal(m)
    prior = tda.DevicePrior.from_distributions(comps)
    post = tda.Posterior(prior, tda.GaussianLogLike(y, SIGMA2 * np.eye(m)),
                         tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0]))
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(post, tda.MALA(0.06), T, n_chains=N, seed=5, backend="hip", initial_parameters=[truth] * N)
    assert res["backend"] == "hip"
    fam = xp.FamilyPrior(comps)
    states = np.stack([np.stack([ln.parameters for ln in res["chain_%d" % c]]) for c in range(0, N, 8)])
    assert np.all(fam.inside(states.reshape(-1, d)))
    rate = np.mean([np.mean(res["chain_%d" % c].accepted[1:]) for c in range(N)])
    print("acceptance %.3f" % rate)
    assert 0.3 < rate < 0.9
    link = res["chain_3"][-1]
    assert np.isclose(link.prior, fam.logpdf(link.parameters)[0], rtol=1e-10)


# ---- (j) refusals ------------------------------------------------------------------------------------------------------------------
def test_engine_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    d, N = 2, 4
    y = np.array([0.1, 0.2, 0.3])
    src = xm.source() + xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC
    kinds, p, q = np.full(d, PRIOR_SOURCE), np.zeros(d), np.ones(d)
    th0 = np.ones((N, d))

    def refused(e, match):
        with pytest.raises(_lib.EngineError, match=match):
            e.init(th0)

    e = Engine(N, d, seed=1, n_levels=2)  # two levels
    try:
        e.set_prior_joint(kinds, p, q)
        e.set_level_source(0, src, y, 0, SIGMA2)
        e.set_level_source(1, src, y, 0, SIGMA2)
        with pytest.raises(_lib.EngineError, match="MALA is lowered for single-level chains only"):
            e.set_proposal(6, None, scaling=0.1)
    finally:
        e.close()
    e = Engine(N, d, seed=1)  # dense noise
    try:
        e.set_prior_joint(kinds, p, q)
        e.set_level_source(0, src, y, 2, SIGMA2 * np.eye(3))
        e.set_proposal(6, None, scaling=0.1)
        refused(e, "source-defined prior needs source-defined forward models with isotropic / diagonal noise")
    finally:
        e.close()
    m = 2049
    e = Engine(N, d, seed=1)
    try:
        e.set_prior_joint(kinds, p, q)
        e.set_level_source(0, src, np.zeros(m), 0, SIGMA2)
        e.set_proposal(6, None, scaling=0.1)
        refused(e, "at most 2048 outputs")
        # ... a source without the model's gradient, and one without the prior's: each named, and the engine still runs
        e.set_level_source(0, xm.source().split("__device__ double tda_gradient")[0] + xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, y, 0, SIGMA2)
        refused(e, "tda_gradient")
        e.set_level_source(0, xm.source() + xp.LOGNORMAL_SRC, y, 0, SIGMA2)
        refused(e, r"source-defined prior under MALA needs __device__ double tda_logprior_term_grad\(double x, double p, double q, int j\)")
        e.set_level_source(0, src, y, 0, SIGMA2)
        e.init(th0)
        assert np.all(np.isfinite(e.run_host(3)[1]))
        # the same level under the Gaussian prior again: the MALA program is compiled without the switch
        e.set_prior(np.ones(d), np.eye(d))
        e.init(th0)
        assert np.all(np.isfinite(e.run_host(3)[1]))
    finally:
        e.close()
