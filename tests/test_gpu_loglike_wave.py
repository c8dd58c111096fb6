"""Likelihoods that couple outputs on the device (TDA_LOGLIKE_WAVE: tda_loglike_wave of the level's source called by the chain's
whole wave over the outputs in LDS, in tda_user_steps, tda_user_level_action and the MALA kernels; tda_loglike_grad_wave under
MALA): Philox forward mode against the oracle with the NumPy twins of extloglikewave (single level, Delayed Acceptance / MLDA,
MALA), an order constraint between neighbouring outputs, the separable Student-t written in the wave form against the route
through tda_loglike_term (bitwise), the reference's chains replayed (g24), tda_engine_evaluate, checkpoint resume, the rebuild
when a level's source changes form, the engine's refusals and sample(backend='hip').

Every case that is compared with the oracle is conditioned on the oracle's acceptance rate lying in [0.1, 0.9]; the scalings
were chosen on the CPU with the oracle alone."""
import warnings

import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from . import extloglikewave as xlw
from . import extmodel as xm
from . import extprior as xp
from . import extpriorgrad as xg
from . import extpriorwave as xpw
from . import extwave as xwv
from .extengine import (NOISE_SOURCE, assert_levels_resume_bitwise, assert_rate, assert_resume_bitwise, compare, compare_levels,
                        compare_replay, oracle_uniforms, run_forward, run_levels_forward, set_proposal)
from .extloglikewave import full_source, level_of, make_engine, problem
from .test_loglike_wave import G24

pytestmark = pytest.mark.gpu


def grw(d, c, **kw):
    return dict(kind="grw", C=c * np.eye(d), scaling=1.0, **kw)


def am(d, c, **kw):
    return dict(kind="am", C0=c * np.eye(d), t0=40, period=20, **kw)


ADAPT = dict(adaptive=True, gamma=1.01, period=20)

# The two AdaptiveMetropolis cases at d = 65 take epsilon = 1e-4.  Each chain adapts its covariance from at most 120 states in 65
# dimensions, so the empirical part has no full rank and the factor of sd (cov + epsilon I) is as well conditioned as epsilon makes
# it.  With the default 1e-6 the oracle alone, on the CPU, is not reproducible to the bar its covariance is compared at: a relative
# change of theta0 by 1e-14 leaves every accept mask as it is but moves entries of the final covariance by 2.0 - 2.7 times
# rtol 1e-9 / atol 1e-14 under the marginalised likelihood (0.6 - 0.7 times under ar1), and the states by 5 - 10 times their own
# bar.  With 1e-4 the same change moves the covariance by 0.19 - 0.25 (ar1: 0.05 - 0.06) of the bar and the states by 0.1 - 0.3.
# The acceptance rates stay at 0.52 and 0.74.

# ---- 1. Philox forward mode against the oracle -------------------------------------------------------------------------------------
# likelihood, d, m, N, proposal, block_steps, variant (None: extmodel's model under the Gaussian prior; "wave": over extwave's
# wave-form model; "term_prior" / "wave_prior": beside a separable / a coupled DevicePrior).  m = 1: no neighbour, 63 lanes hold
# nothing; 23: one partial pass; 64 / 65: the neighbour of output 64 belongs to lane 63; 130: three passes; d = 65, 128: the second
# parameter per lane; N is no multiple of 16; block_steps 16 / 33 split the 120 steps.
CASES = {
    "ar1_d1_m1_grw": ("ar1", 1, 1, 13, grw(1, 0.3), 0, None),
    "ar1_d5_m23_grw_adaptive_split": ("ar1", 5, 23, 19, grw(5, 1e-3, **ADAPT), 33, None),
    "ar1_d5_m64_pcn": ("ar1", 5, 64, 13, dict(kind="pcn", scaling=0.07), 0, None),
    "ar1_d65_m65_am_split": ("ar1", 65, 65, 19, am(65, 6e-4, epsilon=1e-4), 16, None),
    "ar1_d128_m130_grw_adaptive": ("ar1", 128, 130, 13, grw(128, 1e-5, **ADAPT), 0, None),
    "marginal_d1_m1_grw": ("marginal", 1, 1, 13, grw(1, 0.3), 0, None),
    "marginal_d5_m65_pcn_adaptive": ("marginal", 5, 65, 13, dict(kind="pcn", scaling=0.04, **ADAPT), 0, None),
    "marginal_d65_m64_am_split": ("marginal", 65, 64, 19, am(65, 6e-5, adaptive=True, gamma=1.01, epsilon=1e-4), 33, None),
    "marginal_d128_m130_grw": ("marginal", 128, 130, 13, grw(128, 7e-5), 16, None),
    "softmax_d5_m23_grw": ("softmax", 5, 23, 13, grw(5, 2e-2), 0, None),
    "softmax_d1_m65_am_split": ("softmax", 1, 65, 19, dict(kind="am", C0=6e-2 * np.eye(1), t0=20, period=20), 16, None),
    "softmax_d65_m130_pcn": ("softmax", 65, 130, 13, dict(kind="pcn", scaling=0.07), 0, None),
    "softmax_d128_m64_grw_adaptive_split": ("softmax", 128, 64, 13, grw(128, 1e-4, **ADAPT), 33, None),
    "ar1_d13_m47_wave_model_grw": ("ar1", 13, 47, 13, grw(13, 2e-3), 33, "wave"),
    "marginal_d5_m23_term_prior_am": ("marginal", 5, 23, 13, dict(kind="am", C0=1e-3 * np.eye(5), t0=20, period=20), 0, "term_prior"),
    "ar1_d65_m65_wave_prior_grw": ("ar1", 65, 65, 13, grw(65, 7e-5), 16, "wave_prior"),
}


class NormalTwin:
    """NumPy twin of extprior.NORMAL_SRC (+ extpriorgrad.NORMAL_GRAD_SRC), a separable DevicePrior: p = mean, q = standard deviation"""

    source = xp.NORMAL_SRC + xg.NORMAL_GRAD_SRC

    def __init__(self, p, q):
        self.p, self.q = np.asarray(p, dtype=float), np.asarray(q, dtype=float)
        self.dim, self.mean, self.cov = self.p.shape[0], self.p, np.diag(self.q ** 2)

    def terms(self, theta):
        r = (np.atleast_2d(theta) - self.p) / self.q
        return -0.5 * r * r - np.log(self.q) - 0.9189385332046727

    def logpdf(self, theta):
        out = self.terms(theta).sum(axis=1)
        return out if np.ndim(theta) == 2 else out[0]

    def magnitude(self, theta):
        return np.abs(self.terms(theta)).sum(axis=1)

    def grad(self, theta):
        return (self.p - theta) / (self.q * self.q)


def case_inputs(case):
    """-> d, N, proposal, block_steps, theta0, a function that makes the engine, the oracle level, the prior twin (None: Gaussian)"""
    kind, d, m, N, prop, bs, variant = CASES[case]
    seed = d * 1000 + m
    if variant == "wave":
        y, par, theta0, pm, pv = problem(d, m, kind, N, seed, fn=lambda th: xwv.np_forward(th, m), scale=0.01)
        level = xlw.CoupledLevel(lambda th: xwv.np_forward(th, m), y, par, xlw.KINDS[kind][1], orc.MVNPrior(pm, np.diag(pv)))
        return d, N, prop, bs, theta0, lambda: make_engine(d, N, xwv.source("wave") + xlw.KINDS[kind][0], y, par, pm, pv, prop, bs), level, None
    y, par, theta0, pm, pv = problem(d, m, kind, N, seed)
    if variant in ("term_prior", "wave_prior"):
        prior = NormalTwin(pm, np.sqrt(pv)) if variant == "term_prior" else xpw.cauchy_difference(d)
        if variant == "wave_prior":  # (data and starts at the smooth profile the coupled prior's tests start from)
            y, par, theta0, pm, pv = problem(d, m, kind, N, seed, truth=xpw.starts(prior, 1, np.random.default_rng(0))[0])
        level = level_of(kind, m, y, par, pm, pv, prior=prior)
        return d, N, prop, bs, theta0, lambda: xpw.make_engine(prior, N, [(full_source(kind), y, NOISE_SOURCE, par)], prop, bs), level, prior
    return d, N, prop, bs, theta0, lambda: make_engine(d, N, full_source(kind), y, par, pm, pv, prop, bs), level_of(kind, m, y, par, pm, pv), None


@pytest.mark.parametrize("case", list(CASES))
def test_philox_forward_matches_oracle(case):
    T = 120
    d, N, prop, bs, theta0, make, level, prior = case_inputs(case)
    params, stats, acc, scal, C, z, u = run_forward(make(), theta0, T, prop)
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    # (extengine.compare's rule: above 64 parameters the 128-term proposal sum puts its relative error into every increment; under
    # AM the adapted factor does)
    compare(params, stats, acc, ref, scal, prior=prior, span_form=d > 64 or prop["kind"] == "am")
    if C is not None:
        np.testing.assert_allclose(C, ref["C"], rtol=1e-9, atol=1e-14)


# ---- 2. hierarchies ---------------------------------------------------------------------------------------------------------------------
# levels: (likelihood, or "gauss" for the engine's own diagonal Gaussian noise over the same model; shift; coup); the finest is the model itself
HIER = {
    "da_coupled_coarse_gauss_fine_grw": (5, 23, [("ar1", 0.004, 0.4), ("gauss", 0.0, 0.5)], [3], 25, grw(5, 5e-3), 0),
    "da_gauss_coarse_coupled_fine_pcn": (5, 23, [("gauss", 0.004, 0.4), ("marginal", 0.0, 0.5)], [4], 25, dict(kind="pcn", scaling=0.08, adaptive=True, gamma=1.02, period=15), 0),
    "mlda_coupled_at_all_levels_am": (5, 65, [("ar1", 0.008, 0.3), ("softmax", 0.004, 0.4), ("ar1", 0.0, 0.5)], [3, 2], 14,
                                      dict(kind="am", C0=5e-4 * np.eye(5), t0=20, period=10, adaptive=True, gamma=1.02), 7),
    "da_d96_m130_marginal_grw": (96, 130, [("marginal", 0.002, 0.45), ("marginal", 0.0, 0.5)], [3], 20, grw(96, 2e-5, adaptive=True, gamma=1.01, period=12), 0),
}


def hier_engine(case, N=16, seed=995):
    from tinyda_amd.engine import Engine

    d, m, lv, sl, n_fine, prop, bs = HIER[case]
    y, par, theta0, pm, pv = problem(d, m, "ar1", N, seed=77 + d + m)
    counts = problem(d, m, "softmax", N, seed=77 + d + m)[0]
    e = Engine(N, d, seed=seed, chain_offset=0, block_steps=bs, n_levels=len(lv))
    e.set_prior(pm, np.diag(pv))
    levels = []
    for i, (kind, shift, coup) in enumerate(lv):
        if kind == "gauss":  # the engine's own diagonal Gaussian likelihood, with an inflated variance
            e.set_level_source(i, xm.source(shift=shift, coup=coup), y, 1, par ** 2 * 4.0)
            levels.append(xl.LogLikeLevel(lambda th, sh=shift, cp=coup: xm.np_forward(th, m, shift=sh, coup=cp), y, par ** 2 * 4.0, xl.gauss_terms,
                                          orc.MVNPrior(pm, np.diag(pv))))
        else:
            yk, pk = (counts, np.ones(m)) if kind == "softmax" else (y, par)
            e.set_level_source(i, full_source(kind, shift, coup), yk, NOISE_SOURCE, pk)
            levels.append(level_of(kind, m, yk, pk, pm, pv, shift, coup))
    set_proposal(e, prop)
    e.set_subchains(sl, False)
    e.init(theta0)
    return e, sl, n_fine, prop, theta0, levels


@pytest.mark.parametrize("case", list(HIER))
def test_hierarchy_matches_oracle(case):
    N, seed = 16, 995
    e, sl, n_fine, prop, theta0, levels = hier_engine(case, N, seed)
    rows, z, outs, scal = run_levels_forward(e, n_fine)
    us, ridx = oracle_uniforms(seed, N, rows, sl, None)
    res, pstate = orc.run_multilevel(levels, prop, sl, theta0, np.swapaxes(z, 0, 1), us, n_fine, ridx)
    assert_rate(res[-1]["accepted"][:, 1:])
    assert_rate(res[0]["accepted"])
    np.testing.assert_allclose(scal, pstate.scaling, rtol=1e-12)
    compare_levels(outs, res)


# ---- 3. MALA ----------------------------------------------------------------------------------------------------------------------------
def mala(scaling, adaptive=False):
    return dict(kind="mala", scaling=scaling, adaptive=adaptive, gamma=1.01, period=20)


# likelihood, d, m, N, proposal, block_steps, model: None = extmodel's (tda_forward, tda_gradient), else extwave's (forward, gradient) forms
MALA_CASES = {
    "ar1_d2_m1": ("ar1", 2, 1, 13, mala(0.42), 0, None),
    "ar1_d2_m65_split": ("ar1", 2, 65, 19, mala(0.22), 33, None),
    "ar1_d65_m96_adaptive": ("ar1", 65, 96, 13, mala(0.014, True), 0, None),
    "marginal_d2_m1": ("marginal", 2, 1, 13, mala(0.28), 0, None),
    "marginal_d65_m65_split": ("marginal", 65, 65, 19, mala(0.016), 16, None),
    "marginal_d2_m96_adaptive": ("marginal", 2, 96, 13, mala(0.04, True), 0, None),
    "ar1_d5_m65_wave_wave": ("ar1", 5, 65, 13, mala(0.35), 33, ("wave", "wave")),
    "marginal_d5_m23_wave_per_parameter": ("marginal", 5, 23, 13, mala(0.4), 0, ("wave", "per_parameter")),
    "ar1_d5_m23_per_output_wave": ("ar1", 5, 23, 13, mala(0.4), 0, ("per_output", "wave")),
    "marginal_d2_m2048": ("marginal", 2, 2048, 13, mala(0.014), 0, None),
}


def mala_inputs(case):
    kind, d, m, N, prop, bs, model = MALA_CASES[case]
    if model is None:
        y, par, theta0, pm, pv = problem(d, m, kind, N, seed=d * 1000 + m)
        return d, N, prop, bs, theta0, full_source(kind), y, par, pm, pv, level_of(kind, m, y, par, pm, pv)
    fn = lambda th: xwv.np_forward(th, m)  # noqa: E731
    y, par, theta0, pm, pv = problem(d, m, kind, N, seed=d * 1000 + m, fn=fn, scale=0.05)
    level = xlw.CoupledLevel(fn, y, par, xlw.KINDS[kind][1], orc.MVNPrior(pm, np.diag(pv)), xlw.KINDS[kind][2], vjp=xwv.np_vjp)
    return d, N, prop, bs, theta0, xwv.source(model[0], model[1], m=m) + xlw.KINDS[kind][0], y, par, pm, pv, level


@pytest.mark.parametrize("case", list(MALA_CASES))
def test_mala_matches_oracle(case):
    """against run_mh with the twin's d log L / d F through the model's vector-Jacobian product.  m = 2048 is the doubled LDS
    buffer at its limit (32 KiB of sensitivities and outputs).  The scalings keep the drift contractive: on the CPU oracle a
    relative perturbation of theta0 by 1e-14 leaves every accept mask as it is and moves the log-posterior trace by less than
    1e-13 of itself at most cases (the marginalised likelihood has directions of negative curvature: at d = 2, m = 1 a scaling of
    0.32 instead of 0.28 amplifies the same perturbation to 2e-12, at d = 65, m = 65 one of 0.02 instead of 0.016 to 4e-12)"""
    T = 60 if case.endswith("m2048") else 120
    d, N, prop, bs, theta0, src, y, par, pm, pv, level = mala_inputs(case)
    params, stats, acc, scal, _, z, u = run_forward(make_engine(d, N, src, y, par, pm, pv, prop, bs), theta0, T, prop)
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    compare(params, stats, acc, ref, scal, span_form=d > 64)


def test_mala_beside_a_device_prior_with_its_gradient():
    N, T, d, m = 13, 120, 5, 23
    prior = xpw.cauchy_difference(d)
    y, par, theta0, pm, pv = problem(d, m, "ar1", N, seed=523, truth=xpw.starts(prior, 1, np.random.default_rng(0))[0])
    prop = mala(0.06)
    e = xpw.make_engine(prior, N, [(full_source("ar1"), y, NOISE_SOURCE, par)], prop)
    params, stats, acc, scal, _, z, u = run_forward(e, theta0, T, prop)
    ref = orc.run_mh(level_of("ar1", m, y, par, pm, pv, prior=prior), prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    compare(params, stats, acc, ref, scal, prior=prior)


# ---- 4. an order that neighbouring outputs decide --------------------------------------------------------------------------------------
def monotone_inputs(N=13, nan=False):
    """d = 5, m = 3: a truth whose outputs are in order with small gaps, so that random-walk proposals break the order now and
    then; the scales are a tenth of the gaps' size"""
    d, m = 5, 3
    truth = xlw.MONOTONE_TRUTH
    F = xm.np_forward(truth, m)[0]
    assert np.all(np.diff(F) > 0)
    rng = np.random.default_rng(31)
    par = 0.05 * np.ones(m)
    y = F + par * rng.standard_normal(m)
    theta0 = truth + 0.002 * rng.standard_normal((N, d))
    pm, pv = 0.1 * np.ones(d), 0.5 + 0.01 * np.arange(d)
    nan_f = float(np.max(xm.np_forward(theta0, m)[:, 0])) + 0.01 if nan else None
    return d, m, y, par, theta0, pm, pv, nan_f


def test_proposals_that_break_the_order_are_rejected():
    N, T = 13, 120
    d, m, y, par, theta0, pm, pv, _ = monotone_inputs(N)
    prop = grw(d, 2.5e-3)
    assert np.all(np.isfinite(xlw.monotone()(xm.np_forward(theta0, m), y, par)))
    params, stats, acc, _, _, z, u = run_forward(make_engine(d, N, xm.source() + xlw.monotone_source(), y, par, pm, pv, prop), theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level_of("ar1", m, y, par, pm, pv, loglike=xlw.monotone()), prop, theta0, zz, uu)
    props = ref["theta"][:, :-1] + zz @ np.linalg.cholesky(prop["C"]).T
    broken = np.any(np.diff(xm.np_forward(props.reshape(-1, d), m), axis=1) < 0, axis=1).reshape(N, T)
    print("oracle: %d of %d proposals break the order, acceptance %.3f" % (broken.sum(), broken.size, ref["accepted"][:, 1:].mean()))
    assert_rate(ref["accepted"][:, 1:])
    assert broken.sum() >= 1 and not np.any(ref["accepted"][:, 1:][broken])
    compare(params, stats, acc, ref)
    assert np.all(np.isfinite(stats)) and np.all(np.diff(xm.np_forward(params.reshape(-1, d), m), axis=1) >= 0)


def test_start_outside_the_order_keeps_minus_inf_until_a_move_inside():
    N, T = 13, 60
    d, m, y, par, theta0, pm, pv, _ = monotone_inputs(N)
    theta0 = theta0.copy()
    theta0[::2] = xlw.MONOTONE_OUTSIDE + (theta0[::2] - xlw.MONOTONE_TRUTH)
    assert np.all(np.any(np.diff(xm.np_forward(theta0[::2], m), axis=1) < 0, axis=1))
    prop = grw(d, 2.5e-3)
    e = make_engine(d, N, xm.source() + xlw.monotone_source(), y, par, pm, pv, prop)
    e.init(theta0)
    assert np.all(e.current()[1][::2, 1] == -np.inf) and np.all(np.isfinite(e.current()[1][1::2, 1]))
    z, u = e.set_export(T)
    params, stats, acc = e.run_host(T)
    e.close()
    ref = orc.run_mh(level_of("ar1", m, y, par, pm, pv, loglike=xlw.monotone()), prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert np.all(ref["loglike"][::2, 0] == -np.inf) and np.any(np.isfinite(ref["loglike"][::2, -1]))
    assert np.array_equal(acc, np.swapaxes(ref["accepted"][:, 1:], 0, 1))
    got, want = stats[:, :, 1], np.swapaxes(ref["loglike"][:, 1:], 0, 1)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.all(got[~np.isfinite(want)] == -np.inf)
    np.testing.assert_allclose(got[np.isfinite(want)], want[np.isfinite(want)], rtol=1e-10)


def test_nan_share_rejects():
    """lane 0's share is NaN above a threshold in F_0 that the chains start just below"""
    N, T = 13, 120
    d, m, y, par, theta0, pm, pv, nan_f = monotone_inputs(N, nan=True)
    prop = grw(d, 2.5e-3)
    params, stats, acc, _, _, z, u = run_forward(make_engine(d, N, xm.source() + xlw.monotone_source(nan_f), y, par, pm, pv, prop), theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level_of("ar1", m, y, par, pm, pv, loglike=xlw.monotone(nan_f)), prop, theta0, zz, uu)
    props = ref["theta"][:, :-1] + zz @ np.linalg.cholesky(prop["C"]).T
    is_nan = (xm.np_forward(props.reshape(-1, d), m)[:, 0] > nan_f).reshape(N, T)
    print("oracle: %d of %d proposals have a NaN share" % (is_nan.sum(), is_nan.size))
    assert is_nan.sum() >= 1 and not np.any(ref["accepted"][:, 1:][is_nan])
    compare(params, stats, acc, ref)
    assert np.all(np.isfinite(stats)) and np.all(xm.np_forward(params.reshape(-1, d), m)[:, 0] <= nan_f)


def test_mala_a_rejected_proposal_never_reaches_the_stored_gradient():
    """under MALA a proposal that breaks the order has log L = -inf and is rejected; the gradient the chain keeps is the one of
    its last accepted state, so the chains are the oracle's, which computes the gradient of accepted states only"""
    N, T = 13, 120
    d, m, y, par, theta0, pm, pv, _ = monotone_inputs(N)
    prop = mala(0.09)
    params, stats, acc, _, _, z, u = run_forward(make_engine(d, N, xm.source() + xlw.monotone_source(), y, par, pm, pv, prop), theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    level = level_of("ar1", m, y, par, pm, pv, loglike=xlw.monotone())
    ref = orc.run_mh(level, prop, theta0, zz, uu)
    cur = ref["theta"][:, :-1].reshape(-1, d)
    g = level.grad_logpost(cur, level.forward(cur)).reshape(N, T, d)
    props = ref["theta"][:, :-1] + 0.5 * prop["scaling"] ** 2 * g + prop["scaling"] * zz
    broken = np.any(np.diff(xm.np_forward(props.reshape(-1, d), m), axis=1) < 0, axis=1).reshape(N, T)
    print("oracle: %d of %d proposals break the order, acceptance %.3f" % (broken.sum(), broken.size, ref["accepted"][:, 1:].mean()))
    assert_rate(ref["accepted"][:, 1:])
    assert broken.sum() >= 1 and not np.any(ref["accepted"][:, 1:][broken])
    compare(params, stats, acc, ref)
    assert np.all(np.isfinite(stats))


# ---- 5. the same bits as the separable route ---------------------------------------------------------------------------------------------
BITWISE = {
    "grw_adaptive_d5_m23": (5, 23, grw(5, 1e-3, **ADAPT), 0),
    "am_d96_m130_split": (96, 130, dict(kind="am", C0=3e-4 * np.eye(96), t0=40, period=20), 16),
    "mala_d5_m65_split": (5, 65, mala(0.07), 33),
}


def _t_problem(d, m, N):
    from .test_gpu_loglike_source import problem as t_problem

    return t_problem(d, m, "t", N, seed=d * 1000 + m)


@pytest.mark.parametrize("case", list(BITWISE))
def test_student_t_in_wave_form_is_bitwise_the_separable_route(case):
    """t_wave sums tda_loglike_term's operations over o = lane, lane + 64, ... from 0.0 as the program's separable branch does, the
    outputs take the same values through LDS as from tda_forward in place, and tda_loglike_grad_wave writes the sensitivities the
    separable MALA branch writes: every record is equal bit for bit"""
    d, m, prop, bs = BITWISE[case]
    N, T = 13, 120
    y, par, theta0, pm, pv = _t_problem(d, m, N)
    runs = []
    for src in (xl.STUDENT_T_SRC, xlw.T_WAVE_SRC):
        e = make_engine(d, N, xm.source() + src, y, par, pm, pv, prop, bs)
        e.init(theta0)
        runs.append(e.run_host(T) + (e.proposal_state_scaling(),))
        e.close()
    assert 0.1 <= runs[0][2].mean() <= 0.9
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_student_t_in_wave_form_is_bitwise_the_separable_route_in_delayed_acceptance():
    from tinyda_amd.engine import Engine

    d, m, N, n_fine = 5, 23, 16, 25
    y, par, theta0, pm, pv = _t_problem(d, m, N)
    runs = []
    for src in (xl.STUDENT_T_SRC, xlw.T_WAVE_SRC):
        e = Engine(N, d, seed=991, n_levels=2)
        e.set_prior(pm, np.diag(pv))
        for i, (sh, cp) in enumerate(((0.004, 0.4), (0.0, 0.5))):
            e.set_level_source(i, xm.source(shift=sh, coup=cp) + src, y, NOISE_SOURCE, par)
        set_proposal(e, dict(kind="pcn", scaling=0.08, adaptive=True, gamma=1.02, period=15))
        e.set_subchains([4], False)
        e.init(theta0)
        runs.append(e.run_levels_host(n_fine))
        e.close()
    assert 0.1 <= runs[0][-1][2].mean() <= 0.9
    for la, lb in zip(*runs):
        assert all(np.array_equal(x, y_) for x, y_ in zip(la, lb))


# ---- 6. the reference's chains ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G24)
def test_engine_replays_reference_chain(golden, name):
    g = golden(name)
    is_am = "C0" in g.files
    N, T1, d = g["theta"].shape
    from .extengine import golden_proposal

    e = make_engine(d, N, full_source(str(g["kind"])), g["data"], g["par"], g["prior_mean"], np.diag(g["prior_cov"]), golden_proposal(g), seed=1, chain_offset=0)
    e.init(g["theta0"])
    e.set_replay(np.swapaxes(g["z"], 0, 1), np.swapaxes(g["u"], 0, 1))
    params, stats, acc = e.run_host(T1 - 1)
    state = e.proposal_state(want_am=is_am)
    e.close()
    compare_replay(params, stats, acc, g, loglike=True, **(dict(C=state["C"]) if is_am else dict(scaling=state["scaling"])))
    assert_rate(g["accepted"][:, 1:])


# ---- 7. tda_engine_evaluate, checkpoints, rebuilds, sample() -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,m", [("ar1", 1, 1), ("ar1", 65, 65), ("marginal", 5, 23), ("softmax", 128, 130), ("marginal", 96, 64)])
def test_evaluate_against_numpy_twin(kind, d, m):
    N = 11
    y, par, theta0, pm, pv = problem(d, m, kind, N, seed=d + m)
    e = make_engine(d, N, full_source(kind), y, par, pm, pv, grw(d, 1e-3))
    pts = theta0 + 0.05 * np.random.default_rng(2).standard_normal((N, d))
    got_before_init = e.evaluate(pts)
    e.init(theta0)
    got = e.evaluate(pts)
    e.close()
    lp, ll, _ = level_of(kind, m, y, par, pm, pv).evaluate(pts)
    np.testing.assert_allclose(got[:, 0], lp, rtol=1e-11)
    np.testing.assert_allclose(got[:, 1], ll, rtol=1e-11)
    assert np.array_equal(got, got_before_init)


@pytest.mark.parametrize("case", ["ar1_d65_m65_am_split", "mala:marginal_d65_m65_split"])
def test_checkpoint_resume_is_bitwise(case):
    N = 11
    if case.startswith("mala:"):
        d, _, prop, bs, _, src, y, par, pm, pv, _ = mala_inputs(case[5:])
    else:
        kind, d, m, _, prop, bs, _ = CASES[case]
        y, par, _, pm, pv = problem(d, m, kind, N, seed=d * 1000 + m)
        src = full_source(kind)
    theta0 = problem(d, 1, "ar1", N, seed=d * 1000 + 65)[2]

    def make():
        e = make_engine(d, N, src, y, par, pm, pv, prop, bs)
        e.init(theta0)
        return e

    assert_resume_bitwise(make)


def test_hierarchy_checkpoint_resume_is_bitwise():
    assert_levels_resume_bitwise(hier_engine("mlda_coupled_at_all_levels_am", 12, seed=77)[0])


def test_a_level_whose_source_changes_form_is_built_again():
    """the same engine, its level set to the separable Student-t, then to its wave form, then back, under GRW and under MALA
    (both programs): each run equals the run of an engine that only ever had that source"""
    d, m, N, T = 5, 23, 13, 40
    y, par, theta0, pm, pv = _t_problem(d, m, N)
    for prop in (grw(d, 1e-3), mala(0.05)):
        fresh = []
        for src in (xl.STUDENT_T_SRC, xlw.T_WAVE_SRC):
            e = make_engine(d, N, xm.source() + src, y, par, pm, pv, prop)
            e.init(theta0)
            fresh.append(e.run_host(T))
            e.close()
        e = make_engine(d, N, xm.source() + xl.STUDENT_T_SRC, y, par, pm, pv, prop)
        try:
            for which in (0, 1, 0, 1):
                e.set_level_source(0, xm.source() + (xl.STUDENT_T_SRC, xlw.T_WAVE_SRC)[which], y, NOISE_SOURCE, par)
                e.init(theta0)
                for a, b in zip(e.run_host(T), fresh[which]):
                    assert np.array_equal(a, b)
        finally:
            e.close()
    # a source of the other form that is not complete: the rebuild is refused with the new form's reason, not the old one's
    from tinyda_amd import _lib

    e = make_engine(d, N, xm.source() + xl.STUDENT_T_SRC, y, par, pm, pv, mala(0.05))
    try:
        # a refused source leaves the level as it was: its text, its forms and its programs (here under MALA, the last `fresh`)
        with pytest.raises(_lib.EngineError, match="both tda_loglike_term and tda_loglike_wave"):
            e.set_level_source(0, xm.source() + xl.STUDENT_T_SRC + xlw.AR1_SRC, y, NOISE_SOURCE, par)
        e.init(theta0)
        for a, b in zip(e.run_host(T), fresh[0]):
            assert np.array_equal(a, b)
        e.set_level_source(0, xm.source() + xlw.without_grad(xlw.AR1_SRC), y, NOISE_SOURCE, par)
        with pytest.raises(_lib.EngineError, match="tda_loglike_grad_wave"):
            e.init(theta0)
    finally:
        e.close()


def _posterior(kind, d, m, seed=12, grad=True):
    import tinyda_amd as tda

    y, par, theta0, pm, pv = problem(d, m, kind, 64, seed=seed)
    like = xlw.device_loglike(kind, y, par) if grad else xlw.device_loglike(kind, y, par, source=xlw.without_grad(xlw.KINDS[kind][0]))
    model = tda.DeviceModel(xm.source(), m, reference=lambda th: xm.np_forward(th, m)[0], reference_gradient=lambda th, s: xm.np_vjp(th, s)[0])
    return tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), like, model), theta0


def test_sample_api_against_the_host_protocol():
    """sample(backend='hip') and sample(backend='host') on a 2-parameter problem under the marginalised-variance likelihood: the
    links of the device chains are the host's own evaluation at the same parameters (1e-10), and the pooled posterior means
    agree.  The bound on the means: both runs are started at the same points near the mode and keep their second half; the
    host's 8 chains x 150 kept steps at an acceptance near 0.4 hold at least 8 x 150 / 40 = 30 independent draws (an
    integrated autocorrelation time of 40 steps is several times what a random walk with this acceptance has in two dimensions), the device's 64 chains
    eight times as many, so the difference of the means has a standard deviation of at most sd sqrt(1 / 30 + 1 / 240) = 0.2 sd and
    is held to five times that, one posterior standard deviation."""
    import tinyda_amd as tda

    d, m, T = 2, 23, 300
    post, theta0 = _posterior("marginal", d, m)
    assert post.likelihood.coupled
    prop = lambda: tda.GaussianRandomWalk(4e-3 * np.eye(d), adaptive=True, period=20)  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        dev = tda.sample(post, prop(), T, n_chains=64, seed=5, initial_parameters=list(theta0), backend="hip")
    assert dev["backend"] == "hip" and dev["sampler"] == "MH"
    for c in (0, 17, 63):
        link = dev["chain_%d" % c][-1]
        assert np.isclose(link.posterior, post.create_link(link.parameters).posterior, rtol=1e-10)
        assert np.isclose(link.likelihood, xlw.marginal(xm.np_forward(link.parameters, m), post.likelihood.data, post.likelihood.parameters)[0], rtol=1e-10)
    host = tda.sample(post, prop(), T, n_chains=8, seed=5, initial_parameters=list(theta0[:8]), backend="host", force_sequential=True)
    assert host["backend"] == "host"
    X = np.stack([tda.get_samples(dev, burnin=T // 2)["chain_%d" % c] for c in range(64)]).reshape(-1, d)
    H = np.stack([tda.get_samples(host, burnin=T // 2)["chain_%d" % c] for c in range(8)]).reshape(-1, d)
    rate = np.mean([np.mean(dev["chain_%d" % c].accepted[1:]) for c in range(64)])
    print("device acceptance %.3f, means %s against the host's %s, sd %s" % (rate, X.mean(axis=0), H.mean(axis=0), X.std(axis=0)))
    assert 0.1 <= rate <= 0.9
    assert np.all(np.abs(X.mean(axis=0) - H.mean(axis=0)) <= X.std(axis=0))


def test_sample_api_mala_and_delayed_acceptance():
    import tinyda_amd as tda

    d, m, N = 5, 23, 64
    post, theta0 = _posterior("ar1", d, m)
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(post, tda.MALA(0.14), 40, n_chains=N, seed=5, initial_parameters=list(theta0), backend="hip")
        coarse = tda.Posterior(post.prior, post.likelihood, tda.DeviceModel(xm.source(shift=0.004, coup=0.4), m,
                                                                            reference=lambda th: xm.np_forward(th, m, shift=0.004, coup=0.4)[0]))
        da = tda.sample([coarse, post], tda.GaussianRandomWalk(1e-3 * np.eye(d), adaptive=True, period=20), 40, n_chains=N, subchain_length=3, seed=5,
                        initial_parameters=list(theta0), backend="auto")
    assert res["backend"] == "hip" and da["backend"] == "hip" and da["sampler"] == "DA"
    for chains, name in ((res, "chain_%d"), (da, "chain_fine_%d")):
        for c in (0, 17, N - 1):
            link = chains[name % c][-1]
            assert np.isclose(link.posterior, post.create_link(link.parameters).posterior, rtol=1e-10)
        rate = np.mean([np.mean(chains[name % c].accepted[1:]) for c in range(N)])
        assert 0.05 < rate < 0.95


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_engine_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine
    from tinyda_amd.proposals import OperatorWeightedCrankNicolson

    d, m, N = 2, 3, 4
    y, par = np.array([0.1, 0.2, 0.3]), np.ones(m)
    src = full_source("ar1")

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

    # one form per likelihood; a comment does not make a form
    attempt(lambda e: e.set_level_source(0, src + xl.STUDENT_T_SRC, y, NOISE_SOURCE, par), "both tda_loglike_term and tda_loglike_wave", at_init=False)
    e = Engine(N, d, seed=1)
    try:
        e.set_prior(np.zeros(d), np.eye(d))
        e.set_level_source(0, src + "\n// tda_loglike_term(\n/* tda_loglike_term */\n", y, NOISE_SOURCE, par)
    finally:
        e.close()
    # the new rows of the diagnosis table
    attempt(lambda e: e.set_level_source(0, xm.source() + xlw.AR1_SRC.replace("int lane) {\n  double s", "int lane, int more) {\n  double s"), y, NOISE_SOURCE, par),
            r"tda_loglike_wave is not __device__ double tda_loglike_wave\(const double\* f, int n_outputs, const double\* y, const double\* p, int lane\)", at_init=False)
    attempt(lambda e: (e.set_level_source(0, xm.source() + xlw.without_grad(xlw.AR1_SRC), y, NOISE_SOURCE, par), e.set_proposal(6, None, scaling=0.1)),
            r"defines no __device__ void tda_loglike_grad_wave\(const double\* f, int n_outputs, const double\* y, const double\* p, double\* sens, int lane\)")
    # LDS over 64 KiB per chain, with the byte counts: the step program's outputs, and the MALA program's doubled buffer
    big = 8100
    yb, pb = np.zeros(big), np.ones(big)
    attempt(lambda e: e.set_level_source(0, src, yb, NOISE_SOURCE, pb), r"at most 64 KiB of LDS per chain: this source needs 1024 bytes .* \+ 64800 bytes for its 8100 outputs",
            at_init=False)
    work = xm.source() + "\n#define TDA_WORKSPACE 4500\n" + xwv_forward_stub() + xlw.AR1_SRC
    y2, p2 = np.zeros(2048), np.ones(2048)
    attempt(lambda e: (e.set_level_source(0, work, y2, NOISE_SOURCE, p2), e.set_proposal(6, None, scaling=0.1)),
            r"at most 64 KiB of LDS per chain: this source needs \d+ bytes .* \+ 32768 bytes for its 2048 outputs and their sensitivities")
    # every place where a separable DeviceLogLike is refused, with the same reason
    attempt(lambda e: e.set_level(0, np.ones((m, d)), y, NOISE_SOURCE, par), "source-defined likelihood", at_init=False)
    attempt(lambda e: e.set_level_callback(0, lambda th: np.zeros((len(th), m)), y, NOISE_SOURCE, par), "source-defined likelihood", at_init=False)
    attempt(lambda e: (e.set_level_source(0, src, y, NOISE_SOURCE, par), e.set_proposal_dreamz(M0=10)), "a source-defined likelihood under DREAM")
    attempt(lambda e: (e.set_level_source(0, src, y, NOISE_SOURCE, par), e.set_proposal(4, np.eye(d), q_mean=np.zeros(d))),
            "a source-defined likelihood under the Independence and operator-weighted pCN proposals is not lowered")
    ow = OperatorWeightedCrankNicolson(0.5 * np.eye(d), 0.5)._lowering()
    attempt(lambda e: (e.set_level_source(0, src, y, NOISE_SOURCE, par), e.set_proposal(**ow)), "operator-weighted")

    def two_levels(e):
        e.set_level_source(0, src, y, NOISE_SOURCE, par)
        e.set_level_source(1, src, y, NOISE_SOURCE, par)
        e.set_proposal(0, 0.01 * np.eye(d))

    attempt(lambda e: (two_levels(e), e.set_subchains([3], True)), "a source-defined likelihood with randomised subchain lengths is not lowered", n_levels=2)
    attempt(lambda e: (two_levels(e), e.set_subchains([3], False), e.set_error_model("state-independent")),
            "a source-defined likelihood together with an error model is not lowered", n_levels=2)
    attempt(lambda e: (two_levels(e), e.set_subchains([3], False), e.set_proposal_dreamz(M0=10)), "DREAM", n_levels=2)


def xwv_forward_stub():
    """a wave-form model that only claims workspace (the MALA program then holds s_th, the workspace and the doubled buffer)"""
    return ("__device__ void tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane) {\n"
            "  work[lane] = theta[0];\n  __syncthreads();\n  for (int o = lane; o < n_outputs; o += 64) out[o] = work[o & 63] + dim;\n}\n")


def test_sample_refusals_name_the_reason():
    import tinyda_amd as tda
    from tinyda_amd import _lib, api

    d, m = 2, 23
    post, theta0 = _posterior("ar1", d, m, grad=False)
    with pytest.raises(_lib.EngineError, match="tda_loglike_grad_wave"):
        tda.sample(post, tda.MALA(0.02), 5, n_chains=4, seed=5, initial_parameters=list(theta0[:4]), backend="hip")
    assert "tda_loglike_term_grad" not in api._refusal[0]
    full, _ = _posterior("ar1", d, m)
    start = dict(n_chains=4, seed=5, initial_parameters=list(theta0[:4]), backend="hip")
    grw_ = tda.GaussianRandomWalk(1e-3 * np.eye(d))
    for posts, prop, kw, reason in (
            (full, tda.DREAMZ(M0=10), {}, r"DeviceLogLike is not lowered under DREAM\(Z\)"),
            (full, tda.OperatorWeightedCrankNicolson(0.5 * np.eye(d), 0.5), {}, "DeviceLogLike is not lowered under OperatorWeightedCrankNicolson"),
            (full, tda.IndependenceSampler(st.multivariate_normal(theta0[0], 0.01 * np.eye(d))), {}, "DeviceLogLike is not lowered under IndependenceSampler"),
            ([full, full], grw_, dict(subchain_length=3, adaptive_error_model="state-independent"), "DeviceLogLike is not lowered together with an adaptive error model"),
            ([full, full], grw_, dict(subchain_length=3, randomize_subchain_length=True), "DeviceLogLike is not lowered with randomize_subchain_length"),
            ([full] * 5, grw_, dict(subchain_length=2), "DeviceLogLike: hierarchies of at most 4 levels"),
            ([full, full], tda.MALA(0.02), dict(subchain_length=3), "MALA with a DeviceLogLike: single level")):
        with pytest.raises(_lib.EngineError, match=reason):
            tda.sample(posts, prop, 5, **start, **kw)
