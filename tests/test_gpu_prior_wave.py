"""Priors that couple parameters on the device (TDA_PRIOR_WAVE: tda_logprior_wave of the level's source called by the chain's
whole wave in tda_user_steps and the MALA kernels, tda_logprior_grad under MALA): Philox forward mode against the oracle with
the NumPy twins of extpriorwave as the prior (single level, Delayed Acceptance / MLDA, MALA), a support that neighbours decide,
separable terms written in the wave form against the route through tda_logprior_term (bitwise) and the engine's own Gaussian
prior, the reference's chains replayed (g23), tda_engine_evaluate, checkpoint resume, the engine's refusals and
sample(backend='hip').

Every case that is compared with the oracle is conditioned on the oracle's acceptance rate lying in [0.1, 0.9]; the scalings
were chosen on the CPU with the oracle alone."""
import warnings

import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from . import extmodel as xm
from . import extprior as xp
from . import extpriorgrad as xg
from . import extpriorwave as xw
from . import extwave as xwv
from .extengine import (NOISE_SOURCE, PRIOR_SOURCE, assert_levels_resume_bitwise, assert_rate, assert_resume_bitwise, compare, compare_levels,
                        compare_replay, oracle_uniforms, run_forward, run_levels_forward, set_proposal)
from .extpriorwave import SIGMA2, level_of, make_engine
from .test_gpu_prior_source import HIER
from .test_prior_wave import G23, g23_prior, g23_proposal

pytestmark = pytest.mark.gpu

PRIORS = {"cauchy": xw.cauchy_difference, "tv": xw.total_variation, "hier": xw.hierarchical, "ordered": xw.ordered}


def grw(d, scaling, **kw):
    return dict(kind="grw", C=np.eye(d), scaling=scaling, **kw)


# ---- 1. Philox forward mode against the oracle -------------------------------------------------------------------------------------
# prior, d, m, N, proposal, block_steps, variant (None: extmodel's model under isotropic noise; "t": beside the Student-t
# DeviceLogLike; "wave": over extwave's wave-form model).  d = 1: no neighbour; 64 / 65: the difference term crosses from lane 63
# to lane 0's second parameter; N is no multiple of 16.
CASES = {
    "cauchy_d1_m1_grw": ("cauchy", 1, 1, 13, grw(1, 0.3), 0, None),
    "cauchy_d2_m23_grw_adaptive_split": ("cauchy", 2, 23, 19, grw(2, 0.05, adaptive=True, gamma=1.01, period=20), 33, None),
    "cauchy_d64_m70_grw": ("cauchy", 64, 70, 13, grw(64, 0.01), 0, None),
    "cauchy_d65_m70_am_split": ("cauchy", 65, 70, 19, dict(kind="am", C0=1e-4 * np.eye(65), t0=40, period=20), 16, None),
    "cauchy_d128_m300_grw_adaptive": ("cauchy", 128, 300, 13, grw(128, 0.004, adaptive=True, gamma=1.01, period=20), 0, None),
    "tv_d2_m1_am": ("tv", 2, 1, 13, dict(kind="am", C0=2e-2 * np.eye(2), t0=20, period=20), 0, None),
    "tv_d65_m70_grw_split": ("tv", 65, 70, 19, grw(65, 0.01), 33, None),
    "tv_d128_m23_am_adaptive": ("tv", 128, 23, 13, dict(kind="am", C0=1e-4 * np.eye(128), t0=40, period=20, adaptive=True, gamma=1.01), 0, None),
    "hier_d1_m1_grw": ("hier", 1, 1, 13, grw(1, 0.5), 0, None),
    "hier_d64_m23_am": ("hier", 64, 23, 19, dict(kind="am", C0=1.5e-3 * np.eye(64), t0=20, period=20), 0, None),
    "hier_d128_m70_grw_adaptive_split": ("hier", 128, 70, 13, grw(128, 0.008, adaptive=True, gamma=1.01, period=20), 16, None),
    "cauchy_d65_m23_student_loglike_grw": ("cauchy", 65, 23, 13, grw(65, 0.01), 0, "t"),
    "cauchy_d13_m47_wave_model_grw": ("cauchy", 13, 47, 13, grw(13, 0.02), 33, "wave"),
}


def case_inputs(case):
    """-> prior, N, proposal, block_steps, theta0, the engine's level tuple, the oracle level"""
    name, d, m, N, prop, bs, variant = CASES[case]
    prior = PRIORS[name](d)
    y, theta0 = xw.problem(prior, m, N, seed=d * 1000 + m)
    if variant == "t":
        par = 0.1 * (1.0 + 0.1 * np.arange(m) / m)
        level = xl.LogLikeLevel(lambda th: xm.np_forward(th, m), y, par, xl.KINDS["t"][1], prior)
        return prior, N, prop, bs, theta0, (xm.source() + xl.KINDS["t"][0], y, NOISE_SOURCE, par), level
    if variant == "wave":
        rng = np.random.default_rng(d * 1000 + m)
        truth, theta0 = xw.starts(prior, N, rng)
        y = xwv.np_forward(truth, m)[0] + np.sqrt(SIGMA2) * rng.standard_normal(m)
        level = orc.CallableGaussianLevel(lambda th: xwv.np_forward(th, m), y, "iso", SIGMA2, prior)
        return prior, N, prop, bs, theta0, (xwv.source("wave"), y, 0, SIGMA2), level
    return prior, N, prop, bs, theta0, (xm.source(), y, 0, SIGMA2), level_of(prior, m, y)


@pytest.mark.parametrize("case", list(CASES))
def test_philox_forward_matches_oracle(case):
    T = 120
    prior, N, prop, bs, theta0, lvl, level = case_inputs(case)
    params, stats, acc, scal, C, z, u = run_forward(make_engine(prior, N, [lvl], prop, bs), theta0, T, prop)
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    # (above 64 parameters the 128-term proposal sum puts its relative error into every increment; under AM the adapted factor does)
    compare(params, stats, acc, ref, scal, prior=prior, span_form=prior.dim > 64 or prop["kind"] == "am")
    if C is not None:
        np.testing.assert_allclose(C, ref["C"], rtol=1e-9, atol=1e-14)


# ---- 2. a support that neighbours decide -----------------------------------------------------------------------------------------------
def ordered_inputs(d, m, N, nan_above=None):
    prior = xw.ordered(d, nan_above)
    y, theta0 = xw.problem(prior, m, N, seed=404 + d)
    return prior, y, theta0


@pytest.mark.parametrize("d,scaling", [(5, 0.08), (65, 0.001)])
def test_proposals_that_break_the_order_are_rejected(d, scaling):
    N, T, m = 13, 120, 23
    prior, y, theta0 = ordered_inputs(d, m, N)
    prop = grw(d, scaling)
    assert np.all(prior.inside(theta0))
    params, stats, acc, _, _, z, u = run_forward(make_engine(prior, N, [(xm.source(), y, 0, SIGMA2)], prop), theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level_of(prior, m, y), prop, theta0, zz, uu)
    props = ref["theta"][:, :-1] + prop["scaling"] * zz
    broken = ~prior.ordered(props.reshape(-1, d)).reshape(N, T)
    print("oracle: %d of %d proposals break the order, acceptance %.3f" % (broken.sum(), broken.size, ref["accepted"][:, 1:].mean()))
    assert_rate(ref["accepted"][:, 1:])
    assert broken.sum() >= 1 and not np.any(ref["accepted"][:, 1:][broken])
    compare(params, stats, acc, ref, prior=prior, span_form=d > 64)
    assert np.all(np.isfinite(stats)) and np.all(prior.inside(params.reshape(-1, d)))


def test_start_outside_the_order_keeps_minus_inf_until_a_move_inside():
    N, T, d, m = 13, 60, 5, 23
    prior, y, theta0 = ordered_inputs(d, m, N)
    theta0 = theta0.copy()
    theta0[::2, 1] = theta0[::2, 0] - 0.01  # theta_1 < theta_0: inside every box, outside the support
    prop = grw(d, 0.03)
    e = make_engine(prior, N, [(xm.source(), y, 0, SIGMA2)], prop)
    e.init(theta0)
    assert np.all(e.current()[1][::2, 0] == -np.inf) and np.all(np.isfinite(e.current()[1][1::2, 0]))
    z, u = e.set_export(T)
    params, stats, acc = e.run_host(T)
    e.close()
    ref = orc.run_mh(level_of(prior, m, y), prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert np.all(ref["logprior"][::2, 0] == -np.inf) and np.all(np.isfinite(ref["logprior"][::2, -1]))
    assert np.array_equal(acc, np.swapaxes(ref["accepted"][:, 1:], 0, 1))
    got, want = stats[:, :, 0], np.swapaxes(ref["logprior"][:, 1:], 0, 1)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.all(got[~np.isfinite(want)] == -np.inf)
    np.testing.assert_allclose(got[np.isfinite(want)], want[np.isfinite(want)], rtol=1e-10)


def test_nan_share_rejects():
    """lane 0's share is NaN above a threshold in theta_0 that the chains start just below"""
    N, T, d, m = 13, 120, 5, 23
    prior, y, theta0 = ordered_inputs(d, m, N)
    prior = xw.ordered(d, nan_above=float(np.max(theta0[:, 0])) + 0.01)
    prop = grw(d, 0.03)
    params, stats, acc, _, _, z, u = run_forward(make_engine(prior, N, [(xm.source(), y, 0, SIGMA2)], prop), theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level_of(prior, m, y), prop, theta0, zz, uu)
    props = ref["theta"][:, :-1] + prop["scaling"] * zz
    is_nan = np.isnan(prior.logpdf(props.reshape(-1, d))).reshape(N, T)
    print("oracle: %d of %d proposals have a NaN log-prior" % (is_nan.sum(), is_nan.size))
    assert is_nan.sum() >= 1 and not np.any(ref["accepted"][:, 1:][is_nan])
    compare(params, stats, acc, ref, prior=prior)
    assert np.all(np.isfinite(stats)) and np.all(params[:, :, 0] <= prior.nan_above)


# ---- 3. the same bits as the separable route ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,prop,bs", [(5, 23, dict(kind="grw", C=4e-3 * np.eye(5), scaling=1.0, adaptive=True, gamma=1.01, period=20), 0),
                                         (96, 70, dict(kind="am", C0=1e-4 * np.eye(96), t0=40, period=20), 16)])
def test_separable_terms_in_wave_form_are_bitwise_the_separable_route(d, m, prop, bs):
    """the wave form that sums term(theta_j, p_j, q_j, j) over j = lane, lane + 64 does the operations of tda_user_steps'
    separable branch in their order: the records are equal bit for bit"""
    from tinyda_amd.engine import Engine

    N, T = 13, 120
    rng = np.random.default_rng(d)
    p, q = 0.1 * np.arange(d) / d, 0.5 + 0.01 * np.arange(d)
    theta0 = np.exp(p + 0.05 * rng.standard_normal((N, d)))
    y = xm.np_forward(np.exp(p), m)[0] + np.sqrt(SIGMA2) * rng.standard_normal(m)
    runs = []
    for psrc in (xp.LOGNORMAL_SRC, xw.wave_of_term(xp.LOGNORMAL_SRC)):
        e = Engine(N, d, seed=93, chain_offset=5, block_steps=bs)
        e.set_prior_joint(np.full(d, PRIOR_SOURCE), p, q)
        e.set_level_source(0, xm.source() + psrc, y, 0, SIGMA2)
        set_proposal(e, prop)
        e.init(theta0)
        runs.append(e.run_host(T) + (e.proposal_state_scaling(),))
        e.close()
    assert 0.1 <= runs[0][2].mean() <= 0.9
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("d,m,prop,bs", [(5, 23, dict(kind="grw", C=1e-3 * np.eye(5), scaling=1.0, adaptive=True, gamma=1.01, period=20), 0),
                                         (96, 300, dict(kind="am", C0=6e-5 * np.eye(96), t0=40, period=20), 16)])
def test_normal_wave_prior_matches_diagonal_gaussian_prior(d, m, prop, bs):
    """the normal term in wave form against the engine's own prior: the bar (and the cases) of
    test_gpu_prior_source.test_normal_device_prior_matches_diagonal_gaussian_prior"""
    from tinyda_amd.engine import Engine

    from .test_gpu_loglike_source import problem as gauss_problem

    N, T = 13, 120
    y, var, theta0, pm, pv = gauss_problem(d, m, "gauss", N, seed=d * 1000 + m)
    runs = []
    for src_prior in (False, True):
        e = Engine(N, d, seed=93, chain_offset=5, block_steps=bs)
        if src_prior:
            e.set_prior_joint(np.full(d, PRIOR_SOURCE), pm, np.sqrt(pv))
        else:
            e.set_prior(pm, np.diag(pv))
        e.set_level_source(0, xm.source() + (xw.wave_of_term(xp.NORMAL_SRC) if src_prior else ""), y, 1, var)
        set_proposal(e, prop)
        e.init(theta0)
        runs.append(e.run_host(T) + (e.proposal_state_scaling(),))
        e.close()
    (p0, s0, a0, c0), (p1, s1, a1, c1) = runs
    assert np.array_equal(a0, a1) and 0.1 <= a0.mean() <= 0.9
    np.testing.assert_allclose(s1[:, :, 0], s0[:, :, 0], rtol=1e-11)
    np.testing.assert_allclose(s1[:, :, 2], s0[:, :, 2], rtol=1e-11)
    np.testing.assert_allclose(p1, p0, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(c1, c0, rtol=1e-12)


# ---- 4. hierarchies -------------------------------------------------------------------------------------------------------------------
def hier_engine(case, N=16, seed=993):
    """the shapes, fidelities and subchains of test_gpu_prior_source.HIER under the Cauchy-difference prior.

    The data carry three times the modelled noise.  With the modelled noise the log-posterior passes through zero along the
    chains (the log-prior is about +20, from the -log(pi q_j) of thirteen narrow Cauchy terms, and the log-likelihood about
    -m / 2 and below), and a relative bar says nothing there: on the CPU the oracle's own log-posterior trace of mlda_am moves
    by 3.8e-9 of itself when theta0 changes by one part in 1e15, forty times the bar it is compared at.  With this data the
    log-posterior stays below -70 and the same perturbation moves the oracle's trace by 1.7e-12 (da_grw_adaptive: 7e-16)."""
    d, m, lv, sl, n_fine, prop, bs = HIER[case]
    prior = xw.cauchy_difference(d)
    y, theta0 = xw.problem(prior, m, N, seed=77 + d + m, noise=3.0)
    levels = [level_of(prior, m, y, sh, cp) for sh, cp in lv]
    e = make_engine(prior, N, [(xm.source(shift=sh, coup=cp), y, 0, SIGMA2) for sh, cp in lv], prop, bs, seed=seed, chain_offset=0, subchains=sl)
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


# ---- 5. MALA ------------------------------------------------------------------------------------------------------------------------------
def mala(scaling, adaptive=False):
    return dict(kind="mala", scaling=scaling, adaptive=adaptive, gamma=1.01, period=20)


# prior, d, m, N, proposal, block_steps
MALA_CASES = {
    "cauchy_d2_m23": ("cauchy", 2, 23, 13, mala(0.08), 0),
    "cauchy_d64_m70_split": ("cauchy", 64, 70, 19, mala(0.025), 33),
    "cauchy_d65_m70_adaptive": ("cauchy", 65, 70, 13, mala(0.02, True), 0),
    "cauchy_d128_m23": ("cauchy", 128, 23, 13, mala(0.02), 16),
    "hier_d2_m23": ("hier", 2, 23, 13, mala(0.07), 0),
    "hier_d64_m23": ("hier", 64, 23, 13, mala(0.1), 0),
    "hier_d65_m70_split": ("hier", 65, 70, 19, mala(0.08), 33),
    "hier_d128_m70": ("hier", 128, 70, 13, mala(0.06), 0),
}


def mala_inputs(case):
    name, d, m, N, prop, bs = MALA_CASES[case]
    prior = PRIORS[name](d)
    y, theta0 = xw.problem(prior, m, N, seed=d * 1000 + m)
    return prior, N, prop, bs, theta0, (xm.source(), y, 0, SIGMA2), xw.grad_level_of(prior, m, y)


@pytest.mark.parametrize("case", list(MALA_CASES))
def test_mala_matches_oracle(case):
    """against run_mh with the twin's gradient plus the model's vector-Jacobian product (the pattern of extpriorgrad).  The
    scalings keep the drift contractive: on the CPU oracle a relative perturbation of theta0 by 1e-14 leaves every accept mask
    as it is and moves the log-posterior trace by 6e-12 of itself at most (at d = 2 a scaling a quarter larger amplifies the same
    perturbation to 1e-8: both priors have directions of negative curvature)."""
    T = 120
    prior, N, prop, bs, theta0, lvl, level = mala_inputs(case)
    params, stats, acc, scal, _, z, u = run_forward(make_engine(prior, N, [lvl], prop, bs), theta0, T, prop)
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    compare(params, stats, acc, ref, scal, prior=prior, span_form=prior.dim > 64)


@pytest.mark.parametrize("grad_outside", ["0.0", '__builtin_nan("")', "__builtin_inf()", "-__builtin_inf()", "1e300"])
def test_mala_rejects_a_proposal_outside_whatever_the_gradient_returns(grad_outside):
    """the ordered prior is flat inside its support (the oracle's gradient is the model's) and tda_logprior_grad returns
    `grad_outside` outside it: whatever that is, the chains are the oracle's"""
    N, T, d, m = 13, 120, 5, 23
    prior, y, theta0 = ordered_inputs(d, m, N)
    prop = mala(0.06)
    e = make_engine(prior, N, [(xm.source(), y, 0, SIGMA2)], prop, source=xw.ordered_source(grad_outside=grad_outside))
    params, stats, acc, _, _, z, u = run_forward(e, theta0, T, prop)
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    level = xw.grad_level_of(prior, m, y)
    ref = orc.run_mh(level, prop, theta0, zz, uu)
    outside = xg.mala_proposals_outside(ref, prior, level, zz, prop)
    print("proposals outside the support: %d of %d" % (outside.sum(), outside.size))
    assert_rate(ref["accepted"][:, 1:])
    assert outside.sum() >= 1 and not np.any(ref["accepted"][:, 1:][outside])
    compare(params, stats, acc, ref, prior=prior)
    assert np.all(prior.inside(params.reshape(-1, d))) and np.all(np.isfinite(stats))


# ---- 6. the reference's chains ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G23)
def test_engine_replays_reference_chain(golden, name):
    g = golden(name)
    am = "C0" in g.files
    N, T1, d = g["theta"].shape
    prior, prop = g23_prior(g), g23_proposal(g)
    e = make_engine(prior, N, [(xm.source(), g["data"], 0, float(g["sigma2"]))], prop, seed=1, chain_offset=0)
    e.init(g["theta0"])
    e.set_replay(np.swapaxes(g["z"], 0, 1), np.swapaxes(g["u"], 0, 1))
    params, stats, acc = e.run_host(T1 - 1)
    state = e.proposal_state(want_am=am)
    e.close()
    compare_replay(params, stats, acc, g, logprior=True, **(dict(C=state["C"]) if am else dict(scaling=state["scaling"])))
    assert_rate(g["accepted"][:, 1:])


# ---- 7. tda_engine_evaluate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,m", [("cauchy", 65, 23), ("tv", 128, 70), ("hier", 64, 23), ("ordered", 5, 23), ("cauchy", 1, 1)])
def test_evaluate_against_numpy_twin(name, d, m):
    """the prior is set AFTER the level here, so the program is compiled again with the form the source has"""
    from tinyda_amd.engine import Engine

    N = 11
    prior = PRIORS[name](d)
    y, theta0 = xw.problem(prior, m, N, seed=d + m)
    e = Engine(N, d, seed=93)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, xm.source() + "\n" + prior.source, y, 0, SIGMA2)
    e.set_prior_joint(np.full(d, PRIOR_SOURCE), prior.p, prior.q)
    pts = theta0 + 0.05 * np.random.default_rng(2).standard_normal((N, d))
    pts[0] = theta0[0]
    got_before_init = e.evaluate(pts)
    e.set_proposal(0, 1e-3 * np.eye(d))
    e.init(theta0)
    got = e.evaluate(pts)
    e.close()
    lp, ll, _ = level_of(prior, m, y).evaluate(pts)
    fin = np.isfinite(lp)
    assert fin[0] and (name != "ordered" or np.any(~fin))
    assert np.array_equal(fin, np.isfinite(got[:, 0])) and np.all(got[~fin, 0] == -np.inf)
    assert np.all(np.abs(got[fin, 0] - lp[fin]) <= 1e-11 * prior.magnitude(pts[fin]))
    np.testing.assert_allclose(got[:, 1], ll, rtol=1e-11)
    assert np.array_equal(got, got_before_init)


# ---- 8. checkpoints ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cauchy_d65_m70_am_split", "mala:hier_d65_m70_split"])
def test_checkpoint_resume_is_bitwise(case):
    N = 11
    if case.startswith("mala:"):
        prior, _, prop, bs, _, lvl, _ = mala_inputs(case[5:])
    else:
        prior, _, prop, bs, _, lvl, _ = case_inputs(case)
    _, theta0 = xw.problem(prior, 1, N, seed=5)

    def make():
        e = make_engine(prior, N, [lvl], prop, bs)
        e.init(theta0)
        return e

    assert_resume_bitwise(make)


def test_hierarchy_checkpoint_resume_is_bitwise():
    assert_levels_resume_bitwise(hier_engine("da_grw_adaptive", 12, seed=77)[0])


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------
def test_engine_refusals():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    d, N = 2, 4
    y = np.array([0.1, 0.2, 0.3])
    src = xm.source() + xw.CAUCHY_DIFF_SRC
    no_grad = xm.source() + xw.CAUCHY_DIFF_SRC.split("__device__ double tda_logprior_grad")[0]
    kinds, p, q = np.full(d, PRIOR_SOURCE), np.zeros(d), np.ones(d)
    th0 = 0.1 * np.ones((N, d))
    e = Engine(N, d, seed=1)
    try:
        e.set_prior_joint(kinds, p, q)
        with pytest.raises(_lib.EngineError, match="both tda_logprior_term and tda_logprior_wave"):
            e.set_level_source(0, src + xp.LOGNORMAL_SRC, y, 0, SIGMA2)
        # a comment does not make a form
        e.set_level_source(0, src + "\n// tda_logprior_term(\n/* tda_logprior_term */\n", y, 0, SIGMA2)
        with pytest.raises(_lib.EngineError, match=r"tda_logprior_wave\(const double\* theta, int dim, const double\* p, const double\* q, int lane\)"):
            e.set_level_source(0, xm.source() + xw.CAUCHY_DIFF_SRC.replace("int lane)", "int lane, int more)"), y, 0, SIGMA2)
        e.set_level_source(0, no_grad, y, 0, SIGMA2)
        e.set_proposal(6, None, scaling=0.1)
        with pytest.raises(_lib.EngineError, match=r"source-defined prior under MALA needs __device__ double tda_logprior_grad\(const double\* theta"):
            e.init(th0)
        e.set_proposal(0, 0.01 * np.eye(d))
        e.init(th0)  # ... and the engine is still good for what is lowered
        assert np.all(np.isfinite(e.run_host(3)[1]))
        e.set_level_source(0, src, y, 0, SIGMA2)
        e.set_proposal(1, None, scaling=0.1)
        with pytest.raises(_lib.EngineError, match="source-defined prior under pCN"):
            e.init(th0)
        e.set_proposal(0, 0.01 * np.eye(d))
        with pytest.raises(_lib.EngineError, match="explicit initial parameters"):
            e.init(None)
        e.set_proposal_dreamz(M0=10)
        with pytest.raises(_lib.EngineError, match="source-defined prior under DREAM"):
            e.init(th0)
    finally:
        e.close()


# ---- 10. sample() ---------------------------------------------------------------------------------------------------------------------------
def _posteriors(prior, m, fidelities, seed=12):
    import tinyda_amd as tda

    y, _ = xw.problem(prior, m, 1, seed=seed)
    dp = xw.device_prior(prior)
    like = tda.GaussianLogLike(y, SIGMA2 * np.eye(m))
    return [tda.Posterior(dp, like, tda.DeviceModel(xm.source(shift=sh, coup=cp), m, reference=lambda th, sh=sh, cp=cp: xm.np_forward(th, m, shift=sh, coup=cp)[0],
                                                    reference_gradient=lambda th, s: xm.np_vjp(th, s)[0]))
            for sh, cp in fidelities]


def test_sample_api_single_level_am_with_starts_from_rvs():
    import tinyda_amd as tda
    from tinyda_amd import api

    d, m, N, T = 13, 23, 64, 60
    prior = xw.total_variation(d)
    (post,) = _posteriors(prior, m, [(0.0, 0.5)])
    assert post.prior.coupled and not hasattr(prior, "ppf")
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(post, tda.AdaptiveMetropolis(1e-3 * np.eye(d), t0=20, period=20), T, n_chains=N, seed=7, backend="hip", chain_offset=2)
    assert res["sampler"] == "MH" and res["backend"] == "hip" and res["n_chains"] == N
    starts = api._source_prior_starts(post.prior, N, 2, 7)
    assert np.array_equal(starts[5], prior.rvs(random_state=api._host_rng(7, api._TAG_THETA0, 7)))
    for c in (0, 17, N - 1):
        ch = res["chain_%d" % c]
        assert np.array_equal(ch[0].parameters, starts[c])
        link = ch[-1]
        assert abs(link.prior - prior.logpdf(link.parameters)) <= 1e-10 * prior.magnitude(link.parameters)[0]
        assert np.isclose(link.posterior, post.create_link(link.parameters).posterior, rtol=1e-10)
    rate = np.mean([np.mean(res["chain_%d" % c].accepted[1:]) for c in range(N)])
    assert 0.05 < rate < 0.95


def test_sample_api_delayed_acceptance():
    import tinyda_amd as tda

    d, m, N = 5, 23, 64
    prior = xw.cauchy_difference(d)
    posts = _posteriors(prior, m, [(0.004, 0.4), (0.0, 0.5)])
    _, theta0 = xw.problem(prior, m, N, seed=12)
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(posts, tda.GaussianRandomWalk(4e-3 * np.eye(d), adaptive=True, period=20), 40, n_chains=N, subchain_length=3, seed=5,
                         initial_parameters=list(theta0), backend="auto")
    assert res["sampler"] == "DA" and res["backend"] == "hip"
    for c in (0, 17, N - 1):
        link = res["chain_fine_%d" % c][-1]
        assert np.isclose(link.posterior, posts[1].create_link(link.parameters).posterior, rtol=1e-10)
    rate = np.mean([np.mean(res["chain_fine_%d" % c].accepted[1:]) for c in range(N)])
    assert 0.05 < rate < 0.95


def test_sample_api_mala():
    import tinyda_amd as tda

    d, m, N = 13, 23, 64
    prior = xw.cauchy_difference(d)
    (post,) = _posteriors(prior, m, [(0.0, 0.5)])
    _, theta0 = xw.problem(prior, m, N, seed=12)
    with warnings.catch_warnings():
        warnings.simplefilter("error", tda.HostFallbackWarning)
        res = tda.sample(post, tda.MALA(0.02), 40, n_chains=N, seed=5, initial_parameters=list(theta0), backend="hip")
    assert res["backend"] == "hip"
    for c in (0, 17, N - 1):
        link = res["chain_%d" % c][-1]
        assert np.isclose(link.posterior, post.create_link(link.parameters).posterior, rtol=1e-10)
    rate = np.mean([np.mean(res["chain_%d" % c].accepted[1:]) for c in range(N)])
    assert 0.05 < rate < 0.95


def test_sample_api_falls_back_with_one_warning_that_names_the_prior():
    """a proposal the coupled prior is closed to.  Under CrankNicolson the plan is refused with a reason that names DevicePrior,
    but sample() never gets as far as a fallback: like the reference (sampler.py:138-143) it raises TypeError for pCN over any
    prior that is no scipy multivariate normal.  The IndependenceSampler is refused for the same kind of reason and does fall
    back, with one HostFallbackWarning."""
    import scipy.stats as st

    import tinyda_amd as tda
    from tinyda_amd import api

    d, m, N = 3, 5, 2
    prior = xw.cauchy_difference(d)
    (post,) = _posteriors(prior, m, [(0.0, 0.5)])
    _, theta0 = xw.problem(prior, m, N, seed=12)
    assert api._device_plan([post], tda.CrankNicolson(0.05)) is None and "DevicePrior" in api._refusal[0] and "CrankNicolson" in api._refusal[0]
    with pytest.raises(TypeError, match="multivariate_normal for pCN"):
        tda.sample(post, tda.CrankNicolson(0.05), 10, n_chains=N, seed=5, initial_parameters=list(theta0), backend="auto", force_sequential=True)
    q = st.multivariate_normal(theta0[0], 0.01 * np.eye(d))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.IndependenceSampler(q), 10, n_chains=N, seed=5, initial_parameters=list(theta0), backend="auto", force_sequential=True)
    fb = [x for x in w if issubclass(x.category, tda.HostFallbackWarning)]
    assert len(fb) == 1 and "DevicePrior" in str(fb[0].message) and "IndependenceSampler" in str(fb[0].message)
    assert res["backend"] == "host" and len(res["chain_0"]) == 11
