"""Likelihoods that couple outputs (DeviceLogLike with tda_loglike_wave / tda_loglike_grad_wave, TDA_LOGLIKE_WAVE) without a
device: the validation of the source's form, the lowering rules, the NumPy twins' gradients against finite differences of their
own log-likelihood in extended precision, the host protocol and the oracle level against the reference's own chains
(tests/golden/g24_loglike_coupled_*.npz, gen_golden_loglike_coupled.py), the fallback under backend='auto', the hiprtc programs
compiled offline for gfx950 with the new switch, and the build description (csrc/tda_user_build.h) for the new forms through a
stand-alone host program of its own."""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import scipy.stats as st

from . import extloglike as xl
from . import extloglikewave as xlw
from . import extmodel as xm
from . import extprior as xp
from . import extpriorwave as xpw
from . import extwave as xwv
from .extengine import assert_host_classes_replay, assert_oracle_replays
from .extprogram import CSRC, MALA_KERNELS, ROOT, STEP_KERNELS, assembly, assert_switch_is_an_option_only, assert_without_scratch, compile_program, needs_hipcc

G24 = ("g24_loglike_coupled_grw", "g24_loglike_coupled_am")
SOURCES = {"ar1": xlw.AR1_SRC, "marginal": xlw.MARGINAL_SRC, "softmax": xlw.SOFTMAX_SRC, "monotone": xlw.monotone_source(0.9), "t_wave": xlw.T_WAVE_SRC}


def _posterior(like, d=2, model="device", prior=None):
    import tinyda_amd as tda

    m = like.data.shape[0]
    if model == "device":
        mdl = tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0], reference_gradient=lambda t, s: xm.np_vjp(t, s)[0])
    elif model == "wave":
        mdl = tda.DeviceModel(xwv.source("wave", "wave"), m, reference=lambda t: xwv.np_forward(t, m)[0])
    elif model == "nograd":
        mdl = tda.DeviceModel(xm.source().split("__device__ double tda_gradient")[0], m)
    elif model == "batched":
        mdl = tda.BatchedModel(lambda th: xm.np_forward(th, m), m)
    else:
        mdl = tda.LinearModel(np.ones((m, d)))
    return tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)) if prior is None else prior, like, mdl)


def _like(kind="ar1", m=3, grad=True):
    y, par = 0.1 * np.arange(m) + (1.0 if kind == "softmax" else 0.0), np.ones(m)
    return xlw.device_loglike(kind, y, par, source=None if grad else xlw.without_grad(xlw.KINDS[kind][0]))


# ---- 1. DeviceLogLike ----------------------------------------------------------------------------------------------------------------
def test_device_loglike_says_which_form_its_source_has():
    import tinyda_amd as tda

    y = np.zeros(3)
    like = _like("ar1")
    assert like.coupled is True and like.has_gradient is True
    assert tda.DeviceLogLike(xlw.without_grad(xlw.AR1_SRC), y).has_gradient is False
    sep = tda.DeviceLogLike(xl.TERM_ONLY_SRC, y)
    assert sep.coupled is False and sep.has_gradient is False and tda.DeviceLogLike(xl.STUDENT_T_SRC, y).has_gradient is True
    # the separable form's derivative does not make a coupled likelihood's gradient, nor the other way round
    assert tda.DeviceLogLike(xlw.without_grad(xlw.AR1_SRC) + "\n__device__ double tda_loglike_term_grad(double f, double y, double p, int o);", y).has_gradient is False
    assert tda.DeviceLogLike(xl.TERM_ONLY_SRC + "\n" + xlw.GRAD_SIG + ";", y).has_gradient is False
    # comments do not count
    assert tda.DeviceLogLike(xl.STUDENT_T_SRC + "// " + xlw.WAVE_SIG + "\n/* tda_loglike_wave( */", y).coupled is False
    assert tda.DeviceLogLike(xlw.without_grad(xlw.AR1_SRC) + "// " + xlw.GRAD_SIG + "\n/* tda_loglike_term( */", y).has_gradient is False
    with pytest.raises(ValueError, match="both tda_loglike_term and tda_loglike_wave"):
        tda.DeviceLogLike(xl.STUDENT_T_SRC + xlw.AR1_SRC, y)
    with pytest.raises(ValueError, match="tda_loglike_term") as exc:
        tda.DeviceLogLike("// " + xlw.WAVE_SIG + "\n/* tda_loglike_wave( */", y)
    assert "tda_loglike_wave" in str(exc.value)
    # the host methods go through the reference: a scalar, or any array that sums to log L; the gradient is d log L / d F
    F = np.array([0.3, -0.2, 0.5])
    for kind in xlw.KINDS:
        lk = _like(kind)
        assert lk.loglike(F) == xlw.KINDS[kind][1](F, lk.data, lk.parameters)[0]
        assert np.array_equal(lk.grad_loglike(F), xlw.KINDS[kind][2](F, lk.data, lk.parameters)[0])
    scalar = tda.DeviceLogLike(xlw.MARGINAL_SRC, y, reference=lambda x, yy, pp: float(xlw.marginal(x, yy, pp)[0]))
    terms = tda.DeviceLogLike(xlw.AR1_SRC, y, reference=lambda x, yy, pp: xlw.ar1_terms(x, yy, pp))
    assert scalar.loglike(F) == xlw.marginal(F, y, np.ones(3))[0] and np.isclose(terms.loglike(F), xlw.ar1(F, y, np.ones(3))[0], rtol=1e-15)
    assert not hasattr(scalar, "grad_loglike")


# ---- 2. lowering -----------------------------------------------------------------------------------------------------------------------
def test_device_plan_carries_the_form():
    import tinyda_amd as tda
    from tinyda_amd import _lib, api

    for d in (1, 2, 65, 128):
        for kind in xlw.KINDS:
            for model in ("device", "wave"):
                post = _posterior(_like(kind), d, model)
                for prop, k in ((tda.GaussianRandomWalk(np.eye(d)), 0), (tda.GaussianRandomWalk(np.eye(d), adaptive=True), 0), (tda.CrankNicolson(0.1), 1),
                                (tda.AdaptiveMetropolis(np.eye(d)), 2)):
                    plan = api._device_plan([post], prop)
                    assert plan is not None, api._refusal
                    low = plan[0][0]
                    assert plan[1]["kind"] == k and low["noise_kind"] == _lib.NOISE_SOURCE and low["loglike_source"] is True
                    assert low["loglike_coupled"] is True and low["loglike_has_gradient"] is True
                    assert low["source"].index("tda_forward") < low["source"].index("tda_loglike_wave") and low["source"].endswith(post.likelihood.source)
    # a separable likelihood says so, and a coupled one without its gradient
    sep = tda.DeviceLogLike(xl.STUDENT_T_SRC, np.zeros(3))
    low = api._device_plan([_posterior(sep)], tda.GaussianRandomWalk(np.eye(2)))[0][0]
    assert low["loglike_coupled"] is False and low["loglike_has_gradient"] is True
    low = api._device_plan([_posterior(_like("ar1", grad=False))], tda.GaussianRandomWalk(np.eye(2)))[0][0]
    assert low["loglike_coupled"] is True and low["loglike_has_gradient"] is False
    # beside either form of a DevicePrior: model, likelihood, prior
    for prior in (xpw.device_prior(xpw.cauchy_difference(2)), tda.DevicePrior(xp.LOGNORMAL_SRC, 2)):
        plan = api._device_plan([_posterior(_like("marginal"), prior=prior)], tda.AdaptiveMetropolis(np.eye(2)))
        assert plan is not None, api._refusal
        s = plan[0][0]["source"]
        assert s.index("tda_forward") < s.index("tda_loglike_wave") < s.index("tda_logprior_")


def test_device_plan_hierarchies_and_mala():
    import tinyda_amd as tda
    from tinyda_amd import _lib, api

    d = 2
    a, b = _posterior(_like("ar1", 3)), _posterior(_like("marginal", 5))
    gauss = _posterior(tda.GaussianLogLike(np.zeros(3), 0.04 * np.eye(3)))
    grw, am = tda.GaussianRandomWalk(np.eye(d)), tda.AdaptiveMetropolis(np.eye(d))
    for posts, prop in (([a, b], grw), ([a, gauss], grw), ([gauss, b], am), ([a, b, a], am), ([a, b, gauss, b], grw)):
        assert api._device_plan(posts, prop) is not None, api._refusal
    for dd in (2, 65, 128):
        for kind in ("ar1", "marginal", "softmax", "t_wave"):
            for adaptive in (False, True):
                plan = api._device_plan([_posterior(_like(kind), dd)], tda.MALA(0.05, adaptive=adaptive))
                assert plan is not None, api._refusal
                assert plan[1]["kind"] == _lib.PROP_MALA and plan[0][0]["loglike_coupled"] and plan[0][0]["loglike_has_gradient"]
    assert api._device_plan([_posterior(_like("ar1", 2048))], tda.MALA(0.05)) is not None, api._refusal
    assert api._device_plan([_posterior(_like("ar1"), model="wave")], tda.MALA(0.05)) is not None, api._refusal
    assert api._device_plan([_posterior(_like("ar1"), prior=xpw.device_prior(xpw.cauchy_difference(d)))], tda.MALA(0.05)) is not None, api._refusal


def test_device_plan_refusals_are_the_separable_forms():
    """every place where a separable DeviceLogLike is refused refuses the coupled one with the same reason text; under MALA the
    missing function that the reason names is the coupled form's"""
    import tinyda_amd as tda
    from tinyda_amd import api

    d = 2
    grw = tda.GaussianRandomWalk(np.eye(d))
    coupled, separable = _like("ar1"), tda.DeviceLogLike(xl.STUDENT_T_SRC, np.zeros(3), reference=xl.t_terms, reference_gradient=xl.t_terms_grad)

    def reason(like, posts, prop, **kw):
        assert api._device_plan(posts(like), prop, **kw) is None
        return api._refusal[0]

    one = lambda model="device": (lambda like: [_posterior(like, d, model)])  # noqa: E731
    two = lambda like: [_posterior(like, d), _posterior(like, d)]  # noqa: E731
    for posts, prop, kw, needle in ((one("linear"), grw, {}, "DeviceModel"), (one("batched"), grw, {}, "DeviceModel"), (one(), tda.DREAMZ(M0=10), {}, "DREAM(Z)"),
                                    (one(), tda.OperatorWeightedCrankNicolson(0.5 * np.eye(d), 0.5), {}, "OperatorWeightedCrankNicolson"),
                                    (one(), tda.IndependenceSampler(st.multivariate_normal(np.zeros(d), np.eye(d))), {}, "IndependenceSampler"),
                                    (two, grw, dict(error_model="state-independent"), "error model"), (two, grw, dict(randomize=True), "randomize_subchain_length"),
                                    (lambda like: [_posterior(like, d)] * 5, grw, {}, "at most 4 levels"), (two, tda.MALA(0.05), {}, "single level"),
                                    (one("nograd"), tda.MALA(0.05), {}, "tda_gradient")):
        why = reason(coupled, posts, prop, **kw)
        assert needle in why and why == reason(separable, posts, prop, **kw), (why, needle)
    why = reason(_like("ar1", grad=False), one(), tda.MALA(0.05))
    assert "MALA" in why and xlw.GRAD_SIG.replace("__device__ void ", "") in why and "tda_loglike_term_grad" not in why
    why = reason(tda.DeviceLogLike(xl.TERM_ONLY_SRC, np.zeros(3)), one(), tda.MALA(0.05))
    assert "tda_loglike_term_grad(double f, double y, double p, int o)" in why and "tda_loglike_grad_wave" not in why
    assert "2048 outputs" in reason(_like("ar1", 2049), one(), tda.MALA(0.05))


def test_host_mala_takes_the_reference_gradient(monkeypatch):
    import scipy.optimize

    import tinyda_amd as tda

    d, m = 5, 7
    y, par, th, pm, pv = xlw.problem(d, m, "marginal", 1, seed=2)
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), xlw.device_loglike("marginal", y, par), _posterior(_like("ar1", m), d).model)

    def boom(*a, **k):
        raise AssertionError("finite differences")

    monkeypatch.setattr(scipy.optimize, "approx_fprime", boom)
    prop = tda.MALA(0.01)
    prop.setup_proposal(posterior=post)
    got = prop.compute_gradient(post.create_link(th[0]))
    level = xlw.level_of("marginal", m, y, par, pm, pv)
    np.testing.assert_allclose(got, level.grad_logpost(th, level.forward(th))[0], rtol=1e-12)


# ---- 3. the twins ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(xlw.KINDS))
@pytest.mark.parametrize("m", [1, 2, 65])
def test_twin_gradient_equals_finite_differences_of_its_loglike(kind, m):
    """central differences in long double (np.longdouble: 64 bits of mantissa on x86, which leaves eps |log L| / h = 1e-19 * 1e3 /
    1e-5 = 1e-11 of rounding) with h = 1e-5: the truncation error h^2 |f'''| / 6 is below 1e-7 (1 + |grad|) for these smooth
    functions of O(1) residuals.  Where long double is no wider than double the bar is 1e-5 instead (rounding 1e-16 * 1e3 / 1e-5)."""
    wide = np.finfo(np.longdouble).eps < 1e-18
    rng = np.random.default_rng(m)
    F = rng.standard_normal((3, m))
    y = rng.integers(1, 9, m).astype(float) if kind == "softmax" else F[0] + rng.standard_normal(m)
    p = 0.5 + rng.random(m)
    ll, grad = xlw.KINDS[kind][1], xlw.KINDS[kind][2]
    g, h = grad(F, y, p), np.longdouble(1e-5)
    like = xlw.device_loglike(kind, y, p)  # the twins are what the DeviceLogLike runs on the host
    assert like.coupled and like.loglike(F[1]) == ll(F, y, p)[1] and np.array_equal(like.grad_loglike(F[2]), g[2])
    Fl, yl, pl = F.astype(np.longdouble), y.astype(np.longdouble), p.astype(np.longdouble)
    fd = np.empty_like(F)
    for o in range(m):
        e = np.zeros(m, dtype=np.longdouble)
        e[o] = h
        fd[:, o] = ((ll(Fl + e, yl, pl) - ll(Fl - e, yl, pl)) / (2 * h)).astype(float)
    bar = 1e-7 if wide else 1e-5
    assert np.all(np.abs(g - fd) <= bar * (1.0 + np.abs(g))), np.max(np.abs(g - fd) / (1.0 + np.abs(g)))
    assert g.shape == F.shape and (kind == "softmax" and m == 1 or np.all(np.any(g != 0.0, axis=1)))


def test_monotone_twin_support_and_nan():
    import tinyda_amd as tda

    y, p = np.zeros(3), np.ones(3)
    F = np.array([[0.1, 0.2, 0.3], [0.1, 0.3, 0.2], [0.2, 0.2, 0.3], [0.95, 1.0, 1.1], [0.3, 0.2, 0.1]])
    ll = xlw.monotone(0.9)(F, y, p)
    like = tda.DeviceLogLike(xlw.monotone_source(0.9), y, p, reference=xlw.monotone(0.9))
    assert like.coupled and like.has_gradient and like.loglike(F[1]) == -np.inf and np.isnan(like.loglike(F[3])) and like.loglike(F[0]) == ll[0]
    assert ll[0] == xlw.ar1(F[:1], y, p)[0] and ll[1] == -np.inf and np.isfinite(ll[2]) and np.isnan(ll[3]) and ll[4] == -np.inf
    assert np.all(np.diff(xm.np_forward(xlw.MONOTONE_TRUTH, 3)[0]) > 0) and np.any(np.diff(xm.np_forward(xlw.MONOTONE_OUTSIDE, 3)[0]) < 0)
    # t_wave is the separable Student-t
    assert np.array_equal(xlw.t_wave(F, y, p), xl.t_terms(F, y, p).sum(axis=1))


# ---- 4. host protocol and oracle level against the reference's chains ------------------------------------------------------------------
def _g24_posterior(g):
    import tinyda_amd as tda

    m = g["data"].shape[0]
    assert str(g["kind"]) == "ar1"
    return tda.Posterior(st.multivariate_normal(g["prior_mean"], g["prior_cov"]), xlw.device_loglike("ar1", g["data"], g["par"]),
                         tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0]))


@pytest.mark.parametrize("name", G24)
def test_host_classes_replay_reference_chain(golden, monkeypatch, name):
    g = golden(name)
    post = _g24_posterior(g)
    assert post.likelihood.coupled
    assert_host_classes_replay(g, post, monkeypatch)


@pytest.mark.parametrize("name", G24)
def test_oracle_level_replays_reference_chain(golden, name):
    g = golden(name)
    m = g["data"].shape[0]
    ref = assert_oracle_replays(g, xlw.level_of("ar1", m, g["data"], g["par"], g["prior_mean"], np.diag(g["prior_cov"])))
    np.testing.assert_allclose(ref["loglike"], g["loglike"], rtol=1e-10)
    # ... and the level's likelihood is the DeviceLogLike's host side
    like = _g24_posterior(g).likelihood
    F = xm.np_forward(g["theta"][:, -1], m)
    np.testing.assert_allclose([like.loglike(f) for f in F], g["loglike"][:, -1], rtol=1e-10)
    assert g["theta"].shape[1] <= 201 and g["theta"].shape[0] <= 4


def test_sample_falls_back_to_the_host_protocol_with_one_warning():
    """a proposal the likelihood is closed to: backend='auto' runs the host protocol over the reference and says why, once"""
    import tinyda_amd as tda

    d, m, N = 2, 5, 2
    y, par, theta0, pm, pv = xlw.problem(d, m, "marginal", N, seed=12)
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), xlw.device_loglike("marginal", y, par),
                         tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0]))
    q = st.multivariate_normal(theta0[0], 0.01 * np.eye(d))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.IndependenceSampler(q), 10, n_chains=N, seed=5, initial_parameters=list(theta0), backend="auto", force_sequential=True)
    fb = [x for x in w if issubclass(x.category, tda.HostFallbackWarning)]
    assert len(fb) == 1 and "DeviceLogLike" in str(fb[0].message) and "IndependenceSampler" in str(fb[0].message)
    assert res["backend"] == "host" and len(res["chain_0"]) == 11
    link = res["chain_0"][-1]
    assert np.isclose(link.likelihood, xlw.marginal(xm.np_forward(link.parameters, m), y, par)[0], rtol=1e-12)


# ---- 5. the programs with the new switch, compiled offline as shipped ----------------------------------------------------------------
LIKE = ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE"]
# model source, further switches of the step program, of the MALA program
MODELS = {
    "per_output": (lambda: xm.source(), [], []),
    "wave_model": (lambda: xwv.source("wave", "wave"), ["TDA_FORWARD_WAVE"], ["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE"]),
    "wave_forward_only": (lambda: xwv.source("wave", "per_parameter"), ["TDA_FORWARD_WAVE"], ["TDA_FORWARD_WAVE"]),
    "wave_gradient_only": (lambda: xwv.source("per_output", "wave", m=23), [], ["TDA_GRADIENT_WAVE"]),
}


@needs_hipcc
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("like", list(SOURCES))
def test_wave_loglike_programs_compile_for_gfx950_without_scratch(tmp_path, like, model):
    """the step program and the MALA program (d and m are run-time arguments): the kernel sets are what they were, none takes
    scratch or spills.  (The per-output form of extwave's model keeps its state in scratch by design: tests/test_forward_wave.py;
    it is compiled here for its MALA program's wave gradient only, and its kernels are held to the kernel set alone.)"""
    msrc, step_sw, mala_sw = MODELS[model]
    user = msrc() + "\n" + SOURCES[like]
    if model == "wave_gradient_only":
        for name, switches, kernels in (("steps", step_sw, STEP_KERNELS), ("mala", mala_sw + ["TDA_USER_MALA"], MALA_KERNELS)):
            rc, log, usage = compile_program(tmp_path, name, user, LIKE + switches)
            assert rc == 0 and set(usage) == set(kernels), log[-2000:]
        return
    for name, switches, kernels in (("steps", step_sw, STEP_KERNELS), ("mala", mala_sw + ["TDA_USER_MALA"], MALA_KERNELS)):
        assert_without_scratch(tmp_path, name, user, LIKE + switches, kernels)


@needs_hipcc
@pytest.mark.parametrize("prior", ["term", "wave"])
def test_wave_loglike_beside_a_source_prior_compiles_without_scratch(tmp_path, prior):
    from .extpriorgrad import LOGNORMAL_GRAD_SRC

    psrc, psw = (xp.LOGNORMAL_SRC + LOGNORMAL_GRAD_SRC, ["TDA_PRIOR_SOURCE"]) if prior == "term" else (xpw.CAUCHY_DIFF_SRC, ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"])
    user = xm.source() + xlw.MARGINAL_SRC + psrc
    assert_without_scratch(tmp_path, "steps", user, LIKE + psw, STEP_KERNELS)
    assert_without_scratch(tmp_path, "mala", user, LIKE + psw + ["TDA_USER_MALA"], MALA_KERNELS)


@needs_hipcc
def test_missing_functions_name_their_signatures(tmp_path):
    rc, log, _ = compile_program(tmp_path, "no_wave", xm.source(), LIKE)
    assert rc != 0 and "tda_loglike_wave_missing" in log and xlw.WAVE_SIG in log
    # a separable source under the new switch: the term does not stand in for the wave form
    rc, log, _ = compile_program(tmp_path, "term_only", xm.source() + xl.STUDENT_T_SRC, LIKE)
    assert rc != 0 and "tda_loglike_wave_missing" in log
    rc, log, _ = compile_program(tmp_path, "other_sig", xm.source() + xlw.AR1_SRC.replace("int lane) {\n  double s", "int lane, int more) {\n  double s"), LIKE)
    assert rc != 0 and "tda_loglike_wave_missing" in log
    rc, log, _ = compile_program(tmp_path, "no_grad", xm.source() + xlw.without_grad(xlw.AR1_SRC), LIKE + ["TDA_USER_MALA"])
    assert rc != 0 and "tda_loglike_grad_wave_missing" in log and xlw.GRAD_SIG in log and "tda_loglike_wave_missing" not in log
    # the step program asks for no gradient, and a wave source needs neither the term nor its derivative
    rc, log, _ = compile_program(tmp_path, "steps_no_grad", xm.source() + xlw.without_grad(xlw.AR1_SRC), LIKE)
    assert rc == 0 and "tda_loglike_term" not in log, log[-2000:]


def test_program_text_never_defines_the_switch_and_the_documents_state_the_contract():
    header = assert_switch_is_an_option_only("TDA_LOGLIKE_WAVE", ("tda_usermodel.inc", "tda_user_build.h"))
    assert xlw.WAVE_SIG in header and xlw.GRAD_SIG in header and "couple outputs are not covered" not in header
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "tda_loglike_wave" in readme and "couple outputs are not covered" not in readme
    import tinyda_amd as tda

    assert "tda_loglike_wave" in tda.DeviceLogLike.__doc__ and "not covered" not in tda.DeviceLogLike.__doc__


@needs_hipcc
@pytest.mark.parametrize("switches", [[], ["TDA_USER_MALA"], ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"]])
def test_the_wave_switch_alone_changes_no_instruction(tmp_path, switches):
    """every use of the switch is behind the likelihood switch: a program without -DTDA_LOGLIKE_SOURCE (Gaussian noise) has the same
    instructions with and without -DTDA_LOGLIKE_WAVE"""
    user = xm.source() + (xpw.CAUCHY_DIFF_SRC if switches and switches[0] == "TDA_PRIOR_SOURCE" else "")
    assert assembly(tmp_path, "with", user, switches + ["TDA_LOGLIKE_WAVE"]) == assembly(tmp_path, "without", user, switches)
    # ... and behind it the switch selects the form: a source with the wave form alone compiles with both switches only
    rc, log, _ = compile_program(tmp_path, "both", user + xlw.T_WAVE_SRC, switches + LIKE)
    assert rc == 0, log[-2000:]
    rc, log, _ = compile_program(tmp_path, "source_only", user + xlw.T_WAVE_SRC, switches + LIKE[:1])
    assert rc != 0 and "tda_loglike_term_missing" in log


# ---- 6. the build description for the new forms, through a stand-alone host program of its own ---------------------------------------------
CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
MAIN = r"""
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "tda_user_build.h"

static std::string slurp(const char* path) {
  std::ifstream in(path, std::ios::binary);
  std::stringstream ss;
  ss << in.rdbuf();
  return ss.str();
}
int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "forms" && argc == 3) {
    const UserForms f = user_forms(slurp(argv[2]).c_str());
    std::cout << f.loglike_term << f.loglike_wave << f.loglike_grad_wave << " " << f.both_loglike_forms() << " " << f.both_prior_forms() << "\n";
  } else if (cmd == "options" && argc == 5) {
    UserProgramSpec s, t;
    s.mala = atoi(argv[2]), s.loglike_source = atoi(argv[3]), s.loglike_wave = atoi(argv[4]);
    t = s;
    t.loglike_wave = !s.loglike_wave;
    std::cout << (s == s) << (s == t);
    for (const char* o : user_program_options(s)) std::cout << " " << o;
    std::cout << "\n";
  } else if (cmd == "diagnose" && argc == 4) {
    UserProgramSpec s;
    s.mala = atoi(argv[2]), s.loglike_source = true, s.loglike_wave = true;
    const UserBuildError err = diagnose_user_build(slurp(argv[3]), s, 23);
    std::cout << err.code << "\n" << err.message;
  } else {
    return 2;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("loglike_wave_build")
    (work / "main.cpp").write_text(MAIN)
    exe = str(work / "tool")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe, str(work / "main.cpp")], check=True)
    count = iter(range(1000))

    def run(*args, text=None):
        if text is not None:
            path = work / ("input%d" % next(count))
            path.write_bytes(text.encode())
            args += (str(path),)
        return subprocess.run([exe] + [str(a) for a in args], check=True, stdout=subprocess.PIPE, text=True).stdout

    return run


def test_build_description_of_the_new_forms(tool):
    assert tool("forms", text=xm.source() + xlw.AR1_SRC).split() == ["011", "0", "0"]
    assert tool("forms", text=xm.source() + xlw.without_grad(xlw.AR1_SRC)).split() == ["010", "0", "0"]
    assert tool("forms", text=xm.source() + xl.STUDENT_T_SRC).split() == ["100", "0", "0"]
    assert tool("forms", text=xm.source() + xl.STUDENT_T_SRC + xlw.MARGINAL_SRC).split() == ["111", "1", "0"]
    assert tool("forms", text=xm.source() + "// tda_loglike_term tda_loglike_wave\n/* tda_loglike_grad_wave */").split() == ["000", "0", "0"]
    base = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"]
    assert tool("options", 0, 1, 1).split() == ["10"] + base + ["-DTDA_LOGLIKE_SOURCE", "-DTDA_LOGLIKE_WAVE"]
    assert tool("options", 1, 1, 1).split() == ["10"] + base + ["-DTDA_LOGLIKE_SOURCE", "-DTDA_LOGLIKE_WAVE", "-DTDA_USER_MALA"]
    assert tool("options", 0, 1, 0).split() == ["10"] + base + ["-DTDA_LOGLIKE_SOURCE"]
    assert tool("options", 0, 0, 1).split() == ["10"] + base  # (the form means nothing without a source-defined likelihood)


@needs_hipcc
def test_diagnosis_of_real_compiler_logs(tool, tmp_path):
    rc, log, _ = compile_program(tmp_path, "other_sig", xm.source() + xl.STUDENT_T_SRC, LIKE)
    assert rc != 0
    assert tool("diagnose", 0, text=log) == "-1\na source-defined likelihood: the source's tda_loglike_wave is not " + xlw.WAVE_SIG
    rc, log, _ = compile_program(tmp_path, "no_grad", xm.source() + xlw.without_grad(xlw.MARGINAL_SRC), LIKE + ["TDA_USER_MALA"])
    assert rc != 0
    assert tool("diagnose", 1, text=log) == "-1\nMALA with a source-defined likelihood that couples outputs: the source defines no " + xlw.GRAD_SIG
    # static LDS beyond the hardware's: the dynamic buffer quoted beside it is the program's own, doubled under MALA
    lds = "error: local memory (241024) exceeds limit (163840) in function 'tda_user_mala_steps'"
    assert tool("diagnose", 1, text=lds).endswith("more than the 163840 bytes of the hardware, before the 368 bytes for its 23 outputs and their sensitivities")
    assert tool("diagnose", 0, text=lds).endswith("more than the 163840 bytes of the hardware, before the 184 bytes for its 23 outputs")
    # the MALA row does not apply to the step program
    assert tool("diagnose", 0, text="tda_loglike_grad_wave_missing").startswith("-1\nthe forward-model source does not compile: ")
