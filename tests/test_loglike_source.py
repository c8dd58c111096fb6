"""Source-defined log-likelihoods (DeviceLogLike, TDA_NOISE_SOURCE) without a device: the host methods, the lowering
rules, the host protocol and the oracle level against the reference's own chains (tests/golden/g18_loglike_*.npz,
gen_golden_loglike_source.py), and the hiprtc programs assembled and compiled offline for gfx950."""
import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from .extengine import assert_host_classes_replay, assert_oracle_replays
from .extmodel import np_forward, np_vjp, source
from .extprogram import PROGRAM, assembly, assert_switch_is_an_option_only, assert_without_scratch, compile_program, needs_hipcc

G18 = {"g18_loglike_student_grw": "t", "g18_loglike_poisson_am": "poisson"}


def _loglike(kind, data, par, with_reference=True):
    import tinyda_amd as tda

    src, terms, grad = xl.KINDS[kind]
    return tda.DeviceLogLike(src, data, par, reference=terms if with_reference else None,
                             reference_gradient=grad if with_reference else None)


def _posterior(kind="t", d=2, m=3, model="device", prior=None, with_reference=True):
    import tinyda_amd as tda

    prior = st.multivariate_normal(np.zeros(d), np.eye(d)) if prior is None else prior
    data, par = (np.arange(m) % 3).astype(float), 1.0 + 0.1 * np.arange(m)
    if model == "device":
        mdl = tda.DeviceModel(source(), m, reference=lambda t: np_forward(t, m)[0], reference_gradient=lambda t, s: np_vjp(t, s)[0])
    elif model == "linear":
        mdl = tda.LinearModel(np.ones((m, d)))
    else:
        mdl = tda.BatchedModel(lambda th: np_forward(th, m), m)
    return tda.Posterior(prior, _loglike(kind, data, par, with_reference), mdl)


def _gauss_posterior(d=2, m=3, model="device"):
    import tinyda_amd as tda

    mdl = tda.DeviceModel(source(), m) if model == "device" else tda.LinearModel(np.ones((m, d)))
    return tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(np.zeros(m), 0.04 * np.eye(m)), mdl)


# ---- 1. host methods ----------------------------------------------------------------------------------------------------
def test_host_methods_against_closed_forms():
    import tinyda_amd as tda

    rng = np.random.default_rng(3)
    m = 7
    x, y, p = rng.standard_normal(m), rng.standard_normal(m), 0.5 + rng.random(m)
    lt = _loglike("t", y, p)
    # Student-t, nu = 4: log density up to its constant is -(nu + 1) / 2 log(1 + z^2 / nu)
    np.testing.assert_allclose(lt.loglike(x), np.sum(st.t.logpdf((x - y) / p, 4) - st.t.logpdf(0.0, 4)), rtol=1e-13)
    counts = rng.poisson(5.0, m).astype(float)
    lpo = _loglike("poisson", counts, p)
    from scipy.special import gammaln

    np.testing.assert_allclose(lpo.loglike(x), np.sum(st.poisson.logpmf(counts, p * np.exp(x)) + gammaln(counts + 1) - counts * np.log(p)), rtol=1e-12)
    lg = _loglike("gauss", y, p)
    np.testing.assert_allclose(lg.loglike(x), tda.GaussianLogLike(y, np.diag(p)).loglike(x), rtol=1e-14)
    np.testing.assert_allclose(lg.grad_loglike(x), tda.GaussianLogLike(y, np.diag(p)).grad_loglike(x), rtol=1e-14)
    # derivatives against central differences of the terms
    for kind, like in (("t", lt), ("poisson", lpo)):
        h = 1e-6
        fd = (xl.KINDS[kind][1](x + h, like.data, p) - xl.KINDS[kind][1](x - h, like.data, p)) / (2 * h)
        np.testing.assert_allclose(like.grad_loglike(x), fd, rtol=1e-6, atol=1e-8)
    # parameters default to ones; shapes are checked
    assert np.array_equal(tda.DeviceLogLike(xl.STUDENT_T_SRC, y).parameters, np.ones(m))
    with pytest.raises(ValueError):
        tda.DeviceLogLike(xl.STUDENT_T_SRC, y, np.ones(m + 1))
    with pytest.raises(ValueError, match="tda_loglike_term"):
        tda.DeviceLogLike("// __device__ double tda_loglike_term(double f, double y, double p, int o)", y)
    assert lt._lowering()[0] == 4 and np.array_equal(lt._lowering()[1], p)


def test_has_gradient_ignores_comments_and_missing_reference_raises():
    import tinyda_amd as tda

    assert tda.DeviceLogLike(xl.STUDENT_T_SRC, np.zeros(2)).has_gradient
    like = tda.DeviceLogLike(xl.TERM_ONLY_SRC, np.zeros(2))
    assert not like.has_gradient and not hasattr(like, "grad_loglike")  # host MALA: finite differences
    with pytest.raises(TypeError, match="no host reference implementation"):
        like.loglike(np.zeros(2))
    with pytest.raises(TypeError, match="no host reference implementation"):
        tda.DeviceModel(source(), 2)(np.zeros(2))  # (the same TypeError)


# ---- 2. lowering --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 96, 128])
def test_device_plan_single_level(d):
    import tinyda_amd as tda
    from tinyda_amd import api

    post = _posterior("t", d=d)
    for prop, kind in ((tda.GaussianRandomWalk(np.eye(d), adaptive=True), 0), (tda.CrankNicolson(0.1), 1),
                       (tda.AdaptiveMetropolis(np.eye(d)), 2), (tda.MALA(0.05), 6)):
        plan = api._device_plan([post], prop)
        assert plan is not None, api._refusal
        low = plan[0][0]
        assert plan[1]["kind"] == kind and low["noise_kind"] == 4 and low["loglike_source"]
        assert np.array_equal(low["noise"], post.likelihood.parameters)
        # one program: the model's source, then the likelihood's
        assert low["source"].index("tda_forward") < low["source"].index("tda_loglike_term")
    joint = tda.JointPrior([st.norm(0.0, 1.0)] * (d - 1) + [st.uniform(-1.0, 2.0)])
    assert api._device_plan([_posterior("poisson", d=d, prior=joint)], tda.GaussianRandomWalk(np.eye(d))) is not None


def test_device_plan_hierarchies():
    import tinyda_amd as tda
    from tinyda_amd import api

    grw, am = tda.GaussianRandomWalk(np.eye(2)), tda.AdaptiveMetropolis(np.eye(2))
    t, po = _posterior("t"), _posterior("poisson")
    assert api._device_plan([t, po], grw) is not None
    assert api._device_plan([_gauss_posterior(model="linear"), t], grw) is not None  # linear Gaussian coarse level
    assert api._device_plan([t, _gauss_posterior(model="linear")], tda.CrankNicolson(0.1)) is not None
    plan = api._device_plan([_gauss_posterior(), po, t], am)  # MLDA, mixed
    assert plan is not None and [lw["noise_kind"] for lw in plan[0]] == [0, 4, 4]
    assert api._device_plan([t, t, t, po], am) is not None
    p96 = _posterior("t", d=96)
    assert api._device_plan([p96, p96], tda.GaussianRandomWalk(np.eye(96))) is not None


def test_device_plan_refusals():
    import tinyda_amd as tda
    from tinyda_amd import api

    grw = tda.GaussianRandomWalk(np.eye(2))
    t = _posterior("t")

    def refused(posts, prop, *needles, **kw):
        assert api._device_plan(posts, prop, **kw) is None
        assert "DeviceLogLike" in api._refusal[0], api._refusal
        for n in needles:
            assert n in api._refusal[0], api._refusal

    refused([_posterior("t", model="linear")], grw, "DeviceModel")
    refused([_posterior("t", model="batched")], grw, "DeviceModel")
    refused([t, _posterior("t", model="linear")], grw, "DeviceModel")
    refused([t], tda.DREAMZ(M0=10), "DREAM(Z)")
    refused([t], tda.DREAM(M0=10), "DREAM(Z)")
    refused([t], tda.OperatorWeightedCrankNicolson(0.5 * np.eye(2), 0.5), "OperatorWeightedCrankNicolson")
    refused([t], tda.IndependenceSampler(st.multivariate_normal(np.zeros(2), np.eye(2))), "IndependenceSampler")
    refused([t, t], grw, "error model", error_model="state-independent")
    refused([t, t], grw, "error model", error_model="state-independent", diagonal_error_model=True)
    refused([t, t], grw, "randomize_subchain_length", randomize=True)
    refused([t] * 5, grw, "at most 4 levels")
    refused([tda.Posterior(t.prior, _loglike_term_only(), t.model)], tda.MALA(0.05), "tda_loglike_term_grad")
    refused([t, t], tda.MALA(0.05), "MALA")
    joint = tda.JointPrior([st.norm(0.0, 1.0), st.norm(0.0, 1.0)])
    refused([_posterior("t", prior=joint)], tda.MALA(0.05), "MALA")
    dense = st.multivariate_normal(np.zeros(2), np.array([[1.0, 0.3], [0.3, 1.0]]))
    refused([_posterior("t", prior=dense)], tda.MALA(0.05), "MALA")
    # a model source without tda_gradient: the existing rule, with its existing words
    from .test_mala_source import FORWARD_ONLY_SRC

    post = tda.Posterior(t.prior, _loglike("t", np.zeros(1), np.ones(1)), tda.DeviceModel(FORWARD_ONLY_SRC, 1))
    assert api._device_plan([post], tda.MALA(0.05)) is None and "tda_gradient" in api._refusal[0]
    assert api._device_plan([post], grw) is not None


def _loglike_term_only():
    import tinyda_amd as tda

    return tda.DeviceLogLike(xl.TERM_ONLY_SRC, (np.arange(3) % 3).astype(float))


def test_gaussian_posteriors_plan_as_before():
    import tinyda_amd as tda
    from tinyda_amd import api

    for model in ("device", "linear"):
        g = _gauss_posterior(model=model)
        plan = api._device_plan([g], tda.GaussianRandomWalk(np.eye(2)))
        low = plan[0][0]
        assert low["noise_kind"] == 0 and "loglike_source" not in low and "loglike_has_gradient" not in low
        if model == "device":
            assert low["source"] == g.model.source
        assert api._device_plan([g, g], tda.GaussianRandomWalk(np.eye(2)), error_model=None, randomize=True) is not None
    assert api._device_plan([_gauss_posterior()], tda.DREAMZ(M0=10)) is not None


def test_auto_backend_falls_back_with_one_warning():
    import warnings

    import tinyda_amd as tda
    from tinyda_amd.api import HostFallbackWarning

    post = _posterior("t", model="linear")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.GaussianRandomWalk(0.01 * np.eye(2)), 20, n_chains=2, seed=1, backend="auto", force_sequential=True)
    fb = [x for x in w if issubclass(x.category, HostFallbackWarning)]
    assert len(fb) == 1 and "DeviceLogLike" in str(fb[0].message)
    assert res["backend"] == "host" and len(res["chain_0"]) == 21
    with pytest.raises(tda.EngineError, match="DeviceLogLike"):
        tda.sample(post, tda.GaussianRandomWalk(0.01 * np.eye(2)), 20, n_chains=2, seed=1, backend="hip")


# ---- 3. host protocol against the reference's chains -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G18))
def test_host_class_replays_reference_chain(golden, monkeypatch, name):
    import tinyda_amd as tda

    g = golden(name)
    kind = G18[name]
    assert str(g["kind"]) == kind
    m = g["data"].shape[0]
    model = tda.DeviceModel(source(), m, reference=lambda t: np_forward(t, m)[0])
    post = tda.Posterior(st.multivariate_normal(g["prior_mean"], g["prior_cov"]), _loglike(kind, g["data"], g["par"]), model)
    assert_host_classes_replay(g, post, monkeypatch)


# ---- 4. the oracle level (which the GPU tests lean on) against the reference's chains ---------------------------------------
@pytest.mark.parametrize("name", list(G18))
def test_oracle_level_replays_reference_chain(golden, name):
    g = golden(name)
    kind = G18[name]
    m = g["data"].shape[0]
    level = xl.LogLikeLevel(lambda t: np_forward(t, m), g["data"], g["par"], xl.KINDS[kind][1], orc.MVNPrior(g["prior_mean"], g["prior_cov"]))
    assert_oracle_replays(g, level)


def test_oracle_level_gradient_against_differences():
    d, m = 4, 9
    rng = np.random.default_rng(5)
    theta = 0.3 * rng.standard_normal((3, d))
    y, p = rng.standard_normal(m), 0.5 + rng.random(m)
    for kind in ("t", "poisson"):
        _, terms, grad = xl.KINDS[kind]
        level = xl.LogLikeLevel(lambda t: np_forward(t, m), y, p, terms, orc.MVNPrior(np.zeros(d), np.eye(d)), grad)
        g = level.grad_logpost(theta, level.forward(theta))
        for j in range(d):
            e = np.zeros(d)
            e[j] = 1e-6
            lp1, ll1, _ = level.evaluate(theta + e)
            lp0, ll0, _ = level.evaluate(theta - e)
            np.testing.assert_allclose(g[:, j], ((lp1 + ll1) - (lp0 + ll0)) / 2e-6, rtol=1e-6, atol=1e-7)


# ---- 5. the hiprtc programs: the shipped file compiled offline as it stands, with the options the engine passes ---------------
PROGRAMS = {  # name -> (likelihood kind or None for the Gaussian program, MALA program?, kernels)
    "gauss_steps": (None, False, ("tda_user_steps", "tda_user_level_action", "tda_user_eval")),
    "gauss_mala": (None, True, ("tda_user_mala_steps", "tda_user_mala_grad0")),
    "t_steps": ("t", False, ("tda_user_steps", "tda_user_level_action", "tda_user_eval")),
    "t_mala": ("t", True, ("tda_user_mala_steps", "tda_user_mala_grad0")),
    "poisson_steps": ("poisson", False, ("tda_user_steps", "tda_user_level_action", "tda_user_eval")),
    "poisson_mala": ("poisson", True, ("tda_user_mala_steps", "tda_user_mala_grad0")),
}


@needs_hipcc
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_programs_compile_for_gfx950_without_scratch(tmp_path, name):
    kind, mala, kernels = PROGRAMS[name]
    user = source() + (xl.KINDS[kind][0] if kind else "")
    assert_without_scratch(tmp_path, name, user, (["TDA_LOGLIKE_SOURCE"] if kind else []) + (["TDA_USER_MALA"] if mala else []), kernels)


@needs_hipcc
def test_missing_functions_fail_with_a_message_naming_the_signature(tmp_path):
    rc, log, _ = compile_program(tmp_path, "no_term", source(), ["TDA_LOGLIKE_SOURCE"])
    assert rc != 0 and "tda_loglike_term_missing" in log
    assert "__device__ double tda_loglike_term(double f, double y, double p, int o)" in log
    rc, log, _ = compile_program(tmp_path, "no_term_mala", source(), ["TDA_LOGLIKE_SOURCE", "TDA_USER_MALA"])
    assert rc != 0 and "tda_loglike_term_missing" in log
    rc, log, _ = compile_program(tmp_path, "no_grad", source() + xl.TERM_ONLY_SRC, ["TDA_LOGLIKE_SOURCE", "TDA_USER_MALA"])
    assert rc != 0 and "tda_loglike_term_grad_missing" in log and "tda_loglike_term_missing" not in log
    assert "__device__ double tda_loglike_term_grad(double f, double y, double p, int o)" in log
    # the same source serves the step program, which needs no derivative
    rc, log, _ = compile_program(tmp_path, "term_only_steps", source() + xl.TERM_ONLY_SRC, ["TDA_LOGLIKE_SOURCE"])
    assert rc == 0, log[-2000:]


def test_gaussian_program_text_is_free_of_the_likelihood_switch():
    """kinds 0-3 are compiled without the switch: the program file and the header it includes never define TDA_LOGLIKE_SOURCE,
    and one place in the host code talks to hiprtc (its option list: tests/test_user_build.py)"""
    assert_switch_is_an_option_only("TDA_LOGLIKE_SOURCE")
    assert "#ifdef TDA_LOGLIKE_SOURCE" in open(PROGRAM).read()


@needs_hipcc
@pytest.mark.parametrize("mala", [False, True])
def test_gaussian_programs_do_not_see_a_likelihood_in_the_source(tmp_path, mala):
    """without -DTDA_LOGLIKE_SOURCE the instructions of a program are the same whether or not its source holds a tda_loglike_term"""
    switches = ["TDA_USER_MALA"] if mala else []
    assert assembly(tmp_path, "with_term", source() + xl.STUDENT_T_SRC, switches) == assembly(tmp_path, "without", source(), switches)
