"""Priors that couple parameters (DevicePrior with tda_logprior_wave / tda_logprior_grad, TDA_PRIOR_WAVE) without a device: the
validation of the source's form, the lowering rules, the host MALA over the reference gradient, the NumPy twins' gradients
against finite differences of their own logpdf, the host protocol and the oracle level against the reference's own chains
(tests/golden/g23_prior_coupled_*.npz, gen_golden_prior_coupled.py), and the hiprtc programs compiled offline for gfx950 with
the new switch -- and, without it, to the object they compiled to before."""
import os
import subprocess

import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from . import extmodel as xm
from . import extprior as xp
from . import extpriorwave as xw
from . import extwave as xwv
from .extengine import assert_host_classes_replay, assert_oracle_replays, golden_proposal as g23_proposal  # noqa: F401 (test_gpu_prior_wave)
from .extprogram import (CSRC, MALA_KERNELS, PROGRAM, STEP_KERNELS as KERNELS, assembly, assert_switch_is_an_option_only, assert_without_scratch,
                         compile_program as _compile, needs_hipcc)

G23 = ("g23_prior_coupled_grw", "g23_prior_coupled_am")
TWINS = {"cauchy": xw.cauchy_difference, "tv": xw.total_variation, "hier": xw.hierarchical, "ordered": xw.ordered}


def _posterior(prior, m=3, model="device", like=None):
    import tinyda_amd as tda

    if model == "device":
        mdl = tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0], reference_gradient=lambda t, s: xm.np_vjp(t, s)[0])
    elif model == "wave":
        mdl = tda.DeviceModel(xwv.source("wave", "wave"), m, reference=lambda t: xwv.np_forward(t, m)[0])
    elif model == "nograd":
        mdl = tda.DeviceModel(xm.source().split("__device__ double tda_gradient")[0], m)
    else:
        mdl = tda.LinearModel(np.ones((m, prior.dim)))
    return tda.Posterior(prior, tda.GaussianLogLike(np.zeros(m), 0.04 * np.eye(m)) if like is None else like, mdl)


def _without_grad(src):
    return src.split("__device__ double tda_logprior_grad")[0]


# ---- 1. DevicePrior ------------------------------------------------------------------------------------------------------------
def test_device_prior_says_which_form_its_source_has():
    import tinyda_amd as tda

    d = 4
    twin = xw.cauchy_difference(d)
    dp = xw.device_prior(twin)
    assert dp.coupled is True and dp.has_gradient is True
    assert tda.DevicePrior(_without_grad(xw.CAUCHY_DIFF_SRC), d).has_gradient is False
    sep = tda.DevicePrior(xp.LOGNORMAL_SRC, d)
    assert sep.coupled is False and sep.has_gradient is False
    # the separable form's gradient does not make a coupled prior's, nor the other way round
    assert tda.DevicePrior(_without_grad(xw.CAUCHY_DIFF_SRC) + "\n__device__ double tda_logprior_term_grad(double x, double p, double q, int j);", d).has_gradient is False
    assert tda.DevicePrior(xp.LOGNORMAL_SRC + "\n" + xw.GRAD_SIG + ";", d).has_gradient is False
    # comments do not count
    assert tda.DevicePrior(xp.LOGNORMAL_SRC + "// " + xw.WAVE_SIG + "\n/* tda_logprior_wave( */", d).coupled is False
    assert tda.DevicePrior(_without_grad(xw.CAUCHY_DIFF_SRC) + "// " + xw.GRAD_SIG + "\n/* tda_logprior_term( */", d).has_gradient is False
    with pytest.raises(ValueError, match="both tda_logprior_term and tda_logprior_wave"):
        tda.DevicePrior(xp.LOGNORMAL_SRC + xw.CAUCHY_DIFF_SRC, d)
    with pytest.raises(ValueError, match="tda_logprior_term") as exc:
        tda.DevicePrior("// " + xw.WAVE_SIG + "\n/* tda_logprior_wave( */", d)
    assert "tda_logprior_wave" in str(exc.value)
    # the host methods go through the reference: a coupled reference has rvs and no ppf
    th = twin.rvs(random_state=3)
    assert dp.logpdf(th) == twin.logpdf(th) and np.array_equal(dp.grad_logpdf(th), twin.grad(th))
    assert np.asarray(dp.rvs()).shape == (d,)
    with pytest.raises(TypeError, match="no host reference implementation of ppf"):
        dp.ppf(np.zeros(d))
    kinds, p, q, src = dp._source_lowering()
    assert np.all(kinds == 2) and np.array_equal(p, twin.p) and np.array_equal(q, twin.q) and src == xw.CAUCHY_DIFF_SRC


def test_source_prior_starts_draw_from_rvs_chain_by_chain():
    from tinyda_amd import api

    for name, make in TWINS.items():
        twin = make(6)
        dp = xw.device_prior(twin)
        a, b = api._source_prior_starts(dp, 3, 5, 1), api._source_prior_starts(dp, 1, 7, 1)
        assert np.array_equal(a[2], b[0]) and not np.array_equal(a[0], a[1]), name
        assert np.array_equal(a[1], twin.rvs(random_state=api._host_rng(1, api._TAG_THETA0, 6)))
        assert np.all(np.isfinite(twin.logpdf(np.stack(a)))), name
    with pytest.raises(TypeError, match="initial_parameters"):
        api._source_prior_starts(xw.device_prior(xw.hierarchical(3), reference=False), 2, 0, 1)


# ---- 2. lowering ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 65, 128])
def test_device_plan_single_level(d):
    import tinyda_amd as tda
    from tinyda_amd import _lib, api

    for name, make in TWINS.items():
        prior = xw.device_prior(make(d), reference=name != "tv")
        for model in ("device", "wave"):
            post = _posterior(prior, model=model)
            for prop, kind in ((tda.GaussianRandomWalk(np.eye(d)), 0), (tda.GaussianRandomWalk(np.eye(d), adaptive=True), 0),
                               (tda.AdaptiveMetropolis(np.eye(d)), 2), (tda.AdaptiveMetropolis(np.eye(d), adaptive=True), 2)):
                plan = api._device_plan([post], prop)
                assert plan is not None, api._refusal
                low = plan[0][0]
                assert plan[1]["kind"] == kind and np.all(low["prior_joint"][0] == _lib.PRIOR_SOURCE)
                assert np.array_equal(low["prior_joint"][1], prior.p) and np.array_equal(low["prior_joint"][2], prior.q)
                ps = low["prior_source"]
                assert ps["coupled"] is True and ps["has_gradient"] is True and ps["label"] == "DevicePrior" and ps["source"] == prior.source
                assert low["source"].index("tda_forward") < low["source"].index("tda_logprior_wave") and low["source"].endswith(prior.source)
    # a separable prior says so
    sep = tda.DevicePrior(xp.LOGNORMAL_SRC, d)
    assert api._device_plan([_posterior(sep)], tda.GaussianRandomWalk(np.eye(d)))[0][0]["prior_source"]["coupled"] is False
    assert api._device_plan([_posterior(tda.JointPrior(xp.components(d)))], tda.GaussianRandomWalk(np.eye(d)))[0][0]["prior_source"]["coupled"] is False
    # diagonal noise, and a DeviceLogLike: model, likelihood, prior
    m = 3
    prior = xw.device_prior(xw.cauchy_difference(d))
    diag = tda.GaussianLogLike(np.zeros(m), np.diag(0.04 + 0.01 * np.arange(m)))
    assert api._device_plan([_posterior(prior, like=diag)], tda.GaussianRandomWalk(np.eye(d))) is not None, api._refusal
    like = tda.DeviceLogLike(xl.STUDENT_T_SRC, np.zeros(m), np.ones(m))
    plan = api._device_plan([_posterior(prior, like=like)], tda.AdaptiveMetropolis(np.eye(d)))
    assert plan is not None, api._refusal
    s = plan[0][0]["source"]
    assert s.index("tda_forward") < s.index("tda_loglike_term") < s.index("tda_logprior_wave") and plan[0][0]["noise_kind"] == _lib.NOISE_SOURCE


def test_device_plan_hierarchies_and_mala():
    import tinyda_amd as tda
    from tinyda_amd import _lib, api

    d = 2
    prior = xw.device_prior(xw.cauchy_difference(d))
    grw, am = tda.GaussianRandomWalk(np.eye(d)), tda.AdaptiveMetropolis(np.eye(d))
    a, b = _posterior(prior, m=3), _posterior(prior, m=5)
    assert api._device_plan([a, b], grw) is not None, api._refusal
    assert api._device_plan([a, b, a], am) is not None, api._refusal
    assert api._device_plan([a, b, a, b], grw) is not None, api._refusal
    p96 = _posterior(xw.device_prior(xw.hierarchical(96)))
    assert api._device_plan([p96, p96], tda.GaussianRandomWalk(np.eye(96))) is not None, api._refusal
    other = xw.device_prior(xw.CauchyDifference(prior.p + 1.0, prior.q))
    assert api._device_plan([a, _posterior(other)], grw) is None and "share one prior" in api._refusal[0]
    # MALA: single level, with both gradients
    for dd in (2, 65, 128):
        pr = xw.device_prior(xw.hierarchical(dd))
        for adaptive in (False, True):
            plan = api._device_plan([_posterior(pr)], tda.MALA(0.05, adaptive=adaptive))
            assert plan is not None, api._refusal
            assert plan[1]["kind"] == _lib.PROP_MALA and plan[0][0]["prior_source"]["coupled"] and plan[0][0]["prior_source"]["has_gradient"]
    assert api._device_plan([_posterior(prior, model="wave")], tda.MALA(0.05)) is not None, api._refusal
    poisson = tda.DeviceLogLike(xl.POISSON_SRC, np.ones(3), np.ones(3))
    assert api._device_plan([_posterior(prior, like=poisson)], tda.MALA(0.05)) is not None, api._refusal


def test_device_plan_refusals():
    import scipy.stats as st

    import tinyda_amd as tda
    from tinyda_amd import api

    d = 2
    twin = xw.cauchy_difference(d)
    prior = xw.device_prior(twin)
    grw = tda.GaussianRandomWalk(np.eye(d))
    t = _posterior(prior)

    def refused(posts, prop, *needles, **kw):
        assert api._device_plan(posts, prop, **kw) is None
        for n in ("DevicePrior",) + needles:
            assert n in api._refusal[0], api._refusal

    refused([_posterior(prior, model="linear")], grw, "DeviceModel")
    refused([t, _posterior(prior, model="linear")], grw, "DeviceModel")
    refused([_posterior(prior, like=tda.GaussianLogLike(np.zeros(3), 0.04 * np.eye(3) + 0.01))], grw, "isotropic / diagonal noise")
    refused([t], tda.DREAMZ(M0=10), "DREAM(Z)")
    refused([t], tda.CrankNicolson(0.1), "CrankNicolson", "Gaussian prior")
    refused([t], tda.OperatorWeightedCrankNicolson(0.5 * np.eye(d), 0.5), "OperatorWeightedCrankNicolson")
    refused([t], tda.IndependenceSampler(st.multivariate_normal(np.zeros(d), np.eye(d))), "IndependenceSampler")
    refused([t, t], grw, "error model", error_model="state-independent")
    refused([t, t], grw, "randomize_subchain_length", randomize=True)
    refused([t] * 5, grw, "at most 4 levels")
    # MALA: the coupled form's own gradient is what is missing, and the reason names it
    no_grad = tda.DevicePrior(_without_grad(xw.CAUCHY_DIFF_SRC), d, twin.p, twin.q)
    refused([_posterior(no_grad)], tda.MALA(0.05), "MALA", "tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j)")
    assert "tda_logprior_term_grad" not in api._refusal[0]
    refused([_posterior(tda.DevicePrior(xp.LOGNORMAL_SRC, d))], tda.MALA(0.05), "MALA", "tda_logprior_term_grad")
    refused([t, t], tda.MALA(0.05), "MALA", "single level")
    refused([_posterior(prior, model="nograd")], tda.MALA(0.05), "MALA", "tda_gradient")
    big = xw.device_prior(xw.cauchy_difference(129))
    assert api._device_plan([_posterior(big)], tda.GaussianRandomWalk(np.eye(129))) is None and "128 parameters" in api._refusal[0]


def test_host_mala_takes_the_reference_gradient(monkeypatch):
    import scipy.optimize

    import tinyda_amd as tda

    d, m = 5, 7
    twin = xw.cauchy_difference(d)
    y, th = xw.problem(twin, m, 1, seed=2)
    post = tda.Posterior(xw.device_prior(twin), tda.GaussianLogLike(y, xw.SIGMA2 * np.eye(m)), _posterior(xw.device_prior(twin), m=m).model)

    def boom(*a, **k):
        raise AssertionError("finite differences")

    monkeypatch.setattr(scipy.optimize, "approx_fprime", boom)
    prop = tda.MALA(0.01)
    prop.setup_proposal(posterior=post)
    got = prop.compute_gradient(post.create_link(th[0]))
    level = xw.grad_level_of(twin, m, y)
    np.testing.assert_allclose(got, level.grad_logpost(th, level.forward(th))[0], rtol=1e-12)


# ---- 3. the twins ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cauchy", "tv", "hier", "ordered"])
@pytest.mark.parametrize("d", [1, 2, 65])
def test_twin_gradient_equals_finite_differences_of_its_logpdf(name, d):
    """central differences with h = 1e-6 on points whose neighbours differ by far more than h (so |x| has no kink inside a
    stencil): the truncation error is h^2 |f'''| / 6 and the rounding error eps |f| / h, both below 1e-6 (1 + |grad|) for the
    O(1) .. O(100) values of these priors"""
    twin = TWINS[name](d)
    rng = np.random.default_rng(d)
    _, th = xw.starts(twin, 4, rng, spread=0.02)
    if name == "tv" and d > 1:
        assert np.min(np.abs(np.diff(th, axis=1))) > 1e-4
    assert np.all(np.isfinite(twin.logpdf(th)))
    g, h = twin.grad(th), 1e-6
    fd = np.empty_like(th)
    for j in range(d):
        e = np.zeros(d)
        e[j] = h
        fd[:, j] = (twin.logpdf(th + e) - twin.logpdf(th - e)) / (2 * h)
    assert np.all(np.abs(g - fd) <= 1e-6 * (1.0 + np.abs(g))), np.max(np.abs(g - fd) / (1.0 + np.abs(g)))
    if name != "ordered":
        assert np.all(np.any(g != 0.0, axis=1))
    # magnitude bounds the density, and the single-point forms agree with the batched ones
    assert np.all(twin.magnitude(th) >= np.abs(twin.logpdf(th))) and twin.logpdf(th[0]) == twin.logpdf(th)[0]
    assert np.array_equal(twin.grad(th[0]), g[0]) and twin.rvs(random_state=1).shape == (d,) and twin.rvs(3, random_state=1).shape == (3, d)


def test_ordered_twin_support_and_nan():
    twin = xw.ordered(4, nan_above=0.5)
    th = np.array([[0.1, 0.2, 0.3, 0.4], [0.1, 0.3, 0.2, 0.4], [0.1, 0.2, 0.3, 1.2], [0.2, 0.2, 0.3, 0.4], [0.6, 0.7, 0.8, 0.9]])
    lp = twin.logpdf(th)
    assert lp[0] == -4 * np.log(1.25) and np.all(lp[1:4] == -np.inf) and np.isnan(lp[4])
    assert np.array_equal(twin.inside(th), [True, False, False, False, True]) and np.array_equal(twin.ordered(th), [True, False, True, False, True])
    assert np.all(twin.inside(twin.rvs(50, random_state=0)))


# ---- 4. host protocol and oracle level against the reference's chains ---------------------------------------------------------------
def g23_prior(g):
    name = str(g["prior"])
    return {"cauchy": xw.CauchyDifference, "ordered": xw.Ordered}[name](g["p"], g["q"])


@pytest.mark.parametrize("name", G23)
def test_host_classes_replay_reference_chain(golden, monkeypatch, name):
    import tinyda_amd as tda

    g = golden(name)
    m = g["data"].shape[0]
    post = tda.Posterior(xw.device_prior(g23_prior(g)), tda.GaussianLogLike(g["data"], float(g["sigma2"]) * np.eye(m)),
                         tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0]))
    assert post.prior.coupled and len(post.prior._source_lowering()) == 4
    assert_host_classes_replay(g, post, monkeypatch)


@pytest.mark.parametrize("name", G23)
def test_oracle_level_replays_reference_chain(golden, name):
    g = golden(name)
    m = g["data"].shape[0]
    prior = g23_prior(g)
    level = orc.CallableGaussianLevel(lambda t: xm.np_forward(t, m), g["data"], "iso", float(g["sigma2"]), prior)
    ref = assert_oracle_replays(g, level)
    np.testing.assert_allclose(ref["logprior"], g["logprior"], rtol=1e-10)
    assert g["theta"].shape[1] <= 201
    if str(g["prior"]) == "ordered":  # proposals leave the support, and no recorded state does
        assert int(g["n_outside"]) >= 1 and np.all(prior.inside(g["theta"].reshape(-1, prior.dim)))


# ---- 5. the programs with the new switch, compiled offline as shipped ----------------------------------------------------------------
SOURCES = {"cauchy": lambda: xw.CAUCHY_DIFF_SRC, "tv": lambda: xw.TV_SRC, "hier": lambda: xw.HIERARCHICAL_SRC, "ordered": lambda: xw.ordered_source(0.9)}
# model (+ likelihood) source, further switches of the step program, of the MALA program
MODELS = {
    "plain": (lambda: xm.source(), [], []),
    "student_loglike": (lambda: xm.source() + xl.KINDS["t"][0], ["TDA_LOGLIKE_SOURCE"], ["TDA_LOGLIKE_SOURCE"]),
    "wave_model": (lambda: xwv.source("wave", "wave"), ["TDA_FORWARD_WAVE"], ["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE"]),
}


@needs_hipcc
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("prior", list(SOURCES))
def test_wave_prior_programs_compile_for_gfx950_without_scratch(tmp_path, prior, model):
    """the step program and the MALA program (d is a run-time argument: one object serves d = 128): the kernel sets are what
    they were, none takes scratch or spills"""
    msrc, step_sw, mala_sw = MODELS[model]
    user = msrc() + "\n" + SOURCES[prior]()
    for name, switches, kernels in (("steps", step_sw, KERNELS), ("mala", mala_sw + ["TDA_USER_MALA"], MALA_KERNELS)):
        assert_without_scratch(tmp_path, name, user, ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"] + switches, kernels)


@needs_hipcc
def test_missing_functions_name_their_signatures(tmp_path):
    rc, log, _ = _compile(tmp_path, "no_wave", xm.source(), ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"])
    assert rc != 0 and "tda_logprior_wave_missing" in log and xw.WAVE_SIG in log
    # a separable source under the new switch: the term does not stand in for the wave form
    rc, log, _ = _compile(tmp_path, "term_only", xm.source() + xp.LOGNORMAL_SRC, ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"])
    assert rc != 0 and "tda_logprior_wave_missing" in log
    # another signature is not the contract's
    rc, log, _ = _compile(tmp_path, "other_sig", xm.source() + xw.CAUCHY_DIFF_SRC.replace("int lane)", "int lane, int more)"), ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"])
    assert rc != 0 and "tda_logprior_wave_missing" in log
    rc, log, _ = _compile(tmp_path, "no_grad", xm.source() + _without_grad(xw.CAUCHY_DIFF_SRC), ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE", "TDA_USER_MALA"])
    assert rc != 0 and "tda_logprior_grad_missing" in log and xw.GRAD_SIG in log and "tda_logprior_wave_missing" not in log
    # the step program asks for no gradient, and a wave source needs neither the term nor its derivative
    rc, log, _ = _compile(tmp_path, "steps_no_grad", xm.source() + _without_grad(xw.CAUCHY_DIFF_SRC), ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"])
    assert rc == 0 and "tda_logprior_term" not in log, log[-2000:]
    # the switch alone changes nothing: without TDA_PRIOR_SOURCE the Gaussian program compiles from a source with no prior at all
    rc, log, usage = _compile(tmp_path, "wave_switch_alone", xm.source(), ["TDA_PRIOR_WAVE"])
    assert rc == 0 and set(usage) == set(KERNELS), log[-2000:]


@needs_hipcc
@pytest.mark.parametrize("switches", [["TDA_PRIOR_SOURCE"], ["TDA_PRIOR_SOURCE", "TDA_USER_MALA"], []])
def test_without_the_switch_the_programs_are_the_parent_commits(tmp_path, switches):
    """over a separable prior (the lognormal with its gradient) the object of the program as shipped equals, byte for byte, the
    object of the parent commit's program text: the new code sits strictly behind -DTDA_PRIOR_WAVE"""
    root = os.path.dirname(os.path.dirname(CSRC))
    r = subprocess.run(["git", "show", "HEAD~:tinyda_amd/csrc/tda_user_program.hip"], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    if r.returncode != 0 or "tda_user_steps" not in r.stdout:
        pytest.skip("the parent commit's program text is not available (no git history here)")
    from .extpriorgrad import LOGNORMAL_GRAD_SRC

    user = xm.source() + xp.LOGNORMAL_SRC + LOGNORMAL_GRAD_SRC
    for name, text in (("mine", open(PROGRAM).read()), ("parent", r.stdout)):
        rc, log, _ = _compile(tmp_path, name, user, switches, text)
        assert rc == 0, log[-3000:]
    mine, parents = (tmp_path / "mine" / "program.out").read_bytes(), (tmp_path / "parent" / "program.out").read_bytes()
    assert len(mine) > 1000 and mine == parents


def test_program_text_never_defines_the_wave_switch():
    """the file and its headers never define the switch, and the public header does not name it (the host's option list:
    tests/test_user_build.py)"""
    header = assert_switch_is_an_option_only("TDA_PRIOR_WAVE", ("tda_prior_families.h", "tda_usermodel.inc", "tda_user_build.h"))
    assert "#ifdef TDA_PRIOR_WAVE" not in open(PROGRAM).read()
    assert xw.WAVE_SIG in header and xw.GRAD_SIG.split(";")[0] in header and "TDA_PRIOR_WAVE" not in header
    assert "couple components are not covered" not in header


@needs_hipcc
@pytest.mark.parametrize("mala", [False, True])
def test_the_wave_switch_alone_changes_no_instruction(tmp_path, mala):
    """every use of the switch is behind the prior switch: a program without -DTDA_PRIOR_SOURCE (the Gaussian prior) has the
    same instructions with and without -DTDA_PRIOR_WAVE"""
    switches = ["TDA_USER_MALA"] if mala else []
    assert assembly(tmp_path, "with", xm.source(), switches + ["TDA_PRIOR_WAVE"]) == assembly(tmp_path, "without", xm.source(), switches)
