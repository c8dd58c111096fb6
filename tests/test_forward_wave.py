"""Wave-cooperative forward models (tda_forward_wave / tda_gradient_wave) without a device: the test model's NumPy twin
(tests/extwave.py) and its adjoint, the oracle level over the twin against the reference's own chains
(tests/golden/g20_wave_*.npz, gen_golden_forward_wave.py), the DeviceModel flags, the lowering rules, and the shipped hiprtc
program compiled offline for gfx950 with the options the engine would pass."""
import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from . import extprior as xp
from . import extwave as xw
from .extengine import assert_oracle_replays
from .extprogram import (MALA_KERNELS, PROGRAM, STEP_KERNELS, assembly, assert_switch_is_an_option_only, assert_without_scratch,
                         compile_program as _compile, needs_hipcc)

G20 = ("g20_wave_grw", "g20_wave_am")
FORWARD_SIG = "__device__ void tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane)"
GRADIENT_SIG = ("__device__ void tda_gradient_wave(const double* theta, int dim, const double* sensitivity, int n_outputs, double* grad, "
                "double* work, int lane)")


# ---- 1. the twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,bound", [(5, 23, 3e-8), (96, 130, 6e-6)])
def test_twin_vjp_against_central_differences(d, m, bound):
    """the bounds are the noise of central differences of step 1e-6 on outputs of magnitude 1: rounding eps / step = 2e-10 per
    output, times the sum of |sens| over up to 130 outputs, plus the step's own h^2 error"""
    rng = np.random.default_rng(d + m)
    theta, sens = 0.5 * rng.standard_normal((3, d)), rng.standard_normal((3, m))
    for ksteps in (12, 48):
        g = xw.np_vjp(theta, sens, ksteps)
        for j in range(d):
            e = np.zeros(d)
            e[j] = 1e-6
            fd = ((xw.np_forward(theta + e, m, ksteps) - xw.np_forward(theta - e, m, ksteps)) * sens).sum(axis=1) / 2e-6
            assert np.max(np.abs(g[:, j] - fd)) <= bound, (ksteps, j, np.max(np.abs(g[:, j] - fd)))


@pytest.mark.parametrize("d,m", [(1, 1), (5, 23), (64, 64), (96, 130), (128, 300)])
def test_twin_properties(d, m):
    """every parameter moves some output (64 .. 127 through r alone), the outputs differ from one another, the state stays in
    (0, 1), and a last-bit change of the coefficients (the device's exp against libm's) does not grow along the solve"""
    rng = np.random.default_rng(7)
    theta = 0.5 * rng.standard_normal(d)
    F = xw.np_forward(theta, m)[0]
    assert np.all(np.isfinite(F)) and np.all((F > 0.0) & (F < 1.0)) and len(np.unique(F)) == m
    moved = [np.max(np.abs(xw.np_forward(theta + 1e-3 * np.eye(d)[j], max(m, 130))[0] - xw.np_forward(theta, max(m, 130))[0])) for j in range(d)]
    assert min(moved) > 1e-7, (np.argmin(moved), min(moved))
    F1 = xw.np_forward(np.nextafter(theta, np.inf), m)[0]
    assert np.max(np.abs(F1 - F)) <= 48 * np.finfo(float).eps  # (at most one rounding of an O(1) state apart per step, never amplified)


def test_twin_unwritten_and_nan_outputs():
    theta = np.array([[0.1, 0.2], [0.6, 0.2]])
    F = xw.np_forward(theta, 7, skip_last=True)
    assert np.all(np.isnan(F[:, 6])) and np.all(np.isfinite(F[:, :6]))
    F = xw.np_forward(theta, 7, nan_above=0.5)
    assert np.all(np.isfinite(F[0])) and np.all(np.isnan(F[1]))


# ---- 2. the oracle level over the twin (which the GPU tests lean on) against the reference's chains ---------------------------------
@pytest.mark.parametrize("name", G20)
def test_oracle_level_replays_reference_chain(golden, name):
    g = golden(name)
    m = g["data"].shape[0]
    assert g["theta0"].shape == (4, 5 if name == "g20_wave_grw" else 13) and m == (23 if name == "g20_wave_grw" else 100)
    level = orc.CallableGaussianLevel(lambda t: xw.np_forward(t, m), g["data"], "iso", float(g["sigma2"]), orc.MVNPrior(g["prior_mean"], g["prior_cov"]))
    assert_oracle_replays(g, level)
    assert g["theta"].shape[1] == 301


# ---- 3. DeviceModel ------------------------------------------------------------------------------------------------------------------
def test_device_model_flags():
    import tinyda_amd as tda

    wave = tda.DeviceModel(xw.source(), 23)
    assert wave.has_forward_wave and not wave.has_gradient_wave and not wave.has_gradient
    both = tda.DeviceModel(xw.source("both", "wave", m=23), 23)
    assert both.has_forward_wave and both.has_gradient_wave and both.has_gradient
    mixed = tda.DeviceModel(xw.source("wave", "per_parameter"), 23)
    assert mixed.has_forward_wave and not mixed.has_gradient_wave and mixed.has_gradient
    per_output = tda.DeviceModel(xw.source("per_output", m=23) + "// tda_forward_wave and /* tda_gradient_wave */ in comments do not count\n", 23)
    assert not per_output.has_forward_wave and not per_output.has_gradient_wave and not per_output.has_gradient
    with pytest.raises(ValueError, match="tda_forward_wave"):
        tda.DeviceModel("__device__ double model(const double* theta) { return 0.0; }", 1)
    assert "tda_forward_wave" in tda.DeviceModel.__doc__ and "tda_gradient_wave" in tda.DeviceModel.__doc__ and "TDA_WORKSPACE" in tda.DeviceModel.__doc__


def test_names_in_literals_and_longer_identifiers_do_not_count():
    """the flags come from whole identifiers outside comments, string literals and character literals (a '"' opens no string)"""
    import tinyda_amd as tda

    src = xw.source("per_output", m=23) + "__device__ char wv_quote() { return '\"'; }  // tda_forward_wave \" tda_gradient_wave\n" \
                                          "__device__ const char* wv_name() { return \"tda_forward_wave \\\" tda_gradient\"; }\n" \
                                          "__device__ double my_tda_gradient_wave_helper(double tda_gradient_scale) { return tda_gradient_scale; }\n"
    model = tda.DeviceModel(src, 23)
    assert not model.has_forward_wave and not model.has_gradient_wave and not model.has_gradient
    with pytest.raises(ValueError, match="tda_forward_wave"):  # tda_forward only as part of a longer name, in a comment and in a string
        tda.DeviceModel("__device__ double tda_forward_model(const double* theta) { return 0.0; }  // tda_forward\nconst char* s = \"tda_forward\";", 1)
    only_wave = tda.DeviceModel("__device__ void tda_forward_wave(const double* theta, int dim, double* out, int n, double* work, int lane) {}", 1)
    assert only_wave.has_forward_wave and not only_wave.has_gradient


# ---- 4. lowering: a wave model lowers wherever a DeviceModel does -----------------------------------------------------------------
def _posterior(d=5, m=23, forward="wave", gradient=None, ksteps=48, prior=None, like=None):
    import tinyda_amd as tda

    prior = st.multivariate_normal(np.zeros(d), np.eye(d)) if prior is None else prior
    like = tda.GaussianLogLike(np.zeros(m), 1e-4 * np.eye(m)) if like is None else like
    model = tda.DeviceModel(xw.source(forward, gradient, m=m, ksteps=ksteps), m, reference=lambda t: xw.np_forward(t, m, ksteps)[0],
                            reference_gradient=None if gradient is None else (lambda t, s: xw.np_vjp(t, s, ksteps)[0]))
    return tda.Posterior(prior, like, model)


@pytest.mark.parametrize("d", [5, 96])
def test_device_plan_single_level(d):
    import tinyda_amd as tda
    from tinyda_amd import api

    post = _posterior(d)
    for prop, kind in ((tda.GaussianRandomWalk(np.eye(d), adaptive=True), 0), (tda.CrankNicolson(0.1), 1), (tda.AdaptiveMetropolis(np.eye(d)), 2)):
        plan = api._device_plan([post], prop)
        assert plan is not None, api._refusal
        low = plan[0][0]
        assert plan[1]["kind"] == kind and low["has_forward_wave"] and not low["has_gradient_wave"] and low["source"] == post.model.source
    # a per-output model carries the flags too, unset
    low = api._device_plan([_posterior(d, forward="per_output")], tda.CrankNicolson(0.1))[0][0]
    assert not low["has_forward_wave"] and not low["has_gradient_wave"]


@pytest.mark.parametrize("forward", ["wave", "per_output"])
@pytest.mark.parametrize("gradient", ["wave", "per_parameter"])
def test_device_plan_mala(forward, gradient):
    import tinyda_amd as tda
    from tinyda_amd import api

    plan = api._device_plan([_posterior(forward=forward, gradient=gradient)], tda.MALA(0.05))
    assert plan is not None, api._refusal
    low = plan[0][0]
    assert plan[1]["kind"] == 6 and low["has_gradient"]
    assert low["has_forward_wave"] == (forward == "wave") and low["has_gradient_wave"] == (gradient == "wave")
    # without a gradient of either form: the existing rule, with its existing words
    assert api._device_plan([_posterior(forward=forward)], tda.MALA(0.05)) is None and "tda_gradient" in api._refusal[0]


def test_device_plan_hierarchy_dreamz_and_source_switches():
    import tinyda_amd as tda
    from tinyda_amd import api

    d, m = 5, 23
    posts = [_posterior(ksteps=k) for k in (12, 24, 48)]
    plan = api._device_plan(posts, tda.AdaptiveMetropolis(np.eye(d)))
    assert plan is not None and [lw["has_forward_wave"] for lw in plan[0]] == [True] * 3, api._refusal
    assert api._device_plan([posts[2]], tda.DREAMZ(M0=10)) is not None, api._refusal
    # beside a DeviceLogLike and a source-defined prior: one program, the model first
    like = tda.DeviceLogLike(xl.STUDENT_T_SRC, np.zeros(m), np.ones(m), reference=xl.KINDS["t"][1], reference_gradient=xl.KINDS["t"][2])
    joint = tda.JointPrior(xp.components(d, ("lognorm", "gamma", "beta", "norm", "uniform")))
    plan = api._device_plan([_posterior(prior=joint, like=like)], tda.AdaptiveMetropolis(np.eye(d)))
    assert plan is not None, api._refusal
    src = plan[0][0]["source"]
    assert src.index("tda_forward_wave") < src.index("tda_loglike_term") < src.index("tda_logprior_term")
    # refused wherever a DeviceModel is: five levels
    assert api._device_plan([posts[0]] * 5, tda.GaussianRandomWalk(np.eye(d))) is None


# ---- 5. the hiprtc program with the wave switches, compiled offline as shipped ------------------------------------------------------
def _user_source(name):
    if name == "steps_gauss":
        return xw.source()
    if name == "steps_student_t":
        return xw.source() + xl.KINDS["t"][0]
    if name == "steps_source_prior":
        import tinyda_amd as tda

        return xw.source() + xl.KINDS["t"][0] + "\n" + tda.JointPrior(xp.components(128))._source_lowering()[3]
    return xw.source(gradient="per_parameter" if name == "mala_forward_wave" else "wave")


PROGRAMS = {  # name -> (switches, kernels)
    "steps_gauss": (["TDA_FORWARD_WAVE"], STEP_KERNELS),
    "steps_student_t": (["TDA_FORWARD_WAVE", "TDA_LOGLIKE_SOURCE"], STEP_KERNELS),
    "steps_source_prior": (["TDA_FORWARD_WAVE", "TDA_LOGLIKE_SOURCE", "TDA_PRIOR_SOURCE"], STEP_KERNELS),
    "mala_forward_wave": (["TDA_FORWARD_WAVE", "TDA_USER_MALA"], MALA_KERNELS),
    "mala_both": (["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE", "TDA_USER_MALA"], MALA_KERNELS),
}


@needs_hipcc
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_wave_programs_compile_for_gfx950_without_scratch(tmp_path, name):
    """every program holds exactly its kernels, without scratch memory and without spilled vector registers (mala_forward_wave:
    the per-parameter tda_gradient over the trajectory that tda_forward_wave left, its tangent in a column of LDS per lane)"""
    switches, kernels = PROGRAMS[name]
    assert_without_scratch(tmp_path, name, _user_source(name), switches, kernels)


@needs_hipcc
def test_wrong_signatures_fail_with_a_message_naming_the_contract(tmp_path):
    no_work = xw.source().replace("tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane) {",
                                  "tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, int lane) {\n  double* work = out;")
    assert no_work != xw.source()
    rc, log, _ = _compile(tmp_path, "forward_without_work", no_work, ["TDA_FORWARD_WAVE"])
    assert rc != 0 and "tda_forward_wave_missing" in log and FORWARD_SIG in log
    # the switch without the function at all
    rc, log, _ = _compile(tmp_path, "no_forward_wave", xw.source("per_output", m=23), ["TDA_FORWARD_WAVE"])
    assert rc != 0 and "tda_forward_wave_missing" in log and FORWARD_SIG in log
    rc, log, _ = _compile(tmp_path, "no_gradient_wave", xw.source(gradient="per_parameter"), ["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE", "TDA_USER_MALA"])
    assert rc != 0 and "tda_gradient_wave_missing" in log and GRADIENT_SIG in log and "tda_forward_wave_missing" not in log
    # the wave form alone serves: no tda_forward, no tda_gradient
    rc, log, _ = _compile(tmp_path, "wave_only", xw.source(gradient="wave"), ["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE", "TDA_USER_MALA"])
    assert rc == 0, log[-2000:]
    # a source with both forms compiles either way
    both = xw.source("both", m=23)
    assert _compile(tmp_path, "both_wave", both, ["TDA_FORWARD_WAVE"])[0] == 0 and _compile(tmp_path, "both_per_output", both, [])[0] == 0


def test_program_text_never_defines_the_wave_switches():
    """a source without the wave functions is compiled without the switches, and its programs are what they were: the file and
    its header never define them (the host's option list and its scan of the source: tests/test_user_build.py)"""
    header = assert_switch_is_an_option_only(r"TDA_(FORWARD|GRADIENT)_WAVE\b")
    prog = open(PROGRAM).read()
    assert "#ifdef TDA_FORWARD_WAVE" in prog and "#ifdef TDA_GRADIENT_WAVE" in prog
    assert FORWARD_SIG in header and "TDA_WORKSPACE" in header and "64 KiB" in header


@needs_hipcc
def test_step_program_does_not_see_the_gradient_switch(tmp_path):
    """the step program calls no gradient: its instructions do not change under -DTDA_GRADIENT_WAVE"""
    from .extmodel import source

    assert assembly(tmp_path, "with", source(), ["TDA_GRADIENT_WAVE"]) == assembly(tmp_path, "without", source(), [])
