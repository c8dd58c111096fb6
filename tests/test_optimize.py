"""get_MAP / get_ML / maximize -- what needs no device: the two builds of the optimiser program compiled offline for gfx950 as hiprtc
compiles them, the build description (csrc/tda_user_build.h) through a stand-alone host program (tests/map_build_main.cpp, also
built with the address and undefined-behaviour sanitizers), the third ABI table, the NumPy twin of the kernel on the closed-form
problem and against scipy, the host route, and the twin over the starts of every case of tests/test_gpu_optimize.py."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import scipy.stats as st
from scipy.optimize import minimize

import tinyda_amd as tda

from . import extloglikewave as xlw
from . import extmodel as xm
from . import extoptimize as xo
from . import extprior as xp
from . import extpriorwave as xpw
from . import extwave as xw
from .extprogram import CSRC, ROOT, assert_switch_is_an_option_only, compile_program, needs_hipcc

SOURCE, DIFFERENCE = ["TDA_USER_MALA", "TDA_USER_MAP"], ["TDA_USER_MAP"]
KERNEL = ("tda_user_maximize",)
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_map.npz"))
GRADIENT_SIG = "__device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, int n_outputs, int j)"


def _family_source():
    return tda.DevicePrior.from_distributions(xp.components(5)).source


# ---- 1. the two builds, compiled offline as shipped ---------------------------------------------------------------------------------------
CASES = [  # name, user source, form switches of the source-gradient build, of the difference build, must take no scratch
    ("extmodel", xm.source(), [], [], True),
    ("ring_wave", xw.source(gradient="wave"), ["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE"], ["TDA_FORWARD_WAVE"], True),
    ("ar1", xm.source() + xlw.AR1_SRC, ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE"], ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE"], False),
    ("cauchy_difference", xm.source() + xpw.CAUCHY_DIFF_SRC, ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"], ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"], False),
    ("families", None, ["TDA_PRIOR_SOURCE"], ["TDA_PRIOR_SOURCE"], False),
]


@needs_hipcc
@pytest.mark.parametrize("name,user,source_switches,difference_switches,clean", CASES, ids=[c[0] for c in CASES])
def test_both_builds_hold_exactly_the_optimiser(tmp_path, name, user, source_switches, difference_switches, clean):
    """For extmodel and the ring's wave form: no scratch memory and no spilled vector register, in both builds.
    Measured (hipcc of ROCm 7, gfx950): neither in any of the ten programs.  The source-gradient build of the ring's wave form
    sits at the 256 vector registers of its gradient function (the same source's tda_user_mala_grad0 does too): with the
    log-densities, the scaling and the last gain carried in registers instead of LDS it spills one double."""
    user = xm.source() + _family_source() if user is None else user
    for build, switches in (("source", SOURCE + source_switches), ("difference", DIFFERENCE + difference_switches)):
        rc, log, usage = compile_program(tmp_path, build, user, switches)
        assert rc == 0, log[-3000:]
        assert set(usage) == set(KERNEL), usage
        print(name, build, usage["tda_user_maximize"])
        if clean:
            assert usage["tda_user_maximize"]["ScratchSize [bytes/lane]"] == 0 and usage["tda_user_maximize"]["VGPRs Spill"] == 0


@needs_hipcc
def test_missing_gradient_functions_name_their_signatures(tmp_path):
    rc, log, _ = compile_program(tmp_path, "no_gradient", xo.without_gradient(xm.source()), SOURCE)
    assert rc != 0 and "tda_gradient_missing" in log and GRADIENT_SIG in log
    rc, log, _ = compile_program(tmp_path, "no_loglike_grad", xm.source() + xlw.without_grad(xlw.AR1_SRC), SOURCE + ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE"])
    assert rc != 0 and "tda_loglike_grad_wave_missing" in log and xlw.GRAD_SIG in log
    rc, log, _ = compile_program(tmp_path, "no_prior_grad", xm.source() + xp.LOGNORMAL_SRC, SOURCE + ["TDA_PRIOR_SOURCE"])
    assert rc != 0 and "tda_logprior_term_grad_missing" in log
    # the difference build asks for none of them
    rc, log, usage = compile_program(tmp_path, "difference", xo.without_gradient(xm.source()) + xlw.without_grad(xlw.AR1_SRC) + xp.LOGNORMAL_SRC,
                                     DIFFERENCE + ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE", "TDA_PRIOR_SOURCE"])
    assert rc == 0 and set(usage) == set(KERNEL), log[-3000:]


def test_no_file_that_reaches_the_compiler_defines_the_new_switch():
    assert_switch_is_an_option_only(r"TDA_USER_MAP\b", ("tda_usermodel.inc", "tda_user_build.h", "tda_host_optimize.inc"))


# ---- 2. the build description, through the stand-alone program ----------------------------------------------------------------------------
CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    """tests/map_build_main.cpp, built once as it is and once with -fsanitize=address,undefined (a stand-alone program: the
    sanitizers' runtimes are linked in, nothing is preloaded); a sanitizer report ends the program with a non-zero status"""
    if CXX is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("map_build_" + request.param)
    exe = str(work / "tool")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    r = subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "map_build_main.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and request.param == "sanitized" and re.search(r"cannot find.*(asan|ubsan)", r.stdout):
        pytest.skip("the sanitizers' runtime libraries are not installed")
    assert r.returncode == 0, r.stdout[-3000:]
    count = iter(range(10000))

    def run(*args, text=None):
        if text is not None:
            path = work / ("input%d" % next(count))
            path.write_bytes(text.encode())
            args += (str(path),)
        return subprocess.run([exe] + [str(a) for a in args], check=True, stdout=subprocess.PIPE, text=True).stdout

    return run


def test_spec_options_and_lds(tool):
    base = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"]
    assert tool("options", 1, 0, 0, 0, 0, 0).split() == ["100"] + base + ["-DTDA_USER_MALA", "-DTDA_USER_MAP"]
    assert tool("options", 0, 0, 0, 0, 0, 0).split() == ["100"] + base + ["-DTDA_USER_MAP"]
    assert tool("options", 1, 1, 1, 1, 1, 2).split() == ["100"] + base + ["-DTDA_LOGLIKE_SOURCE", "-DTDA_LOGLIKE_WAVE", "-DTDA_USER_MALA", "-DTDA_USER_MAP", "-DTDA_PRIOR_SOURCE",
                                                                          "-DTDA_PRIOR_WAVE", "-DTDA_FORWARD_WAVE", "-DTDA_GRADIENT_WAVE"]
    assert tool("options", 0, 1, 0, 0, 0, 1).split() == ["100"] + base + ["-DTDA_USER_MAP", "-DTDA_PRIOR_SOURCE", "-DTDA_FORWARD_WAVE"]
    # dynamic LDS: the sensitivities over the source's gradient (twice under a coupled likelihood), the outputs of a wave form otherwise
    assert tool("lds", 1, 0, 0, 0, 70).split() == ["560", "18528"]
    assert tool("lds", 1, 0, 1, 1, 70).split() == ["1120", "18528"]
    assert tool("lds", 0, 0, 0, 0, 70).split() == ["0", "18528"]
    assert tool("lds", 0, 1, 0, 0, 70).split() == ["560", "18528"]
    assert tool("lds", 0, 0, 1, 1, 70).split() == ["560", "18528"]
    # the twin and the Python names use the kernel's constants
    assert tool("constants").split() == [str(xo.HISTORY), str(xo.HALVINGS), str(int(xo.FLOOR)), "012345"]
    assert tda.optimize.STATUS_NAMES[xo.INFEASIBLE_START] == "INFEASIBLE_START" and len(tda.optimize.STATUS_NAMES) == 6


@needs_hipcc
def test_diagnosis_of_real_compiler_logs(tool, tmp_path):
    rc, log, _ = compile_program(tmp_path, "no_gradient", xo.without_gradient(xm.source()), SOURCE)
    assert rc != 0
    out = tool("diagnose", 1, 0, 0, 23, text=log)
    assert out.startswith("-1\nthe optimiser over the source's gradient needs what MALA needs -- ") and out.endswith("the source defines no " + GRADIENT_SIG)
    # the difference build reads the step program's rows: a gradient's tag is none of them
    assert tool("diagnose", 0, 0, 0, 5, text="tda_gradient_missing").startswith("-1\nthe forward-model source does not compile with the optimiser: ")
    assert tool("diagnose", 1, 0, 0, 5, text="error: x") == "-1\nthe forward-model source does not compile with the optimiser over its gradient: error: x"
    rc, log, _ = compile_program(tmp_path, "no_term", xm.source(), DIFFERENCE + ["TDA_PRIOR_SOURCE"])
    assert rc != 0 and tool("diagnose", 0, 0, 1, 5, text=log).startswith("-1\na source-defined prior: the source defines no __device__ double tda_logprior_term(")


# ---- 3. the third ABI table ----------------------------------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyda_amd_optimize.h")).read(), flags=re.S)
    return set(re.findall(r"\b(tda_[a-z_]+)\s*\(", text))


def test_optimize_header_binding_and_library_agree():
    import ctypes as C

    import __graft_entry__ as g

    g.build()
    from tinyda_amd import _lib

    assert _declared() == set(_lib.OPTIMIZE_SYMBOLS) == {"tda_optimizer_create", "tda_optimizer_run", "tda_optimizer_destroy"}
    assert not set(_lib.OPTIMIZE_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.REPLAY_SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert _declared() <= set(re.findall(r"\bT (tda_[a-z_]+)", out))
    lib = _lib.load()
    assert len(lib.tda_optimizer_run.argtypes) == 9 and len(lib.tda_optimizer_create.argtypes) == 4
    assert C.sizeof(_lib.tda_optimize_problem) == 64 and C.sizeof(_lib.tda_optimize_options) == 24  # (the layouts of the header's structs)
    twin = _lib.load_from(g.CPU_ABI_SO)
    assert twin.tda_version() and not hasattr(twin, "tda_optimizer_create")
    assert tda.get_MAP is tda.optimize.get_MAP and tda.get_ML is tda.optimize.get_ML and tda.maximize is tda.optimize.maximize


# ---- 4. the twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["iso", "diag"])
@pytest.mark.parametrize("d,m,n", xo.CLOSED_FORM_SHAPES)
def test_twin_reaches_the_closed_form_mode(d, m, n, noise):
    case = xo.closed_form_case(d, m, n, noise)
    bound = xo.gradient_test_bound(case["H"], case["gtol"])
    for r in xo.run_twin(case):
        assert r["status"] == xo.CONVERGED_GRADIENT and r["grad_norm"] <= case["gtol"]
        assert np.linalg.norm(r["x"] - case["x_hat"]) <= bound
    assert np.allclose(case["twin"].gradient(case["x_hat"]), 0.0, atol=1e-10)


@pytest.fixture(scope="module")
def fixture_cases():
    return xo.fixture_posteriors()


@pytest.mark.parametrize("name", ["extmodel", "poisson_families", "ring"])
def test_twin_at_least_matches_scipy_l_bfgs_b(fixture_cases, name):
    case = fixture_cases[name]
    twin = case["twin"]
    for x0, r in zip(case["starts"], xo.run_twin(case)):
        ref = minimize(lambda x: -twin.value(x), x0, jac=lambda x: -twin.gradient(x), method="L-BFGS-B", options=dict(gtol=case["gtol"], ftol=0.0))
        print(name, "twin", r["value"], "scipy", -ref.fun)
        assert r["status"] == xo.CONVERGED_GRADIENT and r["value"] >= -ref.fun - 1e-10 * abs(ref.fun)


# ---- 5. the host route ---------------------------------------------------------------------------------------------------------------------
def _linear_posterior(dense_noise=False):
    rng = np.random.default_rng(3)
    d, m = 4, 9
    A = rng.standard_normal((m, d))
    y = A @ rng.standard_normal(d) + 0.1 * rng.standard_normal(m)
    cov = 0.04 * np.eye(m) + (0.01 if dense_noise else 0.0) * np.ones((m, m))
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(y, cov), tda.LinearModel(A))
    W = np.linalg.inv(cov)
    return post, np.linalg.solve(A.T @ W @ A + np.eye(d), A.T @ W @ y), np.linalg.solve(A.T @ W @ A, A.T @ W @ y)


def test_host_route_on_a_linear_model_against_the_closed_form():
    post, x_map, x_ml = _linear_posterior()
    with pytest.warns(tda.HostFallbackWarning, match="the device optimiser takes a DeviceModel"):
        got = tda.get_MAP(post, initial_parameters=np.zeros(4))
    assert got.shape == (4,) and np.allclose(got, x_map, atol=1e-5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.allclose(tda.get_ML(post, initial_parameters=np.zeros(4), backend="host"), x_ml, atol=1e-5)
        res = tda.maximize(post, n_starts=3, seed=4, backend="host")
        again = tda.maximize(post, n_starts=3, seed=4, backend="host")
    assert res.backend == "host" and res.x.shape == (3, 4) and np.array_equal(res.x, again.x) and np.allclose(res.x, x_map, atol=1e-5)
    assert np.allclose(res.value, res.logprior + res.loglike) and res.best == int(np.argmax(res.value))
    with pytest.raises(tda.EngineError, match="the device optimiser takes a DeviceModel"):
        tda.get_MAP(post, backend="hip")


def test_method_reaches_scipy():
    post, x_map, _ = _linear_posterior()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # an explicit method is the host route by choice: no warning
        got = tda.get_MAP(post, method="Nelder-Mead", initial_parameters=np.zeros(4), options=dict(xatol=1e-9, fatol=1e-12, maxiter=4000))
        bounded = tda.get_MAP(post, method="differential_evolution", bounds=[(-3, 3)] * 4, seed=1, tol=1e-10)
    assert np.allclose(got, x_map, atol=1e-6) and np.allclose(bounded, x_map, atol=1e-3)
    with pytest.raises(ValueError, match="Unknown solver"):
        tda.get_MAP(post, method="no-such-method", initial_parameters=np.zeros(4))


def test_dense_noise_goes_to_the_host_with_its_reason():
    m = 7
    model = tda.DeviceModel(xm.source(), m, reference=lambda x: xm.np_forward(x, m)[0])
    y = xm.np_forward(np.array([0.2, -0.1, 0.3]), m)[0]
    post = tda.Posterior(st.multivariate_normal(np.zeros(3), np.eye(3)), tda.GaussianLogLike(y, 0.01 * np.eye(m) + 0.001 * np.ones((m, m))), model)
    with pytest.warns(tda.HostFallbackWarning, match="a dense observation covariance is optimised on the host") as seen:
        x = tda.get_MAP(post, initial_parameters=np.zeros(3))
    assert len([w for w in seen if issubclass(w.category, tda.HostFallbackWarning)]) == 1 and x.shape == (3,)
    with pytest.raises(tda.EngineError, match="a dense observation covariance is optimised on the host"):
        tda.maximize(post, initial_parameters=np.zeros(3), backend="hip")
    dense_prior = tda.Posterior(st.multivariate_normal(np.zeros(3), np.eye(3) + 0.1), tda.GaussianLogLike(y, 0.01 * np.eye(m)), model)
    with pytest.raises(tda.EngineError, match="a dense prior covariance is optimised on the host"):
        tda.maximize(dense_prior, initial_parameters=np.zeros(3), backend="hip")
    # without a host reference the host route has nothing to call
    bare = tda.Posterior(post.prior, post.likelihood, tda.DeviceModel(xm.source(), m))
    with pytest.raises(TypeError, match="no host reference"):
        tda.get_MAP(bare, initial_parameters=np.zeros(3), backend="host")


@pytest.mark.parametrize("name", ["extmodel", "poisson_families", "ring"])
def test_host_route_at_least_the_references_value(fixture_cases, name):
    case = fixture_cases[name]
    assert np.array_equal(case["starts"], GOLDEN[name + "_starts"])
    ref = GOLDEN[name + "_logprior"] + GOLDEN[name + "_loglike"]
    # the reference's points evaluate to the recorded densities under this package's classes
    link = case["posterior"].create_link(GOLDEN[name + "_x"][0])
    assert np.isclose(link.prior, GOLDEN[name + "_logprior"][0], rtol=1e-12) and np.isclose(link.likelihood, GOLDEN[name + "_loglike"][0], rtol=1e-12)
    res = tda.maximize(case["posterior"], initial_parameters=case["starts"], backend="host", gtol=1e-7)
    print(name, "host", res.value, "reference", ref)
    assert np.all(res.value >= ref - 1e-10 * np.abs(ref))
    if name == "extmodel":
        ml = tda.maximize(case["posterior"], initial_parameters=case["starts"], objective="likelihood", backend="host", gtol=1e-7)
        assert np.all(ml.value >= GOLDEN["extmodel_ml_loglike"] - 1e-10 * np.abs(GOLDEN["extmodel_ml_loglike"]))


def test_arguments_are_checked():
    post, _, _ = _linear_posterior()
    for bad in (dict(objective="prior"), dict(gradient="adjoint"), dict(backend="cuda"), dict(gtol=-1.0), dict(max_iter=-1)):
        with pytest.raises(ValueError):
            tda.maximize(post, **bad)
    with pytest.raises(ValueError, match=r"\[d\], \[n, d\]"):
        tda.maximize(post, initial_parameters=np.zeros((2, 2, 4)), backend="host")


# ---- 6. the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------
def _all_converge(case):
    rows = xo.run_twin(case)
    d = case["starts"].shape[1]
    for i, r in enumerate(rows):
        assert r["status"] == xo.CONVERGED_GRADIENT and r["iterations"] < 200 * d, (i, r)
    return rows


@pytest.mark.parametrize("name", ["wave", "student_t", "ar1", "families", "cauchy_difference"])
def test_inputs_every_form(name):
    _all_converge(xo.form_cases()[name])


@pytest.mark.parametrize("name", ["extmodel", "joint_families"])
def test_inputs_forward_differences(name):
    case = xo.difference_cases()[name]
    for r in _all_converge(case):
        assert np.max(np.abs(case["twin"].gradient(r["x"]))) <= xo.difference_bound(case["twin"], r["x"], case["gtol"])
        assert r["evaluations"] >= (r["iterations"] + 1) * (case["starts"].shape[1] + 1)


def test_inputs_supports_and_nan():
    case = xo.support_case()
    rows = xo.run_twin(case)
    assert all(r["status"] == xo.CONVERGED_GRADIENT and np.all(r["x"] > 0.0) for r in rows[:-1])
    assert rows[-1]["status"] == xo.INFEASIBLE_START and np.array_equal(rows[-1]["x"], case["starts"][-1]) and rows[-1]["evaluations"] == 1
    assert all(r["status"] == xo.CONVERGED_GRADIENT for r in xo.run_twin(dict(case, objective="likelihood")))
    case = xo.nan_case()
    for r in xo.run_twin(case):
        assert r["status"] in (xo.LINESEARCH_FAILED, xo.MAX_ITER) and np.isfinite(r["value"]) and xo.NAN_ABOVE - 1e-6 < r["x"][0] <= xo.NAN_ABOVE


def test_inputs_two_modes():
    case = xo.two_modes_case()
    rows = _all_converge(case)
    which = [int(np.argmin(np.linalg.norm(case["modes"] - r["x"], axis=1))) for r in rows]
    assert set(which) == {0, 1}
    for r, k in zip(rows, which):
        assert np.linalg.norm(r["x"] - case["modes"][k]) <= 2.0 * xo.gradient_test_bound(case["H"][k], case["gtol"])
    assert all(np.linalg.eigvalsh(H)[0] > 0.0 for H in case["H"]) and all(np.max(np.abs(case["twin"].gradient(x))) < 1e-12 for x in case["modes"])
    assert case["twin"].value(case["modes"][1]) > case["twin"].value(case["modes"][0])


def test_value_test_is_off_at_ftol_zero_and_ends_a_start_otherwise():
    case = xo.closed_form_case(5, 70, 19, "iso")
    loose = xo.maximize_twin(case["twin"], case["starts"][0], gtol=0.0, ftol=1e-6)
    assert loose["status"] == xo.CONVERGED_VALUE and loose["iterations"] < 20
    capped = xo.maximize_twin(case["twin"], case["starts"][0], gtol=0.0, max_iter=3)
    assert capped["status"] == xo.MAX_ITER and capped["iterations"] == 3
