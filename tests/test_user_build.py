"""The HIP-free part of a source-defined program's build (csrc/tda_user_build.h), through a stand-alone host program
(tests/user_build_main.cpp, built here with the system C++ compiler): the scan for the contract's identifiers against Python's
_defines, the option list of every spec, the reading of real compiler logs (tests/extprogram.py), the "both forms" decision."""
import itertools
import os
import shutil
import subprocess

import pytest

from . import extloglike as xl
from . import extmodel as xm
from . import extprior as xp
from . import extpriorwave as xpw
from . import extwave as xw
from .extprogram import CSRC, ROOT, compile_program, needs_hipcc

CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
pytestmark = pytest.mark.skipif(CXX is None, reason="no C++ compiler")

STRING_SRC = xp.LOGNORMAL_SRC + '__device__ const char* note() { return "see tda_logprior_wave(...)"; }\n'
ALIAS_SRC = (xpw.CAUCHY_DIFF_SRC.split("__device__ double tda_logprior_grad")[0] + "#define G tda_logprior_grad\n"
             "__device__ double G(const double* theta, int dim, const double* p, const double* q, int j) { return 0.0; }\n")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    work = tmp_path_factory.mktemp("user_build")
    exe = str(work / "user_build")
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "user_build_main.cpp")], check=True)
    count = itertools.count()

    def run(*args, text=None):
        if text is not None:
            path = work / ("input%d" % next(count))
            path.write_bytes(text.encode())
            args += (str(path),)
        return subprocess.run([exe] + [str(a) for a in args], check=True, stdout=subprocess.PIPE, text=True).stdout

    return run


SCANS = [  # (what, source, name, defined?)
    ("line comment", "double x;  // tda_forward_wave(\n", "tda_forward_wave", False),
    ("block comment", "/* tda_logprior_wave( \n */ double x;", "tda_logprior_wave", False),
    ("string with an escaped quote", 'const char* s = "a \\" tda_gradient_wave(";', "tda_gradient_wave", False),
    ("character literal", "int c = 'tda_forward_wave';", "tda_forward_wave", False),
    ("a quote in a character literal opens no string", "char q = '\"'; double tda_forward_wave; char r = '\"';", "tda_forward_wave", True),
    ("prefix of a longer identifier", "double tda_logprior_term_grad(double x);", "tda_logprior_term", False),
    ("the longer identifier itself", "double tda_logprior_term_grad(double x);", "tda_logprior_term_grad", True),
    ("suffix of a longer identifier", "double my_tda_gradient(double x);", "tda_gradient", False),
    ("whitespace and a newline before the parenthesis", "double tda_forward_wave \t\n  (double x);", "tda_forward_wave", True),
    ("no parenthesis at all", "#define G tda_logprior_grad\n", "tda_logprior_grad", True),
    ("unterminated block comment", "double x; /* tda_forward_wave(", "tda_forward_wave", False),
    ("unterminated string", 'const char* s = "tda_forward_wave(', "tda_forward_wave", False),
    ("a backslash at the end of an unterminated string", '"tda_forward \\', "tda_forward", False),
    ("after a closed block comment", "/* a */ tda_forward /* b", "tda_forward", True),
    ("a separable prior that names the wave form in a string", STRING_SRC, "tda_logprior_wave", False),
    ("... and defines the term", STRING_SRC, "tda_logprior_term", True),
    ("a coupled prior whose gradient is a macro alias", ALIAS_SRC, "tda_logprior_grad", True),
]


@pytest.mark.parametrize("what,source,name,defined", SCANS, ids=[s[0] for s in SCANS])
def test_scan_is_the_same_in_the_engine_and_in_python(tool, what, source, name, defined):
    from tinyda_amd.models import _defines

    assert tool("scan", name, text=source).strip() == str(int(defined))
    assert _defines(source, name) is defined


def test_signatures_are_the_same_in_the_engine_and_in_python(tool):
    """TDA_SIG_* of csrc/tda_user_args.h against tinyda_amd._contract.SIG; tda_forward has no macro"""
    from tinyda_amd._contract import SIG

    printed = dict(ln.split("\t") for ln in tool("signatures").splitlines())
    assert printed == {name: text for name, text in SIG.items() if name != "tda_forward"} and len(printed) == 11
    assert all(text.startswith("__device__ ") and " %s(" % name in text for name, text in SIG.items())


def test_python_classes_decide_as_the_engine_does(tool):
    """the two sources on which the classes used to disagree with the engine"""
    import tinyda_amd as tda

    sep = tda.DevicePrior(STRING_SRC, 3)
    assert sep.coupled is False and tool("forms", text=STRING_SRC).split() == ["001000", "0"]
    alias = tda.DevicePrior(ALIAS_SRC, 3)
    assert alias.coupled is True and alias.has_gradient is True and tool("forms", text=ALIAS_SRC).split() == ["000011", "0"]
    like = tda.DeviceLogLike("#define TERM tda_loglike_term\n__device__ double TERM(double f, double y, double p, int o) { return 0.0; }", [0.0])
    assert like.has_gradient is False


def test_option_list_of_every_spec(tool):
    """exactly these strings in this order, each under its own condition and absent otherwise"""
    got = dict(ln.split(":") for ln in tool("options").splitlines())
    assert len(got) == 48
    for mala, loglike, prior, fwd, grad in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1)):
        want = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"]
        want += ["-DTDA_LOGLIKE_SOURCE"] if loglike else []
        want += ["-DTDA_USER_MALA"] if mala else []
        want += ["-DTDA_PRIOR_SOURCE"] if prior else []
        want += ["-DTDA_PRIOR_WAVE"] if prior == 2 else []
        want += ["-DTDA_FORWARD_WAVE"] if fwd else []
        want += ["-DTDA_GRADIENT_WAVE"] if grad else []
        assert got["%d%d%d%d%d" % (mala, loglike, prior, fwd, grad)].split() == want


def test_both_forms_decision(tool):
    assert tool("forms", text=xp.LOGNORMAL_SRC + xpw.CAUCHY_DIFF_SRC).split() == ["001011", "1"]
    assert tool("forms", text=xp.LOGNORMAL_SRC).split() == ["001000", "0"]
    assert tool("forms", text=xpw.CAUCHY_DIFF_SRC).split() == ["000011", "0"]
    assert tool("forms", text=xw.source("both", "wave", m=23)).split() == ["110000", "0"]
    assert tool("forms", text=xm.source() + "// tda_logprior_term tda_logprior_wave\n").split() == ["000000", "0"]


NO_GRADIENT = xm.source().split("__device__ double tda_gradient")[0]
NO_PRIOR_GRAD = xm.source() + xpw.CAUCHY_DIFF_SRC.split("__device__ double tda_logprior_grad")[0]
TOO_MUCH_LDS = ("__device__ double tda_forward(const double* theta, int dim, int o) {\n  __shared__ double big[30000];\n"
                "  big[threadIdx.x] = theta[0];\n  __syncthreads();\n  return big[o % 64] + dim;\n}\n")
INVALID, UNSUPPORTED = -1, -4
# what, user source, (mala, loglike_source, prior_form, forward_wave, gradient_wave), code, message: the texts of the host's refusals
FAILURES = [
    ("tda_forward_wave", xw.source("per_output", m=23), (0, 0, 0, 1, 0), INVALID,
     "the source's tda_forward_wave is not __device__ void tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane)"),
    ("tda_gradient_wave", xw.source(gradient="per_parameter"), (1, 0, 0, 1, 1), INVALID,
     "the source's tda_gradient_wave is not __device__ void tda_gradient_wave(const double* theta, int dim, const double* sensitivity, int n_outputs, "
     "double* grad, double* work, int lane)"),
    ("tda_gradient", NO_GRADIENT, (1, 0, 0, 0, 0), INVALID,
     "MALA on a source-defined model: the source defines no __device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, "
     "int n_outputs, int j)"),
    ("tda_loglike_term_grad", xm.source() + xl.TERM_ONLY_SRC, (1, 1, 0, 0, 0), INVALID,
     "MALA with a source-defined likelihood: the source defines no __device__ double tda_loglike_term_grad(double f, double y, double p, int o)"),
    ("tda_loglike_term", xm.source(), (0, 1, 0, 0, 0), INVALID,
     "a source-defined likelihood: the source defines no __device__ double tda_loglike_term(double f, double y, double p, int o)"),
    ("tda_logprior_wave", xm.source() + xp.LOGNORMAL_SRC, (0, 0, 2, 0, 0), INVALID,
     "a source-defined prior: the source's tda_logprior_wave is not __device__ double tda_logprior_wave(const double* theta, int dim, const double* p, "
     "const double* q, int lane)"),
    ("tda_logprior_grad", NO_PRIOR_GRAD, (1, 0, 2, 0, 0), INVALID,
     "a source-defined prior under MALA: the source defines no __device__ double tda_logprior_grad(const double* theta, int dim, const double* p, "
     "const double* q, int j)"),
    ("tda_logprior_term_grad", xm.source() + xp.LOGNORMAL_SRC, (1, 0, 1, 0, 0), INVALID,
     "a source-defined prior under MALA: the source defines no __device__ double tda_logprior_term_grad(double x, double p, double q, int j)"),
    ("tda_logprior_term", xm.source(), (0, 0, 1, 0, 0), INVALID,
     "a source-defined prior: the source defines no __device__ double tda_logprior_term(double x, double p, double q, int j) (or, for a prior that couples "
     "parameters, tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane))"),
    ("static LDS", TOO_MUCH_LDS, (0, 0, 0, 0, 0), UNSUPPORTED,
     "a source-defined model holds at most 64 KiB of LDS per chain: this source declares 241024 bytes (parameters, gradient, TDA_WORKSPACE and its own "
     "__shared__ arrays), more than the 163840 bytes of the hardware, before the 184 bytes for its 23 outputs"),
]


@needs_hipcc
@pytest.mark.parametrize("what,user,spec,code,message", FAILURES, ids=[f[0] for f in FAILURES])
def test_diagnosis_of_real_compiler_logs(tool, tmp_path, what, user, spec, code, message):
    switches = [name for name, on in zip(("TDA_USER_MALA", "TDA_LOGLIKE_SOURCE", "TDA_PRIOR_SOURCE", "TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE"), spec) if on]
    switches += ["TDA_PRIOR_WAVE"] if spec[2] == 2 else []
    rc, log, _ = compile_program(tmp_path, "failing", user, switches)
    assert rc != 0, what
    got_code, got_message = tool("diagnose", *spec, 23, text=log).split("\n", 1)
    assert (int(got_code), got_message) == (code, message), log[-2000:]


def test_any_other_failure_quotes_the_truncated_log(tool):
    log = "error: " + "x" * 500
    assert tool("diagnose", 0, 0, 0, 0, 0, 5, text=log) == "-1\nthe forward-model source does not compile: " + log[:400]
    assert tool("diagnose", 1, 0, 0, 0, 0, 5, text=log) == "-1\nthe forward-model source does not compile with the MALA kernels: " + log[:400]
    # a tag of the other program's does not apply
    assert tool("diagnose", 0, 0, 0, 0, 0, 5, text="tda_gradient_missing").startswith("-1\nthe forward-model source does not compile: tda_gradient_missing")
    assert tool("diagnose", 1, 1, 0, 0, 0, 5, text="tda_loglike_term_missing").startswith("-1\nthe forward-model source does not compile with the MALA kernels")
