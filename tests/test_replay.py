"""Model outputs and quantities of interest of a result, on the device (tda_user_replay, include/tinyda_amd_replay.h,
tinyda_amd/replay.py) -- what needs no device: the replay program compiled offline for gfx950 as hiprtc compiles it, the programs
that exist today against the parent commit's, the build description (csrc/tda_user_build.h) through a stand-alone host program
(tests/replay_build_main.cpp, also built with the address and undefined-behaviour sanitizers), DeviceModel's new contract, the
host protocol's quantity of interest and the second ABI table."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.stats as st

from . import extmodel as xm
from . import extqoi as xq
from . import extwave as xw
from .extprogram import CSRC, PROGRAM, ROOT, STEP_KERNELS, assembly, assert_switch_is_an_option_only, compile_program, needs_hipcc

REPLAY = ["TDA_USER_REPLAY"]
KERNEL = ("tda_user_replay",)
RING_WAVE = xw.source()
RING_PER_OUTPUT = xw.source("per_output", m=16)
QOI_SIG = "__device__ double tda_qoi(const double* theta, int dim, const double* f, int n_outputs, int k)"
QOI_WAVE_SIG = "__device__ void tda_qoi_wave(const double* theta, int dim, const double* f, int n_outputs, double* qoi, int n_qoi, double* work, int lane)"


def _parent_program():
    r = subprocess.run(["git", "show", "HEAD~:tinyda_amd/csrc/tda_user_program.hip"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    if r.returncode != 0 or "tda_user_steps" not in r.stdout:
        pytest.skip("the parent commit's program text is not available (no git history here)")
    return r.stdout


# ---- 1. the replay program, compiled offline as shipped ---------------------------------------------------------------------------------
CASES = [  # name, user source, switches beside TDA_USER_REPLAY
    ("extmodel", xm.source(), []),
    ("extmodel_qoi", xm.source() + xq.PER_QUANTITY, ["TDA_QOI"]),
    ("ring_wave", RING_WAVE, ["TDA_FORWARD_WAVE"]),
    ("ring_wave_qoi", RING_WAVE + xq.PER_QUANTITY, ["TDA_FORWARD_WAVE", "TDA_QOI"]),
    ("ring_wave_qoi_wave", RING_WAVE + xq.RING_WAVE, ["TDA_FORWARD_WAVE", "TDA_QOI_WAVE"]),
    ("ring_both_forms", xw.source("both", m=16) + xq.PER_QUANTITY + xq.RING_WAVE, ["TDA_FORWARD_WAVE", "TDA_QOI_WAVE"]),
]


@needs_hipcc
@pytest.mark.parametrize("name,user,switches", CASES, ids=[c[0] for c in CASES])
def test_replay_program_holds_exactly_the_replay_kernel(tmp_path, name, user, switches):
    """... and takes no more scratch memory and spills no more vector registers than the same source's tda_user_eval in the parent
    commit's program.  Measured here (hipcc of ROCm 7, gfx950): 0 bytes of scratch and 0 spilled registers for both kernels of every
    case."""
    rc, log, usage = compile_program(tmp_path, "replay", user, REPLAY + switches)
    assert rc == 0, log[-3000:]
    assert set(usage) == set(KERNEL), usage
    mine = usage["tda_user_replay"]
    print(name, "tda_user_replay", mine)
    rc, log, parent = compile_program(tmp_path, "parent", user, [s for s in switches if s == "TDA_FORWARD_WAVE"], _parent_program())
    assert rc == 0 and set(parent) == set(STEP_KERNELS), log[-3000:]
    print(name, "tda_user_eval (parent commit)", parent["tda_user_eval"])
    for what in ("ScratchSize [bytes/lane]", "VGPRs Spill"):
        assert mine[what] <= parent["tda_user_eval"][what], (what, mine, parent["tda_user_eval"])


@needs_hipcc
def test_ring_per_output_form_takes_scratch_by_design(tmp_path):
    """the per-output form of the ring keeps four 64-double arrays per lane (tests/extwave.py): its scratch is the model's, recorded
    here as the step program's tests record it, and no more than the same source's tda_user_eval takes (measured, hipcc of ROCm 7:
    1616 bytes per lane and 26 spilled vector registers in tda_user_replay, 2656 bytes and none in tda_user_eval)"""
    rc, log, usage = compile_program(tmp_path, "replay", RING_PER_OUTPUT + xq.PER_QUANTITY, REPLAY + ["TDA_QOI"])
    assert rc == 0 and set(usage) == set(KERNEL), log[-3000:]
    rc, log, steps = compile_program(tmp_path, "steps", RING_PER_OUTPUT + xq.PER_QUANTITY, [])
    assert rc == 0, log[-3000:]
    print("ring per output: tda_user_replay", usage["tda_user_replay"], "tda_user_eval", steps["tda_user_eval"])
    assert usage["tda_user_replay"]["ScratchSize [bytes/lane]"] <= steps["tda_user_eval"]["ScratchSize [bytes/lane]"]


@needs_hipcc
@pytest.mark.parametrize("switches", [[], ["TDA_USER_MALA"], ["TDA_FORWARD_WAVE"], ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE"]], ids=lambda s: "+".join(s) or "none")
def test_existing_programs_are_the_parent_commits(tmp_path, switches):
    """under every option list that exists today the object of the program as shipped equals the parent commit's, byte for byte"""
    from . import extloglikewave as xlw

    parent = _parent_program()
    user = (xw.source(gradient="wave") if "TDA_FORWARD_WAVE" in switches else xm.source()) + (xlw.AR1_SRC if "TDA_LOGLIKE_WAVE" in switches else "")
    for name, text in (("mine", open(PROGRAM).read()), ("parent", parent)):
        rc, log, _ = compile_program(tmp_path, name, user, switches, text)
        assert rc == 0, log[-3000:]
    mine, parents = (tmp_path / "mine" / "program.out").read_bytes(), (tmp_path / "parent" / "program.out").read_bytes()
    assert len(mine) > 1000 and mine == parents


@needs_hipcc
def test_the_qoi_switches_alone_change_no_instruction_of_the_step_program(tmp_path):
    user = xm.source() + xq.PER_QUANTITY
    plain = assembly(tmp_path, "without", user, [])
    assert assembly(tmp_path, "with_qoi", user, ["TDA_QOI"]) == plain
    assert assembly(tmp_path, "with_qoi_wave", user, ["TDA_QOI_WAVE"]) == plain


def test_no_file_that_reaches_the_compiler_defines_the_new_switches():
    for switch in ("TDA_USER_REPLAY", "TDA_QOI", "TDA_QOI_WAVE"):
        assert_switch_is_an_option_only(switch + r"\b", ("tda_usermodel.inc", "tda_user_build.h", "tda_host_replay.inc"))


@needs_hipcc
def test_missing_or_mis_signed_functions_name_their_signatures(tmp_path):
    rc, log, _ = compile_program(tmp_path, "no_qoi", xm.source(), REPLAY + ["TDA_QOI"])
    assert rc != 0 and "tda_qoi_missing" in log and QOI_SIG in log
    rc, log, _ = compile_program(tmp_path, "other_sig", xm.source() + xq.PER_QUANTITY.replace("int n_outputs, int k)", "int n_outputs, int k, int more)"), REPLAY + ["TDA_QOI"])
    assert rc != 0 and "tda_qoi_missing" in log and QOI_SIG in log
    rc, log, _ = compile_program(tmp_path, "no_wave", RING_WAVE + xq.PER_QUANTITY, REPLAY + ["TDA_FORWARD_WAVE", "TDA_QOI_WAVE"])
    assert rc != 0 and "tda_qoi_wave_missing" in log and QOI_WAVE_SIG in log and "tda_qoi_missing" not in log
    rc, log, _ = compile_program(tmp_path, "wave_other_sig", RING_WAVE + xq.RING_WAVE.replace("double* work, int lane)", "int lane)"), REPLAY + ["TDA_FORWARD_WAVE", "TDA_QOI_WAVE"])
    assert rc != 0 and "tda_qoi_wave_missing" in log and QOI_WAVE_SIG in log
    # the model's own wave form is asked for as in the step program
    rc, log, _ = compile_program(tmp_path, "no_forward_wave", RING_PER_OUTPUT, REPLAY + ["TDA_FORWARD_WAVE"])
    assert rc != 0 and "tda_forward_wave_missing" in log


# ---- 2. the build description, through the stand-alone program ----------------------------------------------------------------------------
CXX = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    """tests/replay_build_main.cpp, built once as it is and once with -fsanitize=address,undefined (a stand-alone program: the
    sanitizers' runtimes are linked in, nothing is preloaded); a sanitizer report ends the program with a non-zero status"""
    if CXX is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("replay_build_" + request.param)
    exe = str(work / "tool")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    r = subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "replay_build_main.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
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


def test_signatures_are_the_same_in_the_engine_and_in_python(tool):
    from tinyda_amd._contract import QOI_SIG as PY, SIG

    printed = dict(ln.split("\t") for ln in tool("signatures").splitlines())
    assert printed == PY == {"tda_qoi": QOI_SIG, "tda_qoi_wave": QOI_WAVE_SIG}
    assert all(text.startswith("__device__ ") and " %s(" % name in text for name, text in PY.items())
    assert len(SIG) == 12 and not set(SIG) & set(PY)


def test_forms_and_option_strings(tool):
    assert tool("forms", text=xm.source()).split() == ["00", "0"]
    assert tool("forms", text=xm.source() + xq.PER_QUANTITY).split() == ["10", "0"]
    assert tool("forms", text=RING_WAVE + xq.RING_WAVE).split() == ["01", "1"]
    assert tool("forms", text=RING_WAVE + xq.PER_QUANTITY + xq.RING_WAVE).split() == ["11", "1"]
    assert tool("forms", text=xm.source() + "// tda_qoi( tda_qoi_wave(\n/* tda_qoi */ const char* s = \"tda_qoi_wave\"; double my_tda_qoi;").split() == ["00", "0"]
    base = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-DTDA_USER_REPLAY"]
    assert tool("options", 0, 0).split() == ["100"] + base
    assert tool("options", 1, 0).split() == ["100"] + base + ["-DTDA_FORWARD_WAVE"]
    assert tool("options", 0, 1).split() == ["100"] + base + ["-DTDA_QOI"]
    assert tool("options", 1, 2).split() == ["100"] + base + ["-DTDA_FORWARD_WAVE", "-DTDA_QOI_WAVE"]
    assert tool("lds", 16, 3).strip() == "152" and tool("lds", 1024, 0).strip() == "8192"


@pytest.mark.parametrize("rows", [1, 2, 63, 2001])
@pytest.mark.parametrize("n_chains", [1, 16, 4096])
def test_segment_rule(tool, rows, n_chains):
    """every row lies in exactly one segment, no segment is empty, the result lies in [1, rows] -- at the LDS of the smallest
    program (s_th alone), of the ring's (its workspace) and at the 64 KiB limit"""
    got = {}
    for lds in (1024 + 8, 1024 + 8 * (16 + 3 + 3072), 65536):
        seg, n, covered, shortest = (int(v) for v in tool("segment", rows, n_chains, lds).split())
        assert 1 <= seg <= rows and n == -(-rows // seg) and covered == rows and shortest >= 1
        got[lds] = seg
    assert got[1024 + 8] <= got[65536]  # fewer resident workgroups: fewer segments are enough
    if n_chains == 1 and rows == 2001:
        assert got[65536] < rows  # a single chain is cut up
    if rows == 1:
        assert set(got.values()) == {1}


@needs_hipcc
def test_diagnosis_of_real_compiler_logs(tool, tmp_path):
    rc, log, _ = compile_program(tmp_path, "no_qoi", xm.source(), REPLAY + ["TDA_QOI"])
    assert rc != 0
    assert tool("diagnose", 0, 1, 23, text=log) == "-1\na quantity of interest: the source's tda_qoi is not " + QOI_SIG
    rc, log, _ = compile_program(tmp_path, "no_wave", RING_WAVE + xq.PER_QUANTITY, REPLAY + ["TDA_FORWARD_WAVE", "TDA_QOI_WAVE"])
    assert rc != 0
    assert tool("diagnose", 1, 2, 23, text=log) == "-1\na quantity of interest: the source's tda_qoi_wave is not " + QOI_WAVE_SIG
    rc, log, _ = compile_program(tmp_path, "no_forward_wave", RING_PER_OUTPUT, REPLAY + ["TDA_FORWARD_WAVE"])
    assert rc != 0
    assert tool("diagnose", 1, 0, 23, text=log).startswith("-1\nthe source's tda_forward_wave is not __device__ void tda_forward_wave(")
    # any other failure says which program it was; the other programs' rows do not apply
    assert tool("diagnose", 0, 0, 5, text="error: x") == "-1\nthe forward-model source does not compile with the replay kernel: error: x"
    assert tool("diagnose", 0, 0, 5, text="tda_gradient_missing").startswith("-1\nthe forward-model source does not compile with the replay kernel")


# ---- 3. DeviceModel ------------------------------------------------------------------------------------------------------------------
def test_device_model_says_which_form_of_the_quantity_its_source_has():
    import tinyda_amd as tda

    plain = tda.DeviceModel(xm.source(), 5)
    assert plain.n_qoi == 0 and not plain.has_qoi and not plain.has_qoi_wave
    per = tda.DeviceModel(xm.source() + xq.PER_QUANTITY, 5, n_qoi=3)
    assert per.n_qoi == 3 and per.has_qoi and not per.has_qoi_wave
    wave = tda.DeviceModel(RING_WAVE + xq.RING_WAVE, 16, n_qoi=3)
    assert wave.has_qoi and wave.has_qoi_wave
    both = tda.DeviceModel(RING_WAVE + xq.PER_QUANTITY + xq.RING_WAVE, 16, n_qoi=3)
    assert both.has_qoi and both.has_qoi_wave
    # comments, strings and longer identifiers do not count
    quiet = tda.DeviceModel(xm.source() + "// tda_qoi( \n/* tda_qoi_wave( */ __device__ const char* n() { return \"tda_qoi tda_qoi_wave\"; }\n"
                            "__device__ double my_tda_qoi(double tda_qoi_scale) { return tda_qoi_scale; }\n", 5)
    assert not quiet.has_qoi and not quiet.has_qoi_wave
    with pytest.raises(ValueError) as exc:
        tda.DeviceModel(xm.source() + "// tda_qoi\n", 5, n_qoi=2)
    assert QOI_SIG in str(exc.value) and QOI_WAVE_SIG in str(exc.value)
    with pytest.raises(ValueError) as exc:
        tda.DeviceModel(xm.source() + xq.PER_QUANTITY, 5)
    assert QOI_SIG in str(exc.value)
    with pytest.raises(ValueError) as exc:
        tda.DeviceModel(RING_WAVE + xq.RING_WAVE, 16)
    assert QOI_WAVE_SIG in str(exc.value)
    assert "tda_qoi_wave" in tda.DeviceModel.__doc__ and "reference_qoi" in tda.DeviceModel.__doc__


def test_host_call_returns_the_quantity_only_with_reference_qoi():
    import copy

    import tinyda_amd as tda

    m, theta = 7, np.array([0.3, -0.2, 0.5])
    ref = lambda t: xm.np_forward(t, m)[0]
    bare = tda.DeviceModel(xm.source() + xq.PER_QUANTITY, m, n_qoi=4, reference=ref)
    out = bare(theta)
    assert isinstance(out, np.ndarray) and np.array_equal(out, ref(theta))
    full = tda.DeviceModel(xm.source() + xq.PER_QUANTITY, m, n_qoi=4, reference=ref, reference_qoi=lambda t, f: xq.np_per_quantity(t, f, 4)[0])
    out, qoi = full(theta)
    assert np.array_equal(out, ref(theta)) and np.array_equal(qoi, xq.np_per_quantity(theta, ref(theta), 4)[0]) and qoi.shape == (4,)
    with pytest.raises(TypeError, match="no host reference"):
        tda.DeviceModel(xm.source(), m)(theta)
    assert copy.deepcopy(full).n_qoi == 4


def test_host_protocol_records_the_quantity():
    """backend='host': the reference's model protocol (posterior.py:97-101) carries the quantity into every link"""
    import tinyda_amd as tda

    d, m, nq = 3, 7, 4
    rng = np.random.default_rng(5)
    truth = 0.3 * rng.standard_normal(d)
    y = xm.np_forward(truth, m)[0] + 0.05 * rng.standard_normal(m)
    model = tda.DeviceModel(xm.source() + xq.PER_QUANTITY, m, n_qoi=nq, reference=lambda t: xm.np_forward(t, m)[0],
                            reference_qoi=lambda t, f: xq.np_per_quantity(t, f, nq)[0])
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(y, 0.0025 * np.eye(m)), model)
    res = tda.sample(post, tda.GaussianRandomWalk(0.01 * np.eye(d)), 20, n_chains=2, initial_parameters=[truth, truth + 0.01], backend="host", seed=3)
    qoi, par = tda.get_samples(res, "qoi"), tda.get_samples(res, "parameters")
    for c in range(2):
        P, Q = par["chain_%d" % c], qoi["chain_%d" % c]
        assert Q.shape == (P.shape[0], nq) and P.shape[0] >= 20
        assert len(np.unique(P, axis=0)) > 1
        for row in range(P.shape[0]):
            assert np.array_equal(Q[row], xq.np_per_quantity(P[row], xm.np_forward(P[row], m), nq)[0])
    idata = tda.to_inference_data(res)
    assert sorted(idata.qoi) == ["qoi_%d" % k for k in range(nq)] and idata.qoi["qoi_0"].shape == (2, par["chain_0"].shape[0])


# ---- 4. the second ABI table -----------------------------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyda_amd_replay.h")).read(), flags=re.S)
    return set(re.findall(r"\b(tda_[a-z_]+)\s*\(", text))


def test_replay_header_binding_and_library_agree():
    import __graft_entry__ as g

    g.build()
    from tinyda_amd import _lib

    assert _declared() == set(_lib.REPLAY_SYMBOLS) == {"tda_replay_create", "tda_replay_run", "tda_replay_destroy"}
    assert not set(_lib.REPLAY_SYMBOLS) & set(_lib.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert _declared() <= set(re.findall(r"\bT (tda_[a-z_]+)", out))
    lib = _lib.load()
    assert lib.tda_replay_run.argtypes is not None and len(lib.tda_replay_run.argtypes) == 9
    # the CPU twin of the ABI knows nothing of the replay and still binds
    twin = _lib.load_from(g.CPU_ABI_SO)
    assert twin.tda_version() and not hasattr(twin, "tda_replay_create")


def test_replay_refuses_without_a_device():
    """no CPU fallback: on a machine without a GPU evaluate raises instead of computing elsewhere"""
    import tinyda_amd as tda

    try:
        import torch

        if torch.cuda.is_available():
            pytest.skip("GPU present")
    except ImportError:
        pass
    with pytest.raises(tda.EngineError):
        tda.DeviceModel(xm.source(), 3).evaluate(np.zeros((2, 2)))
