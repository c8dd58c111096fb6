"""The source-defined programs compiled offline, as the engine's hiprtc call compiles them (compile_user_program of
csrc/tda_usermodel.inc): the program text -- the shipped csrc/tda_user_program.hip unless another is given -- with the user's
source as its header tda_user_source.h and the switches as -D options.  Every compile runs in a directory of its own and
names its files relative to it, so that no path differs between two builds."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "tinyda_amd", "csrc")
PROGRAM = os.path.join(CSRC, "tda_user_program.hip")
STEP_KERNELS = ("tda_user_steps", "tda_user_level_action", "tda_user_eval")
MALA_KERNELS = ("tda_user_mala_steps", "tda_user_mala_grad0")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc")


def compile_program(tmp_path, name, user_source, switches, program_text=None, output=("-c", "program.out")):
    """(return code, compiler output, {kernel: {resource: count}}) of the program under `switches` (names, without -D); the
    device object is left at tmp_path / name / program.out"""
    work = tmp_path / name
    work.mkdir()
    (work / "tda_user_source.h").write_text(user_source)
    (work / "tda_user_program.hip").write_text(open(PROGRAM).read() if program_text is None else program_text)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-ffp-contract=off", "-std=c++17", output[0],
                        "-Rpass-analysis=kernel-resource-usage", "-I.", "-I" + CSRC] + ["-D" + s for s in switches]
                       + ["tda_user_program.hip", "-o", output[1]], cwd=str(work), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    usage, fn = {}, None
    for ln in r.stdout.splitlines():
        mt = re.search(r"Function Name: (\w+)", ln)
        if mt:
            fn = mt.group(1)
            usage[fn] = {}
        mt = re.search(r"\s(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|VGPRs): (\d+)", ln)
        if mt and fn:
            usage[fn][mt.group(1)] = int(mt.group(2))
    return r.returncode, r.stdout, usage


def assembly(tmp_path, name, user_source, switches, program_text=None):
    """the program's -S assembly, with the one symbol that depends on the option list (__hip_cuid_<hash>) made a fixed word: two
    programs with the same text here have the same instructions, registers and LDS"""
    rc, log, _ = compile_program(tmp_path, name, user_source, switches, program_text, output=("-S", "program.s"))
    assert rc == 0, log[-3000:]
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", (tmp_path / name / "program.s").read_text())


def assert_without_scratch(tmp_path, name, user_source, switches, kernels):
    """the program compiles, holds exactly `kernels`, and none of them takes scratch memory or spills vector registers (scalar
    spills into vector lanes are printed, not asserted)"""
    rc, log, usage = compile_program(tmp_path, name, user_source, switches)
    assert rc == 0, log[-3000:]
    assert set(kernels) == set(usage), (usage, log[-2000:])
    for k in kernels:
        print(name, k, usage[k])
        assert usage[k]["ScratchSize [bytes/lane]"] == 0 and usage[k]["VGPRs Spill"] == 0, (k, usage[k])


def assert_switch_is_an_option_only(switch, extra_files=()):
    """no file that reaches the compiler defines or undefines a switch matching `switch` (a regex), and one place in the host
    code talks to hiprtc; its option list is tests/test_user_build.py's"""
    for f in ("tda_user_program.hip", "tda_user_args.h") + tuple(extra_files):
        assert not re.search(r"#\s*(define|undef)\s+" + switch, open(os.path.join(CSRC, f)).read()), f
    host = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f != "tda_user_program.hip")
    assert host.count("hiprtcCompileProgram(") == 1
    return open(os.path.join(ROOT, "include", "tinyda_amd.h")).read()
