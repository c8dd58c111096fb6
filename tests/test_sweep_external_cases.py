"""CPU checks of the external-model sweep (test_gpu_sweep_external.py) before any GPU time is spent on it: the HIP source
template compiled for the host against its NumPy twin and the twin's vector-Jacobian product, and the committed cases of
the three generators against the shapes the sweep exists for."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from .extmodel import np_forward, np_jacobian, np_vjp, source
from .test_gpu_sweep_external import N_MALA, N_ML, N_SINGLE, _mala_case, _ml_case, _single_case

WRAPPER = r"""
extern "C" void twin_forward(const double* theta, int d, int m, double* F) {
  for (int o = 0; o < m; ++o) F[o] = tda_forward(theta, d, o);
}
extern "C" void twin_gradient(const double* theta, int d, const double* sens, int m, double* g) {
  for (int j = 0; j < d; ++j) g[j] = tda_gradient(theta, d, sens, m, j);
}
"""


@pytest.fixture(scope="module")
def host_twin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    d = tmp_path_factory.mktemp("twin")
    src = d / "twin.cpp"
    src.write_text("#include <cmath>\n" + source(shift=0.003, coup=0.4) + WRAPPER)
    lib = d / "libtwin.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-D__device__=", "-D__forceinline__=inline",
                    "-o", str(lib), str(src)], check=True)
    so = ctypes.CDLL(str(lib))
    dp = ctypes.POINTER(ctypes.c_double)
    so.twin_forward.argtypes = [dp, ctypes.c_int, ctypes.c_int, dp]
    so.twin_gradient.argtypes = [dp, ctypes.c_int, dp, ctypes.c_int, dp]
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.mark.parametrize("d,m", [(1, 1), (1, 64), (2, 65), (17, 3), (64, 64), (65, 65), (128, 63), (128, 2048), (65, 2048)])
def test_source_template_matches_numpy_twin(host_twin, d, m):
    shift, coup = 0.003, 0.4
    rng = np.random.default_rng(d * 10000 + m)
    theta = np.ascontiguousarray(0.3 * rng.standard_normal(d))
    sens = np.ascontiguousarray(rng.standard_normal(m))
    F = np.empty(m)
    host_twin.twin_forward(_p(theta), d, m, _p(F))
    np.testing.assert_allclose(F, np_forward(theta, m, shift=shift, coup=coup)[0], rtol=1e-12, atol=1e-14)
    g = np.empty(d)
    host_twin.twin_gradient(_p(theta), d, _p(sens), m, _p(g))
    np.testing.assert_allclose(g, np_vjp(theta, sens, shift, coup)[0], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(np_jacobian(theta, m, shift, coup).T @ sens, g, rtol=1e-11, atol=1e-13)
    # central differences of s . F(theta) along every parameter
    h = 1e-5
    E = np.eye(d) * h
    fd = np.array([(sens @ np_forward(theta + E[j], m, shift=shift, coup=coup)[0] - sens @ np_forward(theta - E[j], m, shift=shift, coup=coup)[0]) / (2 * h)
                   for j in range(d)])
    np.testing.assert_allclose(g, fd, rtol=1e-5, atol=1e-6 * max(1.0, float(np.abs(sens).sum())))


def _single():
    return [_single_case(i) for i in range(N_SINGLE)]


def _fused_source(c):
    return c["model"] == "source" and c["noise"] != "dense" and c["kind"] not in ("indep", "owcn")


def test_single_level_cases_cover_the_boundaries():
    cases = _single()
    fused = [c for c in cases if _fused_source(c)]
    cb = [c for c in cases if c["model"] == "callback"]
    stepwise = [c for c in cases if c["model"] == "source" and not _fused_source(c)]
    for d in (1, 64, 65, 128):
        assert any(c["d"] == d for c in fused), ("fused source path", d)
        assert any(c["d"] == d for c in cb), ("callback path", d)
    for m in (1, 64, 65):
        assert any(c["m"] == m for c in fused), ("fused source path", m)
    assert any(c["m"] >= 1000 for c in fused)
    assert stepwise and all(c["d"] <= 64 for c in stepwise + [c for c in cb if c["noise"] == "dense" or c["kind"] in ("indep", "owcn")])
    for kind in ("indep", "owcn"):
        assert any(c["kind"] == kind for c in cases), kind
    assert any(c["noise"] == "dense" for c in cases)
    assert any(c["prior"] == "joint" for c in fused) and any(c["prior"] == "joint" for c in cb)
    assert any(c["N"] == 1 for c in cases) and any(c["split"] for c in cases) and any(c["block"] for c in cases)
    for c in cases:  # combinations the engine refuses never reach it
        assert not (c["prior"] == "joint" and (c["kind"].startswith("pcn") or c["kind"] in ("owcn", "indep") or c["noise"] == "dense"))
        assert c["d"] <= 64 or (c["noise"] != "dense" and c["kind"] not in ("indep", "owcn"))
        assert c["noise"] != "dense" or c["m"] <= 300


def test_mala_cases_cover_the_boundaries():
    cases = [_mala_case(i) for i in range(N_MALA)]
    for d in (1, 64, 65, 128):
        assert any(c["d"] == d for c in cases), d
    for m in (1, 64, 65):
        assert any(c["m"] == m for c in cases), m
    assert any(c["m"] == 2048 for c in cases)
    assert any(c["variant"] == "resume" and c["d"] == 128 for c in cases)  # the gradient travels in the checkpoint blob
    assert {c["kind"] for c in cases} == {"mala", "mala_adaptive"} and {c["noise"] for c in cases} == {"iso", "diag"}


def test_hierarchy_cases_cover_the_boundaries():
    cases = [_ml_case(i) for i in range(N_ML)]
    assert any(c["nl"] == 4 and any(mk == "source" for mk in c["models"]) and c["d"] >= 65 for c in cases)
    assert {mk for c in cases for mk in c["models"]} == {"source", "callback", "linear"}
    assert any(c["randomize"] for c in cases) and {c["kind"] for c in cases} >= {"pcn", "grw_adaptive", "am"}
    for m in (64, 65):
        assert any(m in c["ms"] for c in cases), m
    for d in (64, 65, 128):
        assert any(c["d"] == d for c in cases), d
    for c in cases:
        assert any(mk != "linear" for mk in c["models"]) and 2 <= c["nl"] <= 4


def test_record_variants_reach_wide_engines():
    cases = _single() + [_mala_case(i) for i in range(N_MALA)]
    for v in ("thin", "device", "resume"):
        assert any(c["variant"] == v and c["d"] >= 65 for c in cases), v
    assert all(c["thin"] == (3 if c["variant"] == "thin" else 1) for c in cases)
