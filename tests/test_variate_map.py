"""The engine's variate map held to an exact reference, in ulps, without a GPU (tests/extvariate.py).

1. The device branch of tinyda_amd/csrc/tda_philox.h -- tda_log_unit, tda_sincos_turn and normal_pair's lines over them --
   compiled for the host through tests/variate_math_main.cpp (which includes the header and restates nothing), at the chosen
   inputs and 2 10^6 random pairs: ln within 1 ulp, sin and cos within 2, a normal within 4 2^-52 relative with no absolute
   floor -- the header's claims and what follows from them --, exact values on the axes and at u1 = 0, nothing non-finite.
2. The reference itself against mpmath at 120 bits.
3. The float64 maps that every other test trusts -- the oracle's PhiloxStream.normals and the CPU twin's normal_pair -- against
   the exact reference, within the bound that an angle rounded once allows; which is why those tests carry an absolute floor.
4. The source that tests/test_gpu_variate_map.py runs on the device compiles offline as the replay program."""
import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extvariate as xv
from .extprogram import compile_program, needs_hipcc

N_RANDOM = 2_000_000 // xv.SAMPLE_DIVISOR


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def shim(request, tmp_path_factory):
    """the program built once as it is and once with -fsanitize=address,undefined (stand-alone: the runtimes are linked in, nothing
    is preloaded; a report ends the program with a non-zero status)"""
    if xv.CXX is None:
        pytest.skip("no C++ compiler")
    exe, why = xv.build_shim(tmp_path_factory.mktemp("variate_math_" + request.param), sanitized=request.param == "sanitized")
    if exe is None:
        pytest.skip(why)
    return exe


@pytest.fixture(scope="module")
def chosen():
    u1, u2 = xv.chosen_pairs(2 ** 16 // xv.SAMPLE_DIVISOR)
    return u1, u2


# ---- 1. the device branch on the host -----------------------------------------------------------------------------------------------
def test_chosen_inputs_hold_what_they_promise():
    u1, u2 = xv.chosen_u1(16), xv.chosen_u2(16)
    x = 1.0 - u1
    assert np.all((u1 >= 0) & (u1 < 1)) and np.all((u2 >= 0) & (u2 < 1))
    assert np.all(u1 / xv.G == np.rint(u1 / xv.G)) and np.all(u2 / xv.G == np.rint(u2 / xv.G))
    assert {1.0, xv.G, 1.0 - xv.G, 0.75, 0.5, 2.0 ** -52} <= set(x)
    m, _ = np.frexp(x)
    low = m < 0.70710678118654752440
    for k in range(52):  # both sides of the switch in every binade that holds two grid points
        b = (x >= 2.0 ** (-k - 1)) & (x < 2.0 ** -k)
        assert low[b].any() and (~low[b]).any(), k
    a = 4.0 * u2
    assert set(range(8)) <= set((8.0 * u2[(8.0 * u2) == np.rint(8.0 * u2)]).astype(int))
    assert {0.0, 1.0, 2.0, 3.0, 4.0} == set(np.rint(a)) and (1.0 - xv.G) in u2
    assert np.array_equal(np.rint(4.0 * np.array([1, 3, 5, 7]) / 8.0), [0.0, 2.0, 2.0, 4.0])  # the reference's ties go to even


def test_device_branch_on_the_host_at_chosen_inputs(shim, chosen):
    u1, u2 = chosen
    got = xv.shim_map(shim, u1, u2)
    assert all(np.isfinite(g).all() for g in got)
    xv.assert_map_bounds(xv.map_errors(got, u1, u2), "chosen inputs (host build of the device branch)")
    xv.assert_axes_exact(got[1], got[2], got[3], got[4], u1, u2)
    xv.assert_ties_to_even(got[1], got[2], u2)
    # edge values of this build (integer steps, fma and sqrt only: the same on every host)
    at = lambda a, b: int(np.flatnonzero((u1 == a) & (u2 == b))[0])
    i = at(0.5, 0.25)
    assert (got[1][i], got[2][i]) == (1.0, 0.0) and np.signbit(got[2][i])
    assert got[1][np.flatnonzero(u2 == 1.0 - xv.G)[0]] == -6.9757369960172635e-16
    assert got[0][np.flatnonzero(u1 == 1.0 - xv.G)[0]] == -36.736800569677101


def test_device_branch_on_the_host_at_random_inputs(shim):
    u1, u2 = xv.random_pairs(N_RANDOM, 20261020)
    got = xv.shim_map(shim, u1, u2)
    assert all(np.isfinite(g).all() for g in got)
    xv.assert_map_bounds(xv.map_errors(got, u1, u2), "%d random pairs (host build of the device branch)" % N_RANDOM)


def test_wrapper_is_normal_pair_on_the_stream(shim):
    """the program's two-line wrapper at the contract's uniforms = normal_pair itself at the contract's counters, bit for bit; and
    both within the bound of the exact normals of those coordinates"""
    seed, chains, step = (7 << 32) | 12345, np.arange(2 ** 32 - 10, 2 ** 32 + 11) & 0xFFFFFFFF, 2 ** 32 - 3
    for stream, block0 in ((orc.STREAM_PROPOSAL, 0), (xv.STREAM_DREAM_EPS, 3)):
        u1, u2 = xv.stream_uniforms(seed, chains, step, stream, 32, block0)
        z0, z1 = xv.shim_stream(shim, seed, chains, step, stream, 32, block0)
        got = xv.shim_map(shim, u1, u2)
        assert np.array_equal(got[3].reshape(z0.shape), z0) and np.array_equal(got[4].reshape(z1.shape), z1)
        e0, e1 = xv.normals_exact(u1, u2)[:2]
        assert max(xv.rel(z0, e0).max(), xv.rel(z1, e1).max()) <= xv.Z_REL


# ---- 2. the reference is pinned -----------------------------------------------------------------------------------------------------
def _rel_to_mp(ld, mpv):
    """max |ld - mp| / |mp| in units of 2^-60, in mpmath arithmetic (a longdouble is the exact sum of its two fp64 parts)"""
    import mpmath

    worst = mpmath.mpf(0)
    with mpmath.workprec(xv.MP_BITS):
        for a, b in zip(np.ravel(ld), np.ravel(mpv)):
            hi = float(a)
            v = mpmath.mpf(hi) + mpmath.mpf(float(a - xv.LD(hi)))
            if b == 0:
                assert v == 0
                continue
            worst = max(worst, abs(v - b) / abs(b))
        return float(worst * mpmath.mpf(2) ** 60)


def test_longdouble_reference_agrees_with_mpmath():
    """every distinct chosen u1 and u2 (ln and the radius depend on u1 alone, sin and cos on u2 alone; the padding aside) and 2000
    random pairs, the normals included: within 2^-60 relative of the definition evaluated at 120 bits"""
    c1, c2 = xv.chosen_u1(0), xv.chosen_u2(0)
    n = max(len(c1), len(c2))
    r1, r2 = xv.random_pairs(2000 // xv.SAMPLE_DIVISOR, 5)
    e1, e2 = xv.chosen_pairs(0)
    u1 = np.concatenate([np.resize(c1, n), r1, e1[n:]])
    u2 = np.concatenate([np.resize(c2, n), r2, e2[n:]])
    ld, mpv = xv.normals_exact(u1, u2), xv.normals_mp(u1, u2)
    worst = {name: _rel_to_mp(a, b) for name, a, b in zip(("z0", "z1", "ln", "sin", "cos"), ld, mpv)}
    print("longdouble against mpmath, in units of 2^-60:", worst)
    assert max(worst.values()) <= 1.0, worst


# ---- 3. the float64 maps of the oracle and of the CPU twin ---------------------------------------------------------------------------
def _assert_float64_map(z, seed, chains, steps, d, what):
    """|z - z*| <= rad (2 pi 2^-52 + 4 2^-52): the angle 2 pi u2 is rounded once (half an ulp of a number below 2 pi) and pi once
    (2 pi u2 2^-53), which moves sin and cos by up to 2 pi 2^-52 absolutely; the rest -- the library's log, sqrt, sin and cos and one
    product -- are a few roundings of factors of order one.  Relative to a small normal this is unbounded: the `atol` of the
    contract tests."""
    u1, u2 = xv.stream_uniforms(seed, chains, steps, orc.STREAM_PROPOSAL, (d + 1) // 2)
    exact = xv.stream_normals_exact(seed, chains, steps, orc.STREAM_PROPOSAL, d)
    rad = np.repeat(np.sqrt(-2 * np.log1p(-u1.astype(xv.LD))), 2, axis=-1)[..., :d]
    err = np.abs(z.astype(xv.LD) - exact)
    bound = rad * xv.LD((2 * np.pi + 4) * 2.0 ** -52)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))))
    worst_rel = float(np.max(xv.rel(z, exact)))
    print("%s: %d normals, worst error %.3f of the bound; worst relative error %.1f 2^-52" % (what, z.size, worst, worst_rel))
    assert np.isfinite(z).all() and worst <= 1.0, (what, worst)
    return worst_rel


SEED, CHAINS, STEPS, DIM = 0x1234567887654321, np.arange(1000, 1000 + 500), [0, 1, 77, 2 ** 31 + 5], 50  # 10^5 coordinates


def test_oracle_float64_map_against_the_exact_reference():
    st = orc.PhiloxStream(SEED)
    z = np.stack([st.normals(CHAINS, t, DIM) for t in STEPS])
    _assert_float64_map(z, SEED, CHAINS, STEPS, DIM, "PhiloxStream.normals")


def test_cpu_twin_float64_map_against_the_exact_reference():
    import __graft_entry__ as g

    g.build()
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    e = Engine(len(CHAINS), DIM, seed=SEED, chain_offset=int(CHAINS[0]), lib=_lib.load_from(g.CPU_ABI_SO))
    z = np.stack([e.rng_probe(t)[0] for t in STEPS])
    u = np.stack([e.rng_probe(t)[1] for t in STEPS])
    e.close()
    st = orc.PhiloxStream(SEED)
    assert np.array_equal(u, np.stack([st.uniform(CHAINS, t) for t in STEPS]))
    _assert_float64_map(z, SEED, CHAINS, STEPS, DIM, "the CPU twin's normal_pair")


# ---- 4. the probe of tests/test_gpu_variate_map.py compiles as the replay program ----------------------------------------------------
@needs_hipcc
def test_probe_source_compiles_offline(tmp_path):
    rc, log, usage = compile_program(tmp_path, "variate_probe", xv.probe_source(), ["TDA_USER_REPLAY"])
    assert rc == 0, log[-3000:]
    assert set(usage) == {"tda_user_replay"}, usage
    print("variate probe: tda_user_replay", usage["tda_user_replay"])
