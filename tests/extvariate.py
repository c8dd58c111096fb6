"""The engine's variate map (tinyda_amd/csrc/tda_philox.h, normal_pair) against an exact reference, in ulps.

    z0 = sqrt(-2 ln(1 - u1)) cos(2 pi u2),  z1 = sqrt(-2 ln(1 - u1)) sin(2 pi u2),  u1, u2 on the 2^-53 grid of u53

`normals_exact` is that map in np.longdouble (64-bit significand), with the angle reduced exactly the way only a quarter-turn
reduction can be: a = 4 u2 and q = rint(a) are exact in fp64, so the remainder (a - q) pi / 2 carries the rounding of pi alone.
tests/test_variate_map.py pins it against mpmath at 120 bits.  `chosen_u1` / `chosen_u2` are the inputs at which such code goes
wrong and which a random 53-bit uniform never reaches; `stream_uniforms` gives the uniforms of any coordinate of the RNG contract
(include/tinyda_amd.h, "RNG stream") from the oracle's bit-exact, KAT-pinned Philox, so that every normal the engine exports has
an exact value.  The device branch of the header runs on the host through tests/variate_math_main.cpp (`build_shim`) and on the
device through a DeviceModel whose source is the header's text (`probe_source`).  No GPU and no oracle/_ref here."""
import os
import re
import shutil
import subprocess

import numpy as np

from oracle import tinyda_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinyda_amd", "csrc")
HEADER = os.path.join(CSRC, "tda_philox.h")
CXX = shutil.which("g++") or shutil.which("c++")

LD = np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63  # x87 extended; where long double is fp64 the reference is mpmath on every point (a switch, not a skip)
SAMPLE_DIVISOR = 1 if HAVE_LD else 8  # ... over samples eight times smaller
MP_BITS = 120
G = 2.0 ** -53  # the grid of u53
STREAM_DREAM_EPS = 7

# the bounds, derived from the header's claims and not from a run: ln within 1 ulp, -2 ln exact, sqrt correctly rounded, sin and cos within
# 2 ulp, one product: (1/2 * 2 + 1 + 4 + 1) 2^-53 = 3.5 2^-52 relative plus second order
LN_ULPS, SINCOS_ULPS, Z_REL = 1.0, 2.0, 4.0


# ---- the exact map ------------------------------------------------------------------------------------------------------------------
def _to_ld(v):
    """an mpmath number rounded to np.longdouble (through its two leading fp64 parts: exact to 106 bits)"""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def normals_mp(u1, u2):
    """(z0, z1, ln, sin, cos) at 120 bits, straight from the definition -- ln(1 - u1), sin and cos of 2 pi u2, no reduction of its
    own -- as object arrays of mpmath numbers"""
    import mpmath

    mp = mpmath.mp
    u1, u2 = np.broadcast_arrays(np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64))
    out = [np.empty(u1.shape, dtype=object) for _ in range(5)]
    with mpmath.workprec(MP_BITS):
        for i in np.ndindex(u1.shape):
            ln = mp.log(mp.mpf(1) - mp.mpf(float(u1[i])))
            ang = 2 * mp.pi * mp.mpf(float(u2[i]))
            # (at u2 = k / 4 one of the two is an exact zero of the function; 2 pi u2 at 120 bits is not: the zero is put there)
            k4 = 4.0 * float(u2[i])
            s = mp.mpf(0) if k4 in (0.0, 2.0) else mp.sin(ang)
            c = mp.mpf(0) if k4 in (1.0, 3.0) else mp.cos(ang)
            rad = mp.sqrt(-2 * ln)
            for o, v in zip(out, (rad * c, rad * s, ln, s, c)):
                o[i] = v
    return tuple(out)


def normals_exact(u1, u2):
    """(z0, z1, ln, sin, cos) in np.longdouble.  ln = log1p(-u1); the angle by quadrant: a = 4 u2, q = rint(a) (ties to even), y =
    (a - q) pi / 2 with |y| <= pi / 4, and sin, cos(2 pi u2) = those of y turned by q quarter turns, by selection and sign -- exact
    steps, so that the result is as good near the zeros of sin and cos as anywhere (a zero of the function is an exact 0)."""
    u1, u2 = np.broadcast_arrays(np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64))
    if not HAVE_LD:
        return tuple(np.vectorize(_to_ld, otypes=[LD])(v) for v in normals_mp(u1, u2))
    assert np.finfo(LD).nmant >= 63
    ln = np.log1p(-u1.astype(LD))
    rad = np.sqrt(-2 * ln)
    a = 4.0 * u2  # exact
    q = np.rint(a)
    y = (a - q).astype(LD) * LD("1.57079632679489661923132169163975144")  # (a - q: exact in fp64)
    sy, cy = np.sin(y), np.cos(y)
    k = q.astype(np.int64) % 4  # quarter turns: (sin, cos)(y + k pi / 2)
    sn = np.choose(k, [sy, cy, -sy, -cy])
    cs = np.choose(k, [cy, -sy, -cy, sy])
    return rad * cs, rad * sn, ln, sn, cs


def ulps(got, exact):
    """|got - exact| in units of the ulp of the fp64 binade that holds `exact`; where exact = 0 only got = +-0 is without error"""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        _, ex = np.frexp(np.abs(exact))  # |exact| in [2^(ex - 1), 2^ex): ulp = 2^(ex - 53)
        err = np.abs(got.astype(LD) - exact) / np.ldexp(LD(1), ex - 53)
    err = np.where(exact == 0, np.where(got == 0, LD(0), LD(np.inf)), err)
    return np.where(np.isfinite(got), err, LD(np.inf)).astype(np.float64)


def rel(got, exact):
    """|got - exact| / |exact| in units of 2^-52; where exact = 0 only got = +-0 is without error"""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        err = np.abs(got.astype(LD) - exact) / np.abs(exact) * LD(2.0 ** 52)
    err = np.where(exact == 0, np.where(got == 0, LD(0), LD(np.inf)), err)
    return np.where(np.isfinite(got), err, LD(np.inf)).astype(np.float64)


def map_errors(got, u1, u2):
    """worst errors of got = (ln, sin, cos, z0, z1) at (u1, u2) against normals_exact: {"ln", "sin", "cos": ulps, "z": rel}; NaN and
    inf count as infinite error"""
    z0, z1, ln, sn, cs = normals_exact(u1, u2)
    return {"ln": float(np.max(ulps(got[0], ln))), "sin": float(np.max(ulps(got[1], sn))), "cos": float(np.max(ulps(got[2], cs))),
            "z": float(max(np.max(rel(got[3], z0)), np.max(rel(got[4], z1))))}


def assert_map_bounds(errs, what):
    print(what, " ".join("%s %.3f" % kv for kv in sorted(errs.items())))
    assert errs["ln"] <= LN_ULPS, (what, errs)
    assert errs["sin"] <= SINCOS_ULPS and errs["cos"] <= SINCOS_ULPS, (what, errs)
    assert errs["z"] <= Z_REL, (what, errs)


def assert_axes_exact(sn, cs, z0, z1, u1, u2):
    """at u2 = k / 4 the vanishing component is +-0 and the other +-1 exactly; at u1 = 0 both normals are +-0"""
    for k, (s_want, c_want) in enumerate([(0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0)]):
        at = u2 == k / 4.0
        assert at.any()
        assert np.all(sn[at] == s_want) and np.all(cs[at] == c_want), (k, sn[at][:4], cs[at][:4])
    at = u1 == 0.0
    assert at.any() and np.all(z0[at] == 0.0) and np.all(z1[at] == 0.0)


TIE_SIN, TIE_COS = float.fromhex("0x1.6a09e667f3bccp-1"), float.fromhex("0x1.6a09e667f3bcdp-1")


def assert_ties_to_even(sn, cs, u2):
    """at u2 = 1/8, 3/8, 5/8, 7/8, 4 u2 is a tie of rint and goes to the even quadrant 0, 2, 2, 4: the remainder is +-pi / 4 and
    the sine is the SINE kernel's value there, the cosine the cosine kernel's.  Rounded half up (floor(a + 0.5): quadrants 1, 2,
    3, 4) the two kernels change places, which is as accurate and shows only in the last bit: the sine kernel gives sqrt(1/2)
    correctly rounded at pi / 4, the cosine kernel one ulp above (fma arithmetic without contraction: the same bits on the host and
    on the device)."""
    for k, (ss, sc) in zip((1, 3, 5, 7), ((1, 1), (1, -1), (-1, -1), (-1, 1))):
        at = u2 == k / 8.0
        assert at.any()
        assert np.all(sn[at] == ss * TIE_SIN) and np.all(cs[at] == sc * TIE_COS), (k, sn[at][0].hex(), cs[at][0].hex())


# ---- the contract's uniforms --------------------------------------------------------------------------------------------------------
def stream_uniforms(seed, chains, step, stream, n_pairs, block0=0):
    """(u1, u2) of the counter blocks block0 .. block0 + n_pairs - 1 of (global chain ids, step field, stream): [len(chains),
    n_pairs] for one step, [len(step), len(chains), n_pairs] for a vector of steps.  Chain ids and step fields wrap at 2^32 like
    the engine's casts.  DREAM(Z)'s eps normals (tda_kernels_dreamz.h): stream 7, step field step >> 1, block0 = delta + 1."""
    st = orc.PhiloxStream(seed)
    chains = (np.asarray(chains, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    steps = (np.atleast_1d(np.asarray(step, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32)
    blocks = (block0 + np.arange(n_pairs)).astype(np.uint32)
    x0, x1, x2, x3 = st.words(chains[None, :, None], steps[:, None, None], np.uint32(stream), blocks[None, None, :])
    u1, u2 = orc.u53(x0, x1), orc.u53(x2, x3)
    return (u1[0], u2[0]) if np.ndim(step) == 0 else (u1, u2)


def stream_normals_exact(seed, chains, step, stream, d, block0=0):
    """the exact normals [.., len(chains), d] of those coordinates in the exported layout (pair b -> dims 2b, 2b + 1; the z1 of an
    odd d's last pair is dropped), as np.longdouble"""
    u1, u2 = stream_uniforms(seed, chains, step, stream, (d + 1) // 2, block0)
    z0, z1 = normals_exact(u1, u2)[:2]
    z = np.empty(u1.shape[:-1] + (2 * u1.shape[-1],), dtype=LD)
    z[..., 0::2], z[..., 1::2] = z0, z1
    return z[..., :d]


# ---- chosen inputs ------------------------------------------------------------------------------------------------------------------
def _grid_random(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 53, size=n).astype(np.float64) * G


def chosen_u1(n_random=2 ** 16):
    """u1 = 1 - x, x on the 2^-53 grid in [2^-53, 1] (so that 1 - u1 = x exactly): 1; the 4096 grid points below 1 and the 4096
    above 0; 2^-k with both grid neighbours, k = 1 .. 53; the two grid points around sqrt(1/2) 2^-k, k = 0 .. 52 (the `low` switch
    of tda_log_unit in every binade); 0.75 and its neighbours; `n_random` points of default_rng(0) on the grid"""
    j = np.arange(1, 4097, dtype=np.float64)
    x = [np.array([1.0]), 1.0 - j * G, j * G]
    for k in range(1, 54):
        x.append(2.0 ** -k + np.array([-G, 0.0, G]))
    for k in range(0, 53):
        t = np.sqrt(LD(0.5)) * LD(2.0 ** (53 - k))  # sqrt(1/2) 2^-k in grid units: never an integer
        x.append(np.array([float(np.floor(t)), float(np.ceil(t))]) * G)
    x.append(0.75 + np.array([-G, 0.0, G]))
    x = np.concatenate(x)
    x = x[(x >= G) & (x <= 1.0)]
    assert np.all(x / G == np.rint(x / G))
    return np.concatenate([1.0 - x, _grid_random(n_random, 0)])


def chosen_u2(n_random=2 ** 16):
    """0; the 4096 grid points above 0 and below 1; k / 8 for k = 0 .. 7 with their +-2^-53 neighbours (the four ties of rint(4 u2)
    at odd k, which round to even -- 0, 2, 2, 4 --, and the four axes at even k); `n_random` points of default_rng(0) on the grid"""
    j = np.arange(1, 4097, dtype=np.float64)
    u = [np.array([0.0]), j * G, 1.0 - j * G]
    for k in range(8):
        u.append(k / 8.0 + np.array([-G, 0.0, G]))
    u = np.concatenate(u)
    u = u[(u >= 0.0) & (u < 1.0)]
    return np.concatenate([u, _grid_random(n_random, 0)])


def chosen_pairs(n_random=2 ** 16):
    """(u1, u2): the two chosen sets side by side (the shorter one repeated), then every u1 edge with every u2 edge: x in {1, 1 -
    2^-53, 2^-53, 2^-52, 1/2, 3/4, around sqrt(1/2)} times k / 8 and its neighbours"""
    c1, c2 = chosen_u1(n_random), chosen_u2(n_random)
    n = max(len(c1), len(c2))
    r2 = float(np.floor(np.sqrt(LD(0.5)) * LD(2.0 ** 53))) * G
    e1 = 1.0 - np.array([1.0, 1.0 - G, G, 2 * G, 0.5, 0.75, r2, r2 + G])
    e2 = np.concatenate([k / 8.0 + np.array([-G, 0.0, G]) for k in range(8)])
    e2 = e2[(e2 >= 0.0) & (e2 < 1.0)]
    a, b = np.meshgrid(e1, e2, indexing="ij")
    return np.concatenate([np.resize(c1, n), a.ravel()]), np.concatenate([np.resize(c2, n), b.ravel()])


def random_pairs(n, seed):
    return _grid_random(n, (seed, 1)), _grid_random(n, (seed, 2))


# ---- the device branch on the host --------------------------------------------------------------------------------------------------
def build_shim(work, include=CSRC, sanitized=False):
    """tests/variate_math_main.cpp over the tda_philox.h of `include`, as a stand-alone program at work / name: (path, None), or
    (None, why) when the sanitizers' runtime libraries are missing"""
    exe = os.path.join(str(work), "variate_math_sanitized" if sanitized else "variate_math")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitized else []
    r = subprocess.run([CXX, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra"] + flags + ["-I" + str(include), "-o", exe,
                        os.path.join(ROOT, "tests", "variate_math_main.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and sanitized and re.search(r"cannot find.*(asan|ubsan)", r.stdout):
        return None, "the sanitizers' runtime libraries are not installed"
    assert r.returncode == 0, r.stdout[-3000:]
    return exe, None


def shim_map(exe, u1, u2):
    """(ln, sin, cos, z0, z1) of the device branch at (u1, u2)"""
    u = np.stack([np.asarray(u1, dtype=np.float64).ravel(), np.asarray(u2, dtype=np.float64).ravel()], axis=1)
    r = subprocess.run([exe, "map"], input=u.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = np.frombuffer(r.stdout, dtype=np.float64).reshape(-1, 5)
    assert len(out) == len(u)
    return tuple(out[:, i] for i in range(5))


def shim_stream(exe, seed, chains, step, stream, n_pairs, block0=0):
    """(z0, z1) [len(chains), n_pairs] of normal_pair itself at those counters"""
    c, b = np.meshgrid(np.asarray(chains, dtype=np.uint64), (block0 + np.arange(n_pairs)).astype(np.uint64), indexing="ij")
    ctr = np.stack([np.full(c.shape, seed, dtype=np.uint64), c, np.full(c.shape, step, dtype=np.uint64), np.full(c.shape, stream, dtype=np.uint64), b], axis=-1)
    r = subprocess.run([exe, "stream"], input=ctr.tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = np.frombuffer(r.stdout, dtype=np.float64).reshape(c.shape + (2,))
    return out[..., 0], out[..., 1]


# ---- the header's text as a DeviceModel ---------------------------------------------------------------------------------------------
PROBE_OUTPUTS = 6  # ln, sin, cos, sqrt, z0, z1 at theta = (x = 1 - u1, u2, the root's argument, u1, u2)

PROBE_FORWARD = r"""
__device__ double tda_forward(const double* theta, int dim, int o) {
  if (o == 0) return tda::tda_log_unit(theta[0]);
  if (o == 3) return sqrt(theta[2]);
  double s, c;
  if (o < 3) {
    tda::tda_sincos_turn(theta[1], s, c);
    return o == 1 ? s : c;
  }
  const double u1 = theta[3], u2 = theta[4];
  const double rad = sqrt(-2.0 * tda::tda_log_unit(1.0 - u1));
  tda::tda_sincos_turn(u2, s, c);
  return o == 4 ? rad * c : rad * s;
}
"""


def probe_source(header=HEADER):
    """the text of tda_philox.h, read now, without its `#pragma once` and `#include` lines (the program it goes into has included
    hip/hip_runtime.h), with the fixed-width names spelled as the built-in types while that text lasts (hiprtc need not know them),
    and a tda_forward over its functions.  A line that this route cannot carry fails here, by its number."""
    lines = []
    for no, ln in enumerate(open(header).read().splitlines(), 1):
        if re.match(r"\s*#\s*pragma\s+once\b", ln) or re.match(r"\s*#\s*include\b", ln):
            continue
        assert not re.search(r"#\s*(include|import)|__has_include|_Pragma", ln), "tda_philox.h:%d cannot go into a source-defined model: %s" % (no, ln)
        lines.append(ln)
    text = "\n".join(lines)
    for name in ("tda_log_unit", "tda_sincos_turn", "__HIP_DEVICE_COMPILE__"):
        assert name in text, "tda_philox.h no longer holds " + name
    return ("#define uint32_t unsigned int\n#define uint64_t unsigned long long\n" + text
            + "\n#undef uint32_t\n#undef uint64_t\n" + PROBE_FORWARD)


def probe_thetas(u1, u2):
    """[n, 5] parameters of the probe at (u1, u2); the root's argument is -2 ln(1 - u1) rounded to fp64 (2^-52 at u1 = 0, where the
    logarithm vanishes: a root needs a positive argument to say anything)"""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    arg = (-2 * normals_exact(u1, 0.0)[2]).astype(np.float64)
    arg = np.where(arg > 0, arg, 2.0 ** -52)
    return np.stack([1.0 - u1, u2, arg, u1, u2], axis=1)


def probe_split(out):
    """(ln, sin, cos, z0, z1), sqrt of the probe's outputs [n, 6]"""
    return (out[:, 0], out[:, 1], out[:, 2], out[:, 4], out[:, 5]), out[:, 3]
