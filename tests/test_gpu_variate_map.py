"""The variate map on the device against the exact reference of tests/extvariate.py, in ulps.

a. The text of tinyda_amd/csrc/tda_philox.h as a source-defined model (xv.probe_source; tests/test_variate_map.py compiles it
   offline), evaluated by DeviceModel.evaluate at the chosen inputs and 2^16 random pairs: the bounds of the CPU tier -- ln within
   1 ulp, sin and cos within 2, a normal within 4 2^-52 relative --, the exact values on the axes, at the ties and at u1 = 0, and
   the device's sqrt equal to the correctly rounded root, on which the bound of a normal rests.
b. The library's own instances on the real stream: EVERY value that rng_probe / set_export hand out, from each kernel that
   writes exported normals, against the exact normals of its contract coordinate (seed, global chain, step, stream, block):
   within 4 2^-52 relative, no absolute floor, the accept uniforms bit-equal.  21 chains from global id 3 (not a multiple of the
   16-chain tile) or from 2^32 - 10 (the 32-bit id wraps inside the tile), 37 steps (two full 16-step groups and a ragged one),
   a step field next to 2^32 through rng_probe.

tools/variate_map_ulps.py runs the same helpers and records the measured maxima (profiles/variate_map_ulps.json)."""
import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extvariate as xv

pytestmark = pytest.mark.gpu

N, T, M, SEED = 21, 37, 8, (7 << 32) | 12345
OFFSETS = {"offset3": 3, "wrap": 2 ** 32 - 10}


# ---- a. the header's text under hiprtc ------------------------------------------------------------------------------------------------
def device_probe():
    """(u1, u2, (ln, sin, cos, z0, z1), (sqrt, its arguments)) of the probe at the chosen pairs, one DeviceModel.evaluate"""
    import tinyda_amd as tda

    u1, u2 = xv.chosen_pairs(2 ** 16 // xv.SAMPLE_DIVISOR)
    thetas = xv.probe_thetas(u1, u2)
    out = tda.DeviceModel(xv.probe_source(), xv.PROBE_OUTPUTS).evaluate(thetas)
    assert out.shape == (len(u1), xv.PROBE_OUTPUTS)
    got, root = xv.probe_split(out)
    return u1, u2, got, (root, thetas[:, 2])


def test_header_text_on_the_device_at_chosen_inputs():
    u1, u2, got, (root, arg) = device_probe()
    assert all(np.isfinite(g).all() for g in got)
    assert np.array_equal(root, np.sqrt(arg)), "the device's sqrt is not the correctly rounded root at %d of %d arguments" % (
        int((root != np.sqrt(arg)).sum()), len(arg))
    xv.assert_map_bounds(xv.map_errors(got, u1, u2), "chosen inputs (the header's text on the device)")
    xv.assert_axes_exact(got[1], got[2], got[3], got[4], u1, u2)
    xv.assert_ties_to_even(got[1], got[2], u2)


# ---- b. the library's own instances ---------------------------------------------------------------------------------------------------
def _problem(d, levels=1):
    rng = np.random.default_rng(100 + d)
    As = [rng.standard_normal((M, d)) / np.sqrt(d) for _ in range(levels)]
    return As, [rng.standard_normal(M) for _ in range(levels)], 0.1 * rng.standard_normal((N, d))


def _spd(d):
    return 1e-2 * (np.eye(d) + 0.3 * np.ones((d, d)) / d)  # not the identity, not diagonal


def export_k_propose(d, offset, step):
    """rng_probe: k_propose<DPAD>, one step at step field `step`"""
    from tinyda_amd.engine import Engine

    e = Engine(N, d, seed=SEED, chain_offset=offset)
    z, u = e.rng_probe(step)
    e.close()
    return z[None], u[None], np.array([step]), orc.STREAM_PROPOSAL, 0


def export_k_rng(d, offset):
    """a single-level run on the engine's own stream: k_rng<DPAD> (DPAD = 128 above 64 parameters), under a random walk with a
    full covariance (AdaptiveMetropolis above 64 parameters and at d = 33)"""
    from tinyda_amd.engine import Engine

    (A,), (y,), theta0 = _problem(d)
    e = Engine(N, d, seed=SEED, chain_offset=offset)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level(0, A, y, 0, 0.25)
    if d > 64 or d == 33:
        e.set_proposal(2, _spd(d), t0=100, period=100)
    else:
        e.set_proposal(0, _spd(d), scaling=0.7, adaptive=True, period=100)
    e.init(theta0)
    z, u = e.set_export(T)
    e.run(T)
    e.close()
    return z, u, np.arange(T), orc.STREAM_PROPOSAL, 0


def export_k_rng_direct(d, offset):
    """preconditioned Crank-Nicolson under the standard-normal prior in a two-level hierarchy: the proposal factor is the identity
    and the base level's increments are the normals themselves, k_rng_direct<DPAD>; one fine step over a subchain of T"""
    from tinyda_amd.engine import Engine

    As, ys, theta0 = _problem(d, 2)
    e = Engine(N, d, seed=SEED, chain_offset=offset, n_levels=2)
    e.set_prior(np.zeros(d), np.eye(d))
    for k in range(2):
        e.set_level(k, As[k], ys[k], 0, 0.25)
    e.set_proposal(1, None, scaling=0.05, adaptive=True, period=100)
    e.set_subchains([T])
    e.init(theta0)
    assert e.rows_per_level(1)[0] == T
    z, _ = e.set_export(T)
    e.run_levels(1)
    e.close()
    return z, None, np.arange(T), orc.STREAM_PROPOSAL, 0  # (the base level's accept uniforms of a hierarchy: tests/test_gpu_multilevel.py)


def export_dreamz(d, offset, delta=2):
    """DREAM(Z) as tests/test_gpu_dreamz.py sets it up: the eps normals of k_dreamz_draw (dz_normal_pair_call), stream 7, step
    field step >> 1, block delta + 1 + parameter, z0 on even steps and z1 on odd ones"""
    from tinyda_amd.engine import Engine

    M0, rng = 24, np.random.default_rng(1)
    e = Engine(N, d, seed=SEED, chain_offset=offset)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_rosenbrock(0, 1.0, 10.0, 0.0, 1.0)
    e.set_proposal_dreamz(M0, delta=delta, nCR=3, capacity=M0 + T)
    e.set_archive(rng.standard_normal((N, M0, d)))
    e.init(0.3 * rng.standard_normal((N, d)))
    eps, u = e.set_export(T)
    e.run(T)
    e.close()
    return eps, u, np.arange(T), xv.STREAM_DREAM_EPS, delta + 1


CASES = {}
for _d in (7, 64):
    for _o in OFFSETS:
        CASES["k_propose-d%d-%s" % (_d, _o)] = (export_k_propose, _d, _o, {"step": 5})
    CASES["k_propose-d%d-step_wrap" % _d] = (export_k_propose, _d, "offset3", {"step": 2 ** 32 - 3})
for _d in (1, 7, 16, 17, 33, 64):
    CASES["k_rng-d%d-offset3" % _d] = (export_k_rng, _d, "offset3", {})
CASES["k_rng-d17-wrap"] = (export_k_rng, 17, "wrap", {})
for _d in (2, 32, 63):
    CASES["k_rng_direct-d%d-offset3" % _d] = (export_k_rng_direct, _d, "offset3", {})
CASES["k_rng_direct-d63-wrap"] = (export_k_rng_direct, 63, "wrap", {})
for _d in (65, 96):
    CASES["wide-d%d-offset3" % _d] = (export_k_rng, _d, "offset3", {})
CASES["wide-d65-wrap"] = (export_k_rng, 65, "wrap", {})
CASES["dreamz-d5-offset3"] = (export_dreamz, 5, "offset3", {})
CASES["dreamz-d5-wrap"] = (export_dreamz, 5, "wrap", {})


def stream_case(name):
    """run one case: the worst relative error of its exported normals in units of 2^-52 and their number; the accept uniforms are
    asserted bit-equal here"""
    fn, d, off, kw = CASES[name]
    offset = OFFSETS[off]
    z, u, steps, stream, block0 = fn(d, offset, **kw)
    chains = (offset + np.arange(N)) & 0xFFFFFFFF
    assert z.shape == (len(steps), N, d)
    if stream == xv.STREAM_DREAM_EPS:  # one normal per parameter: pair `block0 + j` of step field t >> 1, its z0 or z1 by the step's parity
        u1, u2 = xv.stream_uniforms(SEED, chains, steps >> 1, stream, d, block0)
        z0, z1 = xv.normals_exact(u1, u2)[:2]
        exact = np.where((steps & 1)[:, None, None] == 0, z0, z1)
    else:
        exact = xv.stream_normals_exact(SEED, chains, steps, stream, d, block0)
    if u is not None:
        st = orc.PhiloxStream(SEED)
        want = np.stack([st.uniform(chains, int(t) & 0xFFFFFFFF) for t in steps])
        assert np.array_equal(u, want), "%s: accept uniforms differ from the contract's" % name
    assert np.isfinite(z).all(), name
    return float(np.max(xv.rel(z, exact))), z.size


@pytest.mark.parametrize("name", list(CASES))
def test_exported_normals_are_the_exact_map_of_the_stream(name):
    worst, n = stream_case(name)
    print("%s: %d normals, worst relative error %.3f 2^-52" % (name, n, worst))
    assert worst <= xv.Z_REL, (name, worst)
