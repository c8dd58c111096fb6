"""Wave-cooperative forward models on the device (tda_forward_wave / tda_gradient_wave, -DTDA_FORWARD_WAVE / -DTDA_GRADIENT_WAVE
of tda_user_program.hip): the reference's chains replayed through set_replay (g20), Philox forward mode against the oracle
running the NumPy twin at every lane and stride edge, bit-identity with the same model written per output, hierarchies,
DREAM(Z) (the tda_user_eval path), the program with all three source switches, MALA in the four forward x gradient
combinations, unwritten and NaN outputs, checkpoint resume, the LDS refusals and sample(backend='hip').

The bar is the project's: accept masks bit-exact, log-posterior 1e-10 relative; MALA as in test_gpu_mala_source.py.  The
proposal scales were chosen on the CPU with the oracle alone, for an acceptance rate inside [0.1, 0.9]."""
import warnings

import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from . import extprior as xp
from . import extwave as xw
from .extengine import (NOISE_SOURCE, PRIOR_SOURCE, assert_levels_resume_bitwise, assert_rate, assert_resume_bitwise, compare, compare_levels,
                        compare_replay, oracle_uniforms, run_forward, run_levels_forward, set_proposal)

pytestmark = pytest.mark.gpu

SIGMA = 0.01


def make_engine(src, d, y, N, prop, bs=0, seed=93, chain_offset=5, sigma=SIGMA, prior=None):
    from tinyda_amd.engine import Engine

    pm, pv = (np.zeros(d), np.ones(d)) if prior is None else prior
    e = Engine(N, d, seed=seed, chain_offset=chain_offset, block_steps=bs)
    e.set_prior(pm, np.diag(pv))
    e.set_level_source(0, src, y, 0, [sigma ** 2])
    set_proposal(e, prop)
    return e


def level_of(d, m, y, ksteps=48, sigma=SIGMA, prior=None, **kw):
    pm, pv = (np.zeros(d), np.ones(d)) if prior is None else prior
    return orc.CallableGaussianLevel(lambda th: xw.np_forward(th, m, ksteps, **kw), y, "iso", sigma ** 2, orc.MVNPrior(pm, np.diag(pv)))


def span_form_applies(d, prop):
    """Under AdaptiveMetropolis with t0 < d only.  There the first adapted covariance is the sample covariance of t0 < d states,
    of rank below d, made definite by sd * epsilon * I alone (epsilon = 1e-6, sd = 2.4^2 / d): its condition number is the ratio
    of the chain's variance to that, 1e3 .. 1e4 here, so its Cholesky factor, which the engine and the oracle compute in
    different orders, agrees to about d * 2^-53 * 1e4 = 1e-10 relative (the covariance itself is held to 1e-9 below).  A proposal
    increment of 0.01 .. 0.1 then differs by 1e-12 .. 1e-11 absolute per step, which is above atol = 1e-12 wherever a component
    of the state is within 1e-3 of zero (d64_m63: 12 of 99840 entries miss rtol = 1e-9, atol = 1e-12, the largest error of any
    entry 1.2e-11; d128_m300: 1.2e-10), and has nothing to do with the model under test.  Every other case, above 64 parameters
    too, is held to rtol = 1e-9, atol = 1e-12 (the largest error among them is 3e-12, under MALA at d = 96)."""
    return prop["kind"] == "am" and prop["t0"] < d


# ---- 1. the reference's chains ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [0, 7])
@pytest.mark.parametrize("name", ["g20_wave_grw", "g20_wave_am"])
def test_engine_replays_reference_chain(golden, name, bs):
    g = golden(name)
    am = "C0" in g.files
    N, T1, d = g["theta"].shape
    if am:
        prop = dict(kind="am", C0=g["C0"], sd=float(g["sd"]), epsilon=float(g["epsilon"]), t0=int(g["t0"]), period=int(g["period"]))
    else:
        prop = dict(kind="grw", C=g["C"], scaling=float(g["scaling0"]), adaptive=bool(g["adaptive"]), gamma=float(g["gamma"]), period=int(g["period"]))
    e = make_engine(xw.source(), d, g["data"], N, prop, bs, seed=1, chain_offset=0, sigma=float(np.sqrt(g["sigma2"])))
    e.init(g["theta0"])
    e.set_replay(np.swapaxes(g["z"], 0, 1), np.swapaxes(g["u"], 0, 1))
    params, stats, acc = e.run_host(T1 - 1)
    state = e.proposal_state(want_am=am)
    e.close()
    compare_replay(params, stats, acc, g, **(dict(C=state["C"]) if am else dict(scaling=state["scaling"])))
    assert_rate(g["accepted"][:, 1:])


# ---- 2. Philox forward mode against the oracle ------------------------------------------------------------------------------------
# (d, m): one or two parameters per lane, m below, at and above one stride of 64 -> proposal (the oracle's description), block_steps
CASES = {
    (1, 1): (dict(kind="grw", C=np.eye(1), scaling=0.8), 0),
    (5, 23): (dict(kind="grw", C=1e-3 * np.eye(5), scaling=1.0, adaptive=True, gamma=1.01, period=20), 33),
    (64, 63): (dict(kind="am", C0=3e-4 * np.eye(64), t0=40, period=20), 0),
    (64, 64): (dict(kind="pcn", scaling=0.02), 0),
    (65, 65): (dict(kind="grw", C=2e-5 * np.eye(65), scaling=1.0, adaptive=True, gamma=1.01, period=20), 16),
    (96, 130): (dict(kind="grw", C=1e-5 * np.eye(96), scaling=1.0, adaptive=True, gamma=1.01, period=20), 0),
    (128, 300): (dict(kind="am", C0=5e-6 * np.eye(128), t0=40, period=20, adaptive=True, gamma=1.01), 33),
    (7, 2048): (dict(kind="am", C0=2e-6 * np.eye(7), t0=40, period=20), 0),
}


@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "d%d_m%d" % s)
def test_philox_forward_matches_oracle(shape):
    d, m = shape
    prop, bs = CASES[shape]
    N, T = 13, 120
    _, y, theta0 = xw.problem(d, m, N, seed=d * 1000 + m)
    params, stats, acc, _, C, z, u = run_forward(make_engine(xw.source(), d, y, N, prop, bs), theta0, T, prop)
    ref = orc.run_mh(level_of(d, m, y), prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    compare(params, stats, acc, ref, span_form=span_form_applies(d, prop))
    if C is not None and d <= 64:  # (above 64 parameters the adapted covariance is the subject of test_gpu_wide.py, not of the model's staging)
        np.testing.assert_allclose(C, ref["C"], rtol=1e-9, atol=1e-14)


# ---- 3. the same model written per output: bit-identical ----------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(5, 23), (70, 65), (64, 96)])
def test_bit_identical_to_the_per_output_form(d, m):
    """tda_forward runs the whole solve in its lane and returns output o: the arithmetic is elementwise and in the same order,
    so anything but equality is a fault of the staging through LDS.  (64, 96) is the shape tools/forward_wave_rate.py times."""
    N, T = 13, 60
    _, y, theta0 = xw.problem(d, m, N, seed=31 + d)
    prop = dict(kind="am", C0=(1e-3 if d == 5 else 2e-4 if d == 70 else 2e-5) * np.eye(d), t0=20, period=20)
    outs = []
    for fwd in ("wave", "per_output"):
        e = make_engine(xw.source(fwd, m=m), d, y, N, prop, 16)
        e.init(theta0)
        outs.append(e.run_host(T))
        e.close()
    assert 0.05 < outs[0][2].mean() < 0.95
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---- 4. hierarchies -----------------------------------------------------------------------------------------------------------------
def _linear_surrogate(d, m, at):
    """the model linearised at `at` by central differences: (A, b) with F ~ A theta + b"""
    A = np.empty((m, d))
    for j in range(d):
        e = np.zeros(d)
        e[j] = 1e-5
        A[:, j] = (xw.np_forward(at + e, m)[0] - xw.np_forward(at - e, m)[0]) / 2e-5
    return A, xw.np_forward(at, m)[0] - A @ at


@pytest.mark.parametrize("case", ["da_wave", "mlda_wave", "mlda_mixed"])
def test_hierarchy_matches_oracle(case):
    """wave levels at KSTEPS = 12 / 24 / 48 (base level: tda_user_steps, above: tda_user_level_action), and a hierarchy of a linear
    level, a per-output level and a wave level, against the oracle's Delayed Acceptance / MLDA"""
    from tinyda_amd.engine import Engine

    d, m, N, seed = 5, 23, 16, 993
    truth, y, theta0 = xw.problem(d, m, N, seed=77)
    if case == "da_wave":
        ks, sl, n_fine, bs = [24, 48], [3], 25, 0
        prop = dict(kind="grw", C=1e-3 * np.eye(d), scaling=1.0, adaptive=True, gamma=1.02, period=15)
    else:
        ks, sl, n_fine, bs = [12, 24, 48], [3, 2], 14, 7
        prop = dict(kind="am", C0=1e-3 * np.eye(d), t0=20, period=10)
    nl = len(ks)
    sig = [0.03] * (nl - 1) + [SIGMA]  # (the coarse fidelities are off by more than the noise: their levels carry an inflated variance)
    twins = [lambda th, k=k: xw.np_forward(th, m, k) for k in ks]
    e = Engine(N, d, seed=seed, n_levels=nl, block_steps=bs)
    e.set_prior(np.zeros(d), np.eye(d))
    for i, k in enumerate(ks):
        if case == "mlda_mixed" and i == 0:
            A, b = _linear_surrogate(d, m, truth)
            twins[0] = lambda th: np.atleast_2d(th) @ A.T + b
            e.set_level(0, A, y, 0, sig[0] ** 2, b=b)
        else:
            fwd = "per_output" if case == "mlda_mixed" and i == 1 else "wave"
            e.set_level_source(i, xw.source(fwd, m=m, ksteps=k), y, 0, [sig[i] ** 2])
    set_proposal(e, prop)
    e.set_subchains(sl, False)
    e.init(theta0)
    rows, z, outs, scal = run_levels_forward(e, n_fine)
    us, ridx = oracle_uniforms(seed, N, rows, sl, None)
    prior = orc.MVNPrior(np.zeros(d), np.eye(d))
    levels = [orc.CallableGaussianLevel(twins[i], y, "iso", sig[i] ** 2, prior) for i in range(nl)]
    res, pstate = orc.run_multilevel(levels, prop, sl, theta0, np.swapaxes(z, 0, 1), us, n_fine, ridx)
    assert_rate(res[-1]["accepted"][:, 1:])
    assert_rate(res[0]["accepted"])
    np.testing.assert_allclose(scal, pstate.scaling, rtol=1e-12)
    compare_levels(outs, res)


# ---- 5. DREAM(Z): jump -> tda_user_eval -> accept ------------------------------------------------------------------------------------
def test_dreamz_over_the_wave_model():
    from tests.test_gpu_dreamz import RTOL, _philox_dreamz_variates
    from tinyda_amd.engine import Engine

    d, m, N, T, M0, delta, nCR, seed = 5, 70, 19, 90, 24, 2, 3, 1357
    rng = np.random.default_rng(6)
    truth, y, _ = xw.problem(d, m, N, seed=61, sigma=0.05)
    e = Engine(N, d, seed=seed, block_steps=16)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, xw.source(), y, 0, [0.05 ** 2])
    e.set_proposal_dreamz(M0, delta=delta, nCR=nCR, capacity=M0 + T)
    Z0 = truth + 0.3 * rng.standard_normal((N, M0, d))
    theta0 = truth + 0.1 * rng.standard_normal((N, d))
    e.set_archive(Z0)
    e.init(theta0)
    eps, _ = e.set_export(T)
    params, stats, acc = e.run_host(T)
    e.close()
    v = _philox_dreamz_variates(seed, N, T, d, delta, nCR, M0, None)
    cdf = np.cumsum(np.full(nCR, 1.0 / nCR))
    mcr = np.minimum((v["u_mcr"][..., None] >= cdf).sum(-1), nCR - 1)
    var = dict(r=v["r"], mcr=mcr, sub_u=v["sub_u"], forced=v["forced"], e_u=v["e_u"], eps_n=np.swapaxes(eps, 0, 1), u=v["u"])
    cfg = dict(M0=M0, delta=delta, nCR=nCR, adaptive=False, period=100, gamma=1.01, b=5e-2, b_star=1e-6)
    res = orc.run_dreamz(level_of(d, m, y, sigma=0.05), cfg, theta0, Z0, var)
    assert np.array_equal(acc, res["accepted"][:, 1:].T)
    np.testing.assert_allclose(stats[:, :, 2], res["logpost"][:, 1:].T, rtol=RTOL)
    assert 0.02 < acc.mean() < 0.95


# ---- 6. all three source switches in one program ------------------------------------------------------------------------------------
def test_wave_model_with_source_likelihood_and_source_prior():
    """the wave model + a Student-t DeviceLogLike + a JointPrior of five scipy families under AdaptiveMetropolis"""
    from tinyda_amd.engine import Engine

    d, m, N, T = 13, 70, 13, 120
    names = ("lognorm", "gamma", "beta", "norm", "uniform")
    rng = np.random.default_rng(13070)
    comps = xp.components(d, names)
    truth, theta0 = xp.starts_near_lower_edges(comps, N, rng)
    par = 0.01 * (1.0 + 0.1 * np.arange(m) / m)
    y = xw.np_forward(truth, m)[0] + par * rng.standard_t(4, m)
    p, q, psrc = xp.family_source(comps)
    prop = dict(kind="am", C0=3e-5 * np.eye(d), t0=20, period=20)
    e = Engine(N, d, seed=93, chain_offset=5)
    e.set_prior_joint(np.full(d, PRIOR_SOURCE), p, q)
    e.set_level_source(0, xw.source() + xl.KINDS["t"][0] + "\n" + psrc, y, NOISE_SOURCE, par)
    set_proposal(e, prop)
    params, stats, acc, _, _, z, u = run_forward(e, theta0, T, prop)
    level = xl.LogLikeLevel(lambda th: xw.np_forward(th, m), y, par, xl.KINDS["t"][1], xp.FamilyPrior(comps))
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    compare(params, stats, acc, ref)


# ---- 7. MALA: the four forward x gradient combinations ----------------------------------------------------------------------------
# (the noise and the scalings keep the drift theta -> theta + s^2/2 grad contractive, as test_gpu_mala_source.py explains)
MALA_SIGMA = 0.05
MALA_CASES = {  # forward, gradient, d, m, scaling, adaptive
    "wave_wave_d5_m23": ("wave", "wave", 5, 23, 0.45, False),
    "wave_wave_d96_m130": ("wave", "wave", 96, 130, 0.3, True),
    "wave_per_parameter_d5_m23": ("wave", "per_parameter", 5, 23, 0.45, False),
    "per_output_wave_d5_m23": ("per_output", "wave", 5, 23, 0.45, False),
    "per_output_per_parameter_d5_m23": ("per_output", "per_parameter", 5, 23, 0.45, False),
}


@pytest.mark.parametrize("case", list(MALA_CASES))
def test_mala_matches_oracle(case):
    fwd, grad, d, m, scaling, adaptive = MALA_CASES[case]
    N, T = 13, 100
    prior = (0.1 * np.ones(d), 0.5 + 0.01 * np.arange(d))
    _, y, theta0 = xw.problem(d, m, N, seed=d * 1000 + m + 1, sigma=MALA_SIGMA)
    prop = dict(kind="mala", scaling=scaling, adaptive=adaptive, gamma=1.01, period=20)
    e = make_engine(xw.source(fwd, grad, m=m), d, y, N, prop, 33, seed=91, chain_offset=3, sigma=MALA_SIGMA, prior=prior)
    params, stats, acc, scal, _, z, u = run_forward(e, theta0, T, prop)
    level = xw.GradLevel(lambda th: xw.np_forward(th, m), y, "iso", MALA_SIGMA ** 2, orc.MVNPrior(prior[0], np.diag(prior[1])))
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    assert_rate(ref["accepted"][:, 1:])
    compare(params, stats, acc, ref, scal)  # (MALA: rtol 1e-9, atol 1e-12 at every size, as test_gpu_mala_source.py)


# ---- 8. unwritten and NaN outputs ---------------------------------------------------------------------------------------------------
def test_an_output_left_unwritten_rejects_every_proposal():
    """out is NaN before the call: a model that skips its last output proposes nothing acceptable"""
    d, m, N, T = 5, 23, 13, 40
    _, y, theta0 = xw.problem(d, m, N, seed=5)
    e = make_engine(xw.source(skip_last=True), d, y, N, dict(kind="grw", C=1e-3 * np.eye(d), scaling=1.0))
    e.init(theta0)
    params, stats, acc = e.run_host(T)
    e.close()
    assert not acc.any()
    assert np.array_equal(params, np.broadcast_to(theta0, params.shape))


def test_nan_region_is_rejected():
    d, m, N, T = 5, 23, 13, 120
    _, y, theta0 = xw.problem(d, m, N, seed=5023)
    thr = float(np.max(theta0[:, 0])) + 0.005
    prop = dict(kind="grw", C=1e-3 * np.eye(d), scaling=1.0, adaptive=True, gamma=1.01, period=20)
    params, stats, acc, _, _, z, u = run_forward(make_engine(xw.source(nan_above=thr), d, y, N, prop), theta0, T, prop)
    zs, us = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    ref = orc.run_mh(level_of(d, m, y, nan_above=thr), prop, theta0, zs, us)
    compare(params, stats, acc, ref)
    assert np.all(np.isfinite(stats)) and np.all(params[:, :, 0] <= thr)
    # proposals into the NaN region were made (and rejected): without it the same variates give another trace
    assert not np.array_equal(orc.run_mh(level_of(d, m, y), prop, theta0, zs, us)["accepted"], ref["accepted"])


# ---- 9. checkpoints: no new state ---------------------------------------------------------------------------------------------------
def test_checkpoint_resume_is_bitwise():
    """get_state mid period, set_state into a fresh engine"""
    d, m, N = 13, 100, 12
    _, y, theta0 = xw.problem(d, m, N, seed=9)

    def make():
        e = make_engine(xw.source(), d, y, N, dict(kind="am", C0=1e-4 * np.eye(d), t0=20, period=20), 16)
        e.init(theta0)
        return e

    assert_resume_bitwise(make)


def test_hierarchy_checkpoint_resume_is_bitwise():
    from tinyda_amd.engine import Engine

    d, m, N = 5, 23, 12
    _, y, theta0 = xw.problem(d, m, N, seed=41)
    e = Engine(N, d, seed=77, n_levels=2)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, xw.source(ksteps=24), y, 0, [0.03 ** 2])
    e.set_level_source(1, xw.source(), y, 0, [SIGMA ** 2])
    e.set_proposal(0, 1e-3 * np.eye(d), scaling=1.0, adaptive=True, period=10)
    e.set_subchains([3], False)
    e.init(theta0)
    a = assert_levels_resume_bitwise(e)
    assert a[1][2].any()


# ---- 10. the LDS of a chain is capped at 64 KiB -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["m8100", "workspace8192", "workspace32768"])
def test_more_than_64_kib_of_lds_is_refused(case):
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    d = 5
    if case == "m8100":  # 8 * 8100 bytes of outputs + 1024 bytes of parameters
        m, nbytes = 8100, (8 * 8100, 1024)
        src = "__device__ void tda_forward_wave(const double* theta, int dim, double* out, int n, double* work, int lane) {\n" \
              "  for (int o = lane; o < n; o += 64) out[o] = theta[o % dim];\n}\n"
    else:  # 8 * 8192 bytes of workspace + 1024 + 8 * 64; 8 * 32768 is beyond the hardware's 160 KiB, which the compiler refuses itself
        words = int(case[len("workspace"):])
        m, nbytes = 64, (8 * 64, 8 * words + 1024) + ((160 * 1024,) if words == 32768 else ())
        src = xw.source().replace("#define TDA_WORKSPACE (WV_K * 64)", "#define TDA_WORKSPACE %d" % words)
        assert "TDA_WORKSPACE %d" % words in src
    e = Engine(4, d, seed=1)
    e.set_prior(np.zeros(d), np.eye(d))
    with pytest.raises(_lib.EngineError, match="64 KiB") as err:
        e.set_level_source(0, src, np.zeros(m), 0, [1.0])
    e.close()
    msg = str(err.value)
    assert "TDA_WORKSPACE" in msg and all(str(n) in msg for n in nbytes), msg


# ---- 11. sample() ---------------------------------------------------------------------------------------------------------------------
def test_sample_api_runs_the_wave_model_on_the_device():
    import tinyda_amd as tda
    from tinyda_amd.api import HostFallbackWarning

    d, m = 5, 23
    truth, y, _ = xw.problem(d, m, 1, seed=3)
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(y, SIGMA ** 2 * np.eye(m)),
                         tda.DeviceModel(xw.source(), m, reference=lambda t: xw.np_forward(t, m)[0]))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.AdaptiveMetropolis(1e-3 * np.eye(d), t0=50, period=50), 200, n_chains=12, initial_parameters=truth, seed=3)
    assert not [x for x in w if issubclass(x.category, HostFallbackWarning)]
    assert res["backend"] == "hip" and res["n_chains"] == 12
    link = res["chain_0"][-1]
    assert np.isclose(link.posterior, post.create_link(link.parameters).posterior, rtol=1e-10)
