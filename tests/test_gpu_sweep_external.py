"""Seeded sweep of source-defined (hiprtc) and batched host-callback forward models against the oracle on the exported
Philox stream: the fused kernels (tda_user_steps, tda_user_mala_steps, tda_user_level_action) and the stepwise ones
(k_ext_propose / k_ext_accept / k_ext_level_action) at the shapes where one-wave-per-chain code breaks -- 64 / 65 / 128
parameters (a second parameter per lane), 63 / 64 / 65 outputs (the lanes' output stride), MALA's 2048 outputs of LDS.
Same bar as test_gpu_sweep.py: accept masks bit-exact, log-posterior within 1e-10 relative.  Every generator starts with a
fixed list of boundary cases and fills up with random ones; test_sweep_external_cases.py checks what the lists cover.

The model is tests/extmodel.py: one source whose d and m arrive at run time, its NumPy twin as the oracle's model and as the
callback, and the twin's vector-Jacobian product for MALA."""
import warnings

import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from .extengine import oracle_uniforms
from .extmodel import GradLevel, np_forward, np_jacobian, source, weights
from .test_gpu_sweep import AM_LOOSE_RTOL, RTOL, _small_am, _spd

pytestmark = pytest.mark.gpu

# AdaptiveMetropolis parameters: the device's Cholesky of the swapped-in covariance and LAPACK's differ in the last bits, and the
# proposals carry that into the states -- test_gpu_sweep.py's bar (rtol 1e-8, atol 1e-10) with the absolute part at 5e-10: the first
# run saw 1.6e-11 (single level, d = 17, 140 steps) and 1.5e-10 (hierarchy case 0: d = 128, one chain, 550 base steps)
AM_PARAMS_ATOL = 5e-10

SINGLE_D = [1, 2, 3, 17, 31, 32, 33, 63, 64, 65, 66, 96, 127, 128]
SINGLE_M = [1, 2, 17, 63, 64, 65, 129, 300, 2048]
KINDS = ["grw", "grw_adaptive", "pcn", "pcn_adaptive", "am", "am_adaptive"]

# (model, d, m, kind, noise, prior, variant): kind "indep" / "owcn" and noise "dense" take the stepwise k_ext_* path
SINGLE_FIXED = [
    ("source", 1, 1, "grw", "iso", "identity", None),
    ("source", 64, 64, "am_adaptive", "diag", "diag", None),
    ("source", 65, 65, "pcn_adaptive", "iso", "diag0", "device"),
    ("source", 128, 2048, "grw_adaptive", "diag", "joint", "thin"),
    ("source", 128, 63, "am", "iso", "diag", "resume"),
    ("source", 64, 1, "pcn", "diag", "identity", None),
    ("source", 65, 2048, "grw", "iso", "joint", None),
    ("source", 1, 65, "am_adaptive", "iso", "joint", "device"),
    ("source", 127, 64, "grw", "diag", "identity", "thin"),
    ("callback", 1, 17, "pcn", "diag", "identity", None),
    ("callback", 64, 65, "grw_adaptive", "iso", "joint", "resume"),
    ("callback", 65, 64, "am_adaptive", "diag", "diag", "thin"),
    ("callback", 128, 129, "grw", "iso", "diag", "device"),
    ("source", 33, 300, "grw_adaptive", "dense", "diag", None),
    ("source", 17, 65, "indep", "iso", "diag", None),
    ("callback", 17, 2, "owcn", "diag", "identity", None),
    ("callback", 64, 300, "pcn", "dense", "identity", "thin"),
    ("source", 63, 17, "owcn", "iso", "diag0", "resume"),
]
N_SINGLE = 64


def _single_case(i):
    rng = np.random.default_rng(11000 + i)
    if i < len(SINGLE_FIXED):
        model, d, m, kind, noise, prior, variant = SINGLE_FIXED[i]
    else:
        model = str(rng.choice(["source", "callback"]))
        d = int(rng.choice(SINGLE_D))
        m = int(rng.choice(SINGLE_M))
        kind = str(rng.choice(KINDS + (["indep", "owcn"] if d <= 64 else [])))
        noise = str(rng.choice(["iso", "diag"] + (["dense"] if d <= 64 and m <= 300 else [])))
        if kind in ("pcn", "pcn_adaptive", "owcn"):  # pCN / OWCN ignore the prior mean and need a Gaussian prior
            prior = str(rng.choice(["identity", "diag0"]))
        elif kind == "indep" or noise == "dense":  # the engine refuses uniform components beside dense noise
            prior = str(rng.choice(["identity", "diag"]))
        else:
            prior = str(rng.choice(["identity", "diag", "joint"]))
        variant = [None, None, None, "thin", "device", "resume"][int(rng.integers(0, 6))]
    if kind == "indep":  # (a Gaussian around the mode: above ~20 parameters the model's curvature makes its acceptance collapse)
        d = min(d, 17)
    N = int(rng.choice([1, 2, 15, 17, 33]))
    T = int(rng.choice([1, 37, 90, 140])) if i >= len(SINGLE_FIXED) else int(rng.choice([37, 90, 140]))
    if variant == "resume" and T < 37:
        T = 37
    block = int(rng.choice([0, 7, 16, 33]))
    split = bool(rng.integers(0, 2)) and variant != "resume"
    return dict(i=i, model=model, d=d, m=m, N=N, T=T, kind=kind, noise=noise, prior=prior, block=block, split=split,
                variant=variant, thin=3 if variant == "thin" else 1)


MALA_D = [1, 2, 63, 64, 65, 127, 128]
MALA_M = [1, 63, 64, 65, 1000, 2048]
# (d, m, noise, adaptive, variant)
MALA_FIXED = [
    (1, 1, "iso", False, None),
    (64, 64, "diag", True, None),
    (65, 65, "iso", False, "device"),
    (128, 2048, "diag", True, "resume"),
    (127, 1000, "iso", True, "thin"),
    (63, 63, "diag", False, None),
    (2, 2048, "iso", False, None),
    (128, 1, "diag", False, None),
    (65, 1000, "diag", True, "resume"),
    (64, 65, "iso", True, "thin"),
    (1, 64, "diag", True, "device"),
]
N_MALA = 32


def _mala_case(i):
    rng = np.random.default_rng(12000 + i)
    if i < len(MALA_FIXED):
        d, m, noise, adaptive, variant = MALA_FIXED[i]
    else:
        d, m = int(rng.choice(MALA_D)), int(rng.choice(MALA_M))
        noise = str(rng.choice(["iso", "diag"]))
        adaptive = bool(rng.integers(0, 2))
        variant = [None, None, "thin", "device", "resume"][int(rng.integers(0, 5))]
    N = int(rng.choice([1, 2, 15, 17, 33]))
    T = int(rng.choice([37, 90, 140]))
    block = int(rng.choice([0, 7, 16, 33]))
    split = bool(rng.integers(0, 2)) and variant != "resume"
    return dict(i=i, model="source", d=d, m=m, N=N, T=T, kind="mala_adaptive" if adaptive else "mala", noise=noise, prior="diag",
                block=block, split=split, variant=variant, thin=3 if variant == "thin" else 1)


ML_D = [2, 17, 64, 65, 128]
ML_M = [3, 64, 65, 130]
# (models coarsest first, d, ms, kind, randomize_subchain_length)
ML_FIXED = [
    (("linear", "source", "callback", "source"), 128, (64, 3, 130, 65), "am_adaptive", False),
    (("source", "source"), 65, (65, 64), "pcn", True),
    (("callback", "source", "linear"), 64, (130, 65, 64), "grw_adaptive", False),
    (("source", "callback", "source", "callback"), 65, (3, 65, 64, 130), "pcn", False),
    (("callback", "callback"), 128, (64, 65), "grw_adaptive", True),
    (("linear", "source"), 2, (3, 64), "am", False),
    (("source", "linear", "source"), 17, (65, 130, 3), "am_adaptive", False),
]
N_ML = 24


def _ml_case(i):
    rng = np.random.default_rng(13000 + i)
    if i < len(ML_FIXED):
        models, d, ms, kind, rnd = ML_FIXED[i]
        nl = len(models)
    else:
        nl = int(rng.choice([2, 3, 4]))
        d = int(rng.choice(ML_D))
        models = tuple(str(x) for x in rng.choice(["source", "callback", "linear"], size=nl))
        if all(x == "linear" for x in models):  # at least one external level: the host-sequenced path
            models = models[:-1] + ("source",)
        ms = tuple(int(x) for x in rng.choice(ML_M, size=nl))
        kind = str(rng.choice(["pcn", "grw_adaptive", "am", "am_adaptive"]))
        rnd = None
    sl = [int(x) for x in rng.choice([1, 2, 3, 5], size=nl - 1)]
    randomize = bool(nl == 2 and sl[0] > 1 and rng.integers(0, 2)) if rnd is None else rnd
    if randomize and sl[0] == 1:
        sl[0] = 3
    N = int(rng.choice([1, 2, 15, 17, 33]))
    n_fine = int(rng.choice([6, 11, 40] if int(np.prod(sl)) <= 6 else [6, 11]))
    noise = str(rng.choice(["iso", "diag"]))
    block = int(rng.choice([0, 7, 16]))
    return dict(i=i, nl=nl, models=models, d=d, ms=ms, sl=sl, randomize=randomize, N=N, n_fine=n_fine, kind=kind, noise=noise,
                block=block, T=n_fine)


# ---- problems -----------------------------------------------------------------------------------------------------------
def _noise(rng, kind, m):
    if kind == "iso":
        return 0, 0.01, 0.01
    if kind == "diag":
        nz = 0.01 * (0.5 + rng.random(m))
        return 1, nz, nz
    nz = _spd(rng, m, 0.01)
    return 2, nz, nz


def _prior(rng, kind, d, truth):
    """(engine setter, oracle prior, Gaussian proxy covariance for the curvature, support bounds or None)"""
    if kind in ("identity", "diag", "diag0"):
        pm = np.zeros(d) if kind != "diag" else 0.1 * rng.standard_normal(d)
        pv = np.ones(d) if kind == "identity" else 0.5 + rng.random(d)
        return (lambda e: e.set_prior(pm, np.diag(pv))), orc.MVNPrior(pm, np.diag(pv)), np.diag(pv), None
    kinds = rng.integers(0, 2, size=d)
    a, b = 0.2 + 0.5 * rng.random(d), 0.2 + 0.5 * rng.random(d)
    loc = np.where(kinds == 1, truth - a, 0.1 * rng.standard_normal(d))
    scale = np.where(kinds == 1, a + b, np.sqrt(0.5 + rng.random(d)))
    pr = orc.JointPriorOracle(kinds, loc, scale)
    lo, hi = np.where(kinds == 1, loc, -np.inf), np.where(kinds == 1, loc + scale, np.inf)
    return (lambda e: e.set_prior_joint(kinds, loc, scale)), pr, pr.cov, (lo, hi)


def _mode(truth, y, m, W, Pinv, pmean, shift=0.0, coup=0.5, bounds=None):
    """a few Gauss-Newton steps from the truth towards the posterior mode (Gaussian proxy prior); H there"""
    th = truth.copy()
    for _ in range(6):
        J = np_jacobian(th, m, shift, coup)
        H = J.T @ W @ J + Pinv
        g = J.T @ W @ (y - np_forward(th, m, shift=shift, coup=coup)[0]) + Pinv @ (pmean - th)
        th = th + 0.7 * np.linalg.solve(H, g)
        if bounds is not None:
            gap = np.where(np.isfinite(bounds[0]), 0.05 * (bounds[1] - bounds[0]), 0.0)
            th = np.clip(th, bounds[0] + gap, bounds[1] - gap)
    J = np_jacobian(th, m, shift, coup)
    H = J.T @ W @ J + Pinv
    return th, 0.5 * (H + H.T)


def _single_problem(c):
    d, m, N = c["d"], c["m"], c["N"]
    rng = np.random.default_rng(15000 + c["i"])
    truth = 0.3 * rng.standard_normal(d)
    nk, nz, onz = _noise(rng, c["noise"], m)
    noise_draw = rng.standard_normal(m) * (np.sqrt(np.diag(nz)) if nk == 2 else np.sqrt(nz))
    y = np_forward(truth, m)[0] + noise_draw
    set_prior, prior, pcov, bounds = _prior(rng, c["prior"], d, truth)
    W = np.linalg.inv(nz) if nk == 2 else np.diag(np.broadcast_to(1.0 / np.asarray(nz), (m,)))
    pmean = np.asarray(prior.mean)
    mode, H = _mode(truth, y, m, W, np.linalg.inv(pcov), pmean, bounds=bounds)
    Hinv = np.linalg.inv(H)
    Hinv = 0.5 * (Hinv + Hinv.T)
    Lh = np.linalg.cholesky(Hinv)
    theta0 = mode + 0.5 * (rng.standard_normal((N, d)) @ Lh.T)
    if bounds is not None:
        theta0 = np.clip(theta0, bounds[0] + 1e-3, bounds[1] - 1e-3)
    lam = float(np.linalg.eigvalsh(H)[-1])
    return dict(truth=truth, y=y, nk=nk, nz=nz, onz=onz, set_prior=set_prior, prior=prior, pcov=pcov, bounds=bounds, mode=mode,
                H=H, Hinv=Hinv, lam=lam, W=W, theta0=theta0, rng=rng)


def _proposal(c, p, e):
    """set the engine's proposal and return the oracle's description; scalings from the curvature at the mode"""
    d, rng, kind = c["d"], p["rng"], c["kind"]
    adaptive = kind.endswith("adaptive")
    period = int(rng.choice([10, 16, 25]))
    C0 = (2.38 ** 2 / d) * 0.8 * p["Hinv"]
    if kind.startswith("grw"):
        e.set_proposal(0, C0, scaling=1.0, adaptive=adaptive, period=period, gamma=1.05)
        return dict(kind="grw", C=C0, scaling=1.0, adaptive=adaptive, period=period, gamma=1.05)
    if kind.startswith("am"):
        t0 = int(rng.choice([0, period, 3 * period]))
        e.set_proposal(2, C0, t0=t0, period=period, adaptive=adaptive)
        return dict(kind="am", C0=C0, t0=t0, period=period, adaptive=adaptive)
    # likelihood-ratio proposals: beta^2 tr(H_like C_prior) ~ 1
    Hl = p["H"] - np.linalg.inv(p["pcov"])
    beta2 = 1.0 / max(float(np.trace(Hl @ p["pcov"])), 1.0)
    if kind.startswith("pcn"):
        beta = float(np.sqrt(beta2))
        e.set_proposal(1, None, scaling=beta, adaptive=adaptive, period=period)
        return dict(kind="pcn", scaling=beta, adaptive=adaptive, period=period)
    if kind == "owcn":
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        B = Q @ np.diag(np.linspace(0.4, 1.0, d)) @ Q.T
        S, Nop = orc.owcn_operators(B, beta2)
        e.set_proposal(5, None, state_operator=S, noise_operator=Nop)
        return dict(kind="owcn", B=B, scaling=beta2)
    q_cov = 1.2 * p["Hinv"]  # indep: a Gaussian around the mode
    e.set_proposal(4, q_cov, q_mean=p["mode"])
    return dict(kind="indep", q_mean=p["mode"], q_cov=q_cov)


def _mala_scaling(c, lam):
    # s^2 / 2 * lambda_max = 0.5, lambda_max of the Gauss-Newton Hessian at the mode: at larger drift the last-bit differences of
    # two correct implementations grow step by step (test_gpu_mala_source.py, above CASES)
    del c
    return float(np.sqrt(2 * 0.5 / lam))


def _set_level(e, c, p, level=0, shift=0.0, coup=0.5):
    m = c["m"]
    if c["model"] == "source":
        e.set_level_source(level, source(shift=shift, coup=coup), p["y"], p["nk"], p["nz"])
    else:
        e.set_level_callback(level, lambda t: np_forward(t, m, shift=shift, coup=coup), p["y"], p["nk"], p["nz"])


def _make_engine(c, p):
    from tinyda_amd.engine import Engine

    e = Engine(c["N"], c["d"], seed=60 + c["i"], chain_offset=c["i"] % 7, block_steps=c["block"])
    p["set_prior"](e)
    _set_level(e, c, p)
    if c["kind"].startswith("mala"):
        s = _mala_scaling(c, p["lam"])
        e.set_proposal(6, None, scaling=s, adaptive=c["kind"].endswith("adaptive"), gamma=1.01, period=20)
        prop = dict(kind="mala", scaling=s, adaptive=c["kind"].endswith("adaptive"), gamma=1.01, period=20)
    else:
        prop = _proposal(c, dict(p, rng=np.random.default_rng(17000 + c["i"])), e)
    if c["thin"] > 1:
        e.set_record_thinning(c["thin"])
    e.init(p["theta0"])
    return e, prop


def _runs(e, c, n):
    """records of n iterations: host (pinned) arrays or, for the device variant, torch tensors on the GPU"""
    thin = c["thin"]
    t = e._t_py if getattr(e, "_t_py", None) is not None else e.counters()[0]
    rows = (t + n) // thin - t // thin
    N, d = c["N"], c["d"]
    if c["variant"] == "device":
        import torch

        P = torch.full((rows, N, d), float("nan"), dtype=torch.float64, device="cuda")
        S = torch.full((rows, N, 3), float("nan"), dtype=torch.float64, device="cuda")
        A = torch.full((rows, N), 7, dtype=torch.uint8, device="cuda")
        e.run(n, P, S, A)
        return P.cpu().numpy(), S.cpu().numpy(), A.cpu().numpy()
    from tinyda_amd.engine import pinned_empty

    P, S, A = pinned_empty((rows, N, d)), pinned_empty((rows, N, 3)), pinned_empty((rows, N), dtype=np.uint8)
    P[...], S[...], A[...] = np.nan, np.nan, 7
    e.run(n, P, S, A)
    return P, S, A


def _level_for(c, p):
    m = c["m"]
    fn = lambda t: np_forward(t, m)  # noqa: E731
    noise = {0: "iso", 1: "diag", 2: "dense"}[p["nk"]]
    if c["kind"].startswith("mala"):
        return GradLevel(fn, p["y"], noise, p["onz"], p["prior"])
    return orc.CallableGaussianLevel(fn, p["y"], noise, p["onz"], p["prior"])


def _self_consistent(lvl, params, stats, what):
    """every recorded row: the oracle level at the recorded parameters gives the recorded (lp, ll, lp + ll)"""
    th = params.reshape(-1, params.shape[-1])
    if not len(th):
        return
    lp, ll, _ = lvl.evaluate(th)
    ref = np.stack([lp, ll, lp + ll], axis=1)
    np.testing.assert_allclose(stats.reshape(-1, 3), ref, rtol=1e-10, err_msg=what)


def _eval_points(c, p, rng, n):
    pts = p["mode"] + (rng.standard_normal((n, c["d"])) @ np.linalg.cholesky(p["Hinv"]).T) * 2.0
    if p["bounds"] is not None:  # a third of the points leave the support of a uniform component
        lo, hi = p["bounds"]
        uni = np.flatnonzero(np.isfinite(lo))
        if uni.size:
            for r in range(0, n, 3):
                j = uni[r % uni.size]
                pts[r, j] = hi[j] + 0.1 if r % 2 else lo[j] - 0.1
    return pts


def _run_single(c):
    p = _single_problem(c)
    N, T, thin = c["N"], c["T"], c["thin"]
    e, prop = _make_engine(c, p)
    z, u = e.set_export(T)
    if c["split"] and T > 2:
        k = T // 3
        parts = [_runs(e, c, k), _runs(e, c, T - k)]
        params, stats, acc = (np.concatenate([x[j] for x in parts]) for j in range(3))
    else:
        params, stats, acc = _runs(e, c, T)
    lvl = _level_for(c, p)
    # Engine.evaluate at 2N points (mode 1 of tda_user_steps / k_ext_accept)
    rng = np.random.default_rng(19000 + c["i"])
    ev = []
    for _ in range(2):
        pts = _eval_points(c, p, rng, N)
        ev.append((pts, e.evaluate(pts)))
    scal = e.proposal_state_scaling()
    blob_ok = None
    if c["variant"] == "resume":  # a fresh engine resumed from a mid-run checkpoint continues bitwise
        e.close()
        whole = (params, stats, acc)
        k = T // 2 + 1
        e1, _ = _make_engine(c, p)
        first = _runs(e1, c, k)
        blob = e1.get_state()
        e1.close()
        e2, _ = _make_engine(c, p)
        e2.set_state(blob)
        rest = _runs(e2, c, T - k)
        e2.close()
        blob_ok = all(np.array_equal(w, np.concatenate([f, r])) for w, f, r in zip(whole, first, rest))
    else:
        e.close()
    res = orc.run_mh(lvl, prop, p["theta0"], np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    return p, lvl, prop, (params, stats, acc), res, ev, scal, blob_ok


def _check_single(c, out):
    p, lvl, prop, (params, stats, acc), res, ev, scal, blob_ok = out
    T, thin = c["T"], c["thin"]
    keep = np.arange(thin - 1, T, thin)
    assert params.shape[0] == keep.size
    ref_acc = np.swapaxes(res["accepted"][:, 1:], 0, 1)[keep]
    ref_lp = np.swapaxes(res["logpost"][:, 1:], 0, 1)[keep]
    ref_th = np.swapaxes(res["theta"][:, 1:], 0, 1)[keep]
    flips = int((acc != ref_acc).sum())
    assert flips == 0, "%s: %d accept flips" % (c, flips)
    small = _small_am(c)
    rtol = 1e-9 if small else AM_LOOSE_RTOL if c["kind"].startswith("am") else RTOL
    if keep.size:
        rel = float(np.max(np.abs(stats[:, :, 2] - ref_lp) / np.abs(ref_lp)))
        assert rel <= rtol, (c, rel)
        if not small:
            np.testing.assert_allclose(params, ref_th, rtol=1e-8 if c["kind"].startswith("am") else 1e-9,
                                       atol=AM_PARAMS_ATOL if c["kind"].startswith("am") else 1e-11, err_msg=str(c))
    if c["kind"].startswith("mala") or c["kind"].endswith("adaptive"):
        np.testing.assert_allclose(scal, res["scaling"], rtol=1e-12, err_msg=str(c))
    _self_consistent(lvl, params, stats, str(c))
    for pts, st_ in ev:
        lp, ll, _ = lvl.evaluate(pts)
        np.testing.assert_allclose(st_, np.stack([lp, ll, lp + ll], axis=1), rtol=1e-10, err_msg="evaluate: %s" % c)
    if blob_ok is not None:
        assert blob_ok, "%s: resumed run differs from the uninterrupted one" % c
    if T >= 37:
        rate = float(np.mean(res["accepted"][:, 1:]))
        assert 0.02 < rate < 0.98, (c, rate)


@pytest.mark.parametrize("i", range(N_SINGLE))
def test_external_single_level_configuration(i):
    c = _single_case(i)
    _check_single(c, _run_single(c))


@pytest.mark.parametrize("i", range(N_MALA))
def test_external_mala_configuration(i):
    c = _mala_case(i)
    _check_single(c, _run_single(c))


# ---- hierarchies ------------------------------------------------------------------------------------------------------
def _fidelity(k, nl):
    """level k of nl (coarsest first): coarser levels shift the weights and weaken the coupling"""
    return 0.004 * (nl - 1 - k), 0.5 - 0.1 * (nl - 1 - k)


def _run_multilevel(c):
    from tinyda_amd.engine import Engine

    nl, d, ms, sl, N, n_fine = c["nl"], c["d"], c["ms"], c["sl"], c["N"], c["n_fine"]
    rng = np.random.default_rng(21000 + c["i"])
    truth = 0.3 * rng.standard_normal(d)
    pm, pv = np.zeros(d), 0.5 + rng.random(d)
    prior = orc.MVNPrior(pm, np.diag(pv))
    seed = 700 + c["i"]
    e = Engine(N, d, seed=seed, n_levels=nl, block_steps=c["block"])
    e.set_prior(pm, np.diag(pv))
    levels, wf = [], None
    for k in range(nl):
        shift, coup = _fidelity(k, nl)
        m = ms[k]
        if c["noise"] == "iso":
            nk, nz = 0, 0.01
        else:
            nk, nz = 1, 0.01 * (0.5 + rng.random(m))
        y = np_forward(truth, m, shift=shift, coup=coup)[0] + 0.1 * rng.standard_normal(m)
        noise = "iso" if nk == 0 else "diag"
        wf = np.broadcast_to(1.0 / np.asarray(nz), (m,))  # (the finest level's weights remain)
        if c["models"][k] == "linear":  # the model linearised at the origin
            A = weights(m, d, shift)
            e.set_level(k, A, y, nk, nz)
            levels.append(orc.LinearGaussianLevel(A, y, noise, nz, prior))
        else:
            fn = (lambda t, m=m, shift=shift, coup=coup: np_forward(t, m, shift=shift, coup=coup))
            if c["models"][k] == "source":
                e.set_level_source(k, source(shift=shift, coup=coup), y, nk, nz)
            else:
                e.set_level_callback(k, fn, y, nk, nz)
            levels.append(orc.CallableGaussianLevel(fn, y, noise, nz, prior))
    # proposal scaled to the finest level's curvature at the truth
    fs, fc = _fidelity(nl - 1, nl)
    J = np_jacobian(truth, ms[-1], fs, fc) if c["models"][-1] != "linear" else weights(ms[-1], d, fs)
    Hl = J.T @ (wf[:, None] * J)
    H = Hl + np.diag(1.0 / pv)
    Hinv = np.linalg.inv(H)
    Hinv = 0.5 * (Hinv + Hinv.T)
    theta0 = truth + 0.5 * (rng.standard_normal((N, d)) @ np.linalg.cholesky(Hinv).T)
    period = int(rng.choice([8, 20]))
    C0 = (2.38 ** 2 / d) * 0.8 * Hinv
    if c["kind"] == "pcn":
        beta = float(np.sqrt(1.0 / max(float(np.trace(Hl @ np.diag(pv))), 1.0)))
        prop = dict(kind="pcn", scaling=beta, adaptive=True, gamma=1.01, period=period)
        e.set_proposal(1, None, scaling=beta, adaptive=True, gamma=1.01, period=period)
    elif c["kind"] == "grw_adaptive":
        prop = dict(kind="grw", C=C0, scaling=1.0, adaptive=True, gamma=1.02, period=period)
        e.set_proposal(0, C0, scaling=1.0, adaptive=True, gamma=1.02, period=period)
    else:
        adaptive = c["kind"].endswith("adaptive")
        prop = dict(kind="am", C0=C0, t0=period, period=period, adaptive=adaptive)
        e.set_proposal(2, C0, t0=period, period=period, adaptive=adaptive)
    e.set_subchains(sl, c["randomize"])
    e.init(theta0)
    rows = e.rows_per_level(n_fine)
    z, _ = e.set_export(rows[0])
    outs = e.run_levels_host(n_fine)
    scal = e.proposal_state()["scaling"]
    ev = []
    erng = np.random.default_rng(23000 + c["i"])
    for k in range(nl):
        pts = truth + (erng.standard_normal((N, d)) @ np.linalg.cholesky(Hinv).T) * 2.0
        ev.append((pts, e.evaluate(pts, level=k)))
    e.close()
    us, ridx = oracle_uniforms(seed, N, rows, sl, sl[0] if c["randomize"] else None)
    res, pstate = orc.run_multilevel(levels, prop, sl, theta0, np.swapaxes(z, 0, 1), us, n_fine, ridx)
    return levels, outs, res, pstate, scal, ev, rows


@pytest.mark.parametrize("i", range(N_ML))
def test_external_multilevel_configuration(i):
    c = _ml_case(i)
    levels, outs, res, pstate, scal, ev, rows = _run_multilevel(c)
    nl = c["nl"]
    for k in range(nl):
        ref = res[k]
        sk = slice(1, None) if k == nl - 1 else slice(None)
        flips = int((outs[k][2] != ref["accepted"][:, sk].T).sum())
        assert flips == 0, "%s: level %d, %d accept flips" % (c, k, flips)
        rl = ref["logpost"][:, sk].T
        rel = float(np.max(np.abs(outs[k][1][:, :, 2] - rl) / np.abs(rl)))
        assert rel <= (AM_LOOSE_RTOL if c["kind"].startswith("am") else RTOL), (c, k, rel)
        am = c["kind"].startswith("am")
        np.testing.assert_allclose(outs[k][0], np.swapaxes(ref["theta"][:, sk], 0, 1), rtol=1e-8 if am else 1e-9,
                                   atol=AM_PARAMS_ATOL if am else 1e-11, err_msg="%s level %d" % (c, k))
        _self_consistent(levels[k], outs[k][0], outs[k][1], "%s level %d" % (c, k))
        pts, st_ = ev[k]
        lp, ll, _ = levels[k].evaluate(pts)
        np.testing.assert_allclose(st_, np.stack([lp, ll, lp + ll], axis=1), rtol=1e-10, err_msg="evaluate level %d: %s" % (k, c))
    np.testing.assert_allclose(scal, pstate.scaling, rtol=1e-12)
    if c["T"] >= 37:  # (T: steps of the finest level)
        rate = float(outs[nl - 1][2].mean())
        assert 0.02 < rate < 0.98, (c, rate)


# ---- sample(): the lowering of api._device_plan at 64 / 65 / 128 parameters ----------------------------------------------
def _sample_posterior(d, m, seed, shift=0.0, coup=0.5, batched=False):
    import scipy.stats as st

    import tinyda_amd as tda

    rng = np.random.default_rng(seed)
    truth = 0.3 * rng.standard_normal(d)
    y = np_forward(truth, m, shift=shift, coup=coup)[0] + 0.1 * rng.standard_normal(m)
    pm, pv = np.zeros(d), 0.5 + rng.random(d)
    fn = lambda t: np_forward(t, m, shift=shift, coup=coup)  # noqa: E731
    model = (tda.BatchedModel(fn, m) if batched else
             tda.DeviceModel(source(shift=shift, coup=coup), m, reference=lambda t: fn(t)[0]))
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, 0.01 * np.eye(m)), model)
    J = np_jacobian(truth, m, shift, coup)
    H = J.T @ J / 0.01 + np.diag(1.0 / pv)
    lvl = orc.CallableGaussianLevel(fn, y, "iso", 0.01, orc.MVNPrior(pm, np.diag(pv)))
    return post, lvl, truth, H


def _sample_checked(posts, proposal, T, N, lvls, initial, **kw):
    import tinyda_amd as tda
    from tinyda_amd.api import HostFallbackWarning

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(posts, proposal, T, n_chains=N, initial_parameters=initial, seed=5, backend="hip", **kw)
    assert not [x for x in w if issubclass(x.category, HostFallbackWarning)], [str(x.message) for x in w]
    assert res["n_chains"] == N
    keys = ["chain_%d"] if len(lvls) == 1 else ["chain_coarse_%d", "chain_fine_%d"]
    for key, lvl in zip(keys, lvls):
        for i in range(N):
            ch = res[key % i]
            if key != "chain_coarse_%d":
                assert len(ch) == T + 1
            _self_consistent(lvl, np.asarray(ch.parameters), np.asarray(ch.stats), key % i)
    return res


@pytest.mark.parametrize("d", [64, 65, 128])
@pytest.mark.parametrize("kind", ["mala", "am", "batched_grw"])
def test_sample_external_model_at_lane_boundary(d, kind):
    import tinyda_amd as tda

    m, N, T = 65, 6, 60
    post, lvl, truth, H = _sample_posterior(d, m, seed=d, batched=kind == "batched_grw")
    Hinv = np.linalg.inv(H)
    Hinv = 0.5 * (Hinv + Hinv.T)
    th0 = [truth + 0.3 * np.linalg.cholesky(Hinv) @ np.random.default_rng(j).standard_normal(d) for j in range(N)]
    if kind == "mala":
        prop = tda.MALA(scaling=float(np.sqrt(1.0 / np.linalg.eigvalsh(H)[-1])), adaptive=True, period=20)
    elif kind == "am":
        prop = tda.AdaptiveMetropolis((2.38 ** 2 / d) * 0.8 * Hinv, t0=20, period=20)
    else:
        prop = tda.GaussianRandomWalk((2.38 ** 2 / d) * 0.8 * Hinv)
    res = _sample_checked(post, prop, T, N, [lvl], th0)
    rate = np.mean([np.mean(res["chain_%d" % i].accepted[1:]) for i in range(N)])
    assert 0.02 < rate < 0.98, rate


def test_sample_source_hierarchy_at_65():
    import tinyda_amd as tda

    d, m, N, T = 65, 64, 5, 12
    coarse, lc, truth, _ = _sample_posterior(d, m, seed=3, shift=0.004, coup=0.4)
    fine, lf, _, H = _sample_posterior(d, m, seed=3)
    Hinv = np.linalg.inv(H)
    Hinv = 0.5 * (Hinv + Hinv.T)
    th0 = [truth + 0.3 * np.linalg.cholesky(Hinv) @ np.random.default_rng(j).standard_normal(d) for j in range(N)]
    res = _sample_checked([coarse, fine], tda.GaussianRandomWalk((2.38 ** 2 / d) * 0.8 * Hinv), T, N, [lc, lf], th0, subchain_length=3)
    assert res["sampler"] == "DA"
