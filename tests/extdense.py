"""What the dense-mass tests share: the NumPy twins of tda_user_hmc_steps / tda_user_nuts_steps built with -DTDA_DENSE_MASS, the
admission rule with its extended perturbation, the dense mass DENSE(d), and the table of the forward-mode cases.

The algorithm is the one include/tinyda_amd_dense_mass.h writes out.  Everything that does not touch the mass is exthmc's /
extnuts's own code: the twins here ARE run_hmc / run_nuts, run with a unit diagonal mass (under which p = z, K = 1/2 sum q q and
the U-turn test is a plain dot product, each in exact arithmetic) while the one function of each module that advances a
trajectory -- exthmc.leapfrog, extnuts.leaf_step -- is replaced by its dense form below for the duration of the call.  They take
the factor L, as the C-ABI does.

The kernel forms v = L q and r = L^T g by one fused multiply-add per term over j = 0 .. d - 1; `product` adds the same terms in
the same order without the fusion, so that terms outside the triangle add exact zeros here as there (W = I and W = diag(powers
of 4) give the diagonal twins' numbers bit for bit) and a product differs from the kernel's by at most d roundings."""
import contextlib

import numpy as np

from . import exthmc as xh
from . import extnuts as xn

SEED, CHAIN_OFFSET, N_CHAINS = xh.SEED, xh.CHAIN_OFFSET, xh.N_CHAINS


def DENSE(d, seed=0):
    """W = Q diag(lambda) Q^T, Q from the QR of a seeded normal matrix, lambda = logspace(-1, 0.5, d): symmetric exactly, and its
    factor has no exact zero below the diagonal"""
    Q = np.linalg.qr(np.random.default_rng(1000 + 7 * d + seed).standard_normal((d, d)))[0]
    W = (Q * np.logspace(-1.0, 0.5, d)[None, :]) @ Q.T
    return 0.5 * (W + W.T)


def product(M, x):
    """y[:, i] = sum_j M[i, j] x[:, j] over j = 0, 1, .., d - 1 in that order, from 0.0"""
    acc = np.zeros_like(x)
    for j in range(M.shape[1]):
        acc = acc + M[None, :, j] * x[:, j:j + 1]
    return acc


def _room(d, perturb):
    """the factor on every product under the admission rule: 1 + d 2^-52 (1 - d 2^-52 when the gradients move down), the rounding
    room between the kernel's fused sequential sum and `product`"""
    return 1.0 + (d * 2.0 ** -52 if perturb > 0 else -d * 2.0 ** -52 if perturb < 0 else 0.0)


def _hmc_leapfrog(chol):
    def leapfrog(level, theta, q, grad, eps, w, L, perturb=False):
        """exthmc.leapfrog on the whitened momentum: r = L^T g;  q += c r;  v = L q;  theta += eps v"""
        N, f = theta.shape[0], _room(theta.shape[1], int(bool(perturb)))
        theta, q = theta.copy(), q + (0.5 * eps)[:, None] * (product(chol.T, grad) * f)
        ended = np.zeros(N, dtype=int)
        lp, ll, g = np.full(N, np.nan), np.full(N, np.nan), grad.copy()
        with np.errstate(all="ignore"):
            for i in range(1, L + 1):
                live = ended == 0
                theta = np.where(live[:, None], theta + eps[:, None] * (product(chol, q) * f), theta)
                lp_i, ll_i, F = level.evaluate(theta)
                g_i = np.asarray(level.grad_logpost(theta, F), dtype=float)
                if perturb:
                    g_i = np.nextafter(g_i, np.inf)
                finite = np.isfinite(lp_i + ll_i)
                ended = np.where(live & ~finite, i, ended)
                lp, ll = np.where(live, lp_i, lp), np.where(live, ll_i, ll)
                step = live & finite
                c = eps if i < L else 0.5 * eps
                q = np.where(step[:, None], q + c[:, None] * (product(chol.T, g_i) * f), q)
                g = np.where(step[:, None], g_i, g)
        return theta, q, (lp, ll, g), ended

    return leapfrog


def _nuts_leaf(chol):
    def leaf_step(level, th, q, g, e, w, on, perturb=0):
        """extnuts.leaf_step on the whitened momentum"""
        f = _room(th.shape[1], perturb)
        q = np.where(on[:, None], q + (0.5 * e)[:, None] * (product(chol.T, g) * f), q)
        th = np.where(on[:, None], th + e[:, None] * (product(chol, q) * f), th)
        lp, ll, F = level.evaluate(th)
        fin = on & np.isfinite(lp + ll)
        g_n = xn._gradient(level, th, F, perturb)
        g = np.where(fin[:, None], g_n, g)
        q = np.where(fin[:, None], q + (0.5 * e)[:, None] * (product(chol.T, g) * f), q)
        return th, q, g, lp, ll, fin

    return leaf_step


@contextlib.contextmanager
def _replaced(module, name, fn):
    old = getattr(module, name)
    setattr(module, name, fn)
    try:
        yield
    finally:
        setattr(module, name, old)


def _factor(prop):
    chol = np.asarray(prop["chol"], dtype=float)
    assert chol.ndim == 2 and np.array_equal(chol, np.tril(chol)) and np.all(np.diag(chol) > 0.0)
    return chol, dict({k: v for k, v in prop.items() if k != "chol"}, inv_mass=None)


def run_hmc(level, prop, theta0, z, u, perturb=False):
    """exthmc.run_hmc under the dense inverse mass W = L L^T, L = prop["chol"] (the momentum in the trace's arithmetic is q)"""
    chol, unit = _factor(prop)
    with _replaced(xh, "leapfrog", _hmc_leapfrog(chol)):
        return xh.run_hmc(level, unit, theta0, z, u, perturb)


def run_nuts(level, prop, theta0, z, draws, perturb=0, record=None):
    """extnuts.run_nuts under the dense inverse mass W = L L^T, L = prop["chol"]"""
    chol, unit = _factor(prop)
    with _replaced(xn, "leaf_step", _nuts_leaf(chol)):
        return xn.run_nuts(level, unit, theta0, z, draws, perturb, record)


def assert_admissible(level, prop, theta0, z, draws_or_u, ref=None):
    """exthmc.assert_admissible / extnuts.assert_admissible (by prop["kind"]) with the perturbation extended: every gradient is
    moved by one ulp AND every product v, r is multiplied by 1 + d 2^-52 (`_room`).  A case is compared only if the twin's masks
    and tree decisions survive that.  -> (the unperturbed trace, the largest relative change of the log-posterior, the largest
    change of a state as a share of its bar 1e-12 + 1e-9 |state|)"""
    chol, unit = _factor(prop)
    if prop["kind"] == "hmc":
        with _replaced(xh, "leapfrog", _hmc_leapfrog(chol)):
            ref = xh.assert_admissible(level, unit, theta0, z, draws_or_u, ref)
            moved = xh.run_hmc(level, unit, theta0, z, draws_or_u, perturb=True)
        dpost = float(np.max(np.abs(moved["logpost"] / ref["logpost"] - 1.0)))
        dstate = float(np.max(np.abs(moved["theta"] - ref["theta"]) / (1e-12 + 1e-9 * np.abs(ref["theta"]))))
        return ref, dpost, dstate
    with _replaced(xn, "leaf_step", _nuts_leaf(chol)):
        return xn.assert_admissible(level, unit, theta0, z, draws_or_u, ref)


def set_proposal(e, prop):
    """the twin's description on an engine: the diagonal proposal of exthmc / extnuts with a unit mass, then the factor"""
    unit = dict({k: v for k, v in prop.items() if k != "chol"}, inv_mass=None)
    (xh if prop["kind"] == "hmc" else xn).set_proposal(e, unit)
    e.set_dense_mass(prop["chol"])


# ---- the forward-mode cases: the engine on its own Philox stream against the twin, under DENSE(d) -------------------------------
# tests/test_dense_mass.py admits every case on the CPU, on the engine's variates drawn by the oracle's Philox stream;
# tests/test_gpu_dense_mass.py runs them.  N = 13 chains.  HMC with 4 leapfrog steps, NUTS with max_depth 4, periods of 20 steps.
# The step sizes were chosen on the CPU with the twin alone, so that it meets the admission rule (HMC: acceptance in 0.1 .. 0.9)
# and the trees are of several depths.  d = 2, m = 1 is extmodel's model at its smallest; d = 128 runs in blocks of 16 steps, so
# that a launch boundary falls inside a period.  (d = 2, m = 1: on the problem of the default seed no step size with an acceptance
# below 0.9 passes the one-ulp rule; of the seeds 1 .. 7, seed 3 has one.  NUTS keeps the default problem.)
# kind, d, m, noise, adaptive, block_steps, step size, T, seed of the problem (None: d * 1000 + m, as the HMC tests have it)
FORWARD_CASES = {
    "hmc_d2_m1": ("hmc", 2, 1, "iso", False, 0, 0.2, 60, 3),
    "hmc_d5_m23": ("hmc", 5, 23, "diag", False, 0, 0.07, 60, None),
    "hmc_d64_m23": ("hmc", 64, 23, "diag", True, 0, 0.02, 40, None),
    "hmc_d65_m23": ("hmc", 65, 23, "iso", True, 0, 0.03, 40, None),
    "hmc_d128_m23": ("hmc", 128, 23, "diag", True, 16, 0.014, 40, None),
    "nuts_d2_m1": ("nuts", 2, 1, "iso", False, 0, 0.1, 60, None),
    "nuts_d5_m23": ("nuts", 5, 23, "diag", False, 0, 0.03, 60, None),
    "nuts_d64_m23": ("nuts", 64, 23, "diag", True, 0, 0.035, 40, None),
    "nuts_d65_m23": ("nuts", 65, 23, "iso", True, 0, 0.035, 40, None),
    "nuts_d128_m23": ("nuts", 128, 23, "diag", True, 16, 0.02, 30, None),
}

# The comparison keeps extengine.compare's bars (masks and tree decisions exact, log-posterior 1e-10, states 1e-9 of themselves
# with atol 1e-12).  An admitted case that exceeds one on the device because of summation order alone is listed here, as
# extnuts.TOLERANCE lists its own: case -> (log-posterior rtol, states as a multiple of their bar), twice the deviation from the
# twin measured on the device (the measured value in a comment); no entry beyond ten times the default, which would be a bug.
TOLERANCE = {}
DEFAULT_TOLERANCE = (1e-10, 1.0)


def tolerance(case):
    post_rtol, state_bar = TOLERANCE.get(case, DEFAULT_TOLERANCE)
    assert post_rtol <= 10.0 * DEFAULT_TOLERANCE[0] and state_bar <= 10.0 * DEFAULT_TOLERANCE[1], case
    return post_rtol, state_bar


def dense_proposal(kind, d, eps, adaptive, chol=None):
    chol = np.linalg.cholesky(DENSE(d)) if chol is None else chol
    base = xh.hmc(eps, 4, adaptive) if kind == "hmc" else xn.nuts(eps, 4, adaptive)
    return dict(base, chol=np.tril(chol))


def forward_case(name, N=N_CHAINS):
    """-> the oracle level, the proposal (with its factor), the starts, T, and make() -> the engine (not initialised)"""
    kind, d, m, noise, adaptive, bs, eps, T, seed = FORWARD_CASES[name]
    y, theta0, pm, pv, nz, level = xh.gaussian_problem(d, m, noise, N, seed=d * 1000 + m if seed is None else seed)
    prop = dense_proposal(kind, d, eps, adaptive)

    def make():
        e = xh.gaussian_engine(d, m, noise, N, y, pm, pv, nz, dict(kind="mala", scaling=0.1), bs)
        set_proposal(e, prop)
        return e

    return level, prop, theta0, T, make


def contract_case(name, kind, eps, N=N_CHAINS):
    """one of exthmc.CONTRACT_CASES under DENSE(d): -> level, proposal, starts, T, make()"""
    level, _, theta0, T, make_hmc = xh.contract_case(name, N)
    prop = dense_proposal(kind, theta0.shape[1], eps, False)

    def make():
        e = make_hmc()
        set_proposal(e, prop)
        return e

    return level, prop, theta0, 20, make


# the other source forms, where the new barriers meet source-defined ones: (case of exthmc.CONTRACT_CASES, kind) -> step size
CONTRACT_STEP = {
    ("ring_forward_wave_gradient_wave", "hmc"): 0.08,
    ("ring_forward_wave_gradient_wave", "nuts"): 0.08,
    ("cauchy_difference_prior_wave", "hmc"): 0.022,
    ("cauchy_difference_prior_wave", "nuts"): 0.006,
}


def variates(N, T, d):
    """the engine's unit normals z[N, T, d] and uniforms u[N, T] from the oracle's Philox stream"""
    return xh.philox_variates(SEED, CHAIN_OFFSET, N, T, d)


def compare(case, params, stats, acc, ref, scal=None):
    """the engine's outputs [T, N, ..] against a twin's trace at the case's tolerance; every figure is printed before it is asserted"""
    post_rtol, state_bar = tolerance(case)
    want, post = np.swapaxes(ref["theta"][:, 1:], 0, 1), np.swapaxes(ref["logpost"][:, 1:], 0, 1)
    masks = np.array_equal(acc, np.swapaxes(ref["accepted"][:, 1:], 0, 1))
    dpost = float(np.max(np.abs(stats[:, :, 2] / post - 1.0)))
    dstate = float(np.max(np.abs(params - want) / (1e-12 + 1e-9 * np.abs(want))))
    print("%s: masks equal %s, log-posterior off by %.2e of itself (bar %.1e), states by %.2e of their bar 1e-12 + 1e-9 |state| (allowed %.1f)"
          % (case, masks, dpost, post_rtol, dstate, state_bar))
    assert masks
    np.testing.assert_allclose(stats[:, :, 2], post, rtol=post_rtol)
    np.testing.assert_allclose(params, want, rtol=state_bar * 1e-9, atol=state_bar * 1e-12)
    if scal is not None:
        np.testing.assert_allclose(scal, ref["scaling"], rtol=1e-12)
