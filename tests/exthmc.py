"""What the HMC tests share: the NumPy twin of tda_user_hmc_steps over any oracle level with `evaluate` and `grad_logpost`
(the levels of extmodel, extwave, extloglike, extloglikewave, extpriorgrad and extpriorwave), the engine's Philox variates
drawn on the CPU, the proposal on an engine, and the table of the forward-mode cases with its admission rule.

The reference has no HMC, so the twin is the yardstick; with one leapfrog step and unit mass it is tied to the oracle's MALA
(tests/test_hmc.py).  One step of a chain, operation for operation as the kernel has it (z the step's unit normals, u its uniform,
eps the chain's scaling, w the diagonal inverse mass, g the gradient of the log-posterior at the current state):

    p = z / sqrt(w);  K0 = 0.5 sum_j w_j (p_j p_j);  p = p + (0.5 eps) g
    for i = 1 .. L:   theta' = theta' + eps (w p);  lp', ll' at theta';  not finite: the trajectory ends, reject
                      p = p + c g',  c = eps for i < L and 0.5 eps for i = L
    K1 = 0.5 sum_j w_j (p_j p_j);  alpha = exp((post' - (lp + ll)) + (K0 - K1));  accept iff u < alpha

The kernel sums K over the wave by a butterfly and the twin by numpy's pairwise sum: the two differ in the last bits of a number
of order d, which moves alpha by 1e-14 of itself."""
import numpy as np

from oracle import tinyda_oracle as orc

PROP_HMC = 7
ALPHA_STAR = 0.65


def hmc(scaling, n_leapfrog, adaptive=False, inv_mass=None):
    return dict(kind="hmc", scaling=scaling, n_leapfrog=n_leapfrog, inv_mass=inv_mass, adaptive=adaptive, gamma=1.01, period=20)


def set_proposal(e, prop):
    """the twin's description of the proposal, set on an engine (in place of whatever proposal it had; before init)"""
    e.set_proposal(PROP_HMC, None, scaling=prop["scaling"], adaptive=prop.get("adaptive", False), gamma=prop.get("gamma", 1.01),
                   period=prop.get("period", 100), n_leapfrog=prop["n_leapfrog"], inv_mass=prop.get("inv_mass"))


def philox_variates(seed, chain_offset, N, T, d):
    """the unit normals z[N, T, d] and uniforms u[N, T] of an engine's first T steps, from the oracle's Philox stream"""
    ps, chains = orc.PhiloxStream(seed), chain_offset + np.arange(N)
    z = np.stack([ps.normals(chains, t, d) for t in range(T)], axis=1)
    u = np.stack([ps.uniform(chains, t) for t in range(T)], axis=1)
    return z, u


def leapfrog(level, theta, p, grad, eps, w, L, perturb=False):
    """L leapfrog steps of N trajectories from (theta, p) with the gradient `grad` at theta.  -> the end points, the momenta
    there, (lp, ll, gradient) at the end points, and per trajectory the step at which it left the region where the
    log-posterior is finite (0: it did not).  A trajectory that ended keeps the position at which it did."""
    N = theta.shape[0]
    theta, p = theta.copy(), p + (0.5 * eps)[:, None] * grad
    ended = np.zeros(N, dtype=int)
    lp, ll, g = np.full(N, np.nan), np.full(N, np.nan), grad.copy()
    with np.errstate(all="ignore"):
        for i in range(1, L + 1):
            live = ended == 0
            theta = np.where(live[:, None], theta + eps[:, None] * (w[None, :] * p), theta)
            lp_i, ll_i, F = level.evaluate(theta)
            g_i = np.asarray(level.grad_logpost(theta, F), dtype=float)
            if perturb:
                g_i = np.nextafter(g_i, np.inf)
            finite = np.isfinite(lp_i + ll_i)
            ended = np.where(live & ~finite, i, ended)
            lp, ll = np.where(live, lp_i, lp), np.where(live, ll_i, ll)
            step = live & finite
            c = eps if i < L else 0.5 * eps
            p = np.where(step[:, None], p + c[:, None] * g_i, p)
            g = np.where(step[:, None], g_i, g)
    return theta, p, (lp, ll, g), ended


def run_hmc(level, prop, theta0, z, u, perturb=False):
    """N chains x T steps on recorded variates (z[N, T, d], u[N, T]).  -> the trace dict that extengine.compare reads (theta,
    logprior, loglike, logpost, accepted with the initial link at index 0; the final scaling), and beside it `ended` [N, T]
    (the leapfrog step at which a trajectory left the support, 0: none) and `dH` [N, T] (the energy error of a whole trajectory).
    perturb: every gradient moved up by one ulp, for the admission rule below.  prop["alpha_star"] (0.65 unless given) is the
    adaptation's target: the tie to the oracle's MALA at L = 1 runs the adaptive cases towards MALA's 0.57."""
    theta = np.asarray(theta0, dtype=float).copy()
    N, d = theta.shape
    T, L = z.shape[1], int(prop["n_leapfrog"])
    w = np.ones(d) if prop.get("inv_mass") is None else np.asarray(prop["inv_mass"], dtype=float)
    adaptive, gamma, period = bool(prop.get("adaptive", False)), float(prop.get("gamma", 1.01)), int(prop.get("period", 100))
    eps, alpha_star = np.full(N, float(prop["scaling"])), float(prop.get("alpha_star", ALPHA_STAR))
    lp, ll, F = level.evaluate(theta)
    with np.errstate(all="ignore"):
        grad = np.asarray(level.grad_logpost(theta, F), dtype=float)
    if perturb:
        grad = np.nextafter(grad, np.inf)
    out_theta, out_lp, out_ll = np.empty((N, T + 1, d)), np.empty((N, T + 1)), np.empty((N, T + 1))
    out_acc, ended, dH = np.ones((N, T + 1), dtype=np.uint8), np.zeros((N, T), dtype=int), np.full((N, T), np.nan)
    out_theta[:, 0], out_lp[:, 0], out_ll[:, 0] = theta, lp, ll
    k = 0
    for s in range(T):
        p = z[:, s] / np.sqrt(w)[None, :]
        k0 = 0.5 * np.sum(w[None, :] * (p * p), axis=1)
        th_n, p_n, (lp_n, ll_n, g_n), ended[:, s] = leapfrog(level, theta, p, grad, eps, w, L, perturb)
        k1 = 0.5 * np.sum(w[None, :] * (p_n * p_n), axis=1)
        with np.errstate(all="ignore"):
            post_n = lp_n + ll_n
            dH[:, s] = (post_n - (lp + ll)) + (k0 - k1)
            alpha = np.exp(dH[:, s])
        alpha = np.where((ended[:, s] > 0) | np.isnan(post_n), 0.0, alpha)
        acc = u[:, s] < alpha
        theta, grad = np.where(acc[:, None], th_n, theta), np.where(acc[:, None], g_n, grad)
        lp, ll = np.where(acc, lp_n, lp), np.where(acc, ll_n, ll)
        out_theta[:, s + 1], out_lp[:, s + 1], out_ll[:, s + 1], out_acc[:, s + 1] = theta, lp, ll, acc
        if adaptive and (s + 1) % period == 0:  # the scaling adaptation of the period boundary (run_mh's), towards 0.65
            rate = out_acc[:, : s + 2][:, -period:].mean(axis=1)
            eps = np.exp(np.log(eps) + gamma ** -k * (rate - alpha_star))
            k += 1
    return dict(theta=out_theta, logprior=out_lp, loglike=out_ll, logpost=out_lp + out_ll, accepted=out_acc, scaling=eps, ended=ended, dH=dH)


def assert_admissible(level, prop, theta0, z, u, ref=None, state_share=None):
    """A leapfrog map that is not stable amplifies last-bit differences, and then no tolerance holds: a case is compared only if
    the twin with every gradient moved by one ulp gives the same masks and log-posteriors within 1e-11, and the twin's
    acceptance rate lies in [0.1, 0.9].  state_share: the one ulp moves no state by more than this share of the bar the states are
    compared at (1e-12 + 1e-9 |state|).  -> the unperturbed trace"""
    ref = run_hmc(level, prop, theta0, z, u) if ref is None else ref
    moved = run_hmc(level, prop, theta0, z, u, perturb=True)
    rate = ref["accepted"][:, 1:].mean()
    err = np.max(np.abs(moved["logpost"] / ref["logpost"] - 1.0))
    share = np.max(np.abs(moved["theta"] - ref["theta"]) / (1e-12 + 1e-9 * np.abs(ref["theta"])))
    print("twin: acceptance %.3f, trajectories ended early %d of %d, one ulp on every gradient moves the log-posterior by %.1e and the states "
          "by %.1e of their bar" % (rate, np.count_nonzero(ref["ended"]), ref["ended"].size, err, share))
    assert np.array_equal(moved["accepted"], ref["accepted"])
    assert err <= 1e-11, err
    assert 0.1 <= rate <= 0.9, rate
    assert state_share is None or share <= state_share, share
    return ref


# ---- the forward-mode cases: the engine on its own Philox stream against the twin ---------------------------------------------------
# tests/test_hmc.py admits every case on the CPU (assert_admissible, on the engine's variates drawn by the oracle's Philox stream);
# tests/test_gpu_hmc.py runs them.  N = 13 chains, T L <= 480 model evaluations per chain.  The step sizes were chosen on the
# CPU with the twin alone, so that it meets the admission rule.
SEED, CHAIN_OFFSET, N_CHAINS = 91, 3, 13
MASS = lambda d: 0.5 + 0.5 * (np.arange(d) % 4)  # noqa: E731  (a non-unit diagonal inverse mass: 0.5, 1, 1.5, 2, ...)

# d, m, L, noise, adaptive, non-unit mass, block_steps, step size, T, seed of the problem (None: d * 1000 + m, as the MALA tests have it)
# (one parameter: a leapfrog trajectory on a near-Gaussian posterior keeps its energy until the step size reaches the stability
# limit, where the one-ulp rule fails; of the problem seeds 1 .. 7 and 1001, seed 5 has a posterior on which the twin's acceptance
# falls below 0.9 well inside the limit)
FORWARD_CASES = {
    "d1_m1_L3_iso_fixed": (1, 1, 3, "iso", False, False, 0, 0.3, 120, 5),
    "d5_m23_L1_diag_fixed": (5, 23, 1, "diag", False, False, 0, 0.06, 120, None),
    "d5_m65_L7_iso_adaptive": (5, 65, 7, "iso", True, False, 0, 0.04, 60, None),
    "d64_m23_L4_diag_fixed_mass": (64, 23, 4, "diag", False, True, 0, 0.03, 120, None),
    "d65_m23_L4_iso_adaptive": (65, 23, 4, "iso", True, False, 0, 0.012, 120, None),
    "d128_m300_L2_diag_adaptive_split_mass": (128, 300, 2, "diag", True, True, 16, 0.004, 120, None),
}


def gaussian_problem(d, m, noise, N, seed, nan_above=None):
    """extmodel's model under a diagonal Gaussian prior (the problem of tests/test_gpu_mala_source.py)
    -> data, starts, prior mean and variances, the noise, the oracle level"""
    from . import extmodel as xm

    rng = np.random.default_rng(seed)
    truth = 0.3 * rng.standard_normal(d)
    sd = 0.05 if (d, m) == (5, 23) else 0.1
    y = xm.np_forward(truth, m)[0] + sd * rng.standard_normal(m)
    theta0 = truth + 0.01 * rng.standard_normal((N, d))
    pm, pv = 0.1 * np.ones(d), 0.5 + 0.01 * np.arange(d)
    nz = sd ** 2 if noise == "iso" else sd ** 2 * (1.0 + 0.1 * np.arange(m) / m)
    level = xm.GradLevel(lambda t: xm.np_forward(t, m, nan_above), y, noise, nz, orc.MVNPrior(pm, np.diag(pv)))
    return y, theta0, pm, pv, nz, level


def gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop, block_steps=0, nan_above=None, seed=SEED):
    from tinyda_amd.engine import Engine

    from . import extmodel as xm

    e = Engine(N, d, seed=seed, chain_offset=CHAIN_OFFSET, block_steps=block_steps)
    e.set_prior(pm, np.diag(pv))
    e.set_level_source(0, xm.source(nan_above), y, 0 if noise == "iso" else 1, np.atleast_1d(nz))
    if prop["kind"] == "hmc":
        set_proposal(e, prop)
    else:
        e.set_proposal(6, None, **{k: v for k, v in prop.items() if k != "kind"})
    return e


def forward_case(name, N=N_CHAINS):
    """-> the oracle level, the proposal, the starts, T, and make() -> the engine (not initialised)"""
    d, m, L, noise, adaptive, mass, bs, eps, T, seed = FORWARD_CASES[name]
    y, theta0, pm, pv, nz, level = gaussian_problem(d, m, noise, N, seed=d * 1000 + m if seed is None else seed)
    prop = hmc(eps, L, adaptive, MASS(d) if mass else None)
    return level, prop, theta0, T, lambda: gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop, bs)


# ---- one case for each remaining form of the contract -----------------------------------------------------------------------------
class LognormalGradPrior:
    """extprior.LognormalPrior with the gradient of extpriorgrad.LOGNORMAL_GRAD_SRC (NaN or anything outside the support)"""

    def __new__(cls, p, q):
        from . import extprior as xp
        from . import extpriorgrad as xg

        prior = xp.LognormalPrior(p, q)
        prior.grad = lambda theta: xg.lognormal_grad(np.atleast_2d(theta), prior.p, prior.q)
        return prior


def _ring(N):
    from . import extwave as xw

    d, m, sigma = 5, 24, 0.01
    _, y, theta0 = xw.problem(d, m, N, seed=524, sigma=sigma)
    pm, pv = np.zeros(d), np.ones(d)
    level = xw.GradLevel(lambda t: xw.np_forward(t, m), y, "iso", sigma ** 2, orc.MVNPrior(pm, np.diag(pv)))
    prop = hmc(0.12, 3)

    def make():
        from tinyda_amd.engine import Engine

        e = Engine(N, d, seed=SEED, chain_offset=CHAIN_OFFSET)
        e.set_prior(pm, np.diag(pv))
        e.set_level_source(0, xw.source("wave", "wave"), y, 0, [sigma ** 2])
        set_proposal(e, prop)
        return e

    return level, prop, theta0, 60, make


def _student_t(N):
    from . import extloglike as xl
    from . import extloglikewave as xlw
    from . import extmodel as xm

    d, m = 13, 23
    y, par, theta0, pm, pv = xlw.problem(d, m, "t_wave", N, seed=1323)
    level = xl.LogLikeLevel(lambda t: xm.np_forward(t, m), y, par, xl.KINDS["t"][1], orc.MVNPrior(pm, np.diag(pv)), xl.KINDS["t"][2])
    prop = hmc(0.075, 4)

    def make():
        e = xlw.make_engine(d, N, xm.source() + xl.KINDS["t"][0], y, par, pm, pv, dict(kind="mala", scaling=0.1), seed=SEED, chain_offset=CHAIN_OFFSET)
        set_proposal(e, prop)
        return e

    return level, prop, theta0, 60, make


def _ar1_wave(N):
    from . import extloglikewave as xlw

    d, m = 13, 47
    y, par, theta0, pm, pv = xlw.problem(d, m, "ar1", N, seed=1347)
    level = xlw.level_of("ar1", m, y, par, pm, pv)
    prop = hmc(0.1, 4)

    def make():
        e = xlw.make_engine(d, N, xlw.full_source("ar1"), y, par, pm, pv, dict(kind="mala", scaling=0.1), seed=SEED, chain_offset=CHAIN_OFFSET)
        set_proposal(e, prop)
        return e

    return level, prop, theta0, 60, make


def _lognormal_edge(N):
    """starts near the lower edge of the support: trajectories cross theta_j = 0 at an interior leapfrog step and are rejected"""
    from . import extmodel as xm
    from . import extprior as xp
    from . import extpriorgrad as xg

    d, m = 5, 23
    rng = np.random.default_rng(523)
    prior = LognormalGradPrior(np.log(0.05) * np.ones(d), 1.0 * np.ones(d))
    truth = 0.03 * np.ones(d)
    y = xm.np_forward(truth, m)[0] + np.sqrt(xp.SIGMA2) * rng.standard_normal(m)
    theta0 = truth[None, :] * np.exp(0.3 * rng.standard_normal((N, d)))
    level = xg.gaussian_grad_level(prior, m, y)
    prop = hmc(0.004, 5)

    def make():
        e = xg.make_engine(xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, prior.p, prior.q, N, (xm.source(), y, 0, xp.SIGMA2),
                           dict(kind="mala", scaling=0.1), seed=SEED, chain_offset=CHAIN_OFFSET)
        set_proposal(e, prop)
        return e

    return level, prop, theta0, 90, make


def _cauchy_difference(N):
    from . import extmodel as xm
    from . import extpriorwave as xpw

    d, m = 13, 23
    prior = xpw.cauchy_difference(d)
    y, theta0 = xpw.problem(prior, m, N, seed=1323)
    level = xpw.grad_level_of(prior, m, y)
    prop = hmc(0.025, 4)

    def make():
        e = xpw.make_engine(prior, N, [(xm.source(), y, 0, xpw.SIGMA2)], dict(kind="mala", scaling=0.1), seed=SEED, chain_offset=CHAIN_OFFSET)
        set_proposal(e, prop)
        return e

    return level, prop, theta0, 60, make


CONTRACT_CASES = {
    "ring_forward_wave_gradient_wave": _ring,
    "student_t_loglike": _student_t,
    "ar1_loglike_wave": _ar1_wave,
    "lognormal_prior_at_the_edge": _lognormal_edge,
    "cauchy_difference_prior_wave": _cauchy_difference,
}


def contract_case(name, N=N_CHAINS):
    return CONTRACT_CASES[name](N)


def nan_case(N=N_CHAINS):
    """extmodel's model with every output NaN above a threshold in theta_0 just beyond the starts
    -> the level, the same level without the region, the proposal, the starts, T, the threshold, make() -> the engine"""
    d, m, noise, T = 5, 23, "diag", 120
    y, theta0, pm, pv, nz, free = gaussian_problem(d, m, noise, N, seed=5023)
    thr = float(np.max(theta0[:, 0])) + 0.005
    level = gaussian_problem(d, m, noise, N, seed=5023, nan_above=thr)[5]
    prop = hmc(0.02, 4, adaptive=True)
    return level, free, prop, theta0, T, thr, lambda: gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop, nan_above=thr)
