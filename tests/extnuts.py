"""What the NUTS tests share: the NumPy twin of tda_user_nuts_steps over any oracle level with `evaluate` and `grad_logpost`
(the levels of tests/exthmc.py's cases), the tree draws of Philox stream 8 restated from the oracle's generator, the proposal on
an engine, and the table of the forward-mode cases with its admission rule.

The reference has no NUTS, so the twin is the yardstick; with max_depth = 1 it is tied to HMC's twin (tests/test_nuts.py).  The
algorithm is the one include/tinyda_amd_nuts.h writes out; the twin runs it for N chains at once, every decision under a mask,
operation for operation as the kernel has it.  The kernel sums over the wave by a butterfly and the twin by numpy's pairwise
sum: energies differ in the last bits, so a case is compared only where no decision hangs on those bits (assert_admissible)."""
import numpy as np

from oracle import tinyda_oracle as orc

from . import exthmc as xh

PROP_NUTS = 8
STREAM_TREE = 8
STOP_NAMES = {0: "max_depth", 1: "divergent", 2: "uturn_subtree", 3: "uturn_tree"}
SEED, CHAIN_OFFSET, N_CHAINS, T_STEPS = xh.SEED, xh.CHAIN_OFFSET, xh.N_CHAINS, 120


def nuts(scaling, max_depth, adaptive=False, inv_mass=None, target_accept=0.8, period=20):
    return dict(kind="nuts", scaling=scaling, max_depth=max_depth, inv_mass=inv_mass, adaptive=adaptive, target_accept=target_accept, gamma=1.01, period=period)


def set_proposal(e, prop):
    """the twin's description of the proposal, set on an engine (in place of whatever proposal it had; before init)"""
    e.set_proposal(PROP_NUTS, None, scaling=prop["scaling"], adaptive=prop.get("adaptive", False), gamma=prop.get("gamma", 1.01),
                   period=prop.get("period", 100), max_depth=prop["max_depth"], target_accept=prop.get("target_accept", 0.8), inv_mass=prop.get("inv_mass"))


class PhiloxDraws:
    """the tree draws of the engine: counter = (block, global step, global chain id, stream 8); doubling j is block j (direction
    x.z & 1, uniform u53(x.x, x.y)), the l-th leaf of a step block 32 + l (uniform u53(x.x, x.y))"""

    def __init__(self, seed, chain_offset, N, step0=0):
        self.ps, self.chains, self.step0 = orc.PhiloxStream(seed), (chain_offset + np.arange(N)).astype(np.uint32), step0

    def _words(self, s, block):
        return orc.philox4x32_10(np.uint32(block), np.uint32(self.step0 + s), self.chains, np.uint32(STREAM_TREE), self.ps.k0, self.ps.k1)

    def doubling(self, s, j):
        x0, x1, x2, _ = self._words(s, j)
        return (x2 & np.uint32(1)).astype(bool), orc.u53(x0, x1)

    def leaf(self, s, l):
        x0, x1, _, _ = self._words(s, 32 + l)
        return orc.u53(x0, x1)


class ArrayDraws:
    """recorded draws: fwd[N, T, depth] (bool), u[N, T, depth], leaf_u[N, T, 2^depth] indexed by the leaf's number in its step"""

    def __init__(self, fwd, u, leaf_u):
        self.fwd, self.u, self.leaf_u = fwd, u, leaf_u

    def doubling(self, s, j):
        return self.fwd[:, s, j], self.u[:, s, j]

    def leaf(self, s, l):
        return self.leaf_u[:, s, l]


def logaddexp(a, b):
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    return hi + np.log1p(np.exp(lo - hi))


def _gradient(level, theta, F, perturb):
    g = np.asarray(level.grad_logpost(theta, F), dtype=float)
    return g if not perturb else np.nextafter(g, np.inf if perturb > 0 else -np.inf)


def leaf_step(level, th, p, g, e, w, on, perturb=0):
    """one leaf for the chains of the mask `on`: HMC's leapfrog step of size e[N] (negative: backward) from (th, p) with the
    gradient g at th.  -> th, p, g, lp, ll at the new leaves and the mask of those whose log-posterior is finite (the others keep
    the momentum of the half step and the old gradient); chains outside `on` keep everything"""
    p = np.where(on[:, None], p + (0.5 * e)[:, None] * g, p)
    th = np.where(on[:, None], th + e[:, None] * (w[None, :] * p), th)
    lp, ll, F = level.evaluate(th)
    fin = on & np.isfinite(lp + ll)
    g_n = _gradient(level, th, F, perturb)
    g = np.where(fin[:, None], g_n, g)
    p = np.where(fin[:, None], p + (0.5 * e)[:, None] * g, p)
    return th, p, g, lp, ll, fin


def uturn(w, pa, pb, rho):
    return ~((np.sum((w[None, :] * pa) * rho, axis=1) > 0.0) & (np.sum((w[None, :] * pb) * rho, axis=1) > 0.0))


def run_nuts(level, prop, theta0, z, draws, perturb=0, record=None):
    """N chains x T steps on recorded normals z[N, T, d] and the tree draws of `draws`.  -> the trace dict that extengine.compare
    reads (theta, logprior, loglike, logpost, accepted with the initial link at index 0; the final scaling) and beside it, per
    chain and step, `stop` (STOP_NAMES), `depth`, `selected` (the number of the candidate's leaf in its step, 0: the initial
    state), `n_leaf`, `stat`, `fwd` [N, T, max_depth] (-1: the doubling was not begun) and `left` (the tree stopped at a leaf
    whose log-posterior is not finite), and `totals` [N, 4] as the engine reports them.  perturb = +1 / -1: every gradient moved
    up / down by one ulp, for the admission rule below.  record = c: `trees` is a list with one dict per step of chain c (the
    leaves made, the U-turn checks run, the merged doublings, the tree's final log-weight)."""
    theta = np.asarray(theta0, dtype=float).copy()
    N, d = theta.shape
    T, D = z.shape[1], int(prop["max_depth"])
    w = np.ones(d) if prop.get("inv_mass") is None else np.asarray(prop["inv_mass"], dtype=float)
    adaptive, gamma, period = bool(prop.get("adaptive", False)), float(prop.get("gamma", 1.01)), int(prop.get("period", 100))
    eps, target = np.full(N, float(prop["scaling"])), float(prop.get("target_accept", 0.8))
    with np.errstate(all="ignore"):
        lp, ll, F = level.evaluate(theta)
        grad = _gradient(level, theta, F, perturb)
    out_theta, out_lp, out_ll = np.empty((N, T + 1, d)), np.empty((N, T + 1)), np.empty((N, T + 1))
    out_acc = np.ones((N, T + 1), dtype=np.uint8)
    out_theta[:, 0], out_lp[:, 0], out_ll[:, 0] = theta, lp, ll
    stops, depths, selected, n_leaf = (np.zeros((N, T), dtype=int) for _ in range(4))
    stats, fwds, left = np.zeros((N, T)), -np.ones((N, T, D), dtype=int), np.zeros((N, T), dtype=bool)
    totals, accsum, k, trees = np.zeros((N, 4), dtype=np.int64), np.zeros(N), 0, []
    with np.errstate(all="ignore"):
        for s in range(T):
            p0 = z[:, s] / np.sqrt(w)[None, :]
            h0 = -(lp + ll) + 0.5 * np.sum(w[None, :] * (p0 * p0), axis=1)
            lth, pl, lg, rth, pr, rg = theta.copy(), p0.copy(), grad.copy(), theta.copy(), p0.copy(), grad.copy()
            rho, LW = p0.copy(), np.zeros(N)
            cth, cg, clp, cll, csel = theta.copy(), grad.copy(), lp.copy(), ll.copy(), np.zeros(N, dtype=int)
            asum, nleaf, depth, stop = np.zeros(N), np.zeros(N, dtype=int), np.zeros(N, dtype=int), np.zeros(N, dtype=int)
            tree = dict(leaves=[], checks=[], merged=[])
            for j in range(D):
                build = stop == 0  # every chain here has completed j doublings, 2^j - 1 leaves
                if not build.any():
                    break
                fwd, uj = draws.doubling(s, j)
                fwds[build, s, j] = fwd[build]
                e = np.where(fwd, eps, -eps)
                th, p, g = np.where(fwd[:, None], rth, lth), np.where(fwd[:, None], pr, pl), np.where(fwd[:, None], rg, lg)
                sth, sg, slp, sll, ssel = th.copy(), g.copy(), lp.copy(), ll.copy(), np.zeros(N, dtype=int)
                LWs, rs, ck = np.zeros(N), np.zeros((N, d)), {}
                for n in range(1 << j):
                    if not build.any():
                        break
                    l = (1 << j) + n  # the leaf's number in its step
                    th, p, g, lp_n, ll_n, fin = leaf_step(level, th, p, g, e, w, build, perturb)
                    nleaf[build] += 1
                    left[build & ~fin, s] = True
                    h = -(lp_n + ll_n) + 0.5 * np.sum(w[None, :] * (p * p), axis=1)
                    ok = fin & ~(np.isnan(h) | (h - h0 > 1000.0))
                    stop[build & ~ok] = 1
                    build = build & ok
                    lw = h0 - h
                    asum = np.where(ok, asum + np.minimum(1.0, np.exp(lw)), asum)
                    if n == 0:
                        LWs, rs, take = np.where(ok, lw, LWs), np.where(ok[:, None], p, rs), ok
                    else:
                        LWs, rs = np.where(ok, logaddexp(LWs, lw), LWs), np.where(ok[:, None], rs + p, rs)
                        take = ok & (draws.leaf(s, l) < np.exp(lw - LWs))
                    sth, sg = np.where(take[:, None], th, sth), np.where(take[:, None], g, sg)
                    slp, sll, ssel = np.where(take, lp_n, slp), np.where(take, ll_n, sll), np.where(take, l, ssel)
                    if record is not None and ok[record]:
                        tree["leaves"].append(dict(l=l, j=j, n=n, p=p[record].copy(), lw=lw[record], taken=bool(take[record])))
                    top = bin(n >> 1).count("1")
                    if n % 2 == 0:
                        ck[top] = (p.copy(), rs.copy())
                    else:
                        ones, turn = (n ^ (n + 1)).bit_length() - 1, np.zeros(N, dtype=bool)
                        for kk in range(top, top - ones, -1):
                            pa, ra = ck[kk]
                            t_k = uturn(w, pa, p, (rs - ra) + pa)
                            if record is not None and ok[record]:
                                tree["checks"].append(dict(j=j, n=n, row=kk, turn=bool(t_k[record]), rho=((rs - ra) + pa)[record].copy()))
                            turn |= t_k
                        turn &= ok
                        stop[turn] = 2
                        build = build & ~turn
                # merge, for the chains whose subtree completed
                m = build
                take = m & (uj < np.exp(LWs - LW))
                cth, cg = np.where(take[:, None], sth, cth), np.where(take[:, None], sg, cg)
                clp, cll, csel = np.where(take, slp, clp), np.where(take, sll, cll), np.where(take, ssel, csel)
                LW, rho = np.where(m, logaddexp(LW, LWs), LW), np.where(m[:, None], rho + rs, rho)
                mf, mb = m & fwd, m & ~fwd
                rth, pr, rg = np.where(mf[:, None], th, rth), np.where(mf[:, None], p, pr), np.where(mf[:, None], g, rg)
                lth, pl, lg = np.where(mb[:, None], th, lth), np.where(mb[:, None], p, pl), np.where(mb[:, None], g, lg)
                depth = np.where(m, j + 1, depth)
                stop[m & uturn(w, pl, pr, rho)] = 3
                if record is not None and m[record]:
                    tree["merged"].append(j)
            moved = csel > 0
            theta, grad, lp, ll = cth, cg, clp, cll
            stat = asum / nleaf
            accsum = accsum + stat
            totals += np.stack([nleaf, stop == 1, stop == 0, depth], axis=1)
            stops[:, s], depths[:, s], selected[:, s], n_leaf[:, s], stats[:, s] = stop, depth, csel, nleaf, stat
            out_theta[:, s + 1], out_lp[:, s + 1], out_ll[:, s + 1], out_acc[:, s + 1] = theta, lp, ll, moved
            if record is not None:
                tree.update(LW=LW[record], stop=stop[record], depth=depth[record], selected=csel[record], p0=p0[record].copy())
                trees.append(tree)
            if adaptive and (s + 1) % period == 0:  # the engine's rule of the period boundary, on the mean acceptance statistic
                eps = np.exp(np.log(eps) + gamma ** -k * (accsum / period - target))
                accsum = np.zeros(N)
                k += 1
    return dict(theta=out_theta, logprior=out_lp, loglike=out_ll, logpost=out_lp + out_ll, accepted=out_acc, scaling=eps, stop=stops,
                depth=depths, selected=selected, n_leaf=n_leaf, stat=stats, fwd=fwds, left=left, totals=totals, accsum=accsum, trees=trees)


def coverage(ref, max_depth):
    """what a trace exercised: the counts that the coverage conditions of the forward cases are stated in"""
    fwd_deep = ref["fwd"][:, :, 2:] if ref["fwd"].shape[2] > 2 else ref["fwd"][:, :, :0]
    return dict(uturn_subtree=int(np.sum(ref["stop"] == 2)), uturn_tree_deep=int(np.sum((ref["stop"] == 3) & (ref["depth"] >= 2))),
                max_depth=int(np.sum(ref["stop"] == 0)), stayed=int(np.sum(ref["selected"] == 0)), divergent=int(np.sum(ref["stop"] == 1)),
                left_support=int(np.sum(ref["left"])), forward_deep=int(np.sum(fwd_deep == 1)), backward_deep=int(np.sum(fwd_deep == 0)),
                mean_depth=float(ref["depth"].mean()), at_cap=float(np.mean(ref["depth"] == max_depth)))


def assert_admissible(level, prop, theta0, z, draws, ref=None):
    """A tree decision that hangs on the last bits of an energy comes out either way, and then no tolerance holds: a case is
    compared only if the twin builds the same trees -- the same stop reason and depth, the same selected leaf, the same
    `accepted` mask -- when every gradient is moved up by one ulp and again when it is moved down.  -> the unperturbed trace and
    the largest change between those runs of the log-posterior (relative) and of the states (as a share of the bar they are
    compared at, 1e-12 + 1e-9 |state|)"""
    ref = run_nuts(level, prop, theta0, z, draws) if ref is None else ref
    dpost = dstate = 0.0
    for sign in (+1, -1):
        moved = run_nuts(level, prop, theta0, z, draws, perturb=sign)
        for key in ("stop", "depth", "selected", "accepted"):
            assert np.array_equal(moved[key], ref[key]), (key, sign)
        dpost = max(dpost, float(np.max(np.abs(moved["logpost"] / ref["logpost"] - 1.0))))
        dstate = max(dstate, float(np.max(np.abs(moved["theta"] - ref["theta"]) / (1e-12 + 1e-9 * np.abs(ref["theta"])))))
    print("twin: one ulp on every gradient moves the log-posterior by %.1e of itself and the states by %.1e of their bar (1e-12 + 1e-9 |state|); %s"
          % (dpost, dstate, coverage(ref, prop["max_depth"])))
    return ref, dpost, dstate


# ---- the forward-mode cases: the engine on its own Philox stream against the twin ---------------------------------------------------
# tests/test_nuts.py admits every case on the CPU (assert_admissible, on the engine's variates drawn by the oracle's Philox
# stream) and asserts its coverage conditions; tests/test_gpu_nuts.py runs them.  N = 13 chains, T = 120 steps.  The step sizes
# were chosen on the CPU with the twin alone, until it met both.
# d, m, max_depth, noise, adaptive, non-unit mass, block_steps, step size, prior variance (None: exthmc.gaussian_problem's 0.5 ..)
# (96 parameters under 23 outputs and the wide prior of exthmc.gaussian_problem: 73 directions are as wide as the prior, a tree of
# 16 leaves at a stable step size never turns in them, and every tree ends at the cap.  A prior about as tight as the data makes
# the directions alike, and trees of every kind occur)
MASS_SPREAD = lambda d: 4.0 ** (1 - np.arange(d) % 5)  # noqa: E731  (4, 1, 1/4, 1/16, 1/64, ...: stiff and slow directions in one tree)
FORWARD_CASES = {
    "d5_m23_depth3_diag": (5, 23, 3, "diag", False, False, 0, 0.06, None),
    "d5_m23_depth6_diag_mass": (5, 23, 6, "diag", False, "spread", 0, 0.035, None),
    "d96_m23_depth4_iso_adaptive": (96, 23, 4, "iso", 0.65, False, 0, 0.009, 0.002),
    "d5_m23_depth4_diag_adaptive": (5, 23, 4, "diag", True, False, 16, 0.06, None),
}


# The comparison keeps extengine.compare's tolerances (masks exact, log-posterior 1e-10, states 1e-9 of themselves with atol
# 1e-12) unless ten times what one ulp on every gradient moves in the twin exceeds them; such a case is held to ten times that
# change and no more, and is listed here: case -> (log-posterior rtol, states as a multiple of their bar).
#   d96_m23_depth4_iso_adaptive: one ulp moves the log-posterior by 1.6e-11 of itself (it passes close to zero under the tight
#   prior); the states stay at 4e-3 of their bar.
TOLERANCE = {"d96_m23_depth4_iso_adaptive": (1.6e-10, 1.0)}
DEFAULT_TOLERANCE = (1e-10, 1.0)


def tolerance(case):
    return TOLERANCE.get(case, DEFAULT_TOLERANCE)


def assert_within_tolerance(case, dpost, dstate):
    """ten times the change that one ulp on every gradient makes fits the case's tolerance; a case listed in TOLERANCE needs its
    entry (the default would not hold) and gets no more than ten times the change, rounded up to two digits"""
    post_rtol, state_bar = tolerance(case)
    assert 10.0 * dpost <= post_rtol and 10.0 * dstate <= state_bar, (case, dpost, dstate)
    if case in TOLERANCE:
        assert 10.0 * dpost > DEFAULT_TOLERANCE[0] or 10.0 * dstate > DEFAULT_TOLERANCE[1], "the default tolerance holds: drop the entry"
        assert post_rtol <= max(DEFAULT_TOLERANCE[0], 1.05 * 10.0 * dpost) and state_bar <= max(DEFAULT_TOLERANCE[1], 1.05 * 10.0 * dstate)


def compare(case, params, stats, acc, ref, scal=None):
    """extengine.compare at the case's tolerance, and the per-chain acceptance masks first"""
    from .extengine import compare as compare_default

    post_rtol, state_bar = tolerance(case)
    if (post_rtol, state_bar) == DEFAULT_TOLERANCE:
        return compare_default(params, stats, acc, ref, scal)
    assert np.array_equal(acc, np.swapaxes(ref["accepted"][:, 1:], 0, 1))
    want = np.swapaxes(ref["theta"][:, 1:], 0, 1)
    np.testing.assert_allclose(stats[:, :, 2], np.swapaxes(ref["logpost"][:, 1:], 0, 1), rtol=post_rtol)
    np.testing.assert_allclose(params, want, rtol=state_bar * 1e-9, atol=state_bar * 1e-12)
    if scal is not None:
        np.testing.assert_allclose(scal, ref["scaling"], rtol=1e-12)


def gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop, block_steps=0, nan_above=None, seed=SEED):
    e = xh.gaussian_engine(d, m, noise, N, y, pm, pv, nz, dict(kind="mala", scaling=0.1), block_steps, nan_above, seed)
    set_proposal(e, prop)
    return e


def forward_case(name, N=N_CHAINS):
    """-> the oracle level, the proposal, the starts, T, and make() -> the engine (not initialised)"""
    d, m, D, noise, adaptive, mass, bs, eps, prior_var = FORWARD_CASES[name]
    y, theta0, pm, pv, nz, level = xh.gaussian_problem(d, m, noise, N, seed=d * 1000 + m)
    if prior_var is not None:  # the same data, starts and noise under a tighter prior
        from . import extmodel as xm

        pv = prior_var * (1.0 + 0.01 * np.arange(d))
        level = xm.GradLevel(lambda t: xm.np_forward(t, m), y, noise, nz, orc.MVNPrior(pm, np.diag(pv)))
    prop = nuts(eps, D, bool(adaptive), MASS_SPREAD(d) if mass == "spread" else xh.MASS(d) if mass else None, target_accept=0.8 if adaptive in (False, True) else adaptive)
    return level, prop, theta0, T_STEPS, lambda: gaussian_engine(d, m, noise, N, y, pm, pv, nz, prop, bs)


# the contract cases of tests/exthmc.py at max_depth = 4: the step size of each
CONTRACT_STEP = {
    "ring_forward_wave_gradient_wave": 0.12,
    "student_t_loglike": 0.05,
    "ar1_loglike_wave": 0.05,
    "lognormal_prior_at_the_edge": 0.002,
    "cauchy_difference_prior_wave": 0.008,
}


def contract_case(name, N=N_CHAINS):
    level, _, theta0, _, make_hmc = xh.contract_case(name, N)
    prop = nuts(CONTRACT_STEP[name], 4)

    def make():
        e = make_hmc()
        set_proposal(e, prop)
        return e

    return level, prop, theta0, T_STEPS, make


def nan_case(N=N_CHAINS):
    """exthmc's model with a NaN region just beyond the starts -> the level, the proposal, the starts, T, the threshold, make()"""
    level, _, _, theta0, _, thr, make_hmc = xh.nan_case(N)
    prop = nuts(0.02, 4, adaptive=True)

    def make():
        e = make_hmc()
        set_proposal(e, prop)
        return e

    return level, prop, theta0, T_STEPS, thr, make


def philox_normals(N, T, d, seed=SEED, chain_offset=CHAIN_OFFSET):
    return xh.philox_variates(seed, chain_offset, N, T, d)[0]
