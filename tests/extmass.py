"""What the tests of the mass adaptation share: the NumPy twin of k_mass_accumulate / k_mass_update and of the schedule, written
from the text of include/tinyda_amd_mass.h (same operations, same order), a two-pass reference in np.longdouble with the tolerance
that goes with it, the replay of a run's records through the twin, and a many-chain NUTS on a diagonal Gaussian that pools the
mass as the engine does (the reference of the end-to-end test).

The twin is scalar on purpose: one parameter at a time, one chain at a time, so that the order of every sum can be read off."""
import numpy as np

THREADS = 256


def windows(W, period):
    """the windows in steps, [(first, end exclusive)]: period 0 is a buffer; lengths 1, 2, 4, .. periods; a window of L periods
    at period s with s + 3 L > P takes the rest and is the last"""
    assert W % period == 0 and W >= 2 * period
    P, s, L, out = W // period, 1, 1, []
    while s < P:
        if s + 3 * L > P:
            L = P - s
        out.append((s * period, (s + L) * period))
        s += L
        L *= 2
    return out


def accumulate(mean, M2, n, X):
    """fold the states X [S, N, d] (step order) into the per-chain moments mean, M2 [N, d] that hold n states -> mean, M2, n"""
    mean, M2 = mean.copy(), M2.copy()
    with np.errstate(all="ignore"):
        for x in X:
            n += 1
            delta = x - mean
            mean = mean + delta / float(n)
            M2 = M2 + delta * (x - mean)
    return mean, M2, n


def _pooled_sum(v):
    """thread t adds v[c] for c = t, t + 256, .. in that order; then a[t] += a[t + s] for s = 128 .. 1"""
    a = [0.0] * THREADS
    for c in range(len(v)):
        a[c % THREADS] = a[c % THREADS] + float(v[c])
    s = THREADS // 2
    while s >= 1:
        for t in range(s):
            a[t] = a[t] + a[t + s]
        s //= 2
    return a[0]


def pool(mean, M2, n, inv_mass):
    """a window's end over the moments [N, d] of N chains with n states each -> (the new inverse mass, entries refused)"""
    N, d = mean.shape
    out, refused = np.array(inv_mass, dtype=np.float64), 0
    with np.errstate(all="ignore"):
        for j in range(d):
            mbar = np.float64(_pooled_sum(mean[:, j])) / np.float64(N)
            dm = mean[:, j] - mbar
            B, Wn = np.float64(_pooled_sum(dm * dm)), np.float64(_pooled_sum(M2[:, j]))
            nn = np.float64(n)
            T = nn * np.float64(N)
            var = (Wn + nn * B) / (T - 1.0)
            w = var * T / (T + 5.0) + 1e-3 * 5.0 / (T + 5.0)
            if np.isfinite(w) and w > 0.0:
                out[j] = w
            else:
                refused += 1
    return out, refused


def window_mass(X, inv_mass):
    """the twin over one window's states X [n, N, d] -> (the new inverse mass, entries refused)"""
    n, N, d = X.shape
    mean, M2, k = accumulate(np.zeros((N, d)), np.zeros((N, d)), 0, X)
    return pool(mean, M2, k, inv_mass)


def reference(X):
    """two passes in np.longdouble over the n N states of X [n, N, d] -> (the regularised variance, mean, sd) per parameter"""
    n, N, d = X.shape
    Y = X.reshape(n * N, d).astype(np.longdouble)
    T = np.longdouble(n * N)
    mean = Y.sum(axis=0) / T
    var = ((Y - mean[None, :]) ** 2).sum(axis=0) / (T - 1)
    w = var * T / (T + 5) + np.longdouble(1e-3) * 5 / (T + 5)
    return w, mean, np.sqrt(var)


def tolerance(n, N, mean, sd):
    """relative, per parameter: eight times the first-order bound of the recursion (n steps) plus the strided sums and the tree
    (N / 256 + 8 additions, and the handful of operations of the update), times the conditioning of a variance, 1 + (mean / sd)^2"""
    return np.asarray(8.0 * (n + N / 256.0 + 16.0) * 2.0 ** -53 * (1.0 + (mean / sd) ** 2), dtype=np.float64)


def assert_window(X, got, inv_mass_before, what=""):
    """`got` is the mass after the window whose states are X [n, N, d]: the twin's and the two-pass reference's, each within the
    tolerance of the shape"""
    n, N, _ = X.shape
    want, refused = window_mass(X, inv_mass_before)
    ref, mean, sd = reference(X)
    tol = tolerance(n, N, mean.astype(np.float64), sd.astype(np.float64))
    err_ref = np.abs((got.astype(np.longdouble) - ref) / ref).astype(np.float64)
    err_twin = np.abs(got / want - 1.0)
    print("%s n = %d, N = %d: against the reference %.2e, against the twin %.2e, tolerance %.2e" % (what, n, N, err_ref.max(), err_twin.max(), tol.min()))
    assert refused == 0
    assert np.all(err_ref <= tol), (err_ref, tol)
    assert np.all(err_twin <= tol), (err_twin, tol)


def replay_records(states, W, period, inv_mass0):
    """a run's recorded states [T, N, d] (state s is the one after step s) through the schedule and the twin
    -> [(the step count at which the window ended, the window's states, the mass before, the mass after)]"""
    out, w = [], np.array(inv_mass0, dtype=np.float64)
    for first, end in windows(W, period):
        if end > states.shape[0]:
            break
        new, _ = window_mass(states[first:end], w)
        out.append((end, states[first:end], w, new))
        w = new
    return out


# ---- the end-to-end reference: many-chain NUTS on a diagonal Gaussian with the pooled mass ----------------------------------------
def pooled_nuts_reference(sd, N, T, scaling, period, adapt_mass, seed, max_depth=8, target=0.8, gamma=1.01, start_scale=1.0):
    """N chains of multinomial NUTS (include/tinyda_amd_nuts.h, vectorised over the chains under masks) on N(0, diag(sd^2)), the
    step size adapted per chain at the period boundary, the inverse mass pooled over the chains on the schedule above (0: unit
    mass throughout), k restarted at every update.  Draws from numpy's generator: a statistical reference, not a bitwise one.
    -> dict(inv_mass, updates, depth [T, N])"""
    rng = np.random.default_rng(seed)
    sd = np.asarray(sd, dtype=np.float64)
    d, prec = sd.shape[0], 1.0 / sd ** 2
    theta = start_scale * sd[None, :] * rng.standard_normal((N, d))
    w, eps, k, accsum = np.ones(d), np.full(N, float(scaling)), 0, np.zeros(N)
    wins = windows(adapt_mass, period) if adapt_mass else []
    mean, M2, n, updates = np.zeros((N, d)), np.zeros((N, d)), 0, 0
    depths = np.zeros((T, N), dtype=int)

    def post(th):
        return -0.5 * np.sum(th * th * prec[None, :], axis=1), -th * prec[None, :]

    def lae(a, b):
        hi, lo = np.maximum(a, b), np.minimum(a, b)
        return hi + np.log1p(np.exp(lo - hi))

    def turns(pa, pb, rho):
        return ~((np.sum((w[None, :] * pa) * rho, axis=1) > 0.0) & (np.sum((w[None, :] * pb) * rho, axis=1) > 0.0))

    with np.errstate(all="ignore"):
        for s in range(T):
            lp, g0 = post(theta)
            p0 = rng.standard_normal((N, d)) / np.sqrt(w)[None, :]
            h0 = -lp + 0.5 * np.sum(w[None, :] * p0 * p0, axis=1)
            lth, pl, lg, rth, pr, rg = theta.copy(), p0.copy(), g0.copy(), theta.copy(), p0.copy(), g0.copy()
            rho, LW, cth = p0.copy(), np.zeros(N), theta.copy()
            asum, nleaf, depth, live = np.zeros(N), np.zeros(N), np.zeros(N, dtype=int), np.ones(N, dtype=bool)
            for j in range(max_depth):
                build = live.copy()
                if not build.any():
                    break
                fwd, uj = rng.integers(0, 2, N).astype(bool), rng.random(N)
                e = np.where(fwd, eps, -eps)
                th, p, g = np.where(fwd[:, None], rth, lth), np.where(fwd[:, None], pr, pl), np.where(fwd[:, None], rg, lg)
                sth, LWs, rs, ck = th.copy(), np.zeros(N), np.zeros((N, d)), {}
                for i in range(1 << j):
                    if not build.any():
                        break
                    p = np.where(build[:, None], p + (0.5 * e)[:, None] * g, p)
                    th = np.where(build[:, None], th + e[:, None] * (w[None, :] * p), th)
                    lp_n, g_n = post(th)
                    g = np.where(build[:, None], g_n, g)
                    p = np.where(build[:, None], p + (0.5 * e)[:, None] * g, p)
                    nleaf += build
                    h = -lp_n + 0.5 * np.sum(w[None, :] * p * p, axis=1)
                    ok = build & np.isfinite(lp_n) & ~(np.isnan(h) | (h - h0 > 1000.0))
                    live &= ~(build & ~ok)
                    build = ok
                    lw = h0 - h
                    asum = np.where(ok, asum + np.minimum(1.0, np.exp(lw)), asum)
                    if i == 0:
                        LWs, rs, take = np.where(ok, lw, LWs), np.where(ok[:, None], p, rs), ok
                    else:
                        LWs, rs = np.where(ok, lae(LWs, lw), LWs), np.where(ok[:, None], rs + p, rs)
                        take = ok & (rng.random(N) < np.exp(lw - LWs))
                    sth = np.where(take[:, None], th, sth)
                    top = bin(i >> 1).count("1")
                    if i % 2 == 0:
                        ck[top] = (p.copy(), rs.copy())
                    else:
                        ones, turn = (i ^ (i + 1)).bit_length() - 1, np.zeros(N, dtype=bool)
                        for kk in range(top, top - ones, -1):
                            pa, ra = ck[kk]
                            turn |= turns(pa, p, (rs - ra) + pa)
                        turn &= ok
                        live &= ~turn
                        build = build & ~turn
                m = build
                take = m & (uj < np.exp(LWs - LW))
                cth = np.where(take[:, None], sth, cth)
                LW, rho = np.where(m, lae(LW, LWs), LW), np.where(m[:, None], rho + rs, rho)
                mf, mb = m & fwd, m & ~fwd
                rth, pr, rg = np.where(mf[:, None], th, rth), np.where(mf[:, None], p, pr), np.where(mf[:, None], g, rg)
                lth, pl, lg = np.where(mb[:, None], th, lth), np.where(mb[:, None], p, pl), np.where(mb[:, None], g, lg)
                depth = np.where(m, j + 1, depth)
                live &= ~(m & turns(pl, pr, rho))
            theta = cth
            depths[s] = depth
            accsum += asum / nleaf
            if (s + 1) % period == 0:
                eps = np.exp(np.log(eps) + gamma ** -k * (accsum / period - target))
                accsum = np.zeros(N)
                k += 1
            for first, end in wins:
                if first <= s < end:
                    mean, M2, n = accumulate(mean, M2, n, theta[None])
                    if s + 1 == end:
                        w, _ = pool(mean, M2, n, w)
                        mean, M2, n, updates, k = np.zeros((N, d)), np.zeros((N, d)), 0, updates + 1, 0
    return dict(inv_mass=w, updates=updates, depth=depths)
