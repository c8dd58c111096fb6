"""What the tests of the dense mass adaptation share: the NumPy twin of k_dense_mass_shift / accumulate / update, written from the
text of include/tinyda_amd_dense_mass_adaptation.h (same operations, same order; the schedule is extmass.windows), a two-pass
covariance in np.longdouble with the bound that goes with it, the replay of a run's records through the twin, and a many-chain NUTS
on a rotated Gaussian that pools the dense mass as the engine does (the reference of the end-to-end test).

Two things the twin cannot copy: the matrix instruction adds its four products in an order that is not documented (the twin adds
them chain by chain), and the factorisation on the device fuses each multiply-add (NumPy has no fma).  Both are inside the bound
`tolerance`, which is why the device is held to the twin within it and not bitwise."""
import numpy as np

from . import extmass as xms

CH = 16  # chains per chunk


def shift(x):
    """the pooled mean of the states x [N, d], by the summing rule of k_mass_update (extmass._pooled_sum)"""
    N, d = x.shape
    return np.array([np.float64(xms._pooled_sum(x[:, j])) / np.float64(N) for j in range(d)])


def zeros(N, d):
    """S1 [NC, d], S2 [NC, d, d] of NC = ceil(N / 16) chunks"""
    NC = (N + CH - 1) // CH
    return np.zeros((NC, d)), np.zeros((NC, d, d))


def accumulate(S1, S2, a, X):
    """fold the states X [S, N, d] (step order) into the chunks' sums about the shift a: per step and per chain of a chunk in
    ascending order (which is the order g = 0 .. 3, and inside a group the four chains one after the other), S2 += y y^T and
    S1 += y; the chains behind N are exact zeros.  All chunks at once: they do not meet.  -> S1, S2 (the lower triangle counts)"""
    S, N, d = X.shape
    NC = S1.shape[0]
    S1, S2 = S1.copy(), S2.copy()
    with np.errstate(all="ignore"):
        for x in X:
            Y = np.zeros((NC * CH, d))
            Y[:N] = x - a[None, :]
            Y = Y.reshape(NC, CH, d)
            for k in range(CH):
                y = Y[:, k, :]
                S2 = S2 + y[:, :, None] * y[:, None, :]
                S1 = S1 + y
    return S1, S2


def update(S1, S2, n, N, chol):
    """a window's end over the chunks' sums (n states of each of N chains) -> (the factor, 0), or (chol, 1): the whole factor kept"""
    NC, d = S1.shape
    with np.errstate(all="ignore"):
        s1, s2 = np.zeros(d), np.zeros((d, d))
        for c in range(NC):
            s1, s2 = s1 + S1[c], s2 + S2[c]
        T = np.float64(n) * np.float64(N)
        m = s1 / T
        C = (s2 - (T * m)[:, None] * m[None, :]) / (T - 1.0)
        W = C * T / (T + 5.0)
        W[np.diag_indices(d)] += 1e-3 * 5.0 / (T + 5.0)
        L, ok = np.zeros((d, d)), True
        for j in range(d):  # left-looking, a column at a time; the rows of the column side by side
            acc = W[j:, j].copy()
            for k in range(j):
                acc = acc - L[j:, k] * L[j, k]
            piv = np.sqrt(acc[0])
            ok = ok and bool(np.isfinite(acc[0]) and acc[0] > 0.0 and np.isfinite(piv) and piv > 0.0)
            L[j, j] = piv
            L[j + 1:, j] = acc[1:] / piv
        ok = ok and bool(np.all(np.isfinite(L)))
    return (L, 0) if ok else (np.array(chol, dtype=np.float64), 1)


def window_factor(X, chol, a=None, cuts=()):
    """the twin over one window's states X [n, N, d], folded in blocks that end at `cuts`; a: the shift (None: from X[0])
    -> (the factor, refused, the shift)"""
    n, N, d = X.shape
    a = shift(X[0]) if a is None else np.asarray(a, dtype=np.float64)
    S1, S2 = zeros(N, d)
    lo = 0
    for hi in list(cuts) + [n]:
        S1, S2 = accumulate(S1, S2, a, X[lo:hi])
        lo = hi
    L, refused = update(S1, S2, n, N, chol)
    return L, refused, a


def reference(X):
    """two passes in np.longdouble over the n N states of X [n, N, d] -> (the regularised covariance [d, d], mean, sd)"""
    n, N, d = X.shape
    Y = X.reshape(n * N, d).astype(np.longdouble)
    T = np.longdouble(n * N)
    mean = Y.sum(axis=0) / T
    Z = Y - mean[None, :]
    C = np.zeros((d, d), dtype=np.longdouble)
    for lo in range(0, d, 16):  # (the lower triangle by blocks of rows, mirrored: np.longdouble products are slow)
        hi = min(lo + 16, d)
        C[lo:hi, :hi] = Z[:, lo:hi].T @ Z[:, :hi]
    C = (np.tril(C) + np.tril(C, -1).T) / (T - 1)
    W = C * T / (T + 5)
    W[np.diag_indices(d)] += np.longdouble(1e-3) * 5 / (T + 5)
    return W, mean, np.sqrt(np.diag(C))


def tolerance(n, N, d, mean, sd, a, W):
    """absolute, per entry (i, j) of W: 8 (16 n + N / 16 + d + 16) 2^-53 sqrt((1 + delta_i^2)(1 + delta_j^2)) sqrt(W_ii W_jj),
    delta = (mean - a) / sd -- the first-order bound of the 16 n sequential additions of a chunk, the sum over the chunks and the d
    fused steps of the factorisation, against sum |terms| <= T sqrt(M_ii M_jj) of the raw second moments M about a"""
    mean, sd, a = (np.asarray(v, dtype=np.float64) for v in (mean, sd, a))
    with np.errstate(all="ignore"):
        delta = np.where(sd > 0.0, (mean - a) / sd, 0.0)
    cond = np.sqrt(1.0 + delta ** 2)
    scale = np.sqrt(np.diag(np.asarray(W, dtype=np.float64)))
    return 8.0 * (16.0 * n + N / 16.0 + d + 16.0) * 2.0 ** -53 * (cond * scale)[:, None] * (cond * scale)[None, :]


def gram(L):
    """L L^T in np.longdouble"""
    L = np.asarray(L).astype(np.longdouble)
    return L @ L.T


def assert_window(X, got, chol_before, a, what="", ref=None):
    """`got` is the factor after the window whose states are X [n, N, d] and whose shift was a: L L^T within the bound of the
    twin's and of the two-pass reference's covariance (ref: reference(X), where the caller has it already).  -> the twin's factor"""
    n, N, d = X.shape
    want, refused, _ = window_factor(X, chol_before, a)
    ref, mean, sd = reference(X) if ref is None else ref
    tol = tolerance(n, N, d, mean, sd, a, ref)
    G = gram(got)
    err_ref = (np.abs(G - ref).astype(np.float64) / tol).max()
    err_twin = (np.abs(G - gram(want)).astype(np.float64) / tol).max()
    print("%s n = %d, N = %d, d = %d: against the reference %.3g of the bound, against the twin %.3g; the bound lies in %.1e .. %.1e"
          % (what, n, N, d, err_ref, err_twin, tol.min(), tol.max()))
    assert refused == 0
    assert np.array_equal(got, np.tril(got)) and np.all(np.diag(got) > 0.0)
    assert err_ref <= 1.0 and err_twin <= 1.0, (err_ref, err_twin)
    return want


def inputs(n, N, d, seed):
    """the chosen inputs, scaled to the width: standard deviations over six decades, |mean| / sd up to 10 (in the sample's own
    mean and sd), neighbouring parameters correlated -> X [n, N, d]"""
    rng = np.random.default_rng(seed)
    sd = np.logspace(-3.0, 3.0, d) if d > 1 else np.array([1.0])
    ratio = np.resize(np.array([0.0, 0.3, -1.0, 3.0, -10.0, 10.0, 7.0]), d)
    if d < 6:
        ratio[-1] = 10.0
    Z = rng.standard_normal((n, N, d))
    Z[:, :, 1:] = 0.8 * Z[:, :, 1:] + 0.6 * Z[:, :, :-1]  # correlation 0.6 between neighbours (before the line below, about)
    Z = (Z - Z.mean(axis=(0, 1))) / Z.std(axis=(0, 1), ddof=1)
    return (ratio * sd)[None, None, :] + sd[None, None, :] * Z


def replay_records(states, start, W, period):
    """a run's recorded states [T, N, d] (state s is the one after step s; `start` [N, d] the one before step 0) through the
    schedule -> [(the step count at which the window ended, the window's states, its shift: the twin's, of the state before it)]"""
    out = []
    for first, end in xms.windows(W, period):
        if end > states.shape[0]:
            break
        before = states[first - 1] if first > 0 else start
        out.append((end, states[first:end], shift(before)))
    return out


# ---- the end-to-end reference: many-chain NUTS on a rotated Gaussian with the pooled mass ----------------------------------------
def rotated_problem(sd, seed=0):
    """N(0, R diag(sd^2) R^T), R the Q factor of a seeded normal matrix -> (R, the covariance)"""
    d = len(sd)
    R = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))[0]
    return R, (R * np.asarray(sd) ** 2) @ R.T


def pooled_nuts_reference(sd, R, N, T, scaling, period, adapt_mass, adapt_dense, seed, max_depth=8, target=0.8, gamma=1.01):
    """extmass.pooled_nuts_reference on N(0, R diag(sd^2) R^T), started from the posterior, with the whitened momentum of
    include/tinyda_amd_dense_mass.h (q = L^T p: the draw is z, K = 1/2 q . q, a leaf is q += e/2 L^T g; theta += e L q;
    q += e/2 L^T g, the U-turn test a plain dot product) and, at every window's end, the pooled covariance of the twin above
    (adapt_dense) or the pooled variances of extmass (L = diag(sqrt(w))).  Draws from numpy's generator: a statistical reference.
    -> dict(chol, updates, refused, depth [T, N])"""
    rng = np.random.default_rng(seed)
    sd = np.asarray(sd, dtype=np.float64)
    d = sd.shape[0]
    P = (R / sd ** 2) @ R.T
    theta = (sd[None, :] * rng.standard_normal((N, d))) @ R.T
    L, w, eps, k, accsum = np.eye(d), np.ones(d), np.full(N, float(scaling)), 0, np.zeros(N)
    wins = xms.windows(adapt_mass, period) if adapt_mass else []
    mean, M2, n, updates, refused = np.zeros((N, d)), np.zeros((N, d)), 0, 0, 0
    S1, S2 = zeros(N, d)
    a = np.zeros(d)
    depths = np.zeros((T, N), dtype=int)

    def post(th):
        g = -th @ P
        return 0.5 * np.sum(th * g, axis=1), g

    def lae(x, y):
        hi, lo = np.maximum(x, y), np.minimum(x, y)
        return hi + np.log1p(np.exp(lo - hi))

    def turns(pa, pb, rho):
        return ~((np.sum(pa * rho, axis=1) > 0.0) & (np.sum(pb * rho, axis=1) > 0.0))

    with np.errstate(all="ignore"):
        for s in range(T):
            if any(s == first for first, _ in wins) and adapt_dense:
                a = shift(theta)
            lp, g0 = post(theta)
            p0 = rng.standard_normal((N, d))
            h0 = -lp + 0.5 * np.sum(p0 * p0, axis=1)
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
                    p = np.where(build[:, None], p + (0.5 * e)[:, None] * (g @ L), p)
                    th = np.where(build[:, None], th + e[:, None] * (p @ L.T), th)
                    lp_n, g_n = post(th)
                    g = np.where(build[:, None], g_n, g)
                    p = np.where(build[:, None], p + (0.5 * e)[:, None] * (g @ L), p)
                    nleaf += build
                    h = -lp_n + 0.5 * np.sum(p * p, axis=1)
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
                    n += 1
                    if adapt_dense:
                        S1, S2 = accumulate(S1, S2, a, theta[None])
                    else:
                        mean, M2, _ = xms.accumulate(mean, M2, n - 1, theta[None])
                    if s + 1 == end:
                        if adapt_dense:
                            L, r = update(S1, S2, n, N, L)
                            refused += r
                            S1, S2 = zeros(N, d)
                        else:
                            w, _ = xms.pool(mean, M2, n, w)
                            L = np.diag(np.sqrt(w))
                            mean, M2 = np.zeros((N, d)), np.zeros((N, d))
                        n, updates, k = 0, updates + 1, 0
    return dict(chol=L, updates=updates, refused=refused, depth=depths)
