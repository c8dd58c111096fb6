"""Pooled sample moments (tda_engine_reduce_moments, tda_kernels_pooled.h) and PooledAdaptiveMetropolis against exact references:
every row stride of the moment kernels (1 .. 128 parameters), partial last chunks of k_moments_partial, device and host outputs, and
the pooled covariance replayed through the oracle above 64 parameters."""
import numpy as np
import pytest

from oracle import tinyda_oracle as orc

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
CHUNK = 512  # MOM_CHUNK: rows per block of k_moments_partial
DIMS = [1, 7, 8, 9, 16, 31, 33, 63, 64, 65, 96, 127, 128]
NROWS = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 77]


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def exact_moments(X):
    """[n, sum x, sum x x^T] of the rows of X: every product split exactly into two doubles, the terms added in double-double
    (error below n 2^-100 of sum |terms|, 2^-47 under the bound the engine is held to); and sum |terms| for that bound"""
    n, d = X.shape
    s_hi, s_lo = np.zeros(d), np.zeros(d)
    S_hi, S_lo = np.zeros((d, d)), np.zeros((d, d))
    for x in X:
        s_hi, e = _two_sum(s_hi, x)
        s_lo += e
        p, pe = _two_prod(x[:, None], x[None, :])
        S_hi, e = _two_sum(S_hi, p)
        S_lo += e + pe
    exact = np.concatenate([[float(n)], s_hi + s_lo, (S_hi + S_lo).ravel()])
    A = np.abs(X)
    mag = np.concatenate([[0.0], A.sum(0), (A.T @ A).ravel()])
    return exact, mag


def assert_moments(got, X, exact=None, mag=None, what=""):
    """the count exactly; every sum within 2 n eps sum |terms| (a sequence of n fp64 adds / FMAs), no element left unwritten"""
    if exact is None:
        exact, mag = exact_moments(X)
    n = X.shape[0]
    got = np.asarray(got)
    assert got.shape == exact.shape
    assert not np.isnan(got).any(), "%s: %d output elements never written" % (what, int(np.isnan(got).sum()))
    assert got[0] == n, what
    err, bound = np.abs(got - exact), 2 * n * EPS * mag
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, "%s: %d elements outside the bound, first at %d: got %r, exact %r" % (what, bad.size, bad[0], got[bad[0]], exact[bad[0]])


def _rows(rng, n, d):
    """mixed sign, magnitudes over six decades per column, column 0 offset by about 1e3 (ordering errors would show there)"""
    X = rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-3, 2, size=d)
    X[:, 0] += 1e3
    return X


def _engine(d, N=16):
    from tinyda_amd.engine import Engine

    rng = np.random.default_rng(d)
    e = Engine(N, d, seed=5)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level(0, rng.standard_normal((4, d)), rng.standard_normal(4), 0, 1.0)
    e.set_proposal(0, 0.01 * np.eye(d))
    e.init(0.1 * rng.standard_normal((N, d)))
    return e


@pytest.mark.parametrize("d", DIMS)
def test_reduce_moments_against_exact_sums(d):
    """every DPAD of the moment kernels (and 65 .. 128 parameters), whole and partial 512-row chunks, into a device tensor and into
    host memory, both pre-filled with NaN; rows split over two calls add up to the same moments"""
    import torch

    e = _engine(d)
    rng = np.random.default_rng(100 + d)
    try:
        for n in NROWS:
            X = _rows(rng, n, d)
            exact, mag = exact_moments(X)
            rows = torch.from_numpy(X).cuda()
            out_dev = torch.full((1 + d + d * d,), float("nan"), dtype=torch.float64, device="cuda")
            e.reduce_moments(rows, out_dev)
            assert_moments(out_dev.cpu().numpy(), X, exact, mag, "d=%d n=%d device" % (d, n))
            out_host = np.full(1 + d + d * d, np.nan)
            e.reduce_moments(rows, out_host)
            assert_moments(out_host, X, exact, mag, "d=%d n=%d host" % (d, n))
            if n > 1:
                k = max(1, n // 3)
                a, b = np.full(1 + d + d * d, np.nan), np.full(1 + d + d * d, np.nan)
                e.reduce_moments(rows[:k], a)
                e.reduce_moments(rows[k:], b)
                assert_moments(a + b, X, exact, mag, "d=%d n=%d split at %d" % (d, n, k))
    finally:
        e.close()


def _spd(rng, n, scale):
    B = rng.standard_normal((n, n))
    return scale * (np.eye(n) + 0.3 * B @ B.T / n)


@pytest.mark.parametrize("d", [96, 128])
def test_pooled_adaptive_metropolis_above_64_parameters(d):
    """PooledAdaptiveMetropolis on a 96- / 128-parameter GaussianRandomWalk engine (factor tiles, tda_kernels_wide.h): the pooled sums
    are exact to the bound of the moment test, the engine uses the covariance the pooling computed, and every period replays through
    the oracle under the covariance in force then (accept masks bit for bit, log-posteriors to 1e-10)"""
    import torch

    from tinyda_amd.distributed import PooledAdaptiveMetropolis
    from tinyda_amd.engine import Engine

    N, m, period, n_per = 16, 40, 24, 3
    T = period * n_per
    rng = np.random.default_rng(600 + d)
    A = rng.standard_normal((m, d)) / np.sqrt(d)
    truth = 0.7 * rng.standard_normal(d)
    y = A @ truth + 0.1 * rng.standard_normal(m)
    theta0 = truth + 0.05 * rng.standard_normal((N, d))
    C0 = _spd(rng, d, 2e-3 / d)
    e = Engine(N, d, seed=31 + d)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level(0, A, y, 0, 0.01)
    e.set_proposal(0, C0)
    e.init(theta0)
    z, u = e.set_export(T)
    params = torch.empty((T, N, d), dtype=torch.float64, device="cuda")
    stats = torch.empty((T, N, 3), dtype=torch.float64, device="cuda")
    acc = torch.empty((T, N), dtype=torch.uint8, device="cuda")
    pam = PooledAdaptiveMetropolis(e, C0, t0=period, period=period)
    Cs = [C0]
    for p in range(n_per):
        sl = slice(p * period, (p + 1) * period)
        pam.run(period, params[sl], stats[sl], acc[sl])
        Cs.append(pam.C.copy())
    C_engine = e.proposal_state()["C"][0]
    e.close()
    P, S, Acc = params.cpu().numpy(), stats.cpu().numpy(), acc.cpu().numpy()
    assert_moments(pam.sums.cpu().numpy(), P.reshape(-1, d), what="pooled sums")
    np.testing.assert_allclose(C_engine, pam.C, rtol=1e-10, atol=1e-10 * np.abs(pam.C).max())
    lvl = orc.LinearGaussianLevel(A, y, "iso", 0.01, orc.MVNPrior(np.zeros(d), np.eye(d)))
    start = theta0
    for p in range(n_per):
        sl = slice(p * period, (p + 1) * period)
        res = orc.run_mh(lvl, dict(kind="grw", C=Cs[p]), start, np.swapaxes(z[sl], 0, 1), np.swapaxes(u[sl], 0, 1))
        ref_acc = np.swapaxes(res["accepted"][:, 1:], 0, 1)
        assert np.array_equal(Acc[sl], ref_acc), "period %d: %d accept flips" % (p, int((Acc[sl] != ref_acc).sum()))
        np.testing.assert_allclose(S[sl, :, 2], np.swapaxes(res["logpost"][:, 1:], 0, 1), rtol=1e-10)
        start = P[sl][-1]
    assert 0.02 < Acc.mean() < 0.98
