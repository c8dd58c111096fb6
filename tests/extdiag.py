"""Cases for the convergence diagnostics, shared by tests/test_diagnostics.py (NumPy twin against oracle/ess_oracle.py, no GPU) and
tests/test_gpu_diag.py (tda_diag_ess_rhat against the same oracle).

`SHAPES` are histories [draws, chains, dim] at the sizes where tinyda_amd/csrc/tda_diag.inc takes another path: the number of
256-row blocks of the two-stage power-spectrum mean (nb = ceil(2 chains / 256); the benchmark has nb = 32), a short last block, FFT
lengths at and one above a power of two, more draws per half-chain than a workgroup has threads, the history stride at dim = 128, an
odd number of kept draws.  `EDGES` are single quantities [draws, chains] (one of them [draws, chains, 3]) at the values where the
sort-and-rank path can go wrong: signed zeros, tie runs across every chain, constant chains, infinities, a NaN.

ESS is discontinuous in where Geyer's sequence is cut: a case whose truncating pair sum sits at zero would let rounding alone move
the cut and the answer.  `admit` restates the pair sums and measures the distance of every decision from zero; every case is held
to `MARGIN`, so that a deviation between two implementations is never the cut's.  A case that fails gets another seed (noted
beside it), never a smaller margin."""
import functools

import numpy as np

from oracle import ess_oracle as eo

MARGIN = 1e-6


def history(T, N, d, seed, rho=0.9, sticky=0.6):
    """AR(1) chains with repeated values (rejections produce exact ties), different means per chain for d > 1"""
    rng = np.random.default_rng(seed)
    x = np.zeros((T, N, d))
    cur = rng.standard_normal((N, d))
    for t in range(T):
        move = rng.random((N, 1)) > sticky
        prop = rho * cur + np.sqrt(1 - rho ** 2) * rng.standard_normal((N, d))
        cur = np.where(move, prop, cur)
        x[t] = cur
    x[:, :, -1] += 3.0 * np.arange(N)[None, :] / N  # a parameter whose chains disagree: R-hat > 1
    return x


# name: (T, N, d, burnin); n = (T - burnin) // 2 draws per half-chain, m = FFT length, M = 2 N series, nb = ceil(M / 256)
SHAPES = {
    "smallest": (8, 1, 1, 0),  # n = 4, m = 8, M = 2: the smallest history the entry accepts
    "one_block_full": (16, 128, 1, 0),  # M = 256: nb = 1, exactly full
    "second_block_two_rows": (9, 129, 2, 0),  # odd draws, M = 258: nb = 2, the last block holds 2 rows
    "three_blocks_odd_burnin": (24, 257, 3, 7),  # 17 kept draws, the middle one dropped, nb = 3
    "bench_chains": (80, 4096, 2, 16),  # the benchmark's chain count: M = 8192, nb = 32, 262 144 elements to sort
    "long_and_wide": (700, 300, 2, 60),  # n = 320 > 256 (strided loops of k_diag_center), nf = 513 (three column blocks), nb = 3
    "pow2_half": (264, 5, 128, 8),  # n = 128, m = 256, history stride d = 128, every parameter checked
    "pow2_plus_one": (258, 3, 1, 0),  # n = 129, m = 512
}
SHAPE_SEEDS = {name: 1000 + i for i, name in enumerate(SHAPES)}


@functools.lru_cache(maxsize=None)
def shape_history(name):
    T, N, d, _ = SHAPES[name]
    x = history(T, N, d, SHAPE_SEEDS[name])
    x.setflags(write=False)
    return x


EDGE_DRAWS, EDGE_CHAINS = 240, 18
NAN_AT = (170, 7, 1)  # draw, chain, parameter of the NaN in nan_one_parameter
EDGE_SEEDS = dict(signed_zeros=2001, discrete=2002, one_chain_constant=2003, all_constant=2004, infinities=2005, nan_one_parameter=2006)


def _base(seed):
    return history(EDGE_DRAWS, EDGE_CHAINS, 2, seed)[:, :, 0]  # the parameter whose chains agree


@functools.lru_cache(maxsize=None)
def edges():
    """name -> [draws, chains] (nan_one_parameter: [draws, chains, 3])"""
    out = {}
    x = _base(EDGE_SEEDS["signed_zeros"])
    sign = np.where(np.random.default_rng(EDGE_SEEDS["signed_zeros"] + 100).random(x.shape) < 0.5, -1.0, 1.0)
    out["signed_zeros"] = np.maximum(x, 0.0) * sign  # about half the draws are zeros, -0.0 and +0.0 mixed: one tie run, one rank
    out["discrete"] = np.round(2.0 * _base(EDGE_SEEDS["discrete"]))  # about 13 values: every tie run spans every chain
    x = _base(EDGE_SEEDS["one_chain_constant"]).copy()
    x[:, 5] = x[0, 5]
    out["one_chain_constant"] = x  # one chain never moved
    out["all_constant"] = np.full((EDGE_DRAWS, EDGE_CHAINS), 2.5)  # no variance at all: ESS and R-hat are NaN
    x = _base(EDGE_SEEDS["infinities"]).copy()
    x[40, 3] = np.inf
    x[200, 11] = -np.inf
    out["infinities"] = x  # ranks do not care how large a value is
    x = history(EDGE_DRAWS, EDGE_CHAINS, 3, EDGE_SEEDS["nan_one_parameter"])
    x[NAN_AT] = np.nan
    out["nan_one_parameter"] = x
    for v in out.values():
        v.setflags(write=False)
    return out


EDGES = tuple(EDGE_SEEDS)


def nan_replaced():
    """nan_one_parameter with a finite draw (the chain's previous one) in the NaN's place"""
    x = edges()["nan_one_parameter"].copy()
    t, c, j = NAN_AT
    x[t, c, j] = x[t - 1, c, j]
    return x


def columns(x, burnin=0):
    """the [chains, draws] views of every parameter of a history [draws, chains(, dim)], as the CPU estimators take them"""
    x = x[burnin:]
    return [x.T] if x.ndim == 2 else [x[:, :, j].T for j in range(x.shape[2])]


def admit(x):
    """Distance from zero of every decision Geyer's truncation takes on x [chains, draws]: the pair sums P_k = rho_2k + rho_2k+1
    that are kept, the first negative one that cuts the sequence, and rho_2k at the cut, whose positive part is added.  Restated
    here from the paper's equations on the oracle's normal scores; inf where there is no sequence (no variance)."""
    z = eo.normal_scores(eo.split_chains(x))
    m, n = z.shape
    zc = z - z.mean(axis=1, keepdims=True)
    acov = np.array([np.mean(np.sum(zc[:, :n - t] * zc[:, t:], axis=1)) / n for t in range(n)])
    W = acov[0] * n / (n - 1.0)
    var_plus = W * (n - 1.0) / n + (z.mean(axis=1).var(ddof=1) if m > 1 else 0.0)
    if not var_plus > 0:
        return np.inf
    rho = 1.0 - (W - acov) / var_plus
    rho[0] = 1.0
    margin = np.inf
    for k in range(n // 2):
        pk = rho[2 * k] + rho[2 * k + 1]
        margin = min(margin, abs(pk))
        if pk < 0:
            margin = min(margin, abs(rho[2 * k]))
            break
    return float(margin)


@functools.lru_cache(maxsize=None)
def reference(name):
    """oracle (ess [dim], rhat [dim]) of a SHAPES or EDGES case, computed once; nan_one_parameter: of its finite replacement"""
    if name in SHAPES:
        cols = columns(shape_history(name), SHAPES[name][3])
    else:
        cols = columns(nan_replaced() if name == "nan_one_parameter" else edges()[name])
    out = np.array([eo.ess_bulk(c) for c in cols]), np.array([eo.rhat(c) for c in cols])
    for v in out:
        v.setflags(write=False)
    return out


def deviation(got, want):
    """largest relative deviation; NaN against NaN counts as none, NaN against a number as infinite"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    both = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(both, 0.0, np.abs(got - want) / np.abs(want))
    return float(np.max(np.where(np.isnan(rel), np.inf, rel)))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))
