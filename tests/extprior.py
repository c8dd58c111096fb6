"""What the source-defined-prior tests share: the 13 scipy families that JointPrior lowers through the term library
(tinyda_amd/csrc/tda_prior_families.h), cycled to any dimension; FamilyPrior, the same prior as an oracle level's prior
(scipy's own logpdf summed in parameter order); host_library, the shipped library compiled for the host; and a hand-written DevicePrior source (independent lognormals, p = log of
the median, q = sigma of the logarithm) with its NumPy twin; and, for the GPU tests, the engine and the oracle level over
extmodel's forward model under such a prior."""
import ctypes
import subprocess

import numpy as np
import scipy.stats as st

from oracle import tinyda_oracle as orc

from .extengine import PRIOR_SOURCE, set_proposal
from .extmodel import np_forward

SIGMA2 = 0.01  # the noise variance of the problems over extmodel's forward model

FAMILY_NAMES = ("lognorm", "gamma", "beta", "norm", "uniform", "expon", "halfnorm", "invgamma", "laplace", "cauchy", "t",
                "truncnorm", "weibull_min")
# name -> (shape parameters, loc, scale): every family of the library once
FAMILY_PARAMS = {
    "lognorm": ((0.7,), 0.0, 0.3), "gamma": ((2.5,), 0.0, 0.15), "beta": ((2.0, 3.5), 0.0, 1.0), "norm": ((), 0.1, 0.7),
    "uniform": ((), -0.2, 1.0), "expon": ((), 0.0, 0.4), "halfnorm": ((), 0.0, 0.5), "invgamma": ((3.0,), 0.0, 0.8),
    "laplace": ((), 0.1, 0.5), "cauchy": ((), 0.0, 0.5), "t": ((4.0,), 0.1, 0.6), "truncnorm": ((-1.0, 2.0), 0.2, 0.4),
    "weibull_min": ((1.7,), 0.0, 0.5),
}


def component(name, shapes=None, loc=None, scale=None):
    sh, lo, sc = FAMILY_PARAMS[name]
    return getattr(st, name)(*(sh if shapes is None else shapes), loc=lo if loc is None else loc, scale=sc if scale is None else scale)


def components(d, names=FAMILY_NAMES):
    """d frozen scipy components, the families in the order of `names`, cycled"""
    return [component(names[j % len(names)]) for j in range(d)]


def support(dist):
    """closed hull of a frozen component's support"""
    lo, hi = dist.support()
    return float(lo), float(hi)


class FamilyPrior:
    """independent scipy components as the prior of an oracle level: logpdf(theta[N, d]) -> [N], summed in parameter order,
    -inf outside a support; mean and cov as the oracle's MVNPrior has them (placeholders where a family has no moments)"""

    def __init__(self, comps):
        self.comps = list(comps)
        self.dim = len(self.comps)
        with np.errstate(all="ignore"):
            mean = np.array([c.mean() for c in self.comps], dtype=float)
            var = np.array([c.var() for c in self.comps], dtype=float)
        self.mean = np.where(np.isfinite(mean), mean, 0.0)
        self.cov = np.diag(np.where(np.isfinite(var) & (var > 0), var, 1.0))

    def logpdf(self, theta):
        theta = np.atleast_2d(np.asarray(theta, dtype=float))
        out = np.zeros(theta.shape[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            for j, c in enumerate(self.comps):
                out = out + c.logpdf(theta[:, j])
        return out

    def magnitude(self, theta):
        """[N] sum of the magnitudes of the components' log-densities: the scale of the rounding error of logpdf, whose terms
        may cancel"""
        theta = np.atleast_2d(np.asarray(theta, dtype=float))
        out = np.zeros(theta.shape[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            for j, c in enumerate(self.comps):
                out = out + np.abs(c.logpdf(theta[:, j]))
        return out

    def inside(self, theta):
        """[N] True where every component of theta[N, d] lies in its support"""
        theta = np.atleast_2d(theta)
        ok = np.ones(theta.shape[0], dtype=bool)
        for j, c in enumerate(self.comps):
            lo, hi = support(c)
            ok &= (theta[:, j] >= lo) & (theta[:, j] <= hi)
        return ok


def starts_near_lower_edges(comps, n, rng, q0=0.15):
    """n starting points inside the supports, at low quantiles of the components (so that proposals leave the supports)"""
    truth = np.array([c.ppf(q0 + 0.1 * (j % 3)) for j, c in enumerate(comps)])
    th = truth[None, :] + 0.01 * rng.standard_normal((n, len(comps)))
    for j, c in enumerate(comps):
        lo, hi = support(c)
        if np.isfinite(lo):
            th[:, j] = lo + np.abs(th[:, j] - lo)
        if np.isfinite(hi):
            th[:, j] = hi - np.abs(hi - th[:, j])
    return truth, th


def family_source(comps):
    """(p, q, HIP source of the prior) exactly as sample() hands them over"""
    import tinyda_amd as tda

    _, p, q, src = tda.JointPrior(comps)._source_lowering()
    return p, q, src


def level_of(comps, m, y, shift=0.0, coup=0.5, noise=("iso", SIGMA2)):
    return orc.CallableGaussianLevel(lambda th: np_forward(th, m, shift=shift, coup=coup), y, noise[0], noise[1], FamilyPrior(comps))


def make_engine(comps, N, levels, prop, bs=0, seed=93, chain_offset=5, subchains=None):
    """levels: [(model (+ likelihood) source, data, noise kind, noise)]; the prior is set first, so every level compiles once"""
    from tinyda_amd.engine import Engine

    p, q, psrc = family_source(comps)
    e = Engine(N, len(comps), seed=seed, chain_offset=chain_offset, block_steps=bs, n_levels=len(levels))
    e.set_prior_joint(np.full(len(comps), PRIOR_SOURCE), p, q)
    for k, (src, y, kind, noise) in enumerate(levels):
        e.set_level_source(k, src + "\n" + psrc, y, kind, noise)
    set_proposal(e, prop)
    if subchains is not None:
        e.set_subchains(subchains, False)
    return e


def oracle_proposals_outside(ref, prior, z, prop):
    """[N, T] True where the random-walk proposal of step t left a support (fixed scaling, C = I: theta + scaling z)"""
    props = ref["theta"][:, :-1] + prop["scaling"] * z
    N, T, d = props.shape
    return ~prior.inside(props.reshape(-1, d)).reshape(N, T)


def host_library(tmp_path, comps):
    """the library exactly as shipped, behind the prologue generated for `comps`, compiled for the host: term(x, j)"""
    from tinyda_amd import likelihoods as lk

    rows = [lk._family_component(c) for c in comps]
    assert all(r is not None for r in rows)
    src = ("#include <cmath>\nusing std::log; using std::log1p; using std::exp; using std::fabs;\n#define __device__\n"
           + lk._family_prologue(rows) + lk.family_library_source()
           + "\nextern \"C\" void terms(const double* x, const double* p, const double* q, int j, int n, double* out) {\n"
             "  for (int i = 0; i < n; ++i) out[i] = tda_logprior_term(x[i], p[j], q[j], j);\n}\n")
    cpp, so = tmp_path / "lib.cpp", tmp_path / "lib.so"
    cpp.write_text(src)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(cpp)], check=True)
    lib = ctypes.CDLL(str(so))
    p, q = np.array([r[4] for r in rows]), np.array([r[5] for r in rows])

    def term(x, j):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        dp = ctypes.POINTER(ctypes.c_double)
        lib.terms(x.ctypes.data_as(dp), p.ctypes.data_as(dp), q.ctypes.data_as(dp), ctypes.c_int(j), ctypes.c_int(x.size), out.ctypes.data_as(dp))
        return out

    return term, rows


# ---- a hand-written DevicePrior: independent lognormals, p = log median, q = sigma of log theta --------------------------------
LOGNORMAL_SRC = r"""
__device__ double tda_logprior_term(double x, double p, double q, int j) {
  if (!(x > 0.0)) return -__builtin_inf();
  const double l = log(x), r = (l - p) / q;
  return -l - 0.5 * r * r - log(q) - 0.9189385332046727;   // 0.5 log(2 pi)
}
"""

# all-normal components through the source path: p = mean, q = standard deviation
NORMAL_SRC = r"""
__device__ double tda_logprior_term(double x, double p, double q, int j) {
  const double r = (x - p) / q;
  return -0.5 * r * r - log(q) - 0.9189385332046727;
}
"""


def lognormal_terms(theta, p, q):
    theta = np.atleast_2d(np.asarray(theta, dtype=float))
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.log(theta)
        t = -l - 0.5 * ((l - p) / q) ** 2 - np.log(q) - 0.9189385332046727
    return np.where(theta > 0.0, t, -np.inf)


class LognormalPrior:
    """NumPy twin of LOGNORMAL_SRC: oracle prior and `reference=` of the DevicePrior"""

    def __init__(self, p, q):
        self.p, self.q = np.asarray(p, dtype=float), np.asarray(q, dtype=float)
        self.dim = self.p.shape[0]
        self.mean = np.exp(self.p + 0.5 * self.q ** 2)
        self.cov = np.diag((np.exp(self.q ** 2) - 1.0) * self.mean ** 2)

    def logpdf(self, theta):
        out = np.zeros(np.atleast_2d(theta).shape[0])
        t = lognormal_terms(theta, self.p, self.q)
        for j in range(self.dim):
            out = out + t[:, j]
        return out if np.ndim(theta) == 2 else out[0]

    def rvs(self, n_samples=1, random_state=None):
        rng = np.random.default_rng(random_state)
        x = np.exp(self.p + self.q * rng.standard_normal((n_samples, self.dim)))
        return x[0] if n_samples == 1 else x
