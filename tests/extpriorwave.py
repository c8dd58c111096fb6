"""What the tests of priors that couple parameters share (tda_logprior_wave / tda_logprior_grad): four such priors, each as HIP
source with both functions and as a NumPy twin (logpdf, magnitude -- the sum of the magnitudes of the terms, which
extengine.assert_logprior measures the rounding error against --, grad, rvs; mean / cov placeholders as extprior.FamilyPrior has
them), the oracle levels over extmodel's forward model under such a prior, and the engine set up with one.

  1. CauchyDifference   theta_0 ~ N(p_0, q_0^2), theta_j - theta_{j-1} ~ Cauchy(0, q_j): the edge-preserving prior
  2. TotalVariation     -p_j |theta_j - theta_{j-1}| (unnormalised) with theta_0 ~ N(p_0, q_0^2)
  3. Hierarchical       theta_0 = log tau ~ N(0, 1), theta_j | tau ~ N(0, tau^2): every lane reads theta[0]
  4. Ordered            box-uniform on [p_j, p_j + q_j], -inf unless theta_0 < theta_1 < ...: the support is decided by neighbours

Each source spreads its terms over the lanes by `for (j = lane; j < dim; j += 64)`; the twins sum them in parameter order."""
import numpy as np

from oracle import tinyda_oracle as orc

from . import extmodel as xm
from .extengine import PRIOR_SOURCE, set_proposal

SIGMA2 = 0.01
WAVE_SIG = "__device__ double tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane)"
GRAD_SIG = "__device__ double tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j)"
HALF_LOG_2PI = 0.9189385332046727
LOG_PI = 1.1447298858494002

CAUCHY_DIFF_SRC = r"""
__device__ double tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane) {
  double s = 0.0;
  for (int j = lane; j < dim; j += 64) {
    if (j == 0) {
      const double r = (theta[0] - p[0]) / q[0];
      s += -0.5 * r * r - log(q[0]) - 0.9189385332046727;   // 0.5 log(2 pi)
    } else {
      const double r = (theta[j] - theta[j - 1]) / q[j];
      s += -log1p(r * r) - log(q[j]) - 1.1447298858494002;  // log(pi)
    }
  }
  return s;
}
__device__ double tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j) {
  double g;
  if (j == 0) {
    g = (p[0] - theta[0]) / (q[0] * q[0]);
  } else {
    const double r = (theta[j] - theta[j - 1]) / q[j];
    g = -2.0 * r / (1.0 + r * r) / q[j];
  }
  if (j + 1 < dim) {
    const double r = (theta[j + 1] - theta[j]) / q[j + 1];
    g += 2.0 * r / (1.0 + r * r) / q[j + 1];
  }
  return g;
}
"""

TV_SRC = r"""
__device__ double tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane) {
  double s = 0.0;
  for (int j = lane; j < dim; j += 64) {
    if (j == 0) {
      const double r = (theta[0] - p[0]) / q[0];
      s += -0.5 * r * r - log(q[0]) - 0.9189385332046727;
    } else {
      s += -p[j] * fabs(theta[j] - theta[j - 1]);
    }
  }
  return s;
}
__device__ double tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j) {
  double g;
  if (j == 0) {
    g = (p[0] - theta[0]) / (q[0] * q[0]);
  } else {
    const double dl = theta[j] - theta[j - 1];
    g = -p[j] * (dl > 0.0 ? 1.0 : dl < 0.0 ? -1.0 : 0.0);
  }
  if (j + 1 < dim) {
    const double dl = theta[j + 1] - theta[j];
    g += p[j + 1] * (dl > 0.0 ? 1.0 : dl < 0.0 ? -1.0 : 0.0);
  }
  return g;
}
"""

HIERARCHICAL_SRC = r"""
__device__ double tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane) {
  const double t0 = theta[0], w = exp(-2.0 * t0);   // 1 / tau^2
  double s = 0.0;
  for (int j = lane; j < dim; j += 64) {
    if (j == 0) s += -0.5 * t0 * t0 - 0.9189385332046727;
    else s += -0.5 * (theta[j] * theta[j]) * w - t0 - 0.9189385332046727;
  }
  return s;
}
__device__ double tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j) {
  const double w = exp(-2.0 * theta[0]);
  if (j > 0) return -theta[j] * w;
  double g = -theta[0];
  for (int k = 1; k < dim; ++k) g += (theta[k] * theta[k]) * w - 1.0;
  return g;
}
"""

# NAN_ABOVE: above it (in theta_0) lane 0's share is NaN, which must reject like a NaN output of the model
ORDERED_TEMPLATE = r"""
__device__ double tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane) {
  double s = 0.0;
  if (lane == 0 && theta[0] > NAN_ABOVE) return __builtin_nan("");
  for (int j = lane; j < dim; j += 64) {
    if (theta[j] < p[j] || theta[j] > p[j] + q[j]) return -__builtin_inf();
    if (j > 0 && !(theta[j - 1] < theta[j])) return -__builtin_inf();
    s -= log(q[j]);
  }
  return s;
}
__device__ double tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j) {
  for (int k = 0; k < dim; ++k)
    if (theta[k] < p[k] || theta[k] > p[k] + q[k] || (k > 0 && !(theta[k - 1] < theta[k]))) return GRAD_OUTSIDE;
  return 0.0;   // flat inside the support
}
"""


def ordered_source(nan_above=None, grad_outside="0.0"):
    """the ordered prior's source; grad_outside: what tda_logprior_grad returns outside the support, where its value is free"""
    return ORDERED_TEMPLATE.replace("NAN_ABOVE", "1e300" if nan_above is None else repr(float(nan_above))).replace("GRAD_OUTSIDE", grad_outside)


class _Twin:
    """logpdf / magnitude from terms(theta[N, d]) -> [N, d], summed in parameter order; placeholders for the moments"""

    source = None

    def __init__(self, p, q):
        self.p, self.q = np.asarray(p, dtype=float), np.asarray(q, dtype=float)
        self.dim = self.p.shape[0]
        self.mean = np.zeros(self.dim)
        self.cov = np.eye(self.dim)

    def _sum(self, t):
        out = np.zeros(t.shape[0])
        for j in range(self.dim):
            out = out + t[:, j]
        return out

    def logpdf(self, theta):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            out = self._sum(self.terms(np.atleast_2d(np.asarray(theta, dtype=float))))
        return out if np.ndim(theta) == 2 else out[0]

    def magnitude(self, theta):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            return self._sum(np.abs(self.terms(np.atleast_2d(np.asarray(theta, dtype=float)))))

    def grad(self, theta):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            g = self._grad(np.atleast_2d(np.asarray(theta, dtype=float)))
        return g if np.ndim(theta) == 2 else g[0]

    def rvs(self, n_samples=1, random_state=None):
        x = self._rvs(n_samples, np.random.default_rng(random_state))
        return x[0] if n_samples == 1 else x


class CauchyDifference(_Twin):
    source = CAUCHY_DIFF_SRC

    def terms(self, th):
        t = np.empty_like(th)
        r0 = (th[:, 0] - self.p[0]) / self.q[0]
        t[:, 0] = -0.5 * r0 * r0 - np.log(self.q[0]) - HALF_LOG_2PI
        r = (th[:, 1:] - th[:, :-1]) / self.q[1:]
        t[:, 1:] = -np.log1p(r * r) - np.log(self.q[1:]) - LOG_PI
        return t

    def _grad(self, th):
        g = np.empty_like(th)
        g[:, 0] = (self.p[0] - th[:, 0]) / (self.q[0] * self.q[0])
        r = (th[:, 1:] - th[:, :-1]) / self.q[1:]
        c = 2.0 * r / (1.0 + r * r) / self.q[1:]
        g[:, 1:] = -c
        g[:, :-1] += c
        return g

    def _rvs(self, n, rng):
        x = np.empty((n, self.dim))
        x[:, 0] = self.p[0] + self.q[0] * rng.standard_normal(n)
        x[:, 1:] = self.q[1:] * rng.standard_cauchy((n, self.dim - 1))
        return np.cumsum(x, axis=1)


class TotalVariation(_Twin):
    source = TV_SRC

    def terms(self, th):
        t = np.empty_like(th)
        r0 = (th[:, 0] - self.p[0]) / self.q[0]
        t[:, 0] = -0.5 * r0 * r0 - np.log(self.q[0]) - HALF_LOG_2PI
        t[:, 1:] = -self.p[1:] * np.abs(th[:, 1:] - th[:, :-1])
        return t

    def _grad(self, th):
        g = np.empty_like(th)
        g[:, 0] = (self.p[0] - th[:, 0]) / (self.q[0] * self.q[0])
        c = self.p[1:] * np.sign(th[:, 1:] - th[:, :-1])
        g[:, 1:] = -c
        g[:, :-1] += c
        return g

    def _rvs(self, n, rng):
        x = np.empty((n, self.dim))
        x[:, 0] = self.p[0] + self.q[0] * rng.standard_normal(n)
        x[:, 1:] = rng.laplace(0.0, 1.0 / self.p[1:], (n, self.dim - 1))
        return np.cumsum(x, axis=1)


class Hierarchical(_Twin):
    source = HIERARCHICAL_SRC

    def __init__(self, dim):
        super().__init__(np.zeros(dim), np.ones(dim))

    def terms(self, th):
        t = np.empty_like(th)
        t0 = th[:, :1]
        t[:, 0] = -0.5 * t0[:, 0] * t0[:, 0] - HALF_LOG_2PI
        t[:, 1:] = -0.5 * (th[:, 1:] * th[:, 1:]) * np.exp(-2.0 * t0) - t0 - HALF_LOG_2PI
        return t

    def _grad(self, th):
        w = np.exp(-2.0 * th[:, :1])
        g = -th * w
        g[:, 0] = -th[:, 0] + ((th[:, 1:] * th[:, 1:]) * w - 1.0).sum(axis=1)
        return g

    def _rvs(self, n, rng):
        x = rng.standard_normal((n, self.dim))
        x[:, 1:] *= np.exp(x[:, :1])
        return x


class Ordered(_Twin):
    """every component in its box [p_j, p_j + q_j] and theta_0 < theta_1 < ...; nan_above as in ordered_source"""

    def __init__(self, p, q, nan_above=None):
        super().__init__(p, q)
        self.nan_above = nan_above
        self.source = ordered_source(nan_above)

    def inside(self, theta):
        th = np.atleast_2d(theta)
        ok = np.all((th >= self.p) & (th <= self.p + self.q), axis=1)
        return ok & np.all(th[:, :-1] < th[:, 1:], axis=1)

    def ordered(self, theta):
        th = np.atleast_2d(theta)
        return np.all(th[:, :-1] < th[:, 1:], axis=1)

    def terms(self, th):
        t = np.broadcast_to(-np.log(self.q), th.shape).copy()
        t[~self.inside(th), 0] = -np.inf
        if self.nan_above is not None:
            t[th[:, 0] > self.nan_above, 0] = np.nan
        return t

    def _grad(self, th):
        return np.zeros_like(th)

    def _rvs(self, n, rng):
        """(exact when all components share one box: the order statistics of independent uniform draws)"""
        return np.sort(self.p + self.q * rng.random((n, self.dim)), axis=1)


# ---- the problems of the tests ---------------------------------------------------------------------------------------------------
def cauchy_difference(d):
    """the settings the oracle's acceptance rates were checked with: q_0 = 0.7, q_j = 0.05 (1 + 0.5 (j mod 3))"""
    q = 0.05 * (1.0 + 0.5 * (np.arange(d) % 3))
    q[0] = 0.7
    return CauchyDifference(0.1 * np.ones(d), q)


def total_variation(d):
    p = 8.0 * (1.0 + 0.25 * (np.arange(d) % 4))
    p[0] = 0.1
    return TotalVariation(p, 0.7 * np.ones(d))


def hierarchical(d):
    return Hierarchical(d)


def ordered(d, nan_above=None):
    return Ordered(-0.1 * np.ones(d), 1.25 * np.ones(d), nan_above)


def starts(prior, n, rng, spread=0.01):
    """n starting points around a smooth profile with small steps between neighbours (inside the ordered prior's support)"""
    d = prior.dim
    base = (np.arange(d) + 1.0) / (d + 1.0) if isinstance(prior, Ordered) else 0.1 + 0.3 * np.sin(np.arange(d) / 7.0)
    if isinstance(prior, Hierarchical):
        base[0] = -1.0
    if isinstance(prior, Ordered):
        spread = min(spread, 0.1 / (d + 1.0))
    return base, base[None, :] + spread * rng.standard_normal((n, d))


def problem(prior, m, n, seed, spread=0.01, noise=1.0):
    """data from extmodel's forward model at the profile plus noise (`noise` times the modelled standard deviation), n starts
    around it -> y, theta0"""
    rng = np.random.default_rng(seed)
    truth, theta0 = starts(prior, n, rng, spread)
    y = xm.np_forward(truth, m)[0] + noise * np.sqrt(SIGMA2) * rng.standard_normal(m)
    return y, theta0


def level_of(prior, m, y, shift=0.0, coup=0.5, noise=("iso", SIGMA2)):
    """the oracle takes the twin as a level's prior as it is"""
    return orc.CallableGaussianLevel(lambda th: xm.np_forward(th, m, shift=shift, coup=coup), y, noise[0], noise[1], prior)


def grad_level_of(prior, m, y):
    """... with MALA's gradient: the twin's plus the model's vector-Jacobian product (extpriorgrad.gaussian_grad_level)"""
    level = level_of(prior, m, y)
    level.grad_logpost = lambda theta, F: prior.grad(theta) + xm.np_vjp(theta, level.loglike.grad(F))
    return level


def make_engine(prior, N, levels, prop, bs=0, seed=93, chain_offset=5, subchains=None, source=None):
    """levels: [(model (+ likelihood) source, data, noise kind, noise)]; the prior is set first, so every level compiles once"""
    from tinyda_amd.engine import Engine

    e = Engine(N, prior.dim, seed=seed, chain_offset=chain_offset, block_steps=bs, n_levels=len(levels))
    e.set_prior_joint(np.full(prior.dim, PRIOR_SOURCE), prior.p, prior.q)
    for k, (src, y, kind, noise) in enumerate(levels):
        e.set_level_source(k, src + "\n" + (prior.source if source is None else source), y, kind, noise)
    set_proposal(e, prop)
    if subchains is not None:
        e.set_subchains(subchains, False)
    return e


def device_prior(prior, reference=True, source=None):
    import tinyda_amd as tda

    return tda.DevicePrior(prior.source if source is None else source, prior.dim, prior.p, prior.q, reference=prior if reference else None,
                           reference_gradient=prior.grad if reference else None)


# ---- separable terms written in the wave form: the same operations in the same order as the route through tda_logprior_term ----
def wave_of_term(term_src):
    """a tda_logprior_term source -> the wave form that sums term(theta_j, p_j, q_j, j) over j = lane, lane + 64 exactly as
    tda_user_steps sums the separable form (the term is renamed so that the source defines one form only)"""
    assert term_src.count("tda_logprior_term(") == 1
    return term_src.replace("tda_logprior_term(", "wave_term(") + r"""
__device__ double tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane) {
  double pj = lane < dim ? wave_term(theta[lane], p[lane], q[lane], lane) : 0.0;
  if (lane + 64 < dim) pj += wave_term(theta[lane + 64], p[lane + 64], q[lane + 64], lane + 64);
  return pj;
}
"""
