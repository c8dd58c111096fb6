"""What the tests of likelihoods that couple outputs share (tda_loglike_wave / tda_loglike_grad_wave): five such likelihoods, each
as HIP source with both functions and as a NumPy twin (log L per row and d log L / d F), the oracle level over a batched model
under such a likelihood, and the problems (data, scales, starts) the tests run.

  ar1        r = (F - y) / p, rho = 0.6:  log L = -1/2 [(1 - rho^2) r_0^2 + sum_{o >= 1} (r_o - rho r_{o-1})^2]
  marginal   the noise level integrated out, a = 2, b = 1.5:  log L = -(a + m / 2) log(b + 1/2 sum_o r_o^2); the wave reduces
             the sum with __shfl_xor and lane 0 returns the value
  softmax    counts y:  log L = sum_o y_o (F_o - logsumexp F); a max reduction, then a sum reduction
  monotone   ar1 with -inf wherever F_o < F_{o-1}, and NaN where F_0 > NAN_F
  t_wave     the separable Student-t of extloglike written in the wave form: the same operations in the same order as the
             route through tda_loglike_term

Each source spreads its outputs over the lanes by `for (o = lane; o < n_outputs; o += 64)`."""
import numpy as np

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from . import extmodel as xm
from .extengine import NOISE_SOURCE, set_proposal

RHO = 0.6
MARG_A, MARG_B = 2.0, 1.5
WAVE_SIG = "__device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane)"
GRAD_SIG = "__device__ void tda_loglike_grad_wave(const double* f, int n_outputs, const double* y, const double* p, double* sens, int lane)"

AR1_SRC = r"""
__device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane) {
  double s = 0.0;
  for (int o = lane; o < n_outputs; o += 64) {
    const double r = (f[o] - y[o]) / p[o];
    if (o == 0) {
      s += -0.5 * ((1.0 - 0.6 * 0.6) * (r * r));
    } else {
      const double e = r - 0.6 * ((f[o - 1] - y[o - 1]) / p[o - 1]);
      s += -0.5 * (e * e);
    }
  }
  return s;
}
__device__ void tda_loglike_grad_wave(const double* f, int n_outputs, const double* y, const double* p, double* sens, int lane) {
  for (int o = lane; o < n_outputs; o += 64) {
    const double r = (f[o] - y[o]) / p[o];
    double g;
    if (o == 0) {
      g = -((1.0 - 0.6 * 0.6) * r);
    } else {
      g = -(r - 0.6 * ((f[o - 1] - y[o - 1]) / p[o - 1]));
    }
    if (o + 1 < n_outputs) g += 0.6 * ((f[o + 1] - y[o + 1]) / p[o + 1] - 0.6 * r);
    sens[o] = g / p[o];
  }
}
"""

MARGINAL_SRC = r"""
__device__ __forceinline__ double marg_sum(const double* f, int n_outputs, const double* y, const double* p, int lane) {
  double s = 0.0;
  for (int o = lane; o < n_outputs; o += 64) {
    const double r = (f[o] - y[o]) / p[o];
    s += r * r;
  }
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);  // every lane holds the sum
  return s;
}
__device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane) {
  const double s = marg_sum(f, n_outputs, y, p, lane);
  return lane == 0 ? -(2.0 + 0.5 * n_outputs) * log(1.5 + 0.5 * s) : 0.0;
}
__device__ void tda_loglike_grad_wave(const double* f, int n_outputs, const double* y, const double* p, double* sens, int lane) {
  const double c = -(2.0 + 0.5 * n_outputs) / (1.5 + 0.5 * marg_sum(f, n_outputs, y, p, lane));
  for (int o = lane; o < n_outputs; o += 64) sens[o] = c * ((f[o] - y[o]) / p[o]) / p[o];
}
"""

SOFTMAX_SRC = r"""
__device__ __forceinline__ double sm_logsumexp(const double* f, int n_outputs, int lane) {
  double mx = -__builtin_inf();
  for (int o = lane; o < n_outputs; o += 64) mx = fmax(mx, f[o]);
  for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
  double s = 0.0;
  for (int o = lane; o < n_outputs; o += 64) s += exp(f[o] - mx);
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  return mx + log(s);
}
__device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane) {
  const double lse = sm_logsumexp(f, n_outputs, lane);
  double s = 0.0;
  for (int o = lane; o < n_outputs; o += 64) s += y[o] * (f[o] - lse);
  return s;
}
__device__ void tda_loglike_grad_wave(const double* f, int n_outputs, const double* y, const double* p, double* sens, int lane) {
  const double lse = sm_logsumexp(f, n_outputs, lane);
  double n = 0.0;
  for (int o = lane; o < n_outputs; o += 64) n += y[o];
  for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off);
  for (int o = lane; o < n_outputs; o += 64) sens[o] = y[o] - n * exp(f[o] - lse);
}
"""

# NAN_F: above it (in F_0) the share of the lane that holds output 0 is NaN, which must reject like a NaN output of the model
MONOTONE_TEMPLATE = r"""
__device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane) {
  double s = 0.0;
  if (lane == 0 && f[0] > NAN_F) return __builtin_nan("");
  for (int o = lane; o < n_outputs; o += 64) {
    const double r = (f[o] - y[o]) / p[o];
    if (o == 0) {
      s += -0.5 * ((1.0 - 0.6 * 0.6) * (r * r));
    } else {
      if (f[o] < f[o - 1]) return -__builtin_inf();
      const double e = r - 0.6 * ((f[o - 1] - y[o - 1]) / p[o - 1]);
      s += -0.5 * (e * e);
    }
  }
  return s;
}
""" + "__device__ void tda_loglike_grad_wave" + AR1_SRC.split("__device__ void tda_loglike_grad_wave")[1]  # (inside the order: ar1's gradient)


# parameters (d = 5) at which the first three outputs of extmodel's model are in order with gaps of 0.036 and 0.026, and a point
# next to them at which the third is 0.005 below the second
MONOTONE_TRUTH = np.array([-0.08621631, 0.47232248, -0.12983575, -0.22064499, 0.07493561])
MONOTONE_OUTSIDE = np.array([-0.08729667, 0.47549957, -0.02544268, -0.18899783, 0.09253961])


def monotone_source(nan_f=None):
    return MONOTONE_TEMPLATE.replace("NAN_F", "1e300" if nan_f is None else repr(float(nan_f)))


def wave_of_term(term_src):
    """a tda_loglike_term (+ tda_loglike_term_grad) source -> the wave form that sums term(F_o, y_o, p_o, o) over o = lane,
    lane + 64, ... from 0.0 exactly as the program sums the separable form (the functions are renamed so that the source defines
    one form only)"""
    assert term_src.count("tda_loglike_term(") == 1 and term_src.count("tda_loglike_term_grad(") == 1
    return term_src.replace("tda_loglike_term(", "wave_term(").replace("tda_loglike_term_grad(", "wave_term_grad(") + r"""
__device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane) {
  double sum = 0.0;
  for (int o = lane; o < n_outputs; o += 64) sum += wave_term(f[o], y[o], p[o], o);
  return sum;
}
__device__ void tda_loglike_grad_wave(const double* f, int n_outputs, const double* y, const double* p, double* sens, int lane) {
  for (int o = lane; o < n_outputs; o += 64) sens[o] = wave_term_grad(f[o], y[o], p[o], o);
}
"""


T_WAVE_SRC = wave_of_term(xl.STUDENT_T_SRC)


def without_grad(src):
    return src.split("__device__ void tda_loglike_grad_wave")[0]


# ---- the NumPy twins: loglike(F[N, m], y, p) -> [N], grad(F, y, p) -> d log L / d F [N, m] ------------------------------------------
def _rows(F):
    """F as [N, m] in double precision (long double is kept: the finite-difference test evaluates the twins in it)"""
    F = np.asarray(F)
    return np.atleast_2d(F if F.dtype == np.longdouble else F.astype(float))


def _residuals(F, y, p):
    return (_rows(F) - y) / p


def ar1_terms(F, y, p):
    r = _residuals(F, y, p)
    t = np.empty_like(r)
    t[:, 0] = -0.5 * ((1.0 - RHO * RHO) * (r[:, 0] * r[:, 0]))
    e = r[:, 1:] - RHO * r[:, :-1]
    t[:, 1:] = -0.5 * (e * e)
    return t


def ar1(F, y, p):
    return ar1_terms(F, y, p).sum(axis=1)


def ar1_grad(F, y, p):
    r = _residuals(F, y, p)
    g = np.empty_like(r)
    g[:, 0] = -((1.0 - RHO * RHO) * r[:, 0])
    e = r[:, 1:] - RHO * r[:, :-1]
    g[:, 1:] = -e
    g[:, :-1] += RHO * e
    return g / p


def marginal(F, y, p):
    r = _residuals(F, y, p)
    return -(MARG_A + 0.5 * r.shape[1]) * np.log(MARG_B + 0.5 * (r * r).sum(axis=1))


def marginal_grad(F, y, p):
    r = _residuals(F, y, p)
    c = -(MARG_A + 0.5 * r.shape[1]) / (MARG_B + 0.5 * (r * r).sum(axis=1))
    return c[:, None] * r / p


def _logsumexp(F):
    mx = F.max(axis=1, keepdims=True)
    return mx + np.log(np.exp(F - mx).sum(axis=1, keepdims=True))


def softmax(F, y, p):
    F = _rows(F)
    return (y * (F - _logsumexp(F))).sum(axis=1)


def softmax_grad(F, y, p):
    F = _rows(F)
    return y - y.sum() * np.exp(F - _logsumexp(F))


def monotone(nan_f=None):
    def loglike(F, y, p):
        F = _rows(F)
        ll = ar1(F, y, p)
        ll[np.any(F[:, 1:] < F[:, :-1], axis=1)] = -np.inf
        if nan_f is not None:
            ll[F[:, 0] > nan_f] = np.nan
        return ll

    return loglike


def t_wave(F, y, p):
    return xl.t_terms(_rows(F), y, p).sum(axis=1)


def t_wave_grad(F, y, p):
    return xl.t_terms_grad(_rows(F), y, p)


KINDS = {  # name -> (HIP source, log L, d log L / d F)
    "ar1": (AR1_SRC, ar1, ar1_grad),
    "marginal": (MARGINAL_SRC, marginal, marginal_grad),
    "softmax": (SOFTMAX_SRC, softmax, softmax_grad),
    "t_wave": (T_WAVE_SRC, t_wave, t_wave_grad),
}


class CoupledLevel:
    """What oracle.run_mh / run_multilevel ask of a level (evaluate, prior, grad_logpost) for a batched model
    theta[N, d] -> F[N, m] under a likelihood that couples outputs: log L = loglike(F, y, p)[N].  `vjp(theta, sens)` is the
    model's vector-Jacobian product (that of tests/extmodel.py unless given); the prior's gradient is its own `grad` where it
    has one (the twins of extpriorwave), else the Gaussian's."""

    def __init__(self, fn, data, par, loglike, prior, grad=None, shift=0.0, coup=0.5, vjp=None):
        self.fn, self.prior, self.loglike_fn, self.grad_fn = fn, prior, loglike, grad
        self.data, self.par = np.asarray(data, dtype=float), np.asarray(par, dtype=float)
        self.vjp = vjp if vjp is not None else (lambda theta, sens: xm.np_vjp(theta, sens, shift, coup))

    def forward(self, theta):
        return np.asarray(self.fn(theta), dtype=float)

    def evaluate(self, theta):
        F = self.forward(theta)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ll = np.asarray(self.loglike_fn(F, self.data, self.par), dtype=float)
        return self.prior.logpdf(theta), ll, F

    def grad_logpost(self, theta, F):
        if hasattr(self.prior, "grad"):
            g_prior = self.prior.grad(theta)
        else:
            g_prior = (self.prior.mean[None, :] - theta) @ np.linalg.inv(self.prior.cov).T
        return g_prior + self.vjp(theta, self.grad_fn(F, self.data, self.par))


# ---- the problems of the tests -------------------------------------------------------------------------------------------------------
def problem(d, m, kind, N, seed, fn=None, scale=0.1, truth=None):
    """truth 0.3 N(0, I) unless given, data from the model at the truth: AR(1) noise of scale p_o = scale (1 + 0.1 o / m) (ar1, marginal,
    t_wave, monotone), or multinomial counts of 40 m draws from the softmax of the outputs (softmax; p unused).  Starts at
    truth + 0.01 N(0, I); the Gaussian prior of test_gpu_loglike_source.problem.  -> y, p, theta0, prior mean, prior variances"""
    rng = np.random.default_rng(seed)
    truth = 0.3 * rng.standard_normal(d) if truth is None else truth
    F = (fn or (lambda th: xm.np_forward(th, m)))(truth[None, :])[0]
    par = scale * (1.0 + 0.1 * np.arange(m) / m)
    if kind == "softmax":
        pr = np.exp(F - F.max())
        y = rng.multinomial(40 * m, pr / pr.sum()).astype(float)
        par = np.ones(m)
    else:
        eps = rng.standard_normal(m)
        for o in range(1, m):
            eps[o] = RHO * eps[o - 1] + np.sqrt(1.0 - RHO * RHO) * eps[o]
        y = F + par * eps
    theta0 = truth + 0.01 * rng.standard_normal((N, d))
    return y, par, theta0, 0.1 * np.ones(d), 0.5 + 0.01 * np.arange(d)


def level_of(kind, m, y, par, pm, pv, shift=0.0, coup=0.5, loglike=None, prior=None):
    _, ll, g = KINDS[kind]
    return CoupledLevel(lambda th: xm.np_forward(th, m, shift=shift, coup=coup), y, par, loglike or ll,
                        prior if prior is not None else orc.MVNPrior(pm, np.diag(pv)), g, shift, coup)


def full_source(kind, shift=0.0, coup=0.5):
    return xm.source(shift=shift, coup=coup) + KINDS[kind][0]


def make_engine(d, N, src, y, par, pm, pv, prop, bs=0, seed=91, chain_offset=3):
    """a single level under the Gaussian prior N(pm, diag(pv)) with the likelihood of `src`"""
    from tinyda_amd.engine import Engine

    e = Engine(N, d, seed=seed, chain_offset=chain_offset, block_steps=bs)
    e.set_prior(pm, np.diag(pv))
    e.set_level_source(0, src, y, NOISE_SOURCE, par)
    set_proposal(e, prop)
    return e


def device_loglike(kind, y, par, reference=True, source=None):
    import tinyda_amd as tda

    src, ll, g = KINDS[kind]
    return tda.DeviceLogLike(src if source is None else source, y, par, reference=ll if reference else None,
                             reference_gradient=(lambda x, yy, pp: g(x, yy, pp)[0]) if reference else None)
