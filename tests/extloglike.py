"""The source-defined likelihoods that the DeviceLogLike tests share, each written once in HIP and once in NumPy, and the
oracle level that sums their terms over the model of tests/extmodel.py.

    student-t (nu = 4, scale p_o):            term = -5/2 log1p(((f - y) / p)^2 / 4)
    poisson (log link, exposure p_o):         term = y f - p exp(f)          (the constant -log y! dropped)
    gauss (variance p_o):                     term = -1/2 (f - y)^2 / p      (the cross-check against TDA_NOISE_DIAG)

RESTRICTED_T is the student-t with holes: NaN above f > NAN_F, -inf below f < INF_F (a support), for the rejection test."""
import numpy as np

from .extmodel import np_vjp

STUDENT_T_SRC = r"""
__device__ double tda_loglike_term(double f, double y, double p, int o) {
  const double z = (f - y) / p;
  return -2.5 * log1p(0.25 * (z * z));
}
__device__ double tda_loglike_term_grad(double f, double y, double p, int o) {
  const double z = (f - y) / p;
  return -1.25 * z / ((1.0 + 0.25 * (z * z)) * p);
}
"""

POISSON_SRC = r"""
__device__ double tda_loglike_term(double f, double y, double p, int o) { return y * f - p * exp(f); }
__device__ double tda_loglike_term_grad(double f, double y, double p, int o) { return y - p * exp(f); }
"""

GAUSS_SRC = r"""
__device__ double tda_loglike_term(double f, double y, double p, int o) { return -0.5 * (f - y) * (f - y) / p; }
__device__ double tda_loglike_term_grad(double f, double y, double p, int o) { return (y - f) / p; }
"""

TERM_ONLY_SRC = r"""
// no derivative here: __device__ double tda_loglike_term_grad(double f, double y, double p, int o)
__device__ double tda_loglike_term(double f, double y, double p, int o) { return -fabs(f - y) / p; }  /* Laplace */
"""

RESTRICTED_T_TEMPLATE = r"""
__device__ double tda_loglike_term(double f, double y, double p, int o) {
  if (o == 0 && f > NAN_F) return __builtin_nan("");
  if (o == 1 && f < INF_F) return -__builtin_inf();
  const double z = (f - y) / p;
  return -2.5 * log1p(0.25 * (z * z));
}
"""


def restricted_t_source(nan_f, inf_f):
    return RESTRICTED_T_TEMPLATE.replace("NAN_F", repr(float(nan_f))).replace("INF_F", repr(float(inf_f)))


def t_terms(F, y, p):
    z = (F - y) / p
    return -2.5 * np.log1p(0.25 * (z * z))


def t_terms_grad(F, y, p):
    z = (F - y) / p
    return -1.25 * z / ((1.0 + 0.25 * (z * z)) * p)


def poisson_terms(F, y, p):
    return y * F - p * np.exp(F)


def poisson_terms_grad(F, y, p):
    return y - p * np.exp(F)


def gauss_terms(F, y, p):
    return -0.5 * (F - y) * (F - y) / p


def gauss_terms_grad(F, y, p):
    return (y - F) / p


def restricted_t_terms(nan_f, inf_f):
    def terms(F, y, p):
        F = np.atleast_2d(F)
        t = t_terms(F, y, p)
        t[:, 0] = np.where(F[:, 0] > nan_f, np.nan, t[:, 0])
        t[:, 1] = np.where(F[:, 1] < inf_f, -np.inf, t[:, 1])
        return t

    return terms


KINDS = {  # name -> (HIP source, terms, d terms / d f)
    "t": (STUDENT_T_SRC, t_terms, t_terms_grad),
    "poisson": (POISSON_SRC, poisson_terms, poisson_terms_grad),
    "gauss": (GAUSS_SRC, gauss_terms, gauss_terms_grad),
}


class LogLikeLevel:
    """What oracle.run_mh / run_multilevel ask of a level (evaluate, prior, grad_logpost) for a batched model
    theta[N, d] -> F[N, m] under a separable likelihood: log L = sum_o terms(F, y, p)[:, o]."""

    def __init__(self, fn, data, par, terms, prior, terms_grad=None, shift=0.0, coup=0.5):
        self.fn, self.prior, self.terms, self.terms_grad = fn, prior, terms, terms_grad
        self.data, self.par = np.asarray(data, dtype=float), np.asarray(par, dtype=float)
        self.shift, self.coup = shift, coup

    def forward(self, theta):
        return np.asarray(self.fn(theta), dtype=float)

    def evaluate(self, theta):
        F = self.forward(theta)
        with np.errstate(invalid="ignore", over="ignore"):
            ll = np.sum(self.terms(F, self.data, self.par), axis=1)
        return self.prior.logpdf(theta), ll, F

    def grad_logpost(self, theta, F):
        """grad log prior + J^T (d terms / d f), the model's VJP being that of tests/extmodel.py"""
        g_prior = (self.prior.mean[None, :] - theta) @ np.linalg.inv(self.prior.cov).T
        return g_prior + np_vjp(theta, self.terms_grad(F, self.data, self.par), self.shift, self.coup)
