"""The non-linear forward model that the external-model tests share: one HIP source template for DeviceModel /
set_level_source (with `tda_gradient`, so MALA runs over it), its NumPy twin (which is also the batched host callback), the
twin's vector-Jacobian product and Jacobian, and the oracle level that MALA needs.

    F_o(theta) = sin(sum_j w_oj theta_j) + COUP theta_{o % d} theta_{(o + 1) % d},  w_oj = 0.1 + 0.01 ((7 o + 3 j) % 11) + SHIFT

Every output reads every parameter (a dropped second lane shows), outputs differ with o (a wrong output index or stride
shows), and the model is bounded on bounded parameters.  SHIFT and COUP give the fidelities of a hierarchy; above
theta_0 > NAN_ABOVE every output is NaN.  d and m arrive at run time, so one source serves every shape."""
import numpy as np

from oracle import tinyda_oracle as orc

SRC_TEMPLATE = r"""
__device__ __forceinline__ double w_oj(int o, int j) { return 0.1 + 0.01 * ((o * 7 + j * 3) % 11) + SHIFT; }
__device__ double tda_forward(const double* theta, int dim, int o) {
  if (theta[0] > NAN_ABOVE) return __builtin_nan("");
  double s = 0.0;
  for (int j = 0; j < dim; ++j) s += w_oj(o, j) * theta[j];
  return sin(s) + COUP * (theta[o % dim] * theta[(o + 1) % dim]);
}
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int m, int j) {
  double g = 0.0;
  for (int o = 0; o < m; ++o) {
    double s = 0.0;
    for (int k = 0; k < dim; ++k) s += w_oj(o, k) * theta[k];
    double dF = cos(s) * w_oj(o, j);
    if (o % dim == j) dF += COUP * theta[(o + 1) % dim];
    if ((o + 1) % dim == j) dF += COUP * theta[o % dim];
    g += sens[o] * dF;
  }
  return g;
}
"""


def source(nan_above=None, shift=0.0, coup=0.5):
    """the template with its constants written as exact literals (repr round-trips a double)"""
    return (SRC_TEMPLATE.replace("NAN_ABOVE", "1e300" if nan_above is None else repr(float(nan_above)))
            .replace("SHIFT", repr(float(shift))).replace("COUP", repr(float(coup))))


def weights(m, d, shift=0.0):
    return 0.1 + 0.01 * ((np.arange(m)[:, None] * 7 + np.arange(d)[None, :] * 3) % 11) + shift


def np_forward(theta, m, nan_above=None, shift=0.0, coup=0.5):
    theta = np.atleast_2d(theta)
    d = theta.shape[1]
    o = np.arange(m)
    F = np.sin(theta @ weights(m, d, shift).T) + coup * (theta[:, o % d] * theta[:, (o + 1) % d])
    if nan_above is not None:
        F[theta[:, 0] > nan_above] = np.nan
    return F


def np_vjp(theta, sens, shift=0.0, coup=0.5):
    """J(theta)^T sens per row; the coupling terms are added output by output, in the order of the source's loop"""
    theta, sens = np.atleast_2d(theta), np.atleast_2d(sens)
    d, m = theta.shape[1], sens.shape[1]
    W = weights(m, d, shift)
    g = (sens * np.cos(theta @ W.T)) @ W
    o = np.arange(m)
    idx = np.stack([o % d, (o + 1) % d], axis=1).ravel()
    val = np.stack([coup * sens * theta[:, (o + 1) % d], coup * sens * theta[:, o % d]], axis=2).reshape(len(theta), 2 * m)
    for n in range(len(theta)):
        np.add.at(g[n], idx, val[n])
    return g


def np_jacobian(theta, m, shift=0.0, coup=0.5):
    """J(theta) [m, d] at one point"""
    theta = np.asarray(theta, dtype=float)
    d = theta.shape[0]
    W = weights(m, d, shift)
    J = np.cos(W @ theta)[:, None] * W
    o = np.arange(m)
    np.add.at(J, (o, o % d), coup * theta[(o + 1) % d])
    np.add.at(J, (o, (o + 1) % d), coup * theta[o % d])
    return J


class GradLevel(orc.CallableGaussianLevel):
    """CallableGaussianLevel with MALA's gradient (proposal.py:996-998): grad log prior + J^T grad loglike."""

    def __init__(self, fn, data, noise_kind, noise, prior, shift=0.0, coup=0.5):
        super().__init__(fn, data, noise_kind, noise, prior)
        self.shift, self.coup = shift, coup

    def grad_logpost(self, theta, F):
        g_prior = (self.prior.mean[None, :] - theta) @ np.linalg.inv(self.prior.cov).T
        return g_prior + np_vjp(theta, self.loglike.grad(F), self.shift, self.coup)
