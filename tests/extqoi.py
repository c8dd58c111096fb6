"""The quantities of interest that the replay tests share: HIP sources to append to a model's source, and their NumPy twins.

PER_QUANTITY goes with any model: quantity k reads the parameter dim - 1 - k % dim and the output n_outputs - 1 - k % n_outputs,
so that with 65 .. 128 parameters and more than 64 outputs the first quantities read indices >= 64 of both (a dropped second
stride of either shows), and quantities differ with k (a wrong index or stride of the quantities shows).

RING_WAVE goes with the ring model of tests/extwave.py in its wave form: the sum and the maximum over the 64 nodes of the last
trajectory row that tda_forward_wave left in `work` (the state before the last step: np_forward(..., trajectory=True)[1][-1]),
by the wave's shuffles.  Quantity 2 is left unwritten on purpose and stays NaN: n_qoi = 3."""
import numpy as np

from . import extwave as xw

PER_QUANTITY = r"""
__device__ double tda_qoi(const double* theta, int dim, const double* f, int n_outputs, int k) {
  return theta[dim - 1 - k % dim] * f[n_outputs - 1 - k % n_outputs] + 0.125 * k;
}
"""

RING_WAVE = r"""
__device__ void tda_qoi_wave(const double* theta, int dim, const double* f, int n_outputs, double* qoi, int n_qoi, double* work, int lane) {
  const double u = work[(WV_K - 1) * 64 + lane];
  double s = u, mx = u;
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off);
    mx = fmax(mx, __shfl_xor(mx, off));
  }
  if (lane == 0) {
    qoi[0] = s;
    qoi[1] = mx;
  }
}
"""
RING_WAVE_N = 3


def np_per_quantity(theta, F, n_qoi):
    """the twin of PER_QUANTITY, [N, n_qoi]; one multiplication and one addition per entry, as the source has them"""
    theta, F = np.atleast_2d(theta), np.atleast_2d(F)
    d, m = theta.shape[1], F.shape[1]
    k = np.arange(n_qoi)
    return theta[:, d - 1 - k % d] * F[:, m - 1 - k % m] + 0.125 * k


def np_ring_wave(theta, m, ksteps=48):
    """the twin of RING_WAVE, [N, 3]: the sum in the butterfly's order (so that only the device's exp differs from libm's), the
    maximum, NaN"""
    theta = np.atleast_2d(np.asarray(theta, dtype=float))
    u = xw.np_forward(theta, m, ksteps, trajectory=True)[1][-1]
    s = u.copy()
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ off]
    return np.stack([s[:, 0], u.max(axis=1), np.full(len(theta), np.nan)], axis=1)
