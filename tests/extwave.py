"""The wave-cooperative forward model that the tda_forward_wave tests share: one HIP source template and its NumPy twin.

A reaction-diffusion equation on a ring of 64 nodes, explicit Euler, KSTEPS = 48 steps of h = 0.1 (lane = node):

    k_i = 0.05 exp(0.3 theta[i % d]),   r_i = 0.4 + 0.1 theta[(i + 64) % d],   u_i^0 = 0.25 + 0.5 ((37 i) % 64) / 64
    u_i <- u_i + h (k_i ((u_{i-1} - u_i) + (u_{i+1} - u_i)) + r_i (u_i (1 - u_i)))

After every KSTEPS / 12 steps read-out q = 0 .. 11 records ns = ceil(m / 12) sensors: output o = q ns + s is node
(5 s + 3 q) & 63, for o < m.  One solve gives all m outputs, which is what tda_forward_wave is for; the per-output form
(`forward="per_output"`) repeats the solve for every output inside one lane, with the same elementwise arithmetic in the same
order, so the two forms are bit-identical.  Every parameter up to d = 128 moves some output (64 .. 127 through r alone: a
dropped second lane shows), outputs up to m = 768 differ from one another, and the dynamics are dissipative: the last-bit
difference between the device's exp and libm's does not grow.  KSTEPS = 12 / 24 / 48 with h = 0.4 / 0.2 / 0.1 (the same final
time) are the fidelities of a hierarchy.

The vector-Jacobian product is the discrete adjoint over the stored trajectory (KSTEPS x 64 doubles in the workspace, left
there by tda_forward_wave at the same parameters):

    lambda_i <- lambda_i (1 + h (-2 k_i + r_i (1 - 2 u_i))) + h (k_{i-1} lambda_{i-1} + k_{i+1} lambda_{i+1})
    g_k,i += lambda_i h ((u_{i-1} - u_i) + (u_{i+1} - u_i)),   g_r,i += lambda_i h u_i (1 - u_i)

scattered to theta with d k_i / d theta = 0.015 exp(0.3 theta) and d r_i / d theta = 0.1."""
import numpy as np

from oracle import tinyda_oracle as orc

NODES = 64
STEP = {12: 0.4, 24: 0.2, 48: 0.1}  # KSTEPS -> h

# what every form shares: the coefficients, the step, the sensors of a read-out
COMMON = r"""
#define WV_K KSTEPS
#define WV_RO (WV_K / 12)
#define WV_H HSTEP
__device__ __forceinline__ double wv_k(const double* theta, int dim, int i) { return 0.05 * exp(0.3 * theta[i % dim]); }
__device__ __forceinline__ double wv_r(const double* theta, int dim, int i) { return 0.4 + 0.1 * theta[(i + 64) % dim]; }
__device__ __forceinline__ double wv_u0(int i) { return 0.25 + 0.5 * ((37 * i) % 64) / 64.0; }
__device__ __forceinline__ double wv_step(double u, double ul, double ur, double k, double r) {
  return u + WV_H * (k * ((ul - u) + (ur - u)) + r * (u * (1.0 - u)));
}
"""

# all outputs from one solve by the wave: the trajectory goes to WV_ROWS[t * 64 + node] (the state before step t), which is also
# how a lane reads its neighbours.  WV_ROWS is the workspace, except beside the per-parameter gradient, which is not handed the
# workspace: there the trajectory is a __shared__ array of the source's own (and the source asks for no workspace).
ROWS_IN_WORKSPACE = r"""
#define TDA_WORKSPACE (WV_K * 64)
#define WV_ROWS work
"""
ROWS_IN_SOURCE = r"""
__shared__ double wv_trajectory[WV_K * 64];
#define WV_ROWS wv_trajectory
"""
WAVE_FORWARD = r"""
__device__ __forceinline__ void wv_solve(const double* theta, int dim, double* out, int n_outputs, double* work, int lane) {
  const int il = (lane + 63) & 63, ir = (lane + 1) & 63, ns = (n_outputs + 11) / 12;
  const double k = wv_k(theta, dim, lane), r = wv_r(theta, dim, lane);
  double u = wv_u0(lane);
  for (int t = 0; t < WV_K; ++t) {
    double* row = WV_ROWS + t * 64;
    row[lane] = u;
    __syncthreads();
    u = wv_step(u, row[il], row[ir], k, r);
    if ((t + 1) % WV_RO == 0) {
      const int q = (t + 1) / WV_RO - 1;
      for (int s = (13 * (lane - 3 * q)) & 63; s < ns; s += 64) {  // the sensors of this read-out that sit on this node: 5 s + 3 q = lane (mod 64)
        const int o = q * ns + s;
        if (o < n_outputs - SKIP_LAST) out[o] = u;
      }
    }
  }
}
__device__ void tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane) {
  if (theta[0] > NAN_ABOVE) return;  // (the same for every lane; the outputs stay NaN)
  wv_solve(theta, dim, out, n_outputs, work, lane);
}
"""

# the only way to write this model without the wave form: every call repeats the solve up to its read-out, alone in its lane
# (state and coefficients in arrays of the lane's own, which is scratch memory)
PER_OUTPUT_FORWARD = r"""
__device__ double tda_forward(const double* theta, int dim, int o) {
  if (theta[0] > NAN_ABOVE) return __builtin_nan("");
  const int ns = (N_OUTPUTS + 11) / 12, q = o / ns, node = (5 * (o % ns) + 3 * q) & 63;
  double u[64], v[64], k[64], r[64];  // (the coefficients once per call, as the wave form has them once per lane)
  for (int i = 0; i < 64; ++i) {
    u[i] = wv_u0(i);
    k[i] = wv_k(theta, dim, i);
    r[i] = wv_r(theta, dim, i);
  }
  for (int t = 0; t < (q + 1) * WV_RO; ++t) {
    for (int i = 0; i < 64; ++i) v[i] = wv_step(u[i], u[(i + 63) & 63], u[(i + 1) & 63], k[i], r[i]);
    for (int i = 0; i < 64; ++i) u[i] = v[i];
  }
  return u[node];
}
"""

# the adjoint by the wave, backwards over the trajectory in `work`; the neighbours' k lambda come through the wave's shuffles.
# The contributions of the nodes are added per parameter in node order, k before r (np_vjp does the same).
WAVE_GRADIENT = r"""
#ifndef TDA_WORKSPACE
#define TDA_WORKSPACE (WV_K * 64)
#endif
__device__ void tda_gradient_wave(const double* theta, int dim, const double* sens, int n_outputs, double* grad, double* work, int lane) {
  const int il = (lane + 63) & 63, ir = (lane + 1) & 63, ns = (n_outputs + 11) / 12;
  const double k = wv_k(theta, dim, lane), r = wv_r(theta, dim, lane);
#if RECOMPUTE
  {  // per-output forward: nobody left a trajectory
    double u = wv_u0(lane);
    for (int t = 0; t < WV_K; ++t) {
      work[t * 64 + lane] = u;
      __syncthreads();
      u = wv_step(u, work[t * 64 + il], work[t * 64 + ir], k, r);
    }
  }
#endif
  double lam = 0.0, gk = 0.0, gr = 0.0;
  for (int t = WV_K - 1; t >= 0; --t) {
    if ((t + 1) % WV_RO == 0) {
      const int q = (t + 1) / WV_RO - 1;
      for (int s = (13 * (lane - 3 * q)) & 63; s < ns; s += 64)
        if (q * ns + s < n_outputs) lam += sens[q * ns + s];
    }
    const double* row = work + t * 64;
    const double u = row[lane], ul = row[il], ur = row[ir];
    gk += lam * (WV_H * ((ul - u) + (ur - u)));
    gr += lam * (WV_H * (u * (1.0 - u)));
    const double kl = k * lam;
    lam = lam * (1.0 + WV_H * (-2.0 * k + r * (1.0 - 2.0 * u))) + WV_H * (__shfl(kl, il) + __shfl(kl, ir));
  }
  __syncthreads();  // (the trajectory has been read: its first two rows carry the nodes' contributions)
  work[lane] = gk * (0.015 * exp(0.3 * theta[lane % dim]));
  work[64 + lane] = gr * 0.1;
  __syncthreads();
  for (int j = lane; j < dim; j += 64) {
    double g = 0.0;
    for (int i = 0; i < 64; ++i)
      if (i % dim == j) g += work[i];
    for (int i = 0; i < 64; ++i)
      if ((i + 64) % dim == j) g += work[64 + i];
    grad[j] = g;
  }
}
"""

# one parameter per call, alone in its lane: the tangent of the solve along theta_j, updated in place from the saved old values
# of a node's neighbours.  Beside the per-output forward the lane solves the ring itself, state and tangent in arrays of its own
# (scratch memory).  Beside the wave forward it reads the trajectory that tda_forward_wave left at the same parameters and keeps the
# tangent in a column of LDS per lane (32 KiB + the trajectory's 24 KiB), so it needs no array of its own and no scratch memory.
PER_PARAMETER_GRADIENT = r"""
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int n_outputs, int j) {
  const int ns = (n_outputs + 11) / 12;
  double u[64], w[64];  // the state and its derivative by theta_j
  for (int i = 0; i < 64; ++i) {
    u[i] = wv_u0(i);
    w[i] = 0.0;
  }
  double g = 0.0;
  for (int t = 0; t < WV_K; ++t) {
    const double u0 = u[0], w0 = w[0];
    double up = u[63], wp = w[63];  // the old values of node i - 1
    for (int i = 0; i < 64; ++i) {
      const double ui = u[i], wi = w[i], un = i < 63 ? u[i + 1] : u0, wn = i < 63 ? w[i + 1] : w0;
      const double k = wv_k(theta, dim, i), r = wv_r(theta, dim, i);
      const double dk = i % dim == j ? 0.3 * k : 0.0, dr = (i + 64) % dim == j ? 0.1 : 0.0;
      u[i] = wv_step(ui, up, un, k, r);
      w[i] = wi + WV_H * (dk * ((up - ui) + (un - ui)) + k * ((wp - wi) + (wn - wi)) + dr * (ui * (1.0 - ui)) + r * ((1.0 - 2.0 * ui) * wi));
      up = ui;
      wp = wi;
    }
    if ((t + 1) % WV_RO == 0) {
      const int q = (t + 1) / WV_RO - 1;
      for (int s = 0; s < ns && q * ns + s < n_outputs; ++s) g += sens[q * ns + s] * w[(5 * s + 3 * q) & 63];
    }
  }
  return g;
}
"""
PER_PARAMETER_GRADIENT_OVER_TRAJECTORY = r"""
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int n_outputs, int j) {
  __shared__ double wv_tangent[64 * 64];
  double* w = wv_tangent + (threadIdx.x & 63);  // w[64 * i]: the derivative of node i by theta_j, this lane's column
  const int ns = (n_outputs + 11) / 12;
  for (int i = 0; i < 64; ++i) w[64 * i] = 0.0;
  double g = 0.0;
  for (int t = 0; t < WV_K; ++t) {
    const double* u = wv_trajectory + t * 64;  // the state before step t
    const double w0 = w[0];
    double wp = w[64 * 63];  // the old value of node i - 1
    for (int i = 0; i < 64; ++i) {
      const double ui = u[i], up = u[(i + 63) & 63], un = u[(i + 1) & 63], wi = w[64 * i], wn = i < 63 ? w[64 * (i + 1)] : w0;
      const double k = wv_k(theta, dim, i), r = wv_r(theta, dim, i);
      const double dk = i % dim == j ? 0.3 * k : 0.0, dr = (i + 64) % dim == j ? 0.1 : 0.0;
      w[64 * i] = wi + WV_H * (dk * ((up - ui) + (un - ui)) + k * ((wp - wi) + (wn - wi)) + dr * (ui * (1.0 - ui)) + r * ((1.0 - 2.0 * ui) * wi));
      wp = wi;
    }
    if ((t + 1) % WV_RO == 0) {
      const int q = (t + 1) / WV_RO - 1;
      for (int s = 0; s < ns && q * ns + s < n_outputs; ++s) g += sens[q * ns + s] * w[64 * ((5 * s + 3 * q) & 63)];
    }
  }
  return g;
}
"""

FORWARDS = {"wave": WAVE_FORWARD, "per_output": PER_OUTPUT_FORWARD, "both": PER_OUTPUT_FORWARD + WAVE_FORWARD}
GRADIENTS = {None: "", "wave": WAVE_GRADIENT, "per_parameter": PER_PARAMETER_GRADIENT}


def source(forward="wave", gradient=None, m=None, ksteps=48, nan_above=None, skip_last=False):
    """the model as HIP source: `forward` in FORWARDS, `gradient` in GRADIENTS; the per-output form needs the number of
    outputs written in (tda_forward is not told it).  Constants are exact literals."""
    assert ksteps in STEP and (forward == "wave" or m is not None)
    over_trajectory = forward != "per_output" and gradient == "per_parameter"
    src = COMMON + ("" if forward == "per_output" else ROWS_IN_SOURCE if over_trajectory else ROWS_IN_WORKSPACE) + FORWARDS[forward]
    src += PER_PARAMETER_GRADIENT_OVER_TRAJECTORY if over_trajectory else GRADIENTS[gradient]
    return (src.replace("KSTEPS", str(int(ksteps))).replace("HSTEP", repr(STEP[ksteps])).replace("N_OUTPUTS", str(m)).replace("SKIP_LAST", "1" if skip_last else "0")
            .replace("NAN_ABOVE", "1e300" if nan_above is None else repr(float(nan_above)))
            .replace("RECOMPUTE", "0" if forward in ("wave", "both") else "1"))


def _coefficients(theta):
    d = theta.shape[1]
    i = np.arange(NODES)
    return 0.05 * np.exp(0.3 * theta[:, i % d]), 0.4 + 0.1 * theta[:, (i + 64) % d]


def _sensors(m, q):
    """outputs and nodes of read-out q"""
    ns = (m + 11) // 12
    s = np.arange(ns)
    o = q * ns + s
    return o[o < m], ((5 * s + 3 * q) & 63)[o < m]


def _step(u, k, r, h):
    ul, ur = np.roll(u, 1, axis=1), np.roll(u, -1, axis=1)
    return u + h * (k * ((ul - u) + (ur - u)) + r * (u * (1.0 - u)))


def np_forward(theta, m, ksteps=48, nan_above=None, skip_last=False, trajectory=False):
    """F(theta) per row, [N, m]; the elementwise operations are the source's, in its order"""
    theta = np.atleast_2d(np.asarray(theta, dtype=float))
    k, r = _coefficients(theta)
    ro = ksteps // 12
    u = np.tile(0.25 + 0.5 * ((37 * np.arange(NODES)) % 64) / 64.0, (len(theta), 1))
    F = np.full((len(theta), m), np.nan)
    traj = []
    for t in range(ksteps):
        traj.append(u)
        u = _step(u, k, r, STEP[ksteps])
        if (t + 1) % ro == 0:
            o, node = _sensors(m, (t + 1) // ro - 1)
            F[:, o] = u[:, node]
    if skip_last:
        F[:, m - 1] = np.nan
    if nan_above is not None:
        F[theta[:, 0] > nan_above] = np.nan
    return (F, traj) if trajectory else F


def np_vjp(theta, sens, ksteps=48):
    """J(theta)^T sens per row: the discrete adjoint of the source's tda_gradient_wave.  A parameter collects the contributions
    of its nodes one by one in node order, those through k before those through r, as the source's loop adds them."""
    theta, sens = np.atleast_2d(np.asarray(theta, dtype=float)), np.atleast_2d(np.asarray(sens, dtype=float))
    N, d = theta.shape
    m = sens.shape[1]
    k, r = _coefficients(theta)
    ro, h = ksteps // 12, STEP[ksteps]
    _, traj = np_forward(theta, m, ksteps, trajectory=True)
    lam, gk, gr = np.zeros((N, NODES)), np.zeros((N, NODES)), np.zeros((N, NODES))
    for t in range(ksteps - 1, -1, -1):
        if (t + 1) % ro == 0:
            o, node = _sensors(m, (t + 1) // ro - 1)
            for oo, nn in zip(o, node):  # (a node may carry several sensors of one read-out once ns > 64: in sensor order)
                lam[:, nn] += sens[:, oo]
        u = traj[t]
        ul, ur = np.roll(u, 1, axis=1), np.roll(u, -1, axis=1)
        gk += lam * (h * ((ul - u) + (ur - u)))
        gr += lam * (h * (u * (1.0 - u)))
        kl = k * lam
        lam = lam * (1.0 + h * (-2.0 * k + r * (1.0 - 2.0 * u))) + h * (np.roll(kl, 1, axis=1) + np.roll(kl, -1, axis=1))
    i = np.arange(NODES)
    ck, cr = gk * (0.015 * np.exp(0.3 * theta[:, i % d])), gr * 0.1
    g = np.zeros((N, d))
    for n in range(N):
        np.add.at(g[n], i % d, ck[n])
        np.add.at(g[n], (i + 64) % d, cr[n])
    return g


def problem(d, m, n_chains, seed, ksteps=48, sigma=0.01):
    """truth, data (isotropic noise sigma) and starts at truth + 0.01 N(0, I): the setting the golden generator and the tests share"""
    rng = np.random.default_rng(seed)
    truth = 0.5 * rng.standard_normal(d)
    y = np_forward(truth, m, ksteps)[0] + sigma * rng.standard_normal(m)
    theta0 = truth + 0.01 * rng.standard_normal((n_chains, d))
    return truth, y, theta0


class GradLevel(orc.CallableGaussianLevel):
    """CallableGaussianLevel with MALA's gradient (proposal.py:996-998): grad log prior + J^T grad loglike."""

    def __init__(self, fn, data, noise_kind, noise, prior, ksteps=48):
        super().__init__(fn, data, noise_kind, noise, prior)
        self.ksteps = ksteps

    def grad_logpost(self, theta, F):
        g_prior = (self.prior.mean[None, :] - theta) @ np.linalg.inv(self.prior.cov).T
        return g_prior + np_vjp(theta, self.loglike.grad(F), self.ksteps)
