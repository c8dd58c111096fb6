"""Throughput of MALA over a source-defined model (tda_user_mala_steps) against GaussianRandomWalk (tda_user_steps) on the
same model: 4096 chains, m = 256 outputs, d = 32 and 96.  The model is F_o(theta) = sum_j w_oj g(theta_j) with
g(t) = t + 0.1 t^3, so one forward pass costs m d terms per chain and its vector-Jacobian product
(J^T s)_j = g'(theta_j) sum_o w_oj s_o another m d.  Prints one JSON line per (d, proposal) with evals/s (chain-steps per
second) and the MALA / GRW ratio.

    python tools/mala_source_rate.py [steps]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinyda_amd.engine import Engine  # noqa: E402

SRC = r"""
__device__ __forceinline__ double w_oj(int o, int j) { return 0.05 + 0.01 * ((o * 7 + j * 3) % 11); }
__device__ double tda_forward(const double* theta, int dim, int o) {
  double s = 0.0;
  for (int j = 0; j < dim; ++j) {
    const double t = theta[j];
    s += w_oj(o, j) * (t + 0.1 * t * t * t);
  }
  return s;
}
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int m, int j) {
  double s = 0.0;
  for (int o = 0; o < m; ++o) s += w_oj(o, j) * sens[o];
  const double t = theta[j];
  return (1.0 + 0.3 * t * t) * s;
}
"""


def np_forward(theta, m):
    d = theta.shape[-1]
    W = 0.05 + 0.01 * ((np.arange(m)[:, None] * 7 + np.arange(d)[None, :] * 3) % 11)
    return (theta + 0.1 * theta ** 3) @ W.T


def rate(kind, d, m=256, N=4096, T=200, warm=40):
    rng = np.random.default_rng(d)
    truth = 0.3 * rng.standard_normal(d)
    y = np_forward(truth, m) + 0.05 * rng.standard_normal(m)
    e = Engine(N, d, seed=1)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, SRC, y, 0, [0.05 ** 2])
    if kind == "mala":
        e.set_proposal(6, None, scaling=0.01, adaptive=True, period=100)
    else:
        e.set_proposal(0, np.eye(d), scaling=0.005, adaptive=True, period=100)
    t0 = time.perf_counter()
    e.init(truth + 0.01 * rng.standard_normal((N, d)))
    e.sync()
    t_init = time.perf_counter() - t0
    e.run(warm)
    e.sync()
    t0 = time.perf_counter()
    e.run(T)
    e.sync()
    dt = time.perf_counter() - t0
    e.close()
    return dict(proposal=kind, chains=N, d=d, m=m, steps=T, seconds=round(dt, 4), evals_per_s=N * T / dt, ms_per_step=1e3 * dt / T,
                init_s=round(t_init, 3))


if __name__ == "__main__":
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    for d in (32, 96):
        grw, mala = rate("grw", d, T=T), rate("mala", d, T=T)
        print(json.dumps(grw))
        print(json.dumps(dict(mala, mala_over_grw=mala["evals_per_s"] / grw["evals_per_s"])))
