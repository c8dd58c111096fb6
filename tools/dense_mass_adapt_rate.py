"""Warm-up adaptation of the dense mass (k_dense_mass_shift / accumulate / update, include/tinyda_amd_dense_mass_adaptation.h) on one
MI355X, on the ill-conditioned Gaussian of tools/nuts_rate.py: the posterior precision's eigenvalues log-spaced over 1 .. 100 in a
random orthogonal basis, NUTS (max_depth 8, adaptive step size, period 50), 4096 chains started from the posterior.

a. The cost of the three kernels, at d = 64 (m = 96) and d = 128 (m = 192).  An engine with a warm-up of 64 periods (windows
   [1, 2), [2, 4), [4, 8), [8, 16), [16, 32), [32, 64) in periods) is run to the start of period 14, and periods 14, 15, 16 and 17 are
   each one profiled run() of one block: the engine's own device events around every launch (tda_profile: the step kernel under
   `steps`, the adaptation's launches under `adapt`).  Period 14 and 17 hold k_dense_mass_accumulate alone, period 15 ends the
   window [8, 16) and holds the update as well, period 16 starts [16, 32) and holds the shift as well; the update's and the shift's
   times are the differences to the mean of 14 and 17.  The same periods of an engine that adapts the diagonal mass give
   k_mass_accumulate.  `repeats` engine pairs take turns; medians and spreads are reported.  (An event pair around one short kernel
   also holds the gap behind the launch: an upper bound on the kernel.)

b. What it buys (d = 64).  NUTS with adapt_mass = 800, adapt_dense = True from the unit mass, `burn` steps of burn-in, then `draws`
   recorded steps: the row of tools/dense_mass_rate.py (gradient evaluations per second, mean tree depth, step size, bulk ESS per
   gradient evaluation for the worst and the median parameter), and the eigenvalues of the learnt W whitened by the true covariance.

    python tools/dense_mass_adapt_rate.py [--repeats 3] [--burn 1000] [--draws 1000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinyda_amd import summaries  # noqa: E402
from tools.nuts_rate import make_engine, problem  # noqa: E402

PERIOD = 50


def _profiled_period(e):
    e.set_profiling(True)
    e.run(PERIOD)
    e.sync()
    p = e.profile()
    assert p["n_launch_steps"] == 1, p
    return p["ms_adapt"], p["ms_steps"], p["n_launch_adapt"]


def measure_kernels(d, m, repeats=3):
    prob = problem(d=d, m=m)
    N = prob[5].shape[0]
    W = 64 * PERIOD
    rows = {"dense": [], "diagonal": []}
    for r in range(repeats):
        for name, kw in (("dense", dict(adapt_mass=W, adapt_dense=True)), ("diagonal", dict(adapt_mass=W))):
            e = make_engine("nuts", 8, prob, 0.05, seed=3 + r, adaptive=True, period=PERIOD, **kw)
            e.run(14 * PERIOD)
            e.sync()
            got = [_profiled_period(e) for _ in range(4)]  # periods 14, 15, 16, 17
            info = e.get_dense_mass_adaptation() if name == "dense" else e.get_mass()[1]
            e.close()
            assert info["updates"] == 4 and info["refused"] == 0, info
            assert [g[2] for g in got] == ([1, 2, 2, 1] if name == "dense" else [1, 2, 1, 1]), got
            rows[name].append(got)
    dense, diag = np.array(rows["dense"]), np.array(rows["diagonal"])  # [repeats, 4 periods, (ms_adapt, ms_steps, launches)]
    acc = 0.5 * (dense[:, 0, 0] + dense[:, 3, 0])
    steps = 0.5 * (dense[:, 0, 1] + dense[:, 3, 1])
    dacc = 0.5 * (diag[:, 0, 0] + diag[:, 3, 0])
    dsteps = 0.5 * (diag[:, 0, 1] + diag[:, 3, 1])
    update, shift = dense[:, 1, 0] - acc, dense[:, 2, 0] - acc
    need = PERIOD * N * d * 8
    tiles = (d + 15) // 16
    flops = 2.0 * PERIOD * N * (tiles * (tiles + 1) // 2) * 256  # the tile pairs of the lower triangle, 16 x 16 x (chains) each
    med = lambda x: float(np.median(x))  # noqa: E731
    return dict(measurement="dense_mass_kernels", d=d, m=m, chains=N, block_steps=PERIOD, repeats=repeats,
                accumulate_ms=med(acc), accumulate_ms_all=[float(x) for x in acc], accumulate_spread=float((acc.max() - acc.min()) / np.median(acc)),
                nuts_steps_ms=med(steps), share_of_step_kernel=med(acc / steps),
                diagonal_accumulate_ms=med(dacc), diagonal_nuts_steps_ms=med(dsteps), diagonal_share_of_step_kernel=med(dacc / dsteps),
                dense_over_diagonal_accumulate=med(acc / dacc),
                update_ms=med(update), update_ms_all=[float(x) for x in update], shift_ms=med(shift),
                bytes_needed=need, achieved_bytes_per_s=float(need / (np.median(acc) * 1e-3)), matrix_flops=flops,
                achieved_flops_per_s=float(flops / (np.median(acc) * 1e-3)),
                method="hipEvent pairs around each launch (tda_profile), one block per profiled run; includes the launch gap; update and shift by difference")


def measure_ess(prob, burn=1000, draws=1000, W=800):
    import torch

    _, _, _, mean, cov, theta0, cond = prob
    N, d = theta0.shape
    cov = 0.5 * (cov + cov.T)
    e = make_engine("nuts", 8, prob, 0.05, seed=2, adaptive=True, period=PERIOD, adapt_mass=W, adapt_dense=True)
    e.run(burn)
    e.sync()
    before = e.nuts_totals()
    params = torch.empty((draws, N, d), dtype=torch.float64, device="cuda")
    t0 = time.perf_counter()
    e.run(draws, params)
    e.sync()
    dt = time.perf_counter() - t0
    tot = e.nuts_totals() - before
    scal = e.proposal_state_scaling()
    L, info = e.get_dense_mass(), e.get_dense_mass_adaptation()
    e.close()
    Ls = np.linalg.cholesky(cov)
    lam = np.linalg.eigvalsh(np.linalg.solve(Ls, np.linalg.solve(Ls, L @ L.T).T))
    res = summaries.ess_rhat_device(params)
    evals = int(tot[:, 0].sum())
    pooled = params.reshape(-1, d)
    return dict(measurement="ess_per_evaluation", mass="adapt_mass_800_adapt_dense", dense=True, chains=N, d=d, condition_number=cond, period=PERIOD, burn=burn,
                draws=draws, adapt_mass=W, mass_updates=info["updates"], mass_refused=info["refused"],
                eigenvalues_of_whitened_learnt_mass=[float(lam.min()), float(lam.max())],
                seconds=dt, evaluations=evals, evaluations_per_second=evals / dt, evaluations_per_step=evals / (N * draws),
                scaling_median=float(np.median(scal)), mean_tree_depth=float(tot[:, 3].mean() / draws), divergent=int(tot[:, 1].sum()),
                ess_min=float(res["ess"].min()), ess_median=float(np.median(res["ess"])), rhat_max=float(res["rhat"].max()),
                ess_min_per_evaluation=float(res["ess"].min() / evals), ess_median_per_evaluation=float(np.median(res["ess"]) / evals),
                ess_min_per_second=float(res["ess"].min() / dt), ess_median_per_second=float(np.median(res["ess"]) / dt),
                mean_error_max=float(np.abs(pooled.mean(dim=0).cpu().numpy() - mean).max()),
                variance_ratio_range=[float(x) for x in np.percentile(pooled.var(dim=0).cpu().numpy() / np.diag(cov), [0, 100])])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--burn", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for d, m in ((64, 96), (128, 192)):
        out.append(measure_kernels(d, m, a.repeats))
        print(json.dumps(out[-1]), flush=True)
    if a.draws > 0:
        out.append(measure_ess(problem(), burn=a.burn, draws=a.draws))
        print(json.dumps(out[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
