"""Warm-up adaptation of the mass (k_mass_accumulate / k_mass_update, include/tinyda_amd_mass.h) on one MI355X, two measurements on
the ill-conditioned Gaussian of tools/nuts_rate.py: d = 64, m = 96, the posterior precision's eigenvalues log-spaced over 1 .. 100
in a random orthogonal basis, 4096 chains started from the posterior.

a. The cost of the accumulation.  A NUTS engine (max_depth 8, adaptive step size, period 50) with a warm-up so long that the timed
   blocks lie inside one window and no window ends in them; the engine's own device events around every launch (tda_profile: the
   step kernel under `steps`, k_mass_accumulate under `adapt` -- a NUTS engine launches nothing else there).  Per block of S = 50
   steps: the time of k_mass_accumulate, its share of the step kernel's time for the same blocks, and the bytes per second it
   achieves against the S N d 8 bytes of states it must read.  `repeats` engines take turns; the median and the spread over
   them are reported.  (An event pair around one short kernel also holds the gap behind the launch: an upper bound on the kernel.)

b. What the adaptation buys.  NUTS(max_depth 8, adaptive step size towards 0.8) with adapt_mass = W and with the unit mass, W
   steps of warm-up and `burn - W` more of burn-in, then `draws` recorded steps: bulk ESS (summaries.ess_rhat_device) per gradient
   evaluation for the worst and the median parameter, and the mean tree depth over the recorded steps.  The precision of this
   problem is NOT diagonal (its eigenvectors are a random rotation), so a diagonal mass can only learn the marginal variances.

    python tools/mass_rate.py [--repeats 5] [--burn 1000] [--draws 1000] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinyda_amd import summaries  # noqa: E402
from tools.nuts_rate import make_engine, problem  # noqa: E402

PERIOD = 50


def measure_accumulate(prob, repeats=5, blocks=8):
    N, d = prob[5].shape
    W = 64 * PERIOD  # windows [1, 2), [2, 4), [4, 8), [8, 16), [16, 32), [32, 64) in periods: the periods 17 .. 24 end none
    rows = []
    for r in range(repeats):
        e = make_engine("nuts", 8, prob, 0.05, seed=3 + r, adaptive=True, period=PERIOD, adapt_mass=W)
        e.run(17 * PERIOD)  # (warm: every kernel has run, four updates are behind, the last window has begun)
        e.sync()
        assert e.get_mass()[1]["updates"] == 4
        e.set_profiling(True)
        e.run(blocks * PERIOD)
        e.sync()
        p = e.profile()
        info = e.get_mass()[1]
        e.close()
        assert p["n_launch_steps"] == blocks and p["n_launch_adapt"] == blocks and info["updates"] == 4
        rows.append((p["ms_adapt"] / blocks, p["ms_steps"] / blocks))
    acc, steps = np.array(rows).T
    need = PERIOD * N * d * 8
    return dict(measurement="mass_accumulate_per_block", chains=N, d=d, block_steps=PERIOD, repeats=repeats, blocks_per_repeat=blocks,
                accumulate_ms=float(np.median(acc)), accumulate_ms_all=[float(x) for x in acc],
                accumulate_spread=float((acc.max() - acc.min()) / np.median(acc)),
                nuts_steps_ms=float(np.median(steps)), share_of_step_kernel=float(np.median(acc / steps)),
                bytes_needed=need, achieved_bytes_per_s=float(need / (np.median(acc) * 1e-3)),
                method="hipEvent pairs around each launch (tda_profile); includes the launch gap")


def measure_ess(prob, burn=1000, draws=1000, W=800):
    import torch

    _, _, _, mean, cov, theta0, cond = prob
    N, d = theta0.shape
    rows = []
    for name, adapt in (("nuts_unit_mass", 0), ("nuts_adapt_mass", W)):
        e = make_engine("nuts", 8, prob, 0.05, seed=2, adaptive=True, period=PERIOD, adapt_mass=adapt)
        e.run(burn)
        e.sync()
        before = e.nuts_totals()
        params = torch.empty((draws, N, d), dtype=torch.float64, device="cuda")
        e.run(draws, params)
        e.sync()
        tot = e.nuts_totals() - before
        w, info = e.get_mass()
        scal = e.proposal_state_scaling()
        e.close()
        res = summaries.ess_rhat_device(params)
        evals = int(tot[:, 0].sum())
        pooled = params.reshape(-1, d)
        rows.append(dict(measurement="ess_per_evaluation", variant=name, chains=N, d=d, condition_number=cond, adapt_mass=adapt, period=PERIOD,
                         burn=burn, draws=draws, mass_updates=info["updates"], mass_refused=info["refused"],
                         inv_mass_over_marginal_variance=[float(x) for x in np.percentile(w / np.diag(cov), [0, 50, 100])],
                         scaling_median=float(np.median(scal)), mean_tree_depth=float(tot[:, 3].mean() / draws), divergent=int(tot[:, 1].sum()),
                         evaluations=evals, evaluations_per_step=evals / (N * draws), ess_min=float(res["ess"].min()), ess_median=float(np.median(res["ess"])),
                         rhat_max=float(res["rhat"].max()), ess_min_per_evaluation=float(res["ess"].min() / evals),
                         ess_median_per_evaluation=float(np.median(res["ess"]) / evals),
                         mean_error_max=float(np.abs(pooled.mean(dim=0).cpu().numpy() - mean).max()),
                         variance_ratio_range=[float(x) for x in np.percentile(pooled.var(dim=0).cpu().numpy() / np.diag(cov), [0, 100])]))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--burn", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    prob = problem()
    out = [measure_accumulate(prob, repeats=a.repeats)]
    print(json.dumps(out[0]), flush=True)
    ess = measure_ess(prob, burn=a.burn, draws=a.draws) if a.draws > 0 else []
    for r in ess:
        print(json.dumps(r), flush=True)
    out += ess
    if len(ess) == 2:
        ratio = dict(measurement="ess_per_evaluation", adapt_over_unit_min=ess[1]["ess_min_per_evaluation"] / ess[0]["ess_min_per_evaluation"],
                     adapt_over_unit_median=ess[1]["ess_median_per_evaluation"] / ess[0]["ess_median_per_evaluation"],
                     mean_tree_depth_unit=ess[0]["mean_tree_depth"], mean_tree_depth_adapt=ess[1]["mean_tree_depth"])
        print(json.dumps(ratio), flush=True)
        out.append(ratio)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
