"""A dense inverse mass for NUTS on the device (-DTDA_DENSE_MASS, include/tinyda_amd_dense_mass.h) on one MI355X, two measurements
on the ill-conditioned Gaussian of tools/nuts_rate.py: linear model as source, the posterior precision's eigenvalues log-spaced
over 1 .. 100 in a random orthogonal basis, 4096 chains started from the posterior.

a. What the mass buys (d = 64).  NUTS(max_depth 8, adaptive step size towards 0.8, period 50) under four masses: the unit mass, the
   diagonal of the true covariance, the true covariance (dense), and mass_from_samples of a 300-step pilot run under the unit mass
   (its last 200 steps).  `burn` steps of burn-in, then `draws` recorded steps: gradient evaluations per second over the recorded
   steps (wall clock around run + sync), the mean tree depth, bulk ESS (summaries.ess_rhat_device) per gradient evaluation for the
   worst and the median parameter.

b. What a dense leaf costs.  The same engine twice at a fixed step size, with the unit mass (the diagonal kernel) and with
   set_dense_mass(I) (the dense kernel): the trajectories are the same bit for bit, so the leaves are the same and the ratio of
   the step kernels' times (the engine's own device events around each launch, tda_profile) is the ratio per leaf.  d = 64 and
   d = 128 (m = 192), `repeats` engine pairs taking turns, median and spread.

    python tools/dense_mass_rate.py [--burn 1000] [--draws 1000] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tinyda_amd as tda  # noqa: E402
from tinyda_amd import summaries  # noqa: E402
from tinyda_amd.records import DeviceChain, DeviceRecords  # noqa: E402
from tools.nuts_rate import make_engine, problem  # noqa: E402

PERIOD = 50


def pilot_mass(prob, steps=300, keep=200):
    """mass_from_samples of the last `keep` of `steps` steps of NUTS under the unit mass"""
    import torch

    N, d = prob[5].shape
    e = make_engine("nuts", 8, prob, 0.05, seed=5, adaptive=True, period=PERIOD)
    params = torch.empty((steps, N, d), dtype=torch.float64, device="cuda")
    e.run(steps, params)
    e.sync()
    e.close()
    recs = DeviceRecords(params, None, None)
    result = dict(sampler="MH", n_chains=N, **{"chain_%d" % i: DeviceChain(recs, i, None) for i in range(N)})
    return tda.mass_from_samples(result, burnin=steps - keep)


def measure_ess(prob, burn=1000, draws=1000):
    import torch

    _, _, _, mean, cov, theta0, cond = prob
    N, d = theta0.shape
    cov = 0.5 * (cov + cov.T)
    pilot = pilot_mass(prob)
    lam = np.linalg.eigvalsh(np.linalg.solve(np.linalg.cholesky(cov), np.linalg.solve(np.linalg.cholesky(cov), pilot).T))
    masses = (("unit", {}, None), ("diagonal_of_true_covariance", dict(inv_mass=np.diag(cov).copy()), None),
              ("true_covariance", dict(dense_mass=np.linalg.cholesky(cov)), None),
              ("mass_from_samples_of_300_step_pilot", dict(dense_mass=np.linalg.cholesky(pilot)), [float(lam.min()), float(lam.max())]))
    rows = []
    for name, kw, pilot_range in masses:
        e = make_engine("nuts", 8, prob, 0.05, seed=2, adaptive=True, period=PERIOD, **kw)
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
        e.close()
        res = summaries.ess_rhat_device(params)
        evals = int(tot[:, 0].sum())
        pooled = params.reshape(-1, d)
        row = dict(measurement="ess_per_evaluation", mass=name, dense="dense_mass" in kw, chains=N, d=d, condition_number=cond, period=PERIOD, burn=burn, draws=draws,
                   seconds=dt, evaluations=evals, evaluations_per_second=evals / dt, evaluations_per_step=evals / (N * draws),
                   scaling_median=float(np.median(scal)), mean_tree_depth=float(tot[:, 3].mean() / draws), divergent=int(tot[:, 1].sum()),
                   ess_min=float(res["ess"].min()), ess_median=float(np.median(res["ess"])), rhat_max=float(res["rhat"].max()),
                   ess_min_per_evaluation=float(res["ess"].min() / evals), ess_median_per_evaluation=float(np.median(res["ess"]) / evals),
                   ess_min_per_second=float(res["ess"].min() / dt), ess_median_per_second=float(np.median(res["ess"]) / dt),
                   mean_error_max=float(np.abs(pooled.mean(dim=0).cpu().numpy() - mean).max()),
                   variance_ratio_range=[float(x) for x in np.percentile(pooled.var(dim=0).cpu().numpy() / np.diag(cov), [0, 100])])
        if pilot_range is not None:
            row["eigenvalues_of_whitened_pilot_mass"] = pilot_range
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def measure_leaf(d, m, repeats=5, blocks=6, scaling=0.1):
    prob = problem(d=d, m=m)
    N = prob[5].shape[0]
    ms = {"diagonal": [], "dense": []}
    leaves = {}
    for r in range(repeats):
        for name, kw in (("diagonal", {}), ("dense", dict(dense_mass=np.eye(d)))):
            e = make_engine("nuts", 8, prob, scaling, seed=11 + r, period=PERIOD, **kw)
            e.run(PERIOD)  # (warm: the program is built and has run)
            e.sync()
            before = e.nuts_totals()
            e.set_profiling(True)
            e.run(blocks * PERIOD)
            e.sync()
            p = e.profile()
            n = int((e.nuts_totals() - before)[:, 0].sum())
            e.close()
            ms[name].append(p["ms_steps"])
            leaves.setdefault(r, {})[name] = n
        assert leaves[r]["diagonal"] == leaves[r]["dense"]  # the same trajectories
    a, b = np.array(ms["diagonal"]), np.array(ms["dense"])
    n = np.array([leaves[r]["dense"] for r in range(repeats)], dtype=float)
    row = dict(measurement="leaf_time_dense_over_diagonal", d=d, m=m, chains=N, repeats=repeats, steps_per_repeat=blocks * PERIOD, scaling=scaling,
               leaves_per_chain_step=float(np.median(n) / (N * blocks * PERIOD)),
               diagonal_ns_per_leaf_per_chain=float(np.median(a * 1e6 / n * N)), dense_ns_per_leaf_per_chain=float(np.median(b * 1e6 / n * N)),
               diagonal_ms=[float(x) for x in a], dense_ms=[float(x) for x in b], ratio=float(np.median(b / a)),
               ratio_spread=float(((b / a).max() - (b / a).min()) / np.median(b / a)),
               method="hipEvent pairs around each launch of the step kernel (tda_profile); dense_mass = I gives the diagonal kernel's trajectories bit for bit")
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--burn", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = [measure_leaf(64, 96, a.repeats), measure_leaf(128, 192, a.repeats)]
    out += measure_ess(problem(), burn=a.burn, draws=a.draws) if a.draws > 0 else []
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
