"""NUTS against HMC on the device (tda_user_nuts_steps against tda_user_hmc_steps), two measurements on the ill-conditioned
Gaussian of tools/hmc_rate.py: a linear model as DeviceModel source, d = 64, m = 96, the posterior precision's eigenvalues
log-spaced over 1 .. 100, 4096 chains started from the posterior.

1. Gradient evaluations per second.  Variants: hmc_L8 (the parent commit's kernel, the yardstick) and nuts at max_depth 3, 6 and
   8, all at one fixed step size.  An evaluation is one leapfrog step: L per step of HMC, the leaves made for NUTS (read from the
   engine's totals before and after a window, discarded leaves included: they cost the same).  Every variant gets its own
   engine; after a warm-up the variants take turns, `windows` times, each turn ending in a synchronise.  One JSON line per
   variant: the median evaluations/s, the windows and their spread (max - min) / median; then the ratios against hmc_L8.

2. Bulk ESS per gradient evaluation.  HMC(L = 8) and NUTS(max_depth = 8), both with the adaptive step size (towards 0.65
   acceptance and 0.8 mean acceptance statistic), `burn` steps of burn-in, then `draws` recorded steps;
   summaries.ess_rhat_device over the records; ESS / evaluations for the worst and the median parameter, and the ratio NUTS / HMC.

    python tools/nuts_rate.py [--steps 400] [--windows 5] [--draws 1000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinyda_amd import _lib, summaries  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402
from tools.hmc_rate import linear_source  # noqa: E402

VARIANTS = {"hmc_L8": ("hmc", 8), "nuts_depth3": ("nuts", 3), "nuts_depth6": ("nuts", 6), "nuts_depth8": ("nuts", 8)}


def problem(d=64, m=96, N=4096):
    rng = np.random.default_rng(7)
    V, U = np.linalg.qr(rng.standard_normal((d, d)))[0], np.linalg.qr(rng.standard_normal((m, d)))[0]
    lam, nv = np.logspace(0.0, 2.0, d), 0.25
    A = U @ np.diag(np.sqrt(nv * (lam - 1.0))) @ V.T  # N(0, I) prior: the precision is V diag(lam) V^T
    y = A @ rng.standard_normal(d) + np.sqrt(nv) * rng.standard_normal(m)
    cov = np.linalg.inv(np.eye(d) + A.T @ A / nv)
    mean = cov @ (A.T @ y / nv)
    theta0 = mean + rng.standard_normal((N, d)) @ np.linalg.cholesky(cov).T
    return A, y, nv, mean, cov, theta0, float(lam[-1] / lam[0])


def make_engine(kind, arg, prob, scaling, seed, **kw):
    A, y, nv, _, _, theta0, _ = prob
    N, d = theta0.shape
    e = Engine(N, d, seed=seed)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, linear_source(A), y, _lib.NOISE_ISO, nv)
    if kind == "hmc":
        e.set_proposal(_lib.PROP_HMC, None, scaling=scaling, n_leapfrog=arg, **kw)
    else:
        e.set_proposal(_lib.PROP_NUTS, None, scaling=scaling, max_depth=arg, **kw)
    e.init(theta0)
    e.sync()
    return e


def evaluations(e, kind, arg, steps):
    """gradient evaluations of all chains since init (NUTS), or of `steps` steps (HMC)"""
    return int(e.nuts_totals()[:, 0].sum()) if kind == "nuts" else e.n_chains * steps * arg


def measure_rate(variants, prob, steps=400, warm=50, windows=5, scaling=0.1):
    engines = {v: make_engine(*VARIANTS[v], prob, scaling, seed=1) for v in variants}
    done = {}
    for v, e in engines.items():
        e.run(warm)
        e.sync()
        done[v] = evaluations(e, *VARIANTS[v], warm)
    rates, depth = {v: [] for v in variants}, {}
    for _ in range(windows):
        for v in variants:  # the variants alternate inside one call
            e, (kind, arg) = engines[v], VARIANTS[v]
            t0 = time.perf_counter()
            e.run(steps)
            e.sync()
            dt = time.perf_counter() - t0
            now = evaluations(e, kind, arg, steps) if kind == "nuts" else done[v] + evaluations(e, kind, arg, steps)
            rates[v].append((now - done[v]) / dt)
            done[v] = now
    rows = []
    for v in variants:
        kind, arg = VARIANTS[v]
        e = engines[v]
        tot = e.nuts_totals() if kind == "nuts" else None
        acc = float(e.run_host(50)[2].mean())  # (after the timed windows: that the chains move is part of the record)
        e.close()
        r = np.array(rates[v])
        row = dict(measurement="evaluations_per_s", variant=v, chains=e.n_chains, d=prob[5].shape[1], m=prob[0].shape[0], steps=steps, scaling=scaling,
                   evaluations_per_s=float(np.median(r)), windows=[float(x) for x in r], spread=float((r.max() - r.min()) / np.median(r)), moved=acc)
        if tot is not None:
            n_steps = warm + windows * steps
            row.update(max_depth=arg, mean_tree_depth=float(tot[:, 3].mean() / n_steps), evaluations_per_step=float(tot[:, 0].mean() / n_steps),
                       trees_at_max_depth=float(tot[:, 2].mean() / n_steps), divergent=int(tot[:, 1].sum()))
        else:
            row.update(n_leapfrog=arg)
        rows.append(row)
    return rows


def measure_ess(prob, burn=1000, draws=1000):
    import torch

    _, _, _, mean, cov, theta0, cond = prob
    N, d = theta0.shape
    rows = []
    for name, (kind, arg) in (("hmc_L8", ("hmc", 8)), ("nuts_depth8", ("nuts", 8))):
        e = make_engine(kind, arg, prob, 0.05, seed=2, adaptive=True, period=50)
        e.run(burn)
        e.sync()
        before = evaluations(e, kind, arg, burn)
        params = torch.empty((draws, N, d), dtype=torch.float64, device="cuda")
        stats = torch.empty((draws, N, 3), dtype=torch.float64, device="cuda")
        acc = torch.empty((draws, N), dtype=torch.uint8, device="cuda")
        t0 = time.perf_counter()
        e.run(draws, params, stats, acc)
        e.sync()
        seconds = time.perf_counter() - t0
        evals = evaluations(e, kind, arg, draws) - (before if kind == "nuts" else 0)
        scal = e.proposal_state_scaling()
        tot = e.nuts_totals() if kind == "nuts" else None
        e.close()
        res = summaries.ess_rhat_device(params)
        pooled = params.reshape(-1, d)
        row = dict(measurement="ess_per_evaluation", variant=name, chains=N, d=d, condition_number=cond, burn=burn, draws=draws,
                   moved=float(acc.double().mean()), scaling_median=float(np.median(scal)), ess_min=float(res["ess"].min()),
                   ess_median=float(np.median(res["ess"])), rhat_max=float(res["rhat"].max()), evaluations=evals,
                   evaluations_per_step=evals / (N * draws), ess_min_per_evaluation=float(res["ess"].min() / evals),
                   ess_median_per_evaluation=float(np.median(res["ess"]) / evals), seconds=seconds,
                   mean_error_max=float(np.abs(pooled.mean(dim=0).cpu().numpy() - mean).max()),
                   variance_ratio_range=[float(x) for x in np.percentile(pooled.var(dim=0).cpu().numpy() / np.diag(cov), [0, 100])])
        if tot is not None:
            row.update(mean_tree_depth=float(tot[:, 3].mean() / (burn + draws)), divergent=int(tot[:, 1].sum()))
        rows.append(row)
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--burn", type=int, default=1000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    prob = problem()
    rows = measure_rate(a.variants.split(","), prob, steps=a.steps, windows=a.windows)
    by = {r["variant"]: r["evaluations_per_s"] for r in rows}
    for r in rows:
        print(json.dumps(r), flush=True)
    ratios = dict(measurement="evaluations_per_s")
    ratios.update({v + "_over_hmc_L8": by[v] / by["hmc_L8"] for v in by if v != "hmc_L8" and "hmc_L8" in by})
    print(json.dumps(ratios), flush=True)
    ess = measure_ess(prob, burn=a.burn, draws=a.draws) if a.draws > 0 else []
    for r in ess:
        print(json.dumps(r), flush=True)
    out = rows + [ratios] + ess
    if len(ess) == 2:
        ratio = dict(measurement="ess_per_evaluation", nuts_over_hmc_min=ess[1]["ess_min_per_evaluation"] / ess[0]["ess_min_per_evaluation"],
                     nuts_over_hmc_median=ess[1]["ess_median_per_evaluation"] / ess[0]["ess_median_per_evaluation"])
        print(json.dumps(ratio), flush=True)
        out.append(ratio)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
