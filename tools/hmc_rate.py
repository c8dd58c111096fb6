"""HMC against MALA on the device (tda_user_hmc_steps against tda_user_mala_steps), two measurements.

1. Model evaluations per second.  The configuration of tools/prior_source_mala_rate.py's `mvn` variant: 4096 chains, d = 64
   parameters, m = 96 outputs, the model of tests/extmodel.py with its tda_gradient, a diagonal Gaussian prior.  Variants: mala
   (the parent commit's kernel) and hmc with L = 1, 4, 8, 16 leapfrog steps; a step of hmc is L evaluations of the model and its
   gradient, so a window of hmc_L runs `evaluations` / L steps.  Every variant gets its own engine; after a warm-up the variants
   take turns, `windows` times, each turn ending in a synchronise.  One JSON line per variant: the median evaluations/s, the
   windows and their spread (max - min) / median; then the ratios against mala.

2. Bulk ESS per model evaluation on an ill-conditioned Gaussian posterior: a linear model as DeviceModel source, d = 64, the
   posterior precision's eigenvalues log-spaced over 1 .. 100.  MALA and HMC(L = 8), both with the adaptive scaling, `burn` steps
   of burn-in, then `draws` recorded steps; summaries.ess_rhat_device over the records; ESS / (chains x draws x L) for the worst
   and the median parameter, and the ratio HMC / MALA.

    python tools/hmc_rate.py [--evaluations 4000] [--windows 5] [--draws 1000] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import extprior as xp  # noqa: E402
from tests.extmodel import np_forward, source  # noqa: E402
from tinyda_amd import _lib, summaries  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402

VARIANTS = {"mala": 0, "hmc_L1": 1, "hmc_L4": 4, "hmc_L8": 8, "hmc_L16": 16}  # name -> leapfrog steps (0: the MALA kernel)


def set_proposal(e, L, scaling, **kw):
    if L:
        e.set_proposal(_lib.PROP_HMC, None, scaling=scaling, n_leapfrog=L, **kw)
    else:
        e.set_proposal(_lib.PROP_MALA, None, scaling=scaling, **kw)


def make_engine(L, d, m, N, scaling):
    rng = np.random.default_rng(d)
    comps = xp.components(d)
    prior = xp.FamilyPrior(comps)
    truth, theta0 = xp.starts_near_lower_edges(comps, N, rng, q0=0.4)
    y = np_forward(truth, m)[0] + 0.1 * rng.standard_normal(m)
    e = Engine(N, d, seed=1)
    e.set_prior(prior.mean, prior.cov)
    e.set_level_source(0, source(), y, _lib.NOISE_ISO, 0.01)
    set_proposal(e, L, scaling)
    e.init(theta0)
    e.sync()
    return e


def measure_rate(variants, d=64, m=96, N=4096, evaluations=4000, warm=200, windows=5, scaling=0.004):
    engines = {v: make_engine(VARIANTS[v], d, m, N, scaling) for v in variants}
    steps = {v: max(1, evaluations // max(1, VARIANTS[v])) for v in variants}
    for v, e in engines.items():
        e.run(max(1, warm // max(1, VARIANTS[v])))
        e.sync()
    rates = {v: [] for v in variants}
    for _ in range(windows):
        for v in variants:  # the variants alternate inside one call
            e, T, L = engines[v], steps[v], max(1, VARIANTS[v])
            t0 = time.perf_counter()
            e.run(T)
            e.sync()
            rates[v].append(N * T * L / (time.perf_counter() - t0))
    rows = []
    for v in variants:
        acc = float(engines[v].run_host(50)[2].mean())  # (after the timed windows: that the chains move is part of the record)
        engines[v].close()
        r = np.array(rates[v])
        rows.append(dict(measurement="evaluations_per_s", variant=v, n_leapfrog=VARIANTS[v], chains=N, d=d, m=m, steps=steps[v], scaling=scaling,
                         evaluations_per_s=float(np.median(r)), windows=[float(x) for x in r], spread=float((r.max() - r.min()) / np.median(r)),
                         acceptance=acc))
    return rows


def linear_source(A):
    m, d = A.shape
    return r"""
__device__ const double A_[%d] = {%s};
__device__ double tda_forward(const double* theta, int dim, int o) {
  double s = 0.0;
  for (int j = 0; j < dim; ++j) s += A_[o * dim + j] * theta[j];
  return s;
}
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int m, int j) {
  double g = 0.0;
  for (int o = 0; o < m; ++o) g += A_[o * dim + j] * sens[o];
  return g;
}
""" % (m * d, ", ".join("%.17g" % v for v in A.ravel()))


def measure_ess(d=64, m=96, N=4096, burn=2000, draws=1000, L=8):
    import torch

    rng = np.random.default_rng(7)
    V, U = np.linalg.qr(rng.standard_normal((d, d)))[0], np.linalg.qr(rng.standard_normal((m, d)))[0]
    lam, nv = np.logspace(0.0, 2.0, d), 0.25
    A = U @ np.diag(np.sqrt(nv * (lam - 1.0))) @ V.T  # N(0, I) prior: the precision is V diag(lam) V^T
    y = A @ rng.standard_normal(d) + np.sqrt(nv) * rng.standard_normal(m)
    cov = np.linalg.inv(np.eye(d) + A.T @ A / nv)
    mean = cov @ (A.T @ y / nv)
    theta0 = mean + rng.standard_normal((N, d)) @ np.linalg.cholesky(cov).T
    rows = []
    for name, leap, scaling in (("mala", 0, 0.05), ("hmc_L%d" % L, L, 0.05)):
        e = Engine(N, d, seed=2)
        e.set_prior(np.zeros(d), np.eye(d))
        e.set_level_source(0, linear_source(A), y, _lib.NOISE_ISO, nv)
        set_proposal(e, leap, scaling, adaptive=True, period=50)
        e.init(theta0)
        e.run(burn)
        params = torch.empty((draws, N, d), dtype=torch.float64, device="cuda")
        stats = torch.empty((draws, N, 3), dtype=torch.float64, device="cuda")
        acc = torch.empty((draws, N), dtype=torch.uint8, device="cuda")
        t0 = time.perf_counter()
        e.run(draws, params, stats, acc)
        e.sync()
        seconds = time.perf_counter() - t0
        scal = e.proposal_state_scaling()
        e.close()
        res = summaries.ess_rhat_device(params)
        evals = N * draws * max(1, leap)
        pooled = params.reshape(-1, d)
        rows.append(dict(measurement="ess_per_evaluation", variant=name, n_leapfrog=leap, chains=N, d=d, m=m, condition_number=float(lam[-1] / lam[0]),
                         burn=burn, draws=draws, acceptance=float(acc.double().mean()), scaling_median=float(np.median(scal)),
                         ess_min=float(res["ess"].min()), ess_median=float(np.median(res["ess"])), rhat_max=float(res["rhat"].max()),
                         evaluations=evals, ess_min_per_evaluation=float(res["ess"].min() / evals), ess_median_per_evaluation=float(np.median(res["ess"]) / evals),
                         seconds=seconds, mean_error_max=float((pooled.mean(dim=0).cpu().numpy() - mean).__abs__().max()),
                         variance_ratio_range=[float(x) for x in np.percentile(pooled.var(dim=0).cpu().numpy() / np.diag(cov), [0, 100])]))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--evaluations", type=int, default=4000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--burn", type=int, default=2000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = measure_rate(a.variants.split(","), evaluations=a.evaluations, windows=a.windows)
    by = {r["variant"]: r["evaluations_per_s"] for r in rows}
    for r in rows:
        print(json.dumps(r), flush=True)
    ratios = dict(measurement="evaluations_per_s", d=rows[0]["d"], m=rows[0]["m"])
    ratios.update({v + "_over_mala": by[v] / by["mala"] for v in by if v != "mala" and "mala" in by})
    print(json.dumps(ratios), flush=True)
    ess = measure_ess(burn=a.burn, draws=a.draws) if a.draws > 0 else []
    for r in ess:
        print(json.dumps(r), flush=True)
    out = rows + [ratios] + ess
    if len(ess) == 2:
        ratio = dict(measurement="ess_per_evaluation", hmc_over_mala_min=ess[1]["ess_min_per_evaluation"] / ess[0]["ess_min_per_evaluation"],
                     hmc_over_mala_median=ess[1]["ess_median_per_evaluation"] / ess[0]["ess_median_per_evaluation"])
        print(json.dumps(ratio), flush=True)
        out.append(ratio)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
