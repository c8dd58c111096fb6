"""Throughput of source-defined likelihoods (TDA_NOISE_SOURCE, likelihoods.DeviceLogLike) in the fused kernels of a
source-defined model, against the engine's built-in diagonal Gaussian noise on the same model: 4096 chains, m = 256
outputs, d = 32 and 96, the model of tools/mala_source_rate.py, GaussianRandomWalk (tda_user_steps) and MALA
(tda_user_mala_steps).  Variants

    diag      built-in diagonal Gaussian noise (TDA_NOISE_DIAG)
    gauss     the same likelihood as a source term, -1/2 (f - y)^2 / p
    student   Student-t, nu = 4, per-output scale (log1p per output)
    poisson   Poisson counts, log link, per-output exposure (exp per output)
    parent    `diag` on another build of the library (--parent-lib PATH, e.g. the parent commit's), for an A/B in one call

Every variant gets its own engine; after a warm-up the variants take turns, `windows` times, each turn `steps` timed steps
ending in a synchronise.  One JSON line per (d, proposal, variant): the median chain-steps/s, the windows themselves and
their spread (max - min) / median; then the ratios gauss / diag (what the indirection costs) and diag / parent.

    python tools/loglike_source_rate.py [--steps 200] [--windows 5] [--parent-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mala_source_rate import SRC, np_forward  # noqa: E402
from tinyda_amd import _lib  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402

TERMS = {
    "gauss": r"""
__device__ double tda_loglike_term(double f, double y, double p, int o) { return -0.5 * (f - y) * (f - y) / p; }
__device__ double tda_loglike_term_grad(double f, double y, double p, int o) { return (y - f) / p; }
""",
    "student": r"""
__device__ double tda_loglike_term(double f, double y, double p, int o) {
  const double z = (f - y) / p;
  return -2.5 * log1p(0.25 * (z * z));
}
__device__ double tda_loglike_term_grad(double f, double y, double p, int o) {
  const double z = (f - y) / p;
  return -1.25 * z / ((1.0 + 0.25 * (z * z)) * p);
}
""",
    "poisson": r"""
__device__ double tda_loglike_term(double f, double y, double p, int o) { return y * f - p * exp(f); }
__device__ double tda_loglike_term_grad(double f, double y, double p, int o) { return y - p * exp(f); }
""",
}


def make_engine(variant, kind, d, m, N, lib):
    rng = np.random.default_rng(d)
    truth = 0.3 * rng.standard_normal(d)
    F = np_forward(truth, m)
    sd = 0.05 * (1.0 + 0.1 * np.arange(m) / m)
    if variant == "poisson":
        par = 20.0 + np.arange(m) % 7
        y = rng.poisson(par * np.exp(F)).astype(float)
    else:
        y = F + sd * rng.standard_normal(m)
        par = sd if variant == "student" else sd ** 2
    e = Engine(N, d, seed=1, lib=lib)
    e.set_prior(np.zeros(d), np.eye(d))
    if variant in ("diag", "parent"):
        e.set_level_source(0, SRC, y, _lib.NOISE_DIAG, par)
    else:
        e.set_level_source(0, SRC + TERMS[variant], y, _lib.NOISE_SOURCE, par)
    if kind == "mala":
        e.set_proposal(6, None, scaling=0.01, adaptive=True, period=100)
    else:
        e.set_proposal(0, np.eye(d), scaling=0.005, adaptive=True, period=100)
    e.init(truth + 0.01 * rng.standard_normal((N, d)))
    e.sync()
    return e


def measure(kind, d, variants, libs, m=256, N=4096, T=200, warm=40, windows=5):
    engines = {v: make_engine(v, kind, d, m, N, libs.get(v)) for v in variants}
    for e in engines.values():
        e.run(warm)
        e.sync()
    rates = {v: [] for v in variants}
    for _ in range(windows):
        for v in variants:  # the variants alternate inside one call
            e = engines[v]
            t0 = time.perf_counter()
            e.run(T)
            e.sync()
            rates[v].append(N * T / (time.perf_counter() - t0))
    for e in engines.values():
        e.close()
    rows = []
    for v in variants:
        r = np.array(rates[v])
        rows.append(dict(proposal=kind, variant=v, chains=N, d=d, m=m, steps=T, chain_steps_per_s=float(np.median(r)),
                         windows=[float(x) for x in r], spread=float((r.max() - r.min()) / np.median(r))))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    variants = ["diag", "gauss", "student", "poisson"]
    libs = {}
    if a.parent_lib:
        variants.insert(1, "parent")
        libs["parent"] = _lib.load_from(a.parent_lib)
    out = []
    for d in (32, 96):
        for kind in ("grw", "mala"):
            rows = measure(kind, d, variants, libs, T=a.steps, windows=a.windows)
            by = {r["variant"]: r["chain_steps_per_s"] for r in rows}
            for r in rows:
                print(json.dumps(r), flush=True)
            ratios = dict(proposal=kind, d=d, gauss_over_diag=by["gauss"] / by["diag"], student_over_diag=by["student"] / by["diag"],
                          poisson_over_diag=by["poisson"] / by["diag"])
            if "parent" in by:
                ratios["diag_over_parent"] = by["diag"] / by["parent"]
            print(json.dumps(ratios), flush=True)
            out.extend(rows + [ratios])
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
