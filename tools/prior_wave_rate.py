"""Throughput of a prior that couples parameters (TDA_PRIOR_WAVE: tda_logprior_wave called by the chain's whole wave over the
proposal in LDS) in the fused kernels of a source-defined model, against a separable source-defined prior and the engine's
built-in diagonal Gaussian prior on the same problem: 4096 chains, d = 64 parameters, the model of tests/extmodel.py;
AdaptiveMetropolis over m = 1024 outputs, or with --mala MALA over m = 96 outputs (tda_logprior_grad as well).  Variants

    wave      the Cauchy-difference prior of tests/extpriorwave.py: theta_0 normal, theta_j - theta_{j-1} ~ Cauchy(0, q_j); per
              parameter and step one log1p, one log, one division and two reads of LDS
    cauchy    independent scipy.stats.cauchy components through the term library of csrc/tda_prior_families.h (the separable route:
              the term's arguments arrive in registers)
    mvn       multivariate normal prior with diagonal covariance (the programs compile without the prior switches)

Every variant gets its own engine; after a warm-up the variants take turns, `windows` times, each turn `steps` timed steps ending
in a synchronise.  One JSON line per variant: the median chain-steps/s, the windows themselves and their spread (max - min) /
median; then the two ratios wave / cauchy and wave / mvn.

    python tools/prior_wave_rate.py [--mala] [--steps N] [--windows 5] [--variants wave,cauchy,mvn] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.stats as st

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tinyda_amd as tda  # noqa: E402
from tests import extpriorwave as xw  # noqa: E402
from tests.extmodel import np_forward, source  # noqa: E402
from tinyda_amd import _lib  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402


def make_engine(variant, d, m, N, mala, scaling):
    rng = np.random.default_rng(d)
    twin = xw.cauchy_difference(d)
    truth, theta0 = xw.starts(twin, N, rng)
    y = np_forward(truth, m)[0] + 0.1 * rng.standard_normal(m)
    e = Engine(N, d, seed=1)
    src = source()
    if variant == "mvn":
        e.set_prior(truth, np.diag(twin.q ** 2))
    elif variant == "cauchy":
        dp = tda.DevicePrior.from_distributions([st.cauchy(truth[j], twin.q[j]) for j in range(d)])
        e.set_prior_joint(np.full(d, _lib.PRIOR_SOURCE), dp.p, dp.q)
        src += "\n" + dp.source
    else:
        e.set_prior_joint(np.full(d, _lib.PRIOR_SOURCE), twin.p, twin.q)
        src += "\n" + twin.source
    e.set_level_source(0, src, y, _lib.NOISE_ISO, 0.01)
    if mala:
        e.set_proposal(_lib.PROP_MALA, None, scaling=scaling)
    else:
        e.set_proposal(2, 1e-5 * np.eye(d), t0=100, period=100)
    e.init(theta0)
    e.sync()
    return e


def measure(variants, mala, T, d=64, N=4096, windows=5, scaling=0.004):
    m, warm = (96, 200) if mala else (1024, 100)
    engines = {v: make_engine(v, d, m, N, mala, scaling) for v in variants}
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
    rows = []
    for v in variants:
        acc = float(engines[v].run_host(50)[2].mean())  # (after the timed windows: that the chains move is part of the record)
        engines[v].close()
        r = np.array(rates[v])
        rows.append(dict(proposal="mala" if mala else "am", variant=v, chains=N, d=d, m=m, steps=T, chain_steps_per_s=float(np.median(r)),
                         windows=[float(x) for x in r], window_seconds=float(N * T / np.median(r)), spread=float((r.max() - r.min()) / np.median(r)),
                         acceptance=acc))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mala", action="store_true")
    ap.add_argument("--steps", type=int, default=None, help="timed steps per window (default 400; --mala: 4000)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--variants", default="wave,cauchy,mvn")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = measure(a.variants.split(","), a.mala, a.steps or (4000 if a.mala else 400), windows=a.windows)
    by = {r["variant"]: r["chain_steps_per_s"] for r in rows}
    for r in rows:
        print(json.dumps(r), flush=True)
    ratios = dict(proposal=rows[0]["proposal"], d=rows[0]["d"], m=rows[0]["m"])
    ratios.update({"wave_over_" + v: by["wave"] / by[v] for v in by if v != "wave" and "wave" in by})
    print(json.dumps(ratios), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows + [ratios], fh, indent=1)
