"""Throughput of MALA under a source-defined prior (tda_user_mala_steps with TDA_PRIOR_SOURCE: tda_logprior_term and
tda_logprior_term_grad of the level's source) against MALA under the engine's built-in diagonal Gaussian prior on the same
model: 4096 chains, d = 64 parameters, m = 96 outputs, the model of tests/extmodel.py with its tda_gradient.  Variants

    mvn       multivariate normal prior with diagonal covariance (the MALA program compiles without the prior switch, so it is
              what the parent commit runs)
    normal    the same prior through the source path: a hand-written term and its derivative (what the switch itself costs)
    families  DevicePrior.from_distributions of the 13 scipy families of csrc/tda_prior_families.h, cycled over the parameters
              (every branch of both library functions runs for a wave)

Every variant gets its own engine; after a warm-up the variants take turns, `windows` times, each turn `steps` timed steps
ending in a synchronise.  One JSON line per variant: the median chain-steps/s, the windows themselves and their spread
(max - min) / median; then the ratios against `mvn`.

    python tools/prior_source_mala_rate.py [--steps 4000] [--windows 5] [--variants mvn,normal,families] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tinyda_amd as tda  # noqa: E402
from tests import extprior as xp  # noqa: E402
from tests import extpriorgrad as xg  # noqa: E402
from tests.extmodel import np_forward, source  # noqa: E402
from tinyda_amd import _lib  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402


def make_engine(variant, d, m, N, scaling):
    rng = np.random.default_rng(d)
    comps = xp.components(d)
    prior = xp.FamilyPrior(comps)
    truth, theta0 = xp.starts_near_lower_edges(comps, N, rng, q0=0.4)
    y = np_forward(truth, m)[0] + 0.1 * rng.standard_normal(m)
    e = Engine(N, d, seed=1)
    src = source()
    if variant == "mvn":
        e.set_prior(prior.mean, prior.cov)
    elif variant == "normal":
        e.set_prior_joint(np.full(d, _lib.PRIOR_SOURCE), prior.mean, np.sqrt(np.diag(prior.cov)))
        src += xp.NORMAL_SRC + xg.NORMAL_GRAD_SRC
    else:
        dp = tda.DevicePrior.from_distributions(comps)
        e.set_prior_joint(np.full(d, _lib.PRIOR_SOURCE), dp.p, dp.q)
        src += "\n" + dp.source
    e.set_level_source(0, src, y, _lib.NOISE_ISO, 0.01)
    e.set_proposal(_lib.PROP_MALA, None, scaling=scaling)
    e.init(theta0)
    e.sync()
    return e


def measure(variants, d=64, m=96, N=4096, T=4000, warm=200, windows=5, scaling=0.004):
    engines = {v: make_engine(v, d, m, N, scaling) for v in variants}
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
        rows.append(dict(proposal="mala", variant=v, chains=N, d=d, m=m, steps=T, scaling=scaling, chain_steps_per_s=float(np.median(r)),
                         windows=[float(x) for x in r], window_seconds=float(N * T / np.median(r)), spread=float((r.max() - r.min()) / np.median(r)),
                         acceptance=acc))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--variants", default="mvn,normal,families")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = measure(a.variants.split(","), T=a.steps, windows=a.windows)
    by = {r["variant"]: r["chain_steps_per_s"] for r in rows}
    for r in rows:
        print(json.dumps(r), flush=True)
    ratios = dict(proposal="mala", d=rows[0]["d"], m=rows[0]["m"])
    ratios.update({v + "_over_mvn": by[v] / by["mvn"] for v in by if v != "mvn" and "mvn" in by})
    print(json.dumps(ratios), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows + [ratios], fh, indent=1)
