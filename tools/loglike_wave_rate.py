"""Throughput of a likelihood that couples outputs (TDA_LOGLIKE_WAVE: the outputs pass through LDS and tda_loglike_wave is called
by the chain's whole wave) in the fused kernels of a source-defined model, against the separable route and the engine's built-in
diagonal Gaussian noise on the same problem: 4096 chains, d = 64 parameters, the model of tests/extmodel.py, the Gaussian prior;
AdaptiveMetropolis over m = 1024 outputs, or with --mala MALA over m = 96 outputs (tda_loglike_grad_wave as well, and the
doubled LDS buffer).  Variants

    t_wave    the separable Student-t of tests/extloglike.py written in the wave form (tests/extloglikewave.py): the same
              arithmetic as `t`, so its ratio to `t` is the price of passing the outputs through LDS
    ar1       the AR(1) likelihood of tests/extloglikewave.py: per output two residuals, three divisions and two reads of LDS
    t         the separable Student-t through tda_loglike_term (the separable route)
    diag      diagonal Gaussian noise (the programs compile without the likelihood switches)

Every variant gets its own engine; after a warm-up the variants take turns, `windows` times, each turn `steps` timed steps ending
in a synchronise.  One JSON line per variant: the median chain-steps/s, the windows themselves and their spread (max - min) /
median; then the ratios of the two wave forms to the two baselines.

    python tools/loglike_wave_rate.py [--mala | --both] [--steps N] [--windows 5] [--variants t_wave,ar1,t,diag] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import extloglike as xl  # noqa: E402
from tests import extloglikewave as xlw  # noqa: E402
from tests.extmodel import source  # noqa: E402
from tinyda_amd import _lib  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402

SOURCES = {"t_wave": xlw.T_WAVE_SRC, "ar1": xlw.AR1_SRC, "t": xl.STUDENT_T_SRC}


def make_engine(variant, d, m, N, mala, scaling):
    y, par, theta0, pm, pv = xlw.problem(d, m, "ar1", N, seed=d)
    e = Engine(N, d, seed=1)
    e.set_prior(pm, np.diag(pv))
    if variant == "diag":
        e.set_level_source(0, source(), y, _lib.NOISE_DIAG, par ** 2)
    else:
        e.set_level_source(0, source() + SOURCES[variant], y, _lib.NOISE_SOURCE, par)
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
    by = {r["variant"]: r["chain_steps_per_s"] for r in rows}
    ratios = dict(proposal=rows[0]["proposal"], d=d, m=m)
    ratios.update({"%s_over_%s" % (w, b): by[w] / by[b] for w in ("t_wave", "ar1") for b in ("t", "diag") if w in by and b in by})
    return rows + [ratios]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mala", action="store_true")
    ap.add_argument("--both", action="store_true", help="AdaptiveMetropolis, then MALA, in one session (the file holds both lists)")
    ap.add_argument("--steps", type=int, default=None, help="timed steps per window (default 400; MALA: 4000)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--variants", default="t_wave,ar1,t,diag")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for mala in ((False, True) if a.both else (a.mala,)):
        rows += measure(a.variants.split(","), mala, a.steps or (4000 if mala else 400), windows=a.windows)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
