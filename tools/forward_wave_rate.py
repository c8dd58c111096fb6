"""Throughput of a wave-cooperative forward model (tda_forward_wave, -DTDA_FORWARD_WAVE) in the fused step kernel, against the
same model written per output: 4096 chains, d = 64 parameters, m = 96 outputs, the reaction-diffusion ring of tests/extwave.py
with 48 time steps, AdaptiveMetropolis.  Variants

    per_output  tda_forward(theta, dim, o): every call computes the 64 nodes' coefficients once, then repeats the solve up to its
                read-out, alone in its lane with state and coefficients in scratch memory (the only way to write this model
                without the wave form, so it is what the parent commit runs)
    wave        tda_forward_wave: the chain's wave solves once, lane = node, the neighbours through LDS

The two compute the same chains bit for bit (tests/test_gpu_forward_wave.py).  Every variant gets its own engine; after a
warm-up the variants take turns, `windows` times, each turn `steps` (`wave`: `wave-steps`, so that its windows are not a
fraction of the other's) timed steps ending in a synchronise.  One JSON line per variant: the median chain-steps/s, the windows themselves and their spread (max - min) / median; then the ratio.

    python tools/forward_wave_rate.py [--steps 200] [--wave-steps 20000] [--windows 5] [--variants per_output,wave] [--out FILE]

Both variants run the same kernel name (tda_user_steps), so a kernel trace tells them apart only in runs of their own:

    rocprofv3 --kernel-trace --stats -- python3 tools/forward_wave_rate.py --variants wave
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import extwave as xw  # noqa: E402
from tinyda_amd import _lib  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402


def make_engine(variant, d, m, N):
    _, y, theta0 = xw.problem(d, m, N, seed=d)
    e = Engine(N, d, seed=1)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, xw.source(variant, m=m), y, _lib.NOISE_ISO, 1e-4)
    e.set_proposal(2, 2e-5 * np.eye(d), t0=100, period=100)
    e.init(theta0)
    e.sync()
    return e


def measure(variants, steps, d=64, m=96, N=4096, warm=50, windows=5):
    engines = {v: make_engine(v, d, m, N) for v in variants}
    for e in engines.values():
        e.run(warm)
        e.sync()
    rates = {v: [] for v in variants}
    for _ in range(windows):
        for v in variants:  # the variants alternate inside one call
            e = engines[v]
            t0 = time.perf_counter()
            e.run(steps[v])
            e.sync()
            rates[v].append(N * steps[v] / (time.perf_counter() - t0))
    rows = []
    for v in variants:
        acc = float(engines[v].run_host(50)[2].mean())  # (after the timed windows: that the chains move is part of the record)
        engines[v].close()
        r = np.array(rates[v])
        rows.append(dict(proposal="am", variant=v, chains=N, d=d, m=m, ksteps=48, steps=steps[v], window_s=float(N * steps[v] / np.median(r)), chain_steps_per_s=float(np.median(r)),
                         windows=[float(x) for x in r], spread=float((r.max() - r.min()) / np.median(r)), acceptance=acc))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--wave-steps", type=int, default=20000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--variants", default="per_output,wave")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = measure(a.variants.split(","), {"per_output": a.steps, "wave": a.wave_steps}, windows=a.windows)
    by = {r["variant"]: r for r in rows}
    for r in rows:
        print(json.dumps(r), flush=True)
    out = list(rows)
    if "wave" in by and "per_output" in by:
        ratio = dict(proposal="am", d=rows[0]["d"], m=rows[0]["m"], wave_over_per_output=by["wave"]["chain_steps_per_s"] / by["per_output"]["chain_steps_per_s"],
                     spreads_combined=by["wave"]["spread"] + by["per_output"]["spread"])
        print(json.dumps(ratio), flush=True)
        out.append(ratio)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
