"""Throughput of the device optimiser (tda_user_maximize behind tinyda_amd.maximize) against tda_user_mala_steps on the same
model and shape: 4096 starts / chains on

    extmodel  the d = 64, m = 96 model of tools/prior_source_mala_rate.py (tests/extmodel.py with its tda_gradient), diagonal Gaussian prior
    ring      the heat ring of tests/extwave.py (tda_forward_wave + tda_gradient_wave), d = 4, m = 16

One MALA step is one evaluation of the log-posterior plus one gradient, the same model work as one accepted L-BFGS step whose
first trial passes; the MALA program is the parent commit's (this program's text compiles to the same object under its option
list), so its rate is measured here, in the same process.  Per case and build (the source's gradient, forward differences): the
wall time of one maximize() (starts uploaded, results downloaded; the compile is a first call that is not timed), the objective
evaluations and iterations it took, evaluations per second, and for the source-gradient build the ratio of its evaluations per
second to MALA's chain-steps per second.

    python tools/map_rate.py [--starts 4096] [--repeats 5] [--out profiles/map_rate.json]
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
from tests import extwave as xw  # noqa: E402
from tests.extmodel import np_forward, source  # noqa: E402
from tinyda_amd import _lib  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402


def problem(case, N):
    if case == "extmodel":
        d, m, var, src = 64, 96, 0.01, source()
        rng = np.random.default_rng(d)
        truth = 0.3 * rng.standard_normal(d)
        y = np_forward(truth, m)[0] + 0.1 * rng.standard_normal(m)
        starts = truth + 0.05 * rng.standard_normal((N, d))
    else:
        d, m, var, src = 4, 16, 1e-4, xw.source(gradient="wave")
        truth, y, _ = xw.problem(d, m, 1, 7)
        starts = truth + 0.05 * np.random.default_rng(7).standard_normal((N, d))
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(y, var * np.eye(m)), tda.DeviceModel(src, m))
    return d, m, var, src, y, starts, post


def mala_rate(d, src, y, var, starts, steps, repeats, scaling):
    e = Engine(starts.shape[0], d, seed=1)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, src, y, _lib.NOISE_ISO, var)
    e.set_proposal(_lib.PROP_MALA, None, scaling=scaling)
    e.init(starts)
    e.run(50)
    e.sync()
    rates = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        e.run(steps)
        e.sync()
        rates.append(starts.shape[0] * steps / (time.perf_counter() - t0))
    e.close()
    return float(np.median(rates)), [float(r) for r in rates]


def measure(case, N, repeats):
    d, m, var, src, y, starts, post = problem(case, N)
    mala, mala_windows = mala_rate(d, src, y, var, starts, 400, repeats, 0.004 if case == "extmodel" else 0.002)
    rows = []
    for gradient in ("source", "difference"):
        tda.maximize(post, initial_parameters=starts[:64], gradient=gradient, backend="hip")  # compile
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = tda.maximize(post, initial_parameters=starts, gradient=gradient, backend="hip")
            times.append(time.perf_counter() - t0)
        wall = float(np.median(times))
        evals = float(res.evaluations.sum())
        row = dict(case=case, gradient=gradient, starts=N, d=d, m=m, wall_seconds=wall, windows=[float(t) for t in times], evaluations=evals,
                   iterations=float(res.iterations.sum()), evaluations_per_s=evals / wall, statuses={tda.optimize.STATUS_NAMES[s]: int(np.sum(res.status == s)) for s in np.unique(res.status)},
                   mala_chain_steps_per_s=mala, mala_windows=mala_windows)
        if gradient == "source":
            row["evaluations_per_s_over_mala_steps_per_s"] = evals / wall / mala
        rows.append(row)
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for case in ("extmodel", "ring"):
        for row in measure(case, a.starts, a.repeats):
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
