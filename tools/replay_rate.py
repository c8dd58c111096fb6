"""Rate of the replay (tda_user_replay, tinyda_amd/replay.py): outputs and quantities of interest of 4096 chains x 2000 recorded
rows of a real AdaptiveMetropolis run, for two models

    ring      tests/extwave.py in the wave form, d = 4, m = 16, 48 time steps, the wave-form quantity of tests/extqoi.py (n_qoi = 3)
    extmodel  tests/extmodel.py, d = 64, m = 1024, the per-quantity form of tests/extqoi.py (n_qoi = 4)

in two variants (`qoi`: the quantities alone, the outputs stay in LDS; `outputs+qoi`: both are stored) and over a sweep of
segment_rows (1 = every row evaluated, 8, 32, 64, 256, 512, all rows of a chain in one segment) beside the library's own choice (0).
The records are produced here by the engine (the same run's sampling rate is reported for scale) and stay in device memory; the
results go to a device buffer of one chunk of rows (`--chunk-bytes`; the outputs of the whole extmodel run are 67 GB) that is
written again chunk after chunk -- a segment never spans two chunks -- and nothing crosses PCIe.  After a warm-up pass the
settings take turns, `--windows` times; a window is as many passes over all rows as fill `--window-s` seconds (counted from the
warm-up pass) and ends in a synchronise.  One JSON line per
setting: the median rows/s and model evaluations/s, the seconds per pass of every window, their spread (max - min) / median, n_evaluated / rows.
No thresholds: the numbers are the record.

    python tools/replay_rate.py [--models ring,extmodel] [--chains 4096] [--rows 2000] [--windows 3] [--out profiles/replay_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import extmodel as xm  # noqa: E402
from tests import extqoi as xq  # noqa: E402
from tests import extwave as xw  # noqa: E402
import tinyda_amd as tda  # noqa: E402
from tinyda_amd import _lib  # noqa: E402
from tinyda_amd.engine import Engine  # noqa: E402


def problem(name, N):
    """model, data, noise variance, starts, proposal covariance"""
    if name == "ring":
        d, m = 4, 16
        _, y, theta0 = xw.problem(d, m, N, seed=d)
        return tda.DeviceModel(xw.source() + xq.RING_WAVE, m, n_qoi=xq.RING_WAVE_N), y, 1e-4, theta0, 1e-3 * np.eye(d)
    d, m = 64, 1024
    rng = np.random.default_rng(7)
    truth = 0.3 * rng.standard_normal(d)
    y = xm.np_forward(truth, m)[0] + 0.05 * rng.standard_normal(m)
    return tda.DeviceModel(xm.source() + xq.PER_QUANTITY, m, n_qoi=4), y, 0.05 ** 2, truth + 0.01 * rng.standard_normal((N, d)), 1e-5 * np.eye(d)


def sample_records(model, y, var, theta0, C0, T):
    """the AM run: records [T + 1, N, d] in device memory (row 0: the starts), chain-steps/s of the run, acceptance rate"""
    import torch

    N, d = theta0.shape
    e = Engine(N, d, seed=1)
    e.set_prior(np.zeros(d), np.eye(d))
    e.set_level_source(0, model.source, y, _lib.NOISE_ISO, var)
    e.set_proposal(2, C0, t0=100, period=100)
    e.init(theta0)
    params = torch.empty((T + 1, N, d), dtype=torch.float64, device="cuda")
    stats = torch.empty((T + 1, N, 3), dtype=torch.float64, device="cuda")
    acc = torch.empty((T + 1, N), dtype=torch.uint8, device="cuda")
    e.current_into(params[0], stats[0])
    e.sync()
    t0 = time.perf_counter()
    e.run(T, params[1:], stats[1:], acc[1:])
    e.sync()
    dt = time.perf_counter() - t0
    e.close()
    return params, N * T / dt, float(acc[1:].float().mean())


def one_pass(rp, params, fields, seg, chunk_rows):
    """all rows through the replay, chunk by chunk; (seconds, model evaluations)"""
    import torch

    R, n = int(params.shape[0]), 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a in range(0, R, chunk_rows):
        rp.run(params[a:a + chunk_rows], fields, segment_rows=min(seg, chunk_rows, R - a) if seg else 0, count=True)  # (counting synchronises)
        n += rp.n_evaluated
    torch.cuda.synchronize()
    return time.perf_counter() - t0, n


def measure(name, N, T, windows, chunk_bytes, window_s):
    model, y, var, theta0, C0 = problem(name, N)
    params, sampling_rate, acceptance = sample_records(model, y, var, theta0, C0, T)
    R, d = T + 1, theta0.shape[1]
    rows = [dict(model=name, what="sampling", proposal="am", chains=N, d=d, m=model.n_outputs, iterations=T, chain_steps_per_s=sampling_rate, acceptance=acceptance)]
    segs = sorted({1, 8, 32, 64, 256, 512, R} & set(range(1, R + 1))) + [0]
    settings = [(v, s) for v in ("qoi", "outputs+qoi") for s in segs]
    fields = {"qoi": ("qoi",), "outputs+qoi": ("model_output", "qoi")}
    width = {"qoi": model.n_qoi, "outputs+qoi": model.n_outputs + model.n_qoi}
    chunk = {v: max(1, min(R, chunk_bytes // (N * width[v] * 8))) for v in width}
    with tda.Replay(model, d) as rp:
        passes, times, evals = {}, {k: [] for k in settings}, {}
        for k in settings:  # warm-up: two passes per setting (the module is loaded, the buffers are allocated); the second sizes the window
            one_pass(rp, params, fields[k[0]], k[1], chunk[k[0]])
            passes[k] = max(1, int(np.ceil(window_s / one_pass(rp, params, fields[k[0]], k[1], chunk[k[0]])[0])))
        for _ in range(windows):
            for k in settings:  # the settings alternate inside one call
                dt = 0.0
                for _ in range(passes[k]):
                    t, evals[k] = one_pass(rp, params, fields[k[0]], k[1], chunk[k[0]])
                    dt += t
                times[k].append(dt / passes[k])
    for (v, s) in settings:
        t = np.array(times[(v, s)])
        med = float(np.median(t))
        rows.append(dict(model=name, what="replay", variant=v, segment_rows=s if s else "library", chains=N, rows=R, d=d, m=model.n_outputs, n_qoi=model.n_qoi,
                         chunk_rows=chunk[v], passes_per_window=passes[(v, s)], pass_s=med, rows_per_s=N * R / med, evaluations_per_s=evals[(v, s)] / med,
                         evaluations_per_row=evals[(v, s)] / (N * R), pass_s_by_window=[float(x) for x in t], spread=float((t.max() - t.min()) / med)))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="ring,extmodel")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--chunk-bytes", type=int, default=16 << 30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for name in a.models.split(","):
        for r in measure(name, a.chains, a.rows, a.windows, a.chunk_bytes, a.window_s):
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
