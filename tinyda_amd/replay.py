"""Model outputs and quantities of interest of a device result, produced on the device after the run (include/tinyda_amd_replay.h).

The reference's Link carries `model_output` and `qoi` (link.py:23-48), evaluated at every proposal.  The engine records parameters
and log-densities only; a forward model is deterministic, so the outputs and quantities of every recorded row are the model
replayed over the records [R, N, d] -- when somebody asks, and not before: sampling pays nothing for them.  A wave walks a
chain's rows in order and evaluates the model only where the parameters change (a rejected step repeats its predecessor bit for
bit), so the replay costs one evaluation per accepted state, not one per row.

`Replay` is the compiled program of one DeviceModel, `replay_records` runs the records of one level through it in chunks of
whole rows under a byte budget (the outputs of a full-size result are R N m 8 bytes and need not fit beside the records),
`evaluate` is DeviceModel.evaluate.  Everything else (LinearModel, Rosenbrock, BatchedModel, opaque callables) keeps the route
it has: one host call per row."""
import ctypes as C
import threading

import numpy as np

from . import _lib
from .records import DeviceRecords, _is_torch

FIELDS = ("model_output", "qoi")
BUDGET_BYTES = 1 << 30  # device memory of one chunk's results (both fields together)


class Replay:
    """The replay program of `model` (a DeviceModel) for `dim` parameters on `device`: compiled once, run over any number of
    chunks.  A context manager over the handle; `n_evaluated` holds the model evaluations of the last run that counted them."""

    def __init__(self, model, dim, device=0):
        self.lib = _lib.load()
        self.dim, self.n_outputs, self.n_qoi, self.device = int(dim), int(model.n_outputs), int(getattr(model, "n_qoi", 0)), int(device)
        self.n_evaluated = None
        h = C.c_void_p()
        _lib.check(self.lib.tda_replay_create(self.device, model.source.encode(), self.dim, self.n_outputs, self.n_qoi, C.byref(h)), self.lib)
        self.h = h

    def run(self, params, fields=FIELDS, segment_rows=0, count=False):
        """params: a contiguous device tensor [rows, n_chains, dim] -> {field: device tensor [rows, n_chains, width]} for the
        fields asked for ("qoi" of a model without one is refused by the library's caller, not here: it is simply not produced)."""
        import torch

        if self.h is None:
            raise _lib.EngineError("this Replay is closed")
        if not params.is_contiguous() or params.dtype != torch.float64 or params.dim() != 3 or int(params.shape[2]) != self.dim:
            raise ValueError("params must be a contiguous float64 device tensor [rows, n_chains, %d]" % self.dim)
        rows, n = int(params.shape[0]), int(params.shape[1])
        out = {}
        with torch.cuda.device(params.device):
            if "model_output" in fields:
                out["model_output"] = torch.empty((rows, n, self.n_outputs), dtype=torch.float64, device=params.device)
            if "qoi" in fields and self.n_qoi > 0:
                out["qoi"] = torch.empty((rows, n, self.n_qoi), dtype=torch.float64, device=params.device)
            counted = C.c_int64(0)
            ptr = lambda name: C.c_void_p(out[name].data_ptr()) if name in out else None
            _lib.check(self.lib.tda_replay_run(self.h, C.c_void_p(params.data_ptr()), rows, n, int(segment_rows), ptr("model_output"), ptr("qoi"),
                                               C.byref(counted) if count else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), self.lib)
        if count:
            self.n_evaluated = int(counted.value)
        return out

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.tda_replay_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: the library may be gone
            pass


_cache_lock = threading.Lock()


def _replay_of(model, dim, device):
    """the model's compiled replay program for (dim, device), kept on the model: chain[i], .qoi of one chain after another and
    get_samples of two attributes would otherwise compile the same source again and again"""
    with _cache_lock:
        cache = model.__dict__.setdefault("_replays", {})
        key = (int(dim), int(device))
        if key not in cache:
            cache[key] = Replay(model, dim, device)
        return cache[key]


def _device_of(a, device=None):
    if device is not None:
        return int(device)
    return int(a.device.index or 0) if _is_torch(a) and a.device.type != "cpu" else 0


def _on_device(a, device):
    """rows of records as a contiguous float64 tensor on `device` (an upload when they are host memory)"""
    import torch

    if _is_torch(a):
        return a.to("cuda:%d" % device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:%d" % device)


def replay_records(records, model, fields=FIELDS, burnin=0, segment_rows=0, budget_bytes=BUDGET_BYTES, device=None, count=False):
    """Outputs and / or quantities of interest of rows [burnin:] of every chain of `records` (a DeviceRecords of one level, or a
    parameter array [R, N, d]) under `model` (that level's DeviceModel): {field: NumPy [N, R - burnin, width]}, chain-major like
    DeviceRecords.all_chains_host, which is also the way each chunk's results reach the host.  The rows go through the replay in
    chunks of whole rows whose results fit `budget_bytes` of device memory; every chunk starts a fresh segment, so chunking
    cannot change a bit.  Records that live in host memory (to_host(), NumPy) are uploaded chunk by chunk.  With count=True
    the dict also holds "n_evaluated", the number of model evaluations."""
    fields = tuple(fields)
    if not fields or any(f not in FIELDS for f in fields):
        raise ValueError("fields: some of %r" % (FIELDS,))
    if "qoi" in fields and int(getattr(model, "n_qoi", 0)) == 0:
        raise ValueError("this model has no quantity of interest (n_qoi = 0)")
    params = records.parameters if isinstance(records, DeviceRecords) else records
    R, N, d = (int(v) for v in params.shape)
    burnin = max(int(burnin), 0)
    width = {"model_output": int(model.n_outputs), "qoi": int(getattr(model, "n_qoi", 0))}
    res = {f: np.empty((N, max(R - burnin, 0), width[f])) for f in fields}
    if count:
        res["n_evaluated"] = 0
    if R - burnin <= 0 or N == 0:
        return res
    device = _device_of(params, device)
    rp = _replay_of(model, d, device)
    per_row = N * sum(width[f] for f in fields) * 8
    chunk = max(1, int(budget_bytes) // per_row)
    for a in range(burnin, R, chunk):
        b = min(R, a + chunk)
        got = rp.run(_on_device(params[a:b], device), fields, segment_rows, count)
        for f in fields:
            res[f][:, a - burnin:b - burnin] = DeviceRecords(got[f], None, None).all_chains_host("parameters")
        if count:
            res["n_evaluated"] += rp.n_evaluated
    return res


def evaluate(model, thetas, device=0):
    """DeviceModel.evaluate: a replay of one row of n chains"""
    thetas = np.ascontiguousarray(thetas, dtype=np.float64)
    if thetas.ndim != 2:
        raise ValueError("thetas must be [n, dim]")
    n, d = thetas.shape
    if n == 0:
        out = np.empty((0, model.n_outputs))
        return (out, np.empty((0, model.n_qoi))) if model.n_qoi > 0 else out
    got = _replay_of(model, d, device).run(_on_device(thetas[None], device), FIELDS)
    out = got["model_output"][0].cpu().numpy()
    return (out, got["qoi"][0].cpu().numpy()) if model.n_qoi > 0 else out


def chain_rows(records, chain, rows, model, field):
    """[T + 1, width] of ONE chain (DeviceChain.model_output / .qoi): its rows as a replay of one chain, so that the repeated rows
    of rejected steps are copied forward here too"""
    theta = np.ascontiguousarray(records.chain_host("parameters", chain, rows), dtype=np.float64)
    return replay_records(theta[:, None, :], model, (field,), device=_device_of(records.parameters))[field][0]
