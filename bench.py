#!/usr/bin/env python3
"""Headline benchmark: proposal evaluations / s (+ ESS / s) of the many-chain MH hot path, BASELINE.json configs[1]:
64-dim Gaussian-linear posterior, 1024 observations, isotropic noise, AdaptiveMetropolis(t0=100, period=100),
4096 chains per GPU, synthetic data of SURVEY.md §8(d) "C2 synthetic input".

    python bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over one batch: ONE AdaptiveMetropolis PERIOD = 100 Metropolis-Hastings iterations
of every chain on the GPU (k_apply -> k_mh_steps (100 fused iterations: propose, forward model, log-likelihood,
log alpha, accept, record) -> k_adapt (the 100 moment updates) -> k_chol (covariance swap)), i.e. 409 600 proposal
evaluations per GPU.  The driver's `--steps 20 --warmup 5` is SURVEY's C2 run: 2000 iterations per chain after a warm-up.

A plain run does only what the headline needs: set-up (pilot run and burn-in), the warm-up steps, the timed steps,
--dump-outputs, and the line (with `roofline`, `kernel_ms` and `acceptance_rate`, read off the timed steps themselves).
`--full` adds the side measurements, each a run of its own after the headline: ESS/s (the timed window's and a stationary
window), the `configs` block (the other BASELINE configurations) and the CPU baseline; `--no-ess`, `--no-configs` and
`--no-cpu-baseline` leave one of them out.

With --gpus N > 1 and no WORLD_SIZE in the environment this script starts its own N ranks
(`python -m torch.distributed.run ...` as a child process, before anything here touches the GPU) and relays rank 0's line;
under torch.distributed.run it is a rank.  Chains are sharded by global id, there is no data-path collective.
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL (set before the HIP runtime loads)

D, M, SIGMA = 64, 1024, 0.1
CHAINS_PER_GPU = 4096
PERIOD = 100              # MH iterations per bench step (one AdaptiveMetropolis period)
HBM_PEAK = 8.0e12         # B/s, MI355X_MICROARCH.md "HBM3E peak BW"
FP64_MFMA_PEAK = 78.6e12  # FLOP/s dense fp64 matrix (MI355X_MICROARCH.md / AMD spec; tools/mfma_probe measures 75-77 on the box)
FLOPS_PER_EVAL = 2 * M * D + 3 * M + 2 * D  # forward + isotropic log-like + identity prior: 134 272
BYTES_PER_EVAL_STEPS = 8 * D + 8 + (8 * D + 24 + 1)  # k_mh_steps HBM: increment row + uniform in, record out = 1 057 B
DUMP_CHAINS = 512         # --dump-outputs: chains sampled (seeded) from the last step's records: 512 x (100 x 67 + 64 x 64) doubles = 44 MB


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (1 step = %d MH iterations of every chain)" % PERIOD)
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps before the timed window")
    ap.add_argument("--chains", type=int, default=CHAINS_PER_GPU, help="chains per GPU")
    ap.add_argument("--pilot", type=int, default=10000,
                    help="set-up: MH iterations of a pilot run (GaussianRandomWalk, C = 1e-4 I, theta0 ~ prior) whose final states are "
                         "the initial_parameters of the AdaptiveMetropolis run; 0 = AM starts from theta0 ~ prior itself (SURVEY's "
                         "literal recipe: its running covariance then keeps the transient's spread, acceptance falls to 0.5 %% and "
                         "the chains never equilibrate -- R-hat 20 after 80 000 iterations, measured in round 2)")
    ap.add_argument("--burnin", type=int, default=80000,
                    help="set-up: untimed, unrecorded AdaptiveMetropolis iterations before the warm-up steps (the per-chain covariance "
                         "estimates need them: a 20 000-iteration window has R-hat 1.23 right after the pilot, 1.02 after 80 000)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also take the side measurements: ESS/s, the `configs` block and the CPU baseline "
                         "(~30 s more; off by default)")
    ap.add_argument("--ess-iterations", type=int, default=20000,
                    help="--full: length of the separate stationary window ESS/s is measured on (0 = only the timed window)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-baseline-child", action="store_true", help="internal: run only the CPU legs and print their JSON")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="allow --gpus N with fewer than N devices: every rank on cuda:0 over gloo (same as TINYDA_BENCH_ONE_GPU=1)")
    ap.add_argument("--no-ess", action="store_true", help="--full without ESS/s")
    ap.add_argument("--extras", action="store_true", help="side measurements (other proposals / extensions), never the headline")
    ap.add_argument("--no-configs", action="store_true",
                    help="--full without the `configs` block (the other BASELINE configurations at full chain counts, each with its "
                         "own roofline: tools/bench_configs.py; rank 0 at N = 1 only, after the headline is measured, ~15 s)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0's chains, a fixed "
                         "sample of %d of them, float64 / float32, under 64 MB) so that two builds can be compared output for output"
                         % DUMP_CHAINS)
    return ap.parse_args()


def self_launch(args):
    """--gpus N > 1 from a bare shell: run the N ranks as a fresh child process tree (this process has made no GPU call
    and never replaces itself), relay rank 0's JSON line, exit with the children's status."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in r.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
    if line is not None:
        print(line, flush=True)
    else:
        sys.stderr.write(r.stdout[-4000:])
    sys.exit(r.returncode if r.returncode else (0 if line is not None else 1))


def c2_problem(seed=1):
    import numpy as np

    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, D)) / 8
    theta_true = rng.standard_normal(D)
    y = A @ theta_true + SIGMA * rng.standard_normal(M)
    return A, theta_true, y


def effective_cores():
    """Threads this process can actually run at once: the smallest of the CPU count, the scheduler affinity mask and the cgroup
    CPU quota (a GPU box hands a 1-GPU job a SHARE of a 256-thread host: rounds 1-4 started 256 OpenMP threads on it and
    reported `cores: 256` -- 1.2e3 evals/s per "core" was sixteen threads' worth of quota spread over 256)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                if q > 0:
                    n = min(n, max(1, int(q / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read()) + 0.5)))
        except (OSError, ValueError, IndexError):
            pass
    return max(1, n)


CPU_SAMPLE_CHAINS, CPU_SAMPLE_ITERATIONS = 4096, 1000  # the fixed sample of the CPU leg


def cpu_baseline(A, y, budget_seconds=30.0):
    """The same workload through the SAME C-ABI on the host cores: oracle/_build/libtda_cpu_native.so is include/tinyda_amd.h
    compiled for the CPU (oracle/tda_cpu_abi.cpp, kind 'port': one chain per OpenMP thread, the reference's per-step order of
    operations, Philox variates drawn inside the run like on the GPU) with `-O3 -march=native -ffp-contract=off` ON THIS MACHINE
    (__graft_entry__.build_cpu_native; the loops vectorise over outputs / matrix columns without changing a rounding), driven by
    the Engine wrapper the GPU library is driven by.  A FIXED sample -- 4096 chains x 1000 iterations, the headline's chain count
    -- so the figure does not drift with a calibration (rounds 2-4: 5.5 -> 3.8 -> 3.2e5 with the sample size); only a host too
    slow to finish it inside `budget_seconds` gets fewer iterations, and says so.  A reported baseline, not the optimisation target."""
    import numpy as np

    import __graft_entry__ as g

    cores = effective_cores()
    os.environ["OMP_NUM_THREADS"] = str(cores)  # (before libgomp is loaded: this is the child process of cpu_baseline_capped)
    so, flags = g.build_cpu_native(), " ".join(g.CPU_NATIVE_FLAGS)
    if so is None:  # no compiler on this host: the portable build
        so, flags = g.CPU_ABI_SO, "-O2 -ffp-contract=off -fopenmp (portable build: no compiler for -march=native here)"
        if not os.path.exists(so):
            g.build()
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    lib = _lib.load_from(so)

    def run(n_chains, T):
        e = Engine(n_chains, D, seed=7, lib=lib)
        e.set_prior(np.zeros(D), np.eye(D))
        e.set_level(0, A, y, 0, SIGMA ** 2)
        e.set_proposal(2, 1e-4 * np.eye(D), t0=100, period=100, sd=None, epsilon=1e-6)
        e.init(None)
        t0 = time.perf_counter()
        e.run(T)
        dt = time.perf_counter() - t0
        e.close()
        return dt

    n_chains, T = CPU_SAMPLE_CHAINS, CPU_SAMPLE_ITERATIONS
    t_cal = run(n_chains, 20)  # (also warms the thread pool); sizes the sample DOWN only when the host cannot finish the fixed one
    if t_cal / 20 * T > budget_seconds:
        T = max(100, int(budget_seconds / (t_cal / 20)) // 100 * 100)
    dt = run(n_chains, T)
    val = n_chains * T / dt
    out = {"value": val, "unit": "evals/s", "cores": cores, "per_core": val / cores, "kind": "port", "host_threads": os.cpu_count(),
           "flags": flags,
           "sample": "%d chains x %d MH iterations%s of the same workload through the CPU build of the C-ABI (libtda_cpu_native.so: g++ %s, "
                     "OpenMP over chains, %d threads = the job's CPU share of a %d-thread host, %.1f s)"
                     % (n_chains, T, "" if T == CPU_SAMPLE_ITERATIONS else " (host too slow for the fixed 1000)", flags, cores, os.cpu_count() or 1, dt)}
    # the reference's cost profile next to it -- one chain at a time in NumPy / SciPy with the SVD-based draw
    # and scipy's logpdf on every step (oracle/tinyda_oracle.py::reference_shaped_am_chain), one core, ~6 s
    try:
        from oracle import tinyda_oracle as orc

        import contextlib

        try:  # one BLAS thread, as BASELINE.md measured the reference (multithreaded OpenBLAS is slower on these sizes)
            from threadpoolctl import threadpool_limits

            one_thread = threadpool_limits(limits=1)
        except Exception:
            one_thread = contextlib.nullcontext()
        th0 = np.random.default_rng(3).standard_normal(D)
        n_ref = 20000  # ~6 s on one core
        with one_thread:
            orc.reference_shaped_am_chain(A, y, SIGMA ** 2, th0, 20, 1e-4 * np.eye(D))
            t0 = time.perf_counter()
            orc.reference_shaped_am_chain(A, y, SIGMA ** 2, th0, n_ref, 1e-4 * np.eye(D))
            dt_ref = time.perf_counter() - t0
        out["reference_shaped"] = {"value": n_ref / dt_ref, "unit": "evals/s", "cores": 1, "kind": "port",
                                   "sample": "1 chain x %d MH iterations, chain-at-a-time NumPy / SciPy with the reference's per-step "
                                             "calls (SVD-based multivariate_normal draw, scipy logpdf, three outer products), one BLAS thread, %.1f s" % (n_ref, dt_ref)}
    except Exception as ex:  # the port's number above stands on its own
        out["reference_shaped"] = {"error": repr(ex)}
    return out


CPU_BASELINE_CAP_S = 90.0  # wall-clock cap of the CPU legs (child process; they take ~3 (build) + ~10-30 + ~6 s when healthy)


def cpu_baseline_capped():
    """The CPU legs in a CHILD process killed at CPU_BASELINE_CAP_S: a hung OpenMP run or a host with an odd thread count must
    cost the bench line its `cpu_baseline`, not the GPU result that is already measured.  The child never
    touches the GPU (it loads oracle/_build/libtda_cpu.so only)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-child"]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=float(os.environ.get("TINYDA_CPU_BASELINE_CAP_S", CPU_BASELINE_CAP_S)),
                           env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        return None, "timeout: the CPU baseline child exceeded its wall-clock cap and was killed"
    for ln in reversed(r.stdout.splitlines()):
        if ln.startswith("{"):
            return json.loads(ln), None
    return None, "child failed (rc %d): %s" % (r.returncode, r.stderr[-500:])


def kernel_source_blob():
    """git blob hash of the file that defines the dominant kernel (tda_kernels_mh.h: k_mh_steps), computed without git"""
    import hashlib

    data = open(os.path.join(ROOT, "tinyda_amd", "csrc", "tda_kernels_mh.h"), "rb").read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def latest_pmc_traffic():
    """(file, HBM bytes per k_mh_steps launch, stale) from the newest committed PMC pass (tools/pmc_traffic.sh).  The PMC passes
    are separate profiler runs, so `traffic` is a committed measurement, not a live one: the file records the git blob of the
    kernel source it was taken on, and `stale` says whether the source has changed since (True also when the file predates the
    stamp)."""
    pdir = os.path.join(ROOT, "profiles")
    best = None
    try:
        for f in sorted(os.listdir(pdir)):
            if f.endswith("pmc_traffic.json"):
                j = json.load(open(os.path.join(pdir, f)))
                v = j.get("k_mh_steps_hbm_bytes_per_launch")
                if v:
                    best = (f, v, j.get("kernel_source_blob") != kernel_source_blob())
    except Exception:
        return None, None, None
    return best if best else (None, None, None)


def latest_pmc_mfma():
    """Matrix-core counters of k_mh_steps<64,8> from the newest committed pass of tools/pmc_mfma.sh (profiles/*pmc_mfma.json):
    {file, mfma_util_counter (counted MFMA flops / launch time / 78.6 TF), mfma_flops_counted (per 409 600-evaluation launch),
    counted_over_algorithmic, mfma_busy_frac, stale}.  Like `traffic` a committed measurement (PMC passes are separate profiler
    runs), stamped with the git blob of the kernel source it was taken on."""
    pdir = os.path.join(ROOT, "profiles")
    best = None
    try:
        for f in sorted(os.listdir(pdir)):
            if f.endswith("pmc_mfma.json"):
                j = json.load(open(os.path.join(pdir, f)))
                k = j.get("k_mh_steps")
                if k:
                    best = dict(file=f, stale=j.get("source_blobs", {}).get("tda_kernels_mh.h") != kernel_source_blob(), **k)
    except Exception:
        return None
    return best


def main():
    args = parse_args()
    if args.cpu_baseline_child:  # the CPU legs alone (cpu_baseline_capped): no torch, no GPU
        A, _, y = c2_problem()
        print(json.dumps(cpu_baseline(A, y)), flush=True)
        return
    if args.rehearse_on_one_gpu:
        os.environ["TINYDA_BENCH_ONE_GPU"] = "1"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)

    import numpy as np
    import torch

    from tinyda_amd import summaries as diagnostics
    from tinyda_amd import distributed as tdist
    from tinyda_amd.engine import Engine

    # TINYDA_BENCH_ONE_GPU=1 (rehearsing the N > 1 code path on a one-GPU box): every rank on cuda:0, gloo instead of RCCL
    one_gpu = os.environ.get("TINYDA_BENCH_ONE_GPU") == "1"
    if args.gpus > torch.cuda.device_count() and not one_gpu:
        # N ranks on fewer than N devices would time oversubscribed GPUs and print it as an N-GPU number: refused unless the
        # rehearsal switch says that is the point (device_count() does not initialise the GPU)
        raise SystemExit("--gpus %d but only %d device(s) visible: refusing to report a multi-GPU figure (rehearse the N > 1 code "
                         "path with --rehearse-on-one-gpu / TINYDA_BENCH_ONE_GPU=1)" % (args.gpus, torch.cuda.device_count()))
    rank, local_rank, world = tdist.init_process_group("gloo" if one_gpu else None)
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    N, K, W = args.chains, args.steps, args.warmup
    if K < 1 or W < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    burnin, pilot = max(args.burnin, 0), max(args.pilot, 0)
    T_timed, T_warm = K * PERIOD, W * PERIOD

    A, _, y = c2_problem()

    def engine(kind, **kw):
        e = Engine(N, D, seed=2026, device=local_rank, chain_offset=rank * N)  # weak scaling: N chains per GPU
        e.set_prior(np.zeros(D), np.eye(D))
        e.set_level(0, A, y, 0, SIGMA ** 2)
        e.set_proposal(kind, 1e-4 * np.eye(D), **kw)
        return e

    t_b = time.perf_counter()
    theta_start = None  # theta0 ~ prior, Philox stream 2 keyed by global chain id
    if pilot:  # what a user does with the reference: a pilot run, then sample(..., initial_parameters=its last states)
        pe = engine(0)
        pe.init(None)
        pe.run(pilot, None, None, None)
        theta_start, _ = pe.current()
        pe.close()
    eng = engine(2, t0=100, period=PERIOD, sd=None, epsilon=1e-6)
    eng.init(theta_start)

    # every record buffer is sized for the longest run that writes into it
    rows = max(T_timed, min(T_warm, T_timed) if T_warm else 0, 1)
    params = torch.empty((rows, N, D), dtype=torch.float64, device=dev)
    stats = torch.empty((rows, N, 3), dtype=torch.float64, device=dev)
    acc = torch.empty((rows, N), dtype=torch.uint8, device=dev)

    def run_chunked(engine, n_iter, record=True):
        """advance n_iter iterations, writing (and overwriting) records into the first rows of the buffers"""
        left = n_iter
        while left > 0:
            n = min(left, rows)
            if record:
                engine.run(n, params[:n], stats[:n], acc[:n], sync=False)
            else:
                engine.run(n, None, None, None, sync=False)
            left -= n
        engine.sync()

    # set-up: adaptation burn-in (unrecorded), then the W warm-up steps exactly as timed (records on)
    run_chunked(eng, burnin, record=False)
    burnin_s = time.perf_counter() - t_b
    run_chunked(eng, T_warm)
    eng.set_profiling(True)  # HIP events around every kernel launch, on the engine's stream
    torch.cuda.synchronize()
    tdist.barrier()
    t0 = time.perf_counter()
    eng.run(T_timed, params[:T_timed], stats[:T_timed], acc[:T_timed], sync=True)
    torch.cuda.synchronize()
    tdist.barrier()
    dt = tdist.reduce_scalar(time.perf_counter() - t0, "max", dev)
    prof = eng.profile()
    eng.set_profiling(False)
    if args.dump_outputs and rank == 0:  # before the ESS window, which runs on and reuses the record buffers
        dump_outputs(args.dump_outputs, eng, params, stats, acc, T_timed)

    evals = world * N * T_timed
    out = {
        "metric": "proposal evals/sec (node) + ESS/sec, 64-dim AM 4096 chains/GPU",
        "value": evals / dt,
        "unit": "evals/s",
        "n_gpus": world,
        "steps": K,
        "warmup": W,
        "ms_per_step": dt / K * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": "BASELINE configs[1] / SURVEY C2a: d=64 Gaussian-linear posterior, m=1024 obs, isotropic noise, "
                               "prior N(0,I), AdaptiveMetropolis(C0=1e-4 I, t0=100, period=100)",
                   "chains_per_gpu": N, "dim": D, "observations": M,
                   "step": "one AdaptiveMetropolis period = %d MH iterations of every chain (%d proposal evals per GPU)" % (PERIOD, PERIOD * N),
                   "mh_iterations_per_step": PERIOD, "timed_mh_iterations_per_chain": T_timed,
                   "records": "params+stats+accepted of every iteration to HBM",
                   "setup_untimed": {"pilot_grw_mh_iterations": pilot, "am_burnin_mh_iterations": burnin, "seconds": burnin_s,
                                     "start": "pilot run's final states" if pilot else "theta0 ~ prior"},
                   "rccl_ranks": world if (world > 1 and not one_gpu) else (0 if world == 1 else "gloo rehearsal on one GPU")},
    }
    if rank == 0:
        ev_rank = N * T_timed
        try:
            kern = {"k_mh_steps": (prof["ms_steps"], prof["n_launch_steps"]),
                    "k_adapt(+k_chol)": (prof["ms_adapt"], prof["n_launch_adapt"]),
                    "k_apply": (prof["ms_propose"], prof["n_launch_propose"])}  # k_rng runs under k_mh_steps on a 2nd stream
            ms_st, n_st = kern["k_mh_steps"]
            avg_launch_s = ms_st * 1e-3 / max(n_st, 1)
            evals_per_launch = ev_rank / max(n_st, 1)
            pmc_file, traffic, stale = latest_pmc_traffic()
            if traffic is not None and abs(evals_per_launch - PERIOD * CHAINS_PER_GPU) > 0.5:
                traffic = traffic * evals_per_launch / (PERIOD * CHAINS_PER_GPU)  # PMC passes are collected on 100-step launches of 4096 chains
            achieved = FLOPS_PER_EVAL * evals_per_launch / avg_launch_s
            rate_gpu = ev_rank / dt
            out["roofline"] = {"kernel": "k_mh_steps", "bound": "mfma", "achieved": achieved / 1e12, "peak": FP64_MFMA_PEAK / 1e12,
                               "unit": "TFLOP/s", "frac": achieved / FP64_MFMA_PEAK, "traffic": traffic, "traffic_source": pmc_file,
                               "traffic_stale": stale,
                               "flops_per_eval": FLOPS_PER_EVAL, "evals_per_launch": evals_per_launch,
                               "algorithmic_hbm_bytes_per_launch": BYTES_PER_EVAL_STEPS * evals_per_launch,
                               "avg_launch_ms": avg_launch_s * 1e3,
                               "whole_pipeline_frac": rate_gpu * FLOPS_PER_EVAL / FP64_MFMA_PEAK,
                               "whole_pipeline_note": "all kernels of a step (k_apply, k_mh_steps, k_adapt, k_chol; k_rng overlapped) "
                                                      "priced at the step kernel's flops: wall-clock evals/s x flops/eval / peak"}
            mf = latest_pmc_mfma()
            scale = evals_per_launch / (PERIOD * CHAINS_PER_GPU)  # the PMC pass counts 100-step launches of 4096 chains
            out["roofline"].update(
                mfma_util_counter=mf["mfma_util_counter"] if mf else None,
                mfma_flops_counted=mf["mfma_flops_counted_per_launch"] * scale if mf else None,
                mfma_counted_over_algorithmic=mf["counted_over_algorithmic"] if mf else None,
                mfma_busy_frac=mf["mfma_busy_frac"] if mf else None,
                mfma_counter_source=mf["file"] if mf else None, mfma_counter_stale=mf["stale"] if mf else None)
            out["kernel_ms"] = {k: {"total_ms": v[0], "launches": v[1], "ns_per_eval": v[0] * 1e6 / ev_rank} for k, v in kern.items()}
            out["acceptance_rate"] = float(acc[:T_timed].float().mean().item())
        except Exception as exc:  # the headline must survive a failed side computation
            out["roofline_error"] = repr(exc)
        if args.full and not args.no_ess:
            try:
                out.update(ess_section(args, eng, diagnostics, params, stats, acc, rows, N, T_timed, dt, world, local_rank, burnin))
            except Exception as exc:
                out["ess_error"] = repr(exc)
    # (the stationary ESS window is a rank-0 side run; the other ranks wait at the final barrier)
    if rank == 0 and world == 1 and args.extras:
        try:
            out["extras"] = extras(Engine, diagnostics, A, y, N, K, W, params, stats, acc, rows, local_rank, rank)
        except Exception as exc:
            out["extras_error"] = repr(exc)
    if rank == 0 and world == 1 and args.full and not args.no_configs:
        # the other BASELINE configurations (C2b, C3, C4 at exchange intervals 16 / 128, C5-literal, C5 + dense error model),
        # full per-GPU chain counts, each with its own roofline entry; side runs after the headline, never `value`
        try:
            del params, stats, acc
            torch.cuda.empty_cache()
            import importlib.util

            spec = importlib.util.spec_from_file_location("tda_bench_configs", os.path.join(ROOT, "tools", "bench_configs.py"))
            bc = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(bc)
            t_c = time.perf_counter()
            out["configs"] = bc.config_block(log=lambda m: (sys.stderr.write(m + "\n"), sys.stderr.flush()))
            out["configs_seconds"] = time.perf_counter() - t_c
        except Exception as exc:
            out["configs_error"] = repr(exc)
    if rank == 0:
        if world == 1 and args.full and not args.no_cpu_baseline:
            # the GPU result is complete: keep it on stderr in case anything below goes wrong (stdout carries ONE line, at the end)
            sys.stderr.write("[bench] GPU part done: %.4g %s, ms_per_step %.4f; CPU baseline legs follow (capped at %.0f s)\n"
                             % (out["value"], out["unit"], out["ms_per_step"], CPU_BASELINE_CAP_S))
            sys.stderr.flush()
            cb, err = cpu_baseline_capped()
            if cb is not None:
                out["cpu_baseline"] = cb
            else:
                out["cpu_baseline_error"] = err
        print(json.dumps(out), flush=True)
    eng.close()
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()


def dump_outputs(out_dir, eng, params, stats, acc, T_timed):
    """The last timed step's results for a fixed, seeded sample of the chains: the records run() hands its caller (params
    [PERIOD, S, D], stats [PERIOD, S, 3] = log-prior / log-likelihood / log-posterior, accepted [PERIOD, S] as 0 / 1) and the
    proposal covariance the step's adaptation left in use ([S, D, D])."""
    import numpy as np
    import torch

    N = params.shape[1]
    idx = np.sort(np.random.default_rng(0).choice(N, min(N, DUMP_CHAINS), replace=False))
    rows, sel = slice(T_timed - PERIOD, T_timed), torch.from_numpy(idx).to(params.device)
    outs = {"params": params[rows].index_select(1, sel).cpu().numpy(),
            "stats": stats[rows].index_select(1, sel).cpu().numpy(),
            "accepted": acc[rows].index_select(1, sel).cpu().numpy().astype(np.float32),
            "proposal_cov": eng.proposal_state()["C"][idx]}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in outs.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    sys.stderr.write("[bench] --dump-outputs: %s (%d of %d chains, %.1f MB)\n"
                     % (", ".join("%s%s" % (k, list(v.shape)) for k, v in outs.items()), len(idx), N,
                        sum(v.nbytes for v in outs.values()) / 1e6))


def ess_section(args, eng, diagnostics, params, stats, acc, rows, N, T_timed, dt, world, local_rank, burnin):
    """ESS/s = min-over-parameters rank-normalised split bulk ESS (Vehtari et al. 2021) of ALL chains of this
    GPU, on the device (tda_diag_ess_rhat: hipCUB sort + hipFFT).  Chains are independent and identically set up on every GPU,
    so the node figure is world x the rank-0 figure.  Valid only with max R-hat < 1.05."""
    import numpy as np
    import torch

    res = {}
    # (i) the timed window itself, first half dropped as SURVEY prescribes
    if T_timed >= 8:
        dd = diagnostics.ess_rhat_device(params[T_timed // 2:T_timed], device=local_rank)
        e_min, rh = float(np.nanmin(dd["ess"])), float(np.nanmax(dd["rhat"]))
        res["ess_timed_window"] = {"ess_per_sec": e_min * world / dt, "min_bulk_ess_node": e_min * world, "max_rhat": rh,
                                   "valid": bool(rh < 1.05), "draws_per_chain": T_timed - T_timed // 2, "chains_used": N,
                                   "note": "second half of the timed draws; a random-walk sampler in 64 dimensions decorrelates over "
                                           "hundreds of iterations, so windows this short leave R-hat above 1.05 even in stationarity"}
    # (ii) a longer stationary window of the same pipeline continuing the same chains, timed on its own
    L = int(args.ess_iterations)
    if L > 0:
        torch.cuda.synchronize()
        # a buffer sized for the window when the timed run's is shorter
        big = params if L <= rows else torch.empty((L, N, D), dtype=torch.float64, device=params.device)
        t1 = time.perf_counter()
        eng.run(L, big[:L], None, None, sync=True)
        torch.cuda.synchronize()
        dl = time.perf_counter() - t1
        dd = diagnostics.ess_rhat_device(big[L // 2:L], device=local_rank)
        e_min, e_med, rh = float(np.nanmin(dd["ess"])), float(np.nanmedian(dd["ess"])), float(np.nanmax(dd["rhat"]))
        valid = bool(rh < 1.05)
        res["ess_per_sec"] = e_min * world / dl if valid else None
        res["ess_parity"] = ("unpinned (ArviZ unavailable): the estimator restates Vehtari et al. 2021 as ArviZ's summary does, checked "
                             "against oracle/ess_oracle.py and closed forms only; the reference pins no ESS value")
        res["ess"] = {"valid": valid, "max_rhat": rh, "min_bulk_ess_node": e_min * world, "median_bulk_ess_node": e_med * world,
                      "window_mh_iterations": L, "window_seconds": dl, "evals_per_sec_in_window": N * L * world / dl,
                      "draws_per_chain_used": L - L // 2, "chains_used": N,
                      "ess_per_sec_if_counted": e_min * world / dl,
                      "computed": "on device, all chains; first half of the window dropped (SURVEY §8(d)); same engine, same chains, "
                                  "continuing after the timed window; params records only"}
        del big
    elif "ess_timed_window" in res:
        w = res["ess_timed_window"]
        res["ess_per_sec"] = w["ess_per_sec"] if w["valid"] else None
    return res


def extras(Engine, diagnostics, A, y, N, K, W, params, stats, acc, rows, local_rank, rank):
    """Side measurements on the same target (single GPU, --extras only): never `value`."""
    import numpy as np
    import torch

    T = min(K * PERIOD, rows)
    Tw = min(W * PERIOD, rows)
    res = {}

    def timed(e, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        e.run(n, params[:n], stats[:n], acc[:n], sync=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def fresh(seed, kind, C0, **kw):
        e = Engine(N, D, seed=seed, device=local_rank, chain_offset=rank * N)
        e.set_prior(np.zeros(D), np.eye(D))
        e.set_level(0, A, y, 0, SIGMA ** 2)
        e.set_proposal(kind, C0, **kw)
        return e

    # the reference's MALA proposal (proposal.py:861-1005) on the same target from the same start
    e5 = fresh(2026, 6, None, scaling=0.02, adaptive=True, gamma=1.01, period=50)
    e5.init(None)
    if Tw:
        e5.run(Tw, params[:Tw], stats[:Tw], acc[:Tw])
    dtm = timed(e5, T)
    dm = diagnostics.ess_rhat_device(params[T // 2:T], device=local_rank)
    res["mala_same_target"] = {"evals_per_sec_per_gpu": N * T / dtm, "ess_per_sec_per_gpu": float(np.nanmin(dm["ess"])) / dtm,
                               "min_bulk_ess": float(np.nanmin(dm["ess"])), "max_rhat": float(np.nanmax(dm["rhat"])),
                               "acceptance_rate_second_half": float(acc[T // 2:T].float().mean().item()), "seconds": dtm,
                               "proposal": "MALA(scaling=0.02, adaptive=True, period=50), exact gradient c - H theta on the device"}
    e5.close()
    # extension: AdaptiveMetropolis(block_moments=True) -- the running covariance as one rank-S update per block on the
    # matrix cores instead of the reference's elementwise recursion (parity 1e-8 instead of 1e-10)
    e4 = fresh(2026, 2, 1e-4 * np.eye(D), t0=100, period=PERIOD, block_moments=True)
    e4.init(None)
    if Tw:
        e4.run(Tw, params[:Tw], stats[:Tw], acc[:Tw])
    dtb = timed(e4, T)
    res["block_moments_extension"] = {"evals_per_sec_per_gpu": N * T / dtb, "seconds": dtb,
                                      "acceptance_rate": float(acc[:T].float().mean().item())}
    e4.close()
    return res


if __name__ == "__main__":
    main()
