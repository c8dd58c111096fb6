"""Modes of a posterior: get_MAP / get_ML with the reference's call shape (tinyDA/utils.py:204-269), and `maximize`, the
multi-start optimiser behind them (include/tinyda_amd_optimize.h).

The reference minimises -posterior.create_link(x).posterior with scipy.optimize.minimize from one start drawn from the prior: one
Python model call per function evaluation.  A posterior that is stated as HIP source -- a DeviceModel with isotropic / diagonal
noise or a DeviceLogLike, under a diagonal Gaussian prior, a JointPrior or a DevicePrior -- is optimised on the device instead:
one kernel (tda_user_maximize, L-BFGS with a backtracking line search) takes every start from its initial point to its end in one
launch, one wave per start, over the source's own gradient where it has one and over forward differences where it has not.
Everything else (dense noise or prior covariance, LinearModel, Rosenbrock, BatchedModel, plain callables, an explicit `method=`)
runs the reference's route on the host, one start after the other."""
import ctypes as C
import threading
import warnings

import numpy as np

from . import _lib
from .likelihoods import _is_diagonal

STATUS_NAMES = ("CONVERGED_GRADIENT", "CONVERGED_VALUE", "MAX_ITER", "LINESEARCH_FAILED", "INFEASIBLE_START", "NONFINITE_GRADIENT")
OBJECTIVES = ("posterior", "likelihood")
MAX_PARAMETERS = 128


class MaximizeResult:
    """What `maximize` returns, one row per start: x [n, d], value (the objective at x), logprior, loglike, grad_norm (max_j |g_j|;
    NaN where the route does not report a gradient), iterations, evaluations, status (indices into status_names), best (the index
    of the largest finite value, None when no start has one) and backend ('hip' or 'host')."""

    status_names = STATUS_NAMES

    def __init__(self, x, value, logprior, loglike, grad_norm, iterations, evaluations, status, backend):
        self.x, self.value, self.logprior, self.loglike, self.grad_norm = x, value, logprior, loglike, grad_norm
        self.iterations, self.evaluations, self.status, self.backend = iterations, evaluations, status, backend
        finite = np.isfinite(value)
        self.best = int(np.argmax(np.where(finite, value, -np.inf))) if finite.any() else None

    def __repr__(self):
        counts = ", ".join("%s: %d" % (STATUS_NAMES[s], int(np.sum(self.status == s))) for s in np.unique(self.status))
        return "MaximizeResult(%d starts on %s; %s; best value %s)" % (self.x.shape[0], self.backend, counts, None if self.best is None else self.value[self.best])


def _device_problem(posterior):
    """(the posterior's description, None) when the device optimiser takes it, else (None, the reason why not).  The description
    is Posterior._lowering(), read directly: no proposal is involved, so the lowering pass of sample() is not."""
    low = getattr(posterior, "_lowering", lambda: None)()
    if low is None:
        return None, ("a posterior the engine cannot describe (an opaque Python model, a prior other than scipy's multivariate normal / JointPrior / "
                      "DevicePrior, a likelihood outside GaussianLogLike's classes and DeviceLogLike)")
    if "source" not in low:
        return None, "the device optimiser takes a DeviceModel (LinearModel, Rosenbrock, BatchedModel and plain callables are optimised on the host)"
    if low["prior_mean"].shape[0] > MAX_PARAMETERS:
        return None, "more than %d parameters" % MAX_PARAMETERS
    if low["noise_kind"] not in (_lib.NOISE_ISO, _lib.NOISE_DIAG, _lib.NOISE_SOURCE):
        return None, "the device optimiser takes isotropic / diagonal noise or a DeviceLogLike (a dense observation covariance is optimised on the host)"
    if "prior_joint" not in low and not _is_diagonal(low["prior_cov"]):
        return None, "the device optimiser takes a diagonal prior covariance, a JointPrior or a DevicePrior (a dense prior covariance is optimised on the host)"
    return low, None


def _has_source_gradient(low):
    """would the MALA program of this source compile: the model's gradient, and beside a DeviceLogLike / source-defined prior theirs"""
    return bool(low.get("has_gradient") and (low["noise_kind"] != _lib.NOISE_SOURCE or low.get("loglike_has_gradient"))
                and ("prior_source" not in low or low["prior_source"]["has_gradient"]))


def _prior_components(low):
    """(kinds, loc, scale) as tda_optimizer_create takes them"""
    if "prior_joint" in low:
        return low["prior_joint"]
    d = low["prior_mean"].shape[0]
    return np.zeros(d, dtype=np.int32), low["prior_mean"], np.sqrt(np.diag(low["prior_cov"]))


def _draw_starts(posterior, low, n, seed):
    """n starts ~ prior, drawn on the host by the helpers sample() uses for missing initial_parameters: start i comes from the
    generator keyed by (seed, i), whatever n is"""
    from .api import _TAG_THETA0, _host_rng, _joint_rvs, _source_prior_starts

    prior = posterior.prior
    if low is not None and "prior_source" in low:
        return np.stack(_source_prior_starts(prior, n, 0, seed))
    if low is not None:
        joint = _prior_components(low)
        return np.stack([_joint_rvs(joint, 1, _host_rng(seed, _TAG_THETA0, i))[0] for i in range(n)])
    rows = []
    for i in range(n):
        rng = _host_rng(seed, _TAG_THETA0, i)
        if hasattr(prior, "ppf") and getattr(prior, "dim", None) is not None:  # (JointPrior: its rvs takes no generator)
            try:
                rows.append(np.asarray(prior.ppf(rng.random((1, prior.dim))), dtype=np.float64).reshape(prior.dim))
                continue
            except TypeError:
                pass
        try:
            rows.append(np.atleast_1d(np.asarray(prior.rvs(random_state=rng), dtype=np.float64)))
        except TypeError:  # a prior whose rvs takes no generator (the reference's JointPrior): its own stream
            rows.append(np.atleast_1d(np.asarray(prior.rvs(), dtype=np.float64)))
    return np.stack(rows)


def _given_starts(initial_parameters):
    if isinstance(initial_parameters, (list, tuple)):
        starts = np.stack([np.asarray(p, dtype=np.float64).reshape(-1) for p in initial_parameters])
    else:
        starts = np.asarray(initial_parameters, dtype=np.float64)
        if starts.ndim == 0:
            starts = starts.reshape(1, 1)
        elif starts.ndim == 1:
            starts = starts[None]
    if starts.ndim != 2 or starts.shape[0] < 1:
        raise ValueError("initial_parameters must be [d], [n, d] or a list of [d]")
    return np.ascontiguousarray(starts)


class Optimizer:
    """The compiled optimiser of one posterior description (`low`, from Posterior._lowering) on `device`; a context manager over
    the library's handle.  `source_gradient` selects the build."""

    def __init__(self, low, source_gradient, device=0):
        self.lib = _lib.load()
        self.dim, self.device = int(low["prior_mean"].shape[0]), int(device)
        f64 = lambda a: np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
        kinds, loc, scale = _prior_components(low)
        keep = [f64(low["data"]), f64(low["noise"]), np.ascontiguousarray(kinds, dtype=np.int32), f64(loc), f64(scale)]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        prob = _lib.tda_optimize_problem(C.sizeof(_lib.tda_optimize_problem), self.dim, int(keep[0].shape[0]), int(low["noise_kind"]), int(bool(source_gradient)), 0,
                                         *[ptr(a) for a in keep])
        h = C.c_void_p()
        _lib.check(self.lib.tda_optimizer_create(self.device, low["source"].encode(), C.byref(prob), C.byref(h)), self.lib)
        self.h = h

    def run(self, starts, objective, gtol, ftol, max_iter):
        """starts [n, dim] (NumPy) -> (x [n, dim], stats [n, 6], status [n]) as NumPy arrays"""
        import torch

        if self.h is None:
            raise _lib.EngineError("this Optimizer is closed")
        n = int(starts.shape[0])
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.float64)).to(dev)
            x = torch.empty((n, self.dim), dtype=torch.float64, device=dev)
            stats = torch.empty((n, 6), dtype=torch.float64, device=dev)
            status = torch.empty((n,), dtype=torch.int32, device=dev)
            opts = _lib.tda_optimize_options(C.sizeof(_lib.tda_optimize_options), int(max_iter), float(gtol), float(ftol))
            p = lambda t: C.c_void_p(t.data_ptr())
            _lib.check(self.lib.tda_optimizer_run(self.h, p(s), n, OBJECTIVES.index(objective), C.byref(opts), p(x), p(stats), p(status),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), self.lib)
            return x.cpu().numpy(), stats.cpu().numpy(), status.cpu().numpy()

    def close(self):
        if getattr(self, "h", None) is not None:
            self.lib.tda_optimizer_destroy(self.h)
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


_cache, _cache_lock, CACHE_SIZE = [], threading.Lock(), 4


def _optimizer_of(low, source_gradient, device):
    """the compiled optimiser of this description: the last CACHE_SIZE are kept, so that get_MAP, get_ML and repeated calls on one
    posterior compile once (a program takes a second or two to compile, a run over hundreds of starts milliseconds)"""
    kinds, loc, scale = _prior_components(low)
    key = (low["source"], bool(source_gradient), int(device), int(low["noise_kind"])) + tuple(
        np.ascontiguousarray(a).tobytes() for a in (low["data"], low["noise"], kinds, loc, scale))
    with _cache_lock:
        for i, (k, opt) in enumerate(_cache):
            if k == key:
                _cache.append(_cache.pop(i))
                return opt
        opt = Optimizer(low, source_gradient, device)
        _cache.append((key, opt))
        while len(_cache) > CACHE_SIZE:
            _cache.pop(0)[1].close()
        return opt


def _maximize_host(posterior, starts, objective, gtol, max_iter, method, scipy_options):
    """the reference's route: scipy over create_link, one start after the other"""
    from scipy.optimize import differential_evolution, minimize

    def negative(parameters):
        link = posterior.create_link(parameters)
        return -(link.posterior if objective == "posterior" else link.likelihood)

    n, d = starts.shape
    x, stats, status = np.empty((n, d)), np.full((n, 6), np.nan), np.empty(n, dtype=np.int32)
    for i in range(n):
        if method == "differential_evolution":
            res = differential_evolution(negative, **scipy_options)
        else:
            kw = dict(scipy_options)
            if method is None:  # scipy's own choice (BFGS): the tolerances of this call
                options = dict(kw.pop("options", {}))
                options.setdefault("gtol", gtol)
                if max_iter is not None:
                    options.setdefault("maxiter", int(max_iter))
                kw["options"] = options
            res = minimize(negative, starts[i], method=method, **kw)
        x[i] = np.asarray(res["x"], dtype=np.float64).reshape(d)
        link = posterior.create_link(x[i])
        jac = res.get("jac")
        stats[i] = (link.prior, link.likelihood, link.posterior if objective == "posterior" else link.likelihood,
                    np.nan if jac is None else float(np.max(np.abs(jac))), res.get("nit", np.nan), res.get("nfev", np.nan))
        if res.get("success", False):
            status[i] = 0
        elif "aximum number of iterations" in str(res.get("message", "")):
            status[i] = 2
        else:
            status[i] = 3
    return x, stats, status


def maximize(posterior, initial_parameters=None, n_starts=256, objective="posterior", gradient="auto", gtol=1e-5, ftol=0.0, max_iter=None, seed=0,
             backend="auto", device=0, method=None, **scipy_options):
    """Maxima of the log-posterior (objective='posterior') or of the log-likelihood alone ('likelihood': the prior and its
    support are ignored) from many starts.  `initial_parameters` is [d], [n, d] or a list of [d]; without it `n_starts` starts are
    drawn from the prior on the host, start i from the generator keyed by (seed, i).  Returns a MaximizeResult.

    Device route (a DeviceModel posterior, see the module's text): gradient='auto' takes the source's gradient when the source has
    every function that MALA needs and forward differences otherwise, 'source' / 'difference' insist; gtol ends a start at
    max_j |g_j| <= gtol, ftol > 0 at a step that gained <= ftol max(1, |f|), max_iter (default 200 d) bounds the iterations.
    Host route (everything else, or `method=` given: any scipy.optimize.minimize method, or 'differential_evolution'): scipy over
    posterior.create_link, one start after the other; further keywords go to scipy.  backend='hip' raises EngineError where the
    device route does not apply, backend='auto' warns (HostFallbackWarning) and takes the host route, backend='host' takes it silently."""
    from .api import HostFallbackWarning

    if objective not in OBJECTIVES:
        raise ValueError("objective must be 'posterior' or 'likelihood'")
    if gradient not in ("auto", "source", "difference"):
        raise ValueError("gradient must be 'auto', 'source' or 'difference'")
    if backend not in ("auto", "hip", "host"):
        raise ValueError("backend must be 'auto', 'hip' or 'host'")
    if not gtol >= 0.0 or not ftol >= 0.0 or (max_iter is not None and int(max_iter) < 0):
        raise ValueError("gtol, ftol and max_iter must be >= 0")
    low, why = (None, None) if backend == "host" else _device_problem(posterior)
    if method is not None and backend != "host":
        low, why = None, "method=%r selects scipy on the host" % (method,)
    if low is None and backend == "hip":
        raise _lib.EngineError("this posterior cannot be optimised on the HIP engine: %s" % why)
    if low is None and backend == "auto" and method is None:
        warnings.warn("tinyda_amd.maximize: running scipy on the host (one Python model call per function evaluation), not the HIP engine -- %s.  "
                      "backend='hip' turns this into an error, backend='host' silences it." % why, HostFallbackWarning, stacklevel=2)
    if low is not None and scipy_options:
        raise TypeError("maximize() on the device got unexpected keyword arguments %s (scipy's options apply with method=...)" % sorted(scipy_options))
    if initial_parameters is not None:
        starts = _given_starts(initial_parameters)
    else:
        starts = _draw_starts(posterior, low, int(n_starts) if n_starts is not None else 256 if low is not None else 1, seed)
    if low is None:
        x, stats, status = _maximize_host(posterior, starts, objective, gtol, max_iter, method, scipy_options)
        which = "host"
    else:
        d = int(low["prior_mean"].shape[0])
        if starts.shape[1] != d:
            raise ValueError("initial_parameters have %d entries, the prior has %d" % (starts.shape[1], d))
        source_gradient = _has_source_gradient(low) if gradient == "auto" else gradient == "source"
        x, stats, status = _optimizer_of(low, source_gradient, device).run(starts, objective, gtol, ftol, 200 * d if max_iter is None else int(max_iter))
        which = "hip"
    return MaximizeResult(x, stats[:, 2].copy(), stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 3].copy(), stats[:, 4].copy(), stats[:, 5].copy(),
                          status, which)


def _best_point(posterior, objective, kwargs):
    kwargs = dict(kwargs)
    kwargs.setdefault("n_starts", None)  # (256 on the device; on the host one start, as in the reference)
    if kwargs.get("method") is not None:
        kwargs.setdefault("backend", "host")
    res = maximize(posterior, objective=objective, **kwargs)
    if res.best is None:
        raise RuntimeError("no start ended at a finite %s (statuses: %s)" % (objective, sorted({STATUS_NAMES[s] for s in res.status})))
    return res.x[res.best].copy()


def get_MAP(posterior, **kwargs):
    """The maximum a posteriori estimate as a [d] array (utils.py:204-235): `maximize` from `initial_parameters` or from starts
    drawn from the prior, the best end returned.  `method=` (scipy's, or 'differential_evolution') selects the host route as in
    the reference, where further keywords go to scipy."""
    return _best_point(posterior, "posterior", kwargs)


def get_ML(posterior, **kwargs):
    """The maximum likelihood estimate as a [d] array (utils.py:238-269); see get_MAP."""
    return _best_point(posterior, "likelihood", kwargs)
