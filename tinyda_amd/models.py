"""Forward models the device engine can run fused (declared, not opaque Python).

tinyDA's model protocol is "callable theta -> ndarray or (ndarray, qoi)" (posterior.py:95-101).
These classes honour it on the host and additionally expose what the HIP kernels need.
"""
import re

import numpy as np

from ._contract import QOI_SIG, SIG


class LinearModel:
    """F(theta) = A theta (+ b).  All BASELINE.json configurations use linear forward models."""

    def __init__(self, A, b=None):
        self.A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        if self.A.ndim != 2:
            raise ValueError("A must be a 2-D array (observations x parameters)")
        self.b = None if b is None else np.ascontiguousarray(np.asarray(b, dtype=np.float64))
        if self.b is not None and self.b.shape != (self.A.shape[0],):
            raise ValueError("b must have one entry per observation")

    def __call__(self, parameters):
        out = self.A @ np.asarray(parameters, dtype=np.float64)
        return out if self.b is None else out + self.b

    def gradient(self, parameters, sensitivity):
        """J^T s, the method MALA looks for on a model (proposal.py:938-943, :996-998)."""
        return self.A.T @ np.asarray(sensitivity, dtype=np.float64)


class Rosenbrock:
    """The reference's Rosenbrock example (examples/MALA Rosenbrock.ipynb) as a d-parameter chain with one
    scalar output: F(theta) = [ sum_i (a - theta_i)^2 + b (theta_{i+1} - theta_i^2)^2 ].  With data [0] and unit
    variance the log-likelihood is -F^2/2 (BASELINE config 4 uses d = 32, a = 1, b = 10)."""

    def __init__(self, a=1.0, b=10.0):
        self.a, self.b = float(a), float(b)

    def __call__(self, parameters):
        t = np.asarray(parameters, dtype=np.float64)
        return np.array([np.sum((self.a - t[:-1]) ** 2 + self.b * (t[1:] - t[:-1] ** 2) ** 2)])


class DeviceModel:
    """A (possibly non-linear) forward model given as HIP source, compiled at run time into the fused step kernel
    (extension; tinyDA only knows Python callables).  The source must define

        __device__ double tda_forward(const double* theta, int dim, int o);   // output o of F(theta), 0 <= o < n_outputs

    or, for a model whose outputs all come from one solve (an integrator, a time-stepping scheme, a tridiagonal solve), the
    wave-cooperative form, which the 64 lanes of the chain's wave call together, once per evaluation (used when both are there):

        #define TDA_WORKSPACE 3072   // optional: doubles of LDS scratch of the chain's own, handed over as `work` (default: none, null)
        __device__ void tda_forward_wave(const double* theta, int dim, double* out, int n_outputs, double* work, int lane);
        // theta, out: LDS; out is NaN before the call and an entry left unwritten rejects the proposal; __syncthreads() inside
        // is legal and a wave barrier.  LDS per chain = 8 (n_outputs + 128 + TDA_WORKSPACE) bytes, at most 64 KiB.

    and may define the model's vector-Jacobian product, which MALA runs on (the device counterpart of the reference's
    `model.gradient(parameters, sensitivity)`, proposal.py:996-998):

        __device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, int n_outputs, int j);
        // (J(theta)^T sensitivity)_j, 0 <= j < dim

    or that in the wave form, one call for all parameters (grad: LDS, 128 doubles, zero before the call; `work` is what
    tda_forward_wave left at the same theta):

        __device__ void tda_gradient_wave(const double* theta, int dim, const double* sensitivity, int n_outputs, double* grad, double* work, int lane);

    `has_forward_wave` / `has_gradient_wave` say whether the source defines the wave forms, `has_gradient` whether it defines
    either gradient (comments do not count).

    With `n_qoi` > 0 the source also defines the model's quantity of interest (the reference's models return it beside the
    output, posterior.py:97-101), in one of two forms; either goes with either form of the model, and the wave form is used when
    both are there (`has_qoi` / `has_qoi_wave`):

        // quantity k of n_qoi; f: the model's complete outputs at theta (LDS); the lanes stride over k
        __device__ double tda_qoi(const double* theta, int dim, const double* f, int n_outputs, int k);
        // all quantities in one call by the chain's 64 lanes (converged call site; __syncthreads() legal); qoi: LDS, n_qoi doubles,
        // NaN before the call (an entry left unwritten stays NaN); work: what tda_forward_wave left at the same theta (null
        // without TDA_WORKSPACE) -- the solver's state, which is where a quantity of interest usually lives
        __device__ void tda_qoi_wave(const double* theta, int dim, const double* f, int n_outputs, double* qoi, int n_qoi, double* work, int lane);

    A NaN quantity is data, not a rejection.  The step kernels never call these functions: outputs and quantities of the recorded
    rows are produced after the run, when somebody asks (get_samples(..., "model_output" | "qoi"), to_inference_data,
    DeviceChain.model_output / .qoi), by replaying the model over the records on the device (tinyda_amd/replay.py); `evaluate`
    is the same at any parameters.  LDS per chain there: 8 (n_outputs + n_qoi + 128 + TDA_WORKSPACE) bytes, at most 64 KiB.

    `reference`, if given, is a Python callable theta -> outputs used when the model is called on the host (host
    protocol, tests); without it the model only runs on the device.  `reference_gradient(theta, sensitivity)`, if
    given, becomes the model's `gradient` method, so the host MALA takes the exact-gradient branch (finite differences
    otherwise).  `reference_qoi(theta, output) -> n_qoi values`, if given, makes the host call return `(output, qoi)`, the
    reference's model protocol, so the host protocol records the quantity too."""

    def __init__(self, source, n_outputs, n_qoi=0, reference=None, reference_gradient=None, reference_qoi=None):
        self.source = str(source)
        self.n_outputs = int(n_outputs)
        self.n_qoi = int(n_qoi)
        self.reference = reference
        self.reference_qoi = reference_qoi
        self.has_qoi_wave = _defines(self.source, "tda_qoi_wave")
        self.has_qoi = self.has_qoi_wave or _defines(self.source, "tda_qoi")
        if self.n_qoi < 0:
            raise ValueError("n_qoi must be >= 0")
        if self.n_qoi > 0 and not self.has_qoi:
            raise ValueError("n_qoi = %d: the source must define %s or %s" % (self.n_qoi, QOI_SIG["tda_qoi"], QOI_SIG["tda_qoi_wave"]))
        if self.n_qoi == 0 and self.has_qoi:
            raise ValueError("the source defines %s: give n_qoi, the number of quantities"
                             % QOI_SIG["tda_qoi_wave" if self.has_qoi_wave else "tda_qoi"])
        self.has_forward_wave = _defines(self.source, "tda_forward_wave")
        self.has_gradient_wave = _defines(self.source, "tda_gradient_wave")
        if not (self.has_forward_wave or _defines(self.source, "tda_forward")):
            raise ValueError("the source must define %s or %s" % (SIG["tda_forward"], SIG["tda_forward_wave"]))
        self.has_gradient = self.has_gradient_wave or _defines(self.source, "tda_gradient")
        self.reference_gradient = reference_gradient
        if reference_gradient is not None:
            self.gradient = self._reference_gradient  # (an attribute only then: MALA.setup_proposal looks for it)

    def _reference_gradient(self, parameters, sensitivity):
        return np.asarray(self.reference_gradient(np.asarray(parameters, dtype=np.float64), np.asarray(sensitivity, dtype=np.float64)),
                          dtype=np.float64)

    def __call__(self, parameters):
        if self.reference is None:
            raise TypeError("this DeviceModel has no host reference implementation; run it with backend='hip'")
        theta = np.asarray(parameters, dtype=np.float64)
        out = np.atleast_1d(np.asarray(self.reference(theta), dtype=np.float64))
        if self.reference_qoi is None:
            return out
        return out, np.atleast_1d(np.asarray(self.reference_qoi(theta, out), dtype=np.float64))

    def __getstate__(self):  # (copies and pickles leave the compiled replay programs behind: handles of this process)
        return {k: v for k, v in self.__dict__.items() if k != "_replays"}

    def evaluate(self, thetas, device=0):
        """F at every row of `thetas` [n, dim] on the device: outputs [n, n_outputs], or (outputs, qoi [n, n_qoi]) when the model
        has a quantity of interest -- the posterior predictive at any parameters.  (A replay of one row of n chains.)"""
        from .replay import evaluate

        return evaluate(self, thetas, device)


_TOKEN = re.compile(r"""//[^\n]*|/\*.*?(?:\*/|\Z)|"(?:\\.?|[^"\\])*(?:"|\Z)|'(?:\\.?|[^'\\])*(?:'|\Z)|([A-Za-z0-9_]+)""", re.S)


def _defines(source, name):
    """Does the HIP source use the identifier `name` outside // and /* */ comments, string literals and character literals?  The
    engine's own rule (source_defines in csrc/tda_user_build.h, token for token: an unterminated comment or literal runs to the end
    of the text), so that what DeviceModel, DeviceLogLike and DevicePrior report is what the engine compiles."""
    return any(mt.group(1) == name for mt in _TOKEN.finditer(source))


class BatchedModel:
    """An arbitrary host forward model evaluated for ALL chains at once (extension; tinyDA calls the model once per chain
    and step, posterior.py:95-96).  `fn` maps an (n_chains, dim) array of parameters to an (n_chains, n_outputs) array of
    model outputs -- a vectorised NumPy function, a batched solver, a remote service.  On the device path the engine hands
    it each step's proposals in one call and keeps proposals, log-densities, accept test, adaptation and records on the
    GPU; called with a single parameter vector it honours the reference's model protocol.

    inplace=True: `fn(parameters, out)` writes the outputs into `out` (the engine's page-locked staging buffer) instead
    of returning a new array."""

    def __init__(self, fn, n_outputs, inplace=False):
        self.fn = fn
        self.n_outputs = int(n_outputs)
        self.inplace = bool(inplace)

    def batch(self, parameters, out=None):
        parameters = np.asarray(parameters, dtype=np.float64)
        if not self.inplace:
            res = np.asarray(self.fn(parameters), dtype=np.float64)
            if out is None:
                return res
            if res.shape != out.shape:
                raise ValueError("the batched model returned shape %s, expected %s" % (res.shape, out.shape))
            out[...] = res
            return out
        if out is None:
            out = np.empty((parameters.shape[0], self.n_outputs))
        self.fn(parameters, out)
        return out

    single = None  # optional one-vector form of the same model (set when a plain callable was wrapped)

    def __call__(self, parameters):
        if self.single is not None:
            return self.single(parameters)
        return self.batch(np.asarray(parameters, dtype=np.float64)[None, :])[0]
