"""Gaussian log-likelihoods with the reference's API (tinyDA/distributions.py:203-449).

All are *unnormalised* (-1/2 r^T Sigma^-1 r).  `GaussianLogLike` is the reference's factory: a diagonal
covariance with equal entries becomes isotropic, a diagonal one diagonal, anything else dense
(distributions.py:237-243).  Each class also reports how the device engine should see it (`_lowering`).
`DeviceLogLike` (extension) is a log-likelihood given as HIP source, separable or coupling its outputs, for everything that is not Gaussian;
`DevicePrior` (extension) the same for a prior of independent components, and `JointPrior` lowers lists of scipy families
through it with the term library `csrc/tda_prior_families.h`.
"""
import os

import numpy as np

from . import _lib
from ._contract import SIG
from .models import _defines


def _is_diagonal(cov):
    return np.count_nonzero(cov - np.diag(np.diag(cov))) == 0


def _check_covariance(data, covariance):
    # same exceptions as distributions.py:227-235 / :370-378
    if not isinstance(covariance, np.ndarray) or covariance.ndim != 2:
        raise TypeError("Covariance must be a 2-D numpy array.")
    if covariance.shape[0] != data.shape[0]:
        raise ValueError("Dimensions of data and covariance do not match.")
    if covariance.shape[0] != covariance.shape[1]:
        raise ValueError("Covariance must be an NxN array.")


class DefaultGaussianLogLike:
    """Dense covariance; the inverse is formed once (distributions.py:280)."""

    def __init__(self, data, covariance):
        self.data = data
        self.cov = covariance
        self.cov_inverse = np.linalg.inv(covariance)

    def _residual(self, x):
        return x - self.data

    def loglike(self, x):
        r = self._residual(x)
        return -0.5 * np.linalg.multi_dot((r.T, self.cov_inverse, r))

    def grad_loglike(self, x):
        return np.dot(self.cov_inverse, -self._residual(x))

    def _lowering(self):
        return _lib.NOISE_DENSE, np.asarray(self.cov, dtype=np.float64)


class DiagonalGaussianLogLike(DefaultGaussianLogLike):
    def __init__(self, data, covariance):
        self.data = data
        self.cov = np.diag(covariance)

    def loglike(self, x):
        return -0.5 * (self._residual(x) ** 2 / self.cov).sum()

    def grad_loglike(self, x):
        return 1 / self.cov * -self._residual(x)

    def _lowering(self):
        return _lib.NOISE_DIAG, np.asarray(self.cov, dtype=np.float64)


class IsotropicGaussianLogLike(DefaultGaussianLogLike):
    def __init__(self, data, variance):
        self.data = data
        self.var = variance

    def loglike(self, x):
        return -0.5 * np.linalg.norm(self._residual(x)) ** 2 / self.var

    def grad_loglike(self, x):
        return 1 / self.var * -self._residual(x)

    def _lowering(self):
        return _lib.NOISE_ISO, np.array([float(self.var)])


class AdaptiveGaussianLogLike(DefaultGaussianLogLike):
    """Bias-corrected dense likelihood for the adaptive error model (distributions.py:332-449)."""

    def __init__(self, data, covariance):
        _check_covariance(data, covariance)
        super().__init__(data, covariance)
        self.bias = np.zeros(self.data.shape[0])

    def set_bias(self, mean_bias, covariance_bias):
        self.bias = mean_bias
        self.cov_bias = covariance_bias
        # the reference leaves the inverse untouched while every entry is below 1e-9 (:399-402)
        if not np.all(self.cov_bias < 1e-9):
            self.cov_inverse = np.linalg.inv(self.cov + self.cov_bias)

    def _residual(self, x):
        return x + self.bias - self.data

    def loglike_custom_bias(self, x, bias):
        r = x + bias - self.data
        return -0.5 * np.linalg.multi_dot((r.T, self.cov_inverse, r))

    def _lowering(self):
        return _lib.NOISE_ADAPTIVE, np.asarray(self.cov, dtype=np.float64)


def GaussianLogLike(data, covariance):
    """Factory with the reference's dispatch and error behaviour (distributions.py:203-243)."""
    _check_covariance(data, covariance)
    if _is_diagonal(covariance):
        if np.all(np.diag(covariance) == covariance[0, 0]):
            return IsotropicGaussianLogLike(data, covariance[0, 0])
        return DiagonalGaussianLogLike(data, covariance)
    return DefaultGaussianLogLike(data, covariance)


class DeviceLogLike:
    """A log-likelihood given as HIP source, separable or coupling its outputs (extension; the reference takes any object with `loglike`,
    posterior.py:95-108, and evaluates it in Python): log L(F) = sum_o term(F_o, y_o, p_o, o).  The source must define

        __device__ double tda_loglike_term(double f, double y, double p, int o);        // term o

    and may define its derivative with respect to the model output, which MALA needs as the sensitivity:

        __device__ double tda_loglike_term_grad(double f, double y, double p, int o);   // d term / d f

    `data` is y, `parameters` one value per output (a scale, an exposure, a censoring limit; ones when not given);
    constants shared by all outputs are literals in the source.  The functions are pure.  A term that is NaN or -inf
    rejects the proposal.  It is compiled into the program of the level's `DeviceModel`, so it lowers beside such a model only.

    A likelihood that couples outputs (correlated noise such as AR(1) residuals, a noise level integrated out, softmax counts,
    constraints between neighbouring outputs) defines the wave form INSTEAD of the term (a source with both is a ValueError);
    `coupled` is then true:

        __device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane);

    The 64 lanes of the chain's wave call it together, once per evaluation, and the engine sums the 64 return values.  `f` holds
    the model's outputs in LDS, complete before the call; `y` and `p` are the data and the parameters as given.  Every lane is
    called, lanes >= n_outputs too, and the call site is converged; how the work spreads over the lanes is the function's own
    business -- the idiom is `for (int o = lane; o < n_outputs; o += 64)`.  No barriers, no workspace, no writes.  Wave
    shuffles are legal: a likelihood that is a non-linear function of a reduction reduces with `__shfl_xor` and returns the value
    from one lane, 0 from the others.  The noise level integrated out, log L = -(a + m/2) log(b + 1/2 sum_o r_o^2):

        __device__ double tda_loglike_wave(const double* f, int n_outputs, const double* y, const double* p, int lane) {
          double s = 0.0;
          for (int o = lane; o < n_outputs; o += 64) { const double r = (f[o] - y[o]) / p[o]; s += r * r; }
          for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);       // every lane now holds the sum
          return lane == 0 ? -(2.0 + 0.5 * n_outputs) * log(1.5 + 0.5 * s) : 0.0;  // a = 2, b = 1.5
        }

    A NaN or -inf share rejects the proposal.  It lowers wherever the separable form does and is refused in the same places.
    Per chain the step program then holds 8 (m + 128 + TDA_WORKSPACE) bytes of LDS, the MALA program 8 (2 m + 128 +
    TDA_WORKSPACE) (+ 1 KiB beside `tda_gradient_wave`), at most 64 KiB.  Under MALA it needs

        __device__ void tda_loglike_grad_wave(const double* f, int n_outputs, const double* y, const double* p, double* sens, int lane);

    one call by the whole wave that writes d log L / d f_o for every output into `sens` (LDS, NaN before the call: an entry
    left unwritten makes the gradient NaN and rejects the proposal); `has_gradient` then refers to this function.

    `reference(x, data, parameters)`, if given, returns the vector of terms in NumPy (for a coupled likelihood a scalar or any
    array that sums to log L) and serves `loglike` on the host (host protocol, tests); `reference_gradient(x, data, parameters)`
    the vector of derivatives d log L / d F, which becomes `grad_loglike` (an attribute only then, so that the host MALA takes
    the exact-gradient branch)."""

    def __init__(self, source, data, parameters=None, reference=None, reference_gradient=None):
        self.source = str(source)
        self.data = np.atleast_1d(np.asarray(data, dtype=np.float64))
        self.parameters = (np.ones_like(self.data) if parameters is None
                           else np.atleast_1d(np.asarray(parameters, dtype=np.float64)))
        if self.data.ndim != 1 or self.parameters.shape != self.data.shape:
            raise ValueError("data and parameters must be vectors with one entry per model output")
        term = _defines(self.source, "tda_loglike_term")
        self.coupled = _defines(self.source, "tda_loglike_wave")
        if term and self.coupled:
            raise ValueError("the source defines both tda_loglike_term and tda_loglike_wave: a likelihood has one form")
        if not term and not self.coupled:
            raise ValueError("the source must define %s (or, for a likelihood that couples outputs, %s)" % (SIG["tda_loglike_term"], SIG["tda_loglike_wave"]))
        self.has_gradient = _defines(self.source, "tda_loglike_grad_wave" if self.coupled else "tda_loglike_term_grad")
        self.reference = reference
        self.reference_gradient = reference_gradient
        if reference_gradient is not None:
            self.grad_loglike = self._reference_gradient  # (an attribute only then: MALA.setup_proposal looks for it)

    def loglike(self, x):
        if self.reference is None:
            raise TypeError("this DeviceLogLike has no host reference implementation; run it with backend='hip'")
        return np.sum(self.reference(np.asarray(x, dtype=np.float64), self.data, self.parameters))

    def _reference_gradient(self, x):
        return np.asarray(self.reference_gradient(np.asarray(x, dtype=np.float64), self.data, self.parameters), dtype=np.float64)

    def _lowering(self):
        return _lib.NOISE_SOURCE, self.parameters


class DevicePrior:
    """A prior given as HIP source: independent components, or one that couples parameters (extension; the reference's JointPrior takes any
    scipy.stats.rv_continuous per parameter and evaluates it in Python, distributions.py:8-56):
    log p(theta) = sum_j term(theta_j, p_j, q_j, j).  The source must define

        __device__ double tda_logprior_term(double x, double p, double q, int j);       // term of parameter j

    `p` and `q` hold one value per parameter (a location and a scale, say; zeros / ones when not given) and are passed on as
    given; constants shared by all parameters are literals in the source.  The function is pure.  A term that is NaN or -inf
    (outside the support) rejects the proposal.  It is compiled into the programs of the levels' `DeviceModel`s, so it lowers
    beside such models only (all levels of a hierarchy share it).

    A prior that couples parameters (Cauchy-difference and total-variation priors, hierarchical priors, order constraints)
    defines the wave form INSTEAD of the term (a source with both is a ValueError); `coupled` is then true:

        __device__ double tda_logprior_wave(const double* theta, int dim, const double* p, const double* q, int lane);

    The 64 lanes of the chain's wave call it together, once per evaluation, and the engine sums the 64 return values.  `theta`
    is the proposal (entries at index >= dim are unspecified), `p` / `q` the arrays as given.  Every lane is called, lanes >= dim
    too; how the function spreads its terms over the lanes is its own business -- the idiom is
    `for (int j = lane; j < dim; j += 64)`.  It is pure: no barriers, no workspace, no writes.  A NaN or -inf share rejects
    the proposal.  It lowers wherever the separable form does.  Under MALA it needs

        __device__ double tda_logprior_grad(const double* theta, int dim, const double* p, const double* q, int j);  // d log p / d theta_j

    called by the lane that owns parameter j; `has_gradient` then refers to this function.  A proposal whose log-prior is -inf
    is rejected whatever it returns there.

    MALA needs the derivative of the term too, which the source may define:

        __device__ double tda_logprior_term_grad(double x, double p, double q, int j);  // d term / d x

    `has_gradient` says whether it does (comments do not count).  Outside the support the function may return anything: the
    term is -inf there and the proposal is rejected.  With it the prior lowers under MALA beside a single-level `DeviceModel`
    that has `tda_gradient` / `tda_gradient_wave`.

    `reference`, if given, is any object with `logpdf(theta)` (and optionally `rvs` / `ppf`) -- a `JointPrior`, say -- and
    serves the host protocol; `sample()` draws missing initial parameters through its `ppf`, or else from its
    `rvs(random_state=generator)`.  `reference_gradient(theta)`, if given, returns d log p / d theta in NumPy and becomes
    `grad_logpdf` (an attribute only then), which the host MALA uses in place of finite differences of `logpdf`.

    `DevicePrior.from_distributions(distributions)` builds one from frozen scipy.stats components of the families of
    csrc/tda_prior_families.h, gradient included: the route by which such priors reach MALA on the device."""

    def __init__(self, source, dim, p=None, q=None, reference=None, reference_gradient=None):
        self.source = str(source)
        self.dim = int(dim)
        if self.dim < 1:
            raise ValueError("dim must be >= 1")
        self.p = np.zeros(self.dim) if p is None else np.atleast_1d(np.asarray(p, dtype=np.float64))
        self.q = np.ones(self.dim) if q is None else np.atleast_1d(np.asarray(q, dtype=np.float64))
        if self.p.shape != (self.dim,) or self.q.shape != (self.dim,):
            raise ValueError("p and q must be vectors with one entry per parameter")
        if not (np.all(np.isfinite(self.p)) and np.all(np.isfinite(self.q))):
            raise ValueError("p and q must be finite")
        term = _defines(self.source, "tda_logprior_term")
        self.coupled = _defines(self.source, "tda_logprior_wave")
        if term and self.coupled:
            raise ValueError("the source defines both tda_logprior_term and tda_logprior_wave: a prior has one form")
        if not term and not self.coupled:
            raise ValueError("the source must define %s (or, for a prior that couples parameters, %s)" % (SIG["tda_logprior_term"], SIG["tda_logprior_wave"]))
        self.has_gradient = _defines(self.source, "tda_logprior_grad" if self.coupled else "tda_logprior_term_grad")
        self.reference = reference
        self.reference_gradient = reference_gradient
        if reference_gradient is not None:
            self.grad_logpdf = self._reference_gradient  # (an attribute only then: proposals._grad_log_prior looks for it)

    @classmethod
    def from_distributions(cls, distributions):
        """The prior of independent frozen scipy.stats components of the families of csrc/tda_prior_families.h as a DevicePrior:
        the source is the generated tables plus the shipped library (term and gradient), p / q are loc / scale, `reference` is
        JointPrior(distributions) and `reference_gradient` the exact NumPy gradient of the same formulas.  ValueError names the
        first component that is outside the families or does not fit the tables."""
        distributions = list(distributions)
        rows = [_family_component(dist) for dist in distributions]
        for j, row in enumerate(rows):
            if row is None:
                raise ValueError("component %d (%s) is not a frozen scipy.stats distribution of the families of csrc/tda_prior_families.h "
                                 "(%s) with finite shape parameters, or its constant is not finite"
                                 % (j, getattr(getattr(distributions[j], "dist", None), "name", type(distributions[j]).__name__),
                                    ", ".join(name for name, _ in _FAMILIES)))
        if not rows:
            raise ValueError("no components")
        return cls(_family_prologue(rows) + family_library_source(), len(rows), [r[4] for r in rows], [r[5] for r in rows],
                   reference=JointPrior(distributions), reference_gradient=lambda theta: family_gradient(rows, theta))

    def _host(self, name):
        fn = getattr(self.reference, name, None)
        if fn is None:
            raise TypeError("this DevicePrior has no host reference implementation of %s; run it with backend='hip'%s"
                            % (name, " and initial_parameters" if name == "rvs" else ""))
        return fn

    def logpdf(self, x):
        return self._host("logpdf")(x)

    def rvs(self, *args, **kwargs):
        return self._host("rvs")(*args, **kwargs)

    def ppf(self, x):
        return self._host("ppf")(x)

    def _reference_gradient(self, x):
        return np.asarray(self.reference_gradient(np.asarray(x, dtype=np.float64)), dtype=np.float64)

    def _source_lowering(self):
        """(kinds, p, q, source) with every kind = PRIOR_SOURCE: what Posterior._lowering hands to the engine"""
        return np.full(self.dim, _lib.PRIOR_SOURCE, dtype=np.int32), self.p, self.q, self.source


# the scipy.stats families of csrc/tda_prior_families.h, in the order of its ids, with the number of shape parameters
_FAMILIES = (("norm", 0), ("uniform", 0), ("lognorm", 1), ("gamma", 1), ("invgamma", 1), ("beta", 2), ("expon", 0), ("halfnorm", 0),
             ("laplace", 0), ("cauchy", 0), ("t", 1), ("truncnorm", 2), ("weibull_min", 1))
_FAMILY_ID = {name: i for i, (name, _) in enumerate(_FAMILIES)}


def _log_gauss_mass(a, b):
    """log(Phi(b) - Phi(a)) for a < b, to a few roundings of its own magnitude wherever the window lies and however narrow it is"""
    from scipy.special import erf, log_ndtr

    if a <= 0.0 <= b:  # the window holds 0: the two halves add, nothing cancels (log_ndtr of both bounds would sit near log 0.5)
        return float(np.log(0.5 * (erf(b / np.sqrt(2.0)) - erf(a / np.sqrt(2.0)))))
    if a > 0.0:
        a, b = -b, -a
    # a < b < 0.  w = log(phi(b) / phi(a)) bounds log(Phi(b) / Phi(a)) from below (the hazard phi / Phi of a negative t is above |t|)
    w = 0.5 * (b - a) * -(a + b)
    if w < 0.5:
        # a narrow window: the difference of the two tails cancels, so integrate phi(t) / phi(a) = exp(-s (a + s / 2)), t = a + s,
        # over it (entire, rising from 1 to e^w < 1.65 over a width below 1: 16 Gauss-Legendre nodes leave nothing above rounding)
        t, wt = np.polynomial.legendre.leggauss(16)
        s = 0.5 * (b - a) * (t + 1.0)
        return float(-0.5 * a * a - 0.5 * np.log(2.0 * np.pi) + np.log(0.5 * (b - a) * np.sum(wt * np.exp(-s * (a + 0.5 * s)))))
    hi, lo = log_ndtr(b), log_ndtr(a)  # lo - hi <= -w: its rounding stays a rounding of the result
    return float(hi + np.log(-np.expm1(lo - hi)))


def _log_gamma_half_step(x):
    """log(Gamma(x + 1/2) / Gamma(x)): the difference of two gammaln loses |gammaln(x)| eps, so from x = 100 on the asymptotic
    series takes over (its first dropped term is below 2e-21 there)"""
    from scipy.special import gammaln

    if x < 100.0:
        return float(gammaln(x + 0.5) - gammaln(x))
    r = 1.0 / (x * x)
    return 0.5 * np.log(x) - (1.0 / 8.0 - (1.0 / 192.0 - (1.0 / 640.0 - 17.0 / 14336.0 * r) * r) * r) / x


def _family_constant(name, shapes):
    """the part of the family's log-density at z that does not depend on z (the term library adds it, minus log(scale))"""
    from scipy.special import betaln, gammaln

    if name == "norm":
        return -0.5 * np.log(2.0 * np.pi)
    if name == "lognorm":
        return -np.log(shapes[0]) - 0.5 * np.log(2.0 * np.pi)
    if name in ("gamma", "invgamma"):
        return -float(gammaln(shapes[0]))
    if name == "beta":
        return -float(betaln(shapes[0], shapes[1]))
    if name == "halfnorm":
        return 0.5 * np.log(2.0 / np.pi)
    if name == "laplace":
        return -np.log(2.0)
    if name == "cauchy":
        return -np.log(np.pi)
    if name == "t":
        nu = shapes[0]
        return _log_gamma_half_step(0.5 * nu) - 0.5 * np.log(nu * np.pi)
    if name == "truncnorm":
        return -0.5 * np.log(2.0 * np.pi) - _log_gauss_mass(shapes[0], shapes[1])
    if name == "weibull_min":
        return np.log(shapes[0])
    return 0.0  # uniform, expon


def _family_component(dist):
    """(family id, a, b, c, loc, scale) of a frozen scipy.stats distribution of one of _FAMILIES, else None"""
    import scipy.stats as st

    gen = getattr(dist, "dist", None)
    name = getattr(gen, "name", None)
    if not isinstance(gen, st.rv_continuous) or name not in _FAMILY_ID or getattr(st, name, None).__class__ is not gen.__class__:
        return None
    try:  # (_parse_args and _argcheck are scipy's own helpers: where a release lacks them the component stays host-only)
        shapes, loc, scale = gen._parse_args(*dist.args, **dist.kwds)
        shapes = tuple(float(s) for s in shapes)
        loc, scale = float(loc), float(scale)
        valid = len(shapes) == _FAMILIES[_FAMILY_ID[name]][1] and bool(np.all(gen._argcheck(*shapes)))
    except (AttributeError, TypeError, ValueError):
        return None
    if not (valid and np.all(np.isfinite(shapes + (loc, scale))) and scale > 0.0):
        return None
    c = float(_family_constant(name, shapes)) - np.log(scale)
    if not np.isfinite(c):
        return None
    return (_FAMILY_ID[name],) + (shapes + (0.0, 0.0))[:2] + (c, loc, scale)


def _family_prologue(rows):
    """the tables that csrc/tda_prior_families.h reads, one row (family id, a, b, c) per parameter; the numbers are written as
    exact literals (repr round-trips a double)"""
    n = len(rows)

    def table(ctype, name, col, fmt):
        return "static __device__ const %s %s[%d] = {%s};\n" % (ctype, name, n, ", ".join(fmt(r[col]) for r in rows))

    return ("#define TDA_PRIOR_DIM %d\n" % n + table("int", "tda_prior_family", 0, lambda v: "%d" % v)
            + table("double", "tda_prior_a", 1, lambda v: repr(float(v))) + table("double", "tda_prior_b", 2, lambda v: repr(float(v)))
            + table("double", "tda_prior_c", 3, lambda v: repr(float(v))))


def family_gradient(rows, theta):
    """d log p / d theta of the rows (family id, a, b, c, loc, scale) of _family_component at theta[..., dim]: the NumPy twin of
    tda_logprior_term_grad in csrc/tda_prior_families.h, g'(z) / scale with z = (theta - loc) / scale, the same formulas in the
    same order of operations.  Outside a support the value is unspecified (as on the device): the density is -inf there."""
    theta = np.asarray(theta, dtype=np.float64)
    fam = np.array([r[0] for r in rows])
    a, b = np.array([r[1] for r in rows], dtype=np.float64), np.array([r[2] for r in rows], dtype=np.float64)
    loc, scale = np.array([r[4] for r in rows], dtype=np.float64), np.array([r[5] for r in rows], dtype=np.float64)
    z = (theta - loc) / scale
    g = np.full(z.shape, np.nan)
    with np.errstate(all="ignore"):
        for f in np.unique(fam):
            k = fam == f
            zz, aa, bb = z[..., k], a[k], b[k]
            if f in (0, 7, 11):
                v = -zz
            elif f == 1:
                v = np.zeros_like(zz)
            elif f == 2:
                v = (-1.0 - np.log(zz) / (aa * aa)) / zz
            elif f == 3:
                v = (aa - 1.0) / zz - 1.0
            elif f == 4:
                v = (1.0 / zz - (aa + 1.0)) / zz
            elif f == 5:
                v = (aa - 1.0) / zz - (bb - 1.0) / (1.0 - zz)
            elif f == 6:
                v = -np.ones_like(zz)
            elif f == 8:
                v = -np.sign(zz)
            elif f == 9:
                v = -2.0 * zz / (1.0 + zz * zz)
            elif f == 10:
                v = -(aa + 1.0) * zz / (aa + zz * zz)
            else:
                v = ((aa - 1.0) - aa * np.exp(aa * np.log(zz))) / zz
            g[..., k] = v
    return g / scale


def family_library_source():
    """the text of the term library shipped with the package (csrc/tda_prior_families.h)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "tda_prior_families.h")) as fh:
        return fh.read()


class JointPrior:
    """A list of independent scalar priors, one per parameter, in parameter order (tinyDA/distributions.py:8-100)."""

    def __init__(self, distributions):
        self.distributions = distributions
        self.dim = len(distributions)

    def logpdf(self, x):
        # independent components: the joint log-density is the sum of the marginals, accumulated in parameter order
        total = 0.0
        for dist, xi in zip(self.distributions, np.asarray(x).reshape(-1)):
            total = total + dist.logpdf(xi)
        return total

    def rvs(self, n_samples=1):
        # one column per component, drawn in parameter order (the order fixes which variates of the global stream go where)
        draws = np.column_stack([dist.rvs(size=n_samples) for dist in self.distributions])
        return draws[0] if n_samples == 1 else draws

    def ppf(self, x):
        # quantile transform of a [n, dim] array of uniforms (Latin hypercube archives), column by column
        return np.column_stack([dist.ppf(col) for dist, col in zip(self.distributions, np.asarray(x).T)])

    def _lowering(self):
        """(kinds, loc, scale) when every component is a frozen scipy norm or uniform, else None (then _source_lowering may
        still lower the list)."""
        kinds, loc, scale = [], [], []
        for dist in self.distributions:
            name = getattr(getattr(dist, "dist", None), "name", None)
            if name not in ("norm", "uniform"):
                return None
            _, l, s = dist.dist._parse_args(*dist.args, **dist.kwds)
            kinds.append(0 if name == "norm" else 1)
            loc.append(float(l))
            scale.append(float(s))
        return np.array(kinds, dtype=np.int32), np.array(loc), np.array(scale)

    def _source_lowering(self):
        """(kinds, loc, scale, source) with every kind = PRIOR_SOURCE when all components are frozen scipy distributions of the
        families of csrc/tda_prior_families.h -- the source is that library behind a prologue with the components' tables --
        else None (a non-frozen object, an unlisted or discrete family: host protocol).  Posterior._lowering asks for it when
        _lowering() has declined, so lists of norm / uniform alone never come here."""
        rows = [_family_component(dist) for dist in self.distributions]
        if not rows or any(r is None for r in rows):
            return None
        return (np.full(len(rows), _lib.PRIOR_SOURCE, dtype=np.int32), np.array([r[4] for r in rows]), np.array([r[5] for r in rows]),
                _family_prologue(rows) + family_library_source())
