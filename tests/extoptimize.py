"""What the optimiser's tests share (tests/test_optimize.py on the CPU, tests/test_gpu_optimize.py on the device): a NumPy twin of
the algorithm of tda_user_maximize with the same constants, NumPy twins of the posteriors (log-prior, log-likelihood and the
exact gradient of either objective), the closed-form mode of a linear-Gaussian posterior with the bound that a gradient test
implies, the bound of a forward-difference gradient, and the cases themselves -- every GPU case is built here, so that the CPU
test can run the twin over the same starts."""
import numpy as np
import scipy.stats as st

from . import extloglike as xl
from . import extloglikewave as xlw
from . import extmodel as xm
from . import extprior as xp
from . import extpriorwave as xpw
from . import extwave as xw

HISTORY, HALVINGS, ARMIJO, EPS, FLOOR = 8, 40, 1e-4, 2.0 ** -52, 64.0
CONVERGED_GRADIENT, CONVERGED_VALUE, MAX_ITER, LINESEARCH_FAILED, INFEASIBLE_START, NONFINITE_GRADIENT = range(6)
DENSITY_RTOL = 1e-10  # the project's density bar

LINEAR_SRC = r"""
__device__ __forceinline__ double lin_a(int o, int j) { return 0.02 * (((o * 7 + j * 13 + o * j) % 17) - 8); }
__device__ double tda_forward(const double* theta, int dim, int o) {
  double s = 0.0;
  for (int j = 0; j < dim; ++j) s += lin_a(o, j) * theta[j];
  return s;
}
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int m, int j) {
  double g = 0.0;
  for (int o = 0; o < m; ++o) g += sens[o] * lin_a(o, j);
  return g;
}
"""
TWO_MODES_SRC = r"""
__device__ double tda_forward(const double* theta, int dim, int o) { return theta[0] * theta[0] + theta[1]; }
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int m, int j) { return j == 0 ? 2.0 * theta[0] * sens[0] : sens[0]; }
"""


def linear_matrix(m, d):
    o, j = np.arange(m)[:, None], np.arange(d)[None, :]
    return 0.02 * (((o * 7 + j * 13 + o * j) % 17) - 8)


def without_gradient(src):
    """a model source cut before its tda_gradient"""
    return src[:src.index("__device__ double tda_gradient")]


# ---- posteriors in NumPy ----------------------------------------------------------------------------------------------------------------
class Twin:
    """log-prior, log-likelihood and exact gradients of one posterior from its parts (all for one parameter vector)"""

    def __init__(self, forward, vjp, loglike, loglike_grad, logprior, logprior_grad):
        self.forward, self.vjp, self.loglike, self.loglike_grad, self.logprior, self.logprior_grad = forward, vjp, loglike, loglike_grad, logprior, logprior_grad

    def evaluate(self, x):
        with np.errstate(all="ignore"):
            return float(self.logprior(x)), float(self.loglike(self.forward(x)))

    def value(self, x, objective="posterior"):
        lp, ll = self.evaluate(x)
        return lp + ll if objective == "posterior" else ll

    def gradient(self, x, objective="posterior"):
        with np.errstate(all="ignore"):
            g = self.vjp(x, self.loglike_grad(self.forward(x)))
            return g + self.logprior_grad(x) if objective == "posterior" else g

    def magnitude(self, x):
        """the size of what the densities are summed from is not known for every part: |log-prior| + |log-likelihood| and 1"""
        lp, ll = self.evaluate(x)
        return 1.0 + abs(lp) + abs(ll)


def gauss_loglike(y, var):
    """isotropic (scalar var) or diagonal Gaussian noise, unnormalised as GaussianLogLike is"""
    var = np.asarray(var, dtype=float)
    return (lambda F: -0.5 * np.sum((F - y) ** 2 / var)), (lambda F: (y - F) / var)


def gauss_prior(mean, var):
    mean, var = np.asarray(mean, dtype=float), np.asarray(var, dtype=float)
    const = mean.shape[0] * np.log(2.0 * np.pi) + np.sum(np.log(var))
    return (lambda x: -0.5 * (const + np.sum((x - mean) ** 2 / var))), (lambda x: (mean - x) / var)


def extmodel_parts(m, nan_above=None):
    return (lambda x: xm.np_forward(x, m, nan_above)[0]), (lambda x, s: xm.np_vjp(x, s)[0])


def ring_parts(m):
    return (lambda x: xw.np_forward(x, m)[0]), (lambda x, s: xw.np_vjp(x, s)[0])


# ---- the algorithm --------------------------------------------------------------------------------------------------------------------
def difference_gradient(value, x, f0):
    """forward differences with h_j = 2^-26 max(1, |x_j|), backward where the forward point is not finite: (g, evaluations, ok)"""
    g, n, ok = np.zeros_like(x), 0, True
    for j in range(x.shape[0]):
        h = (x[j] + 2.0 ** -26 * max(1.0, abs(x[j]))) - x[j]
        e = np.zeros_like(x)
        e[j] = h
        fj = value(x + e)
        n += 1
        g[j] = (fj - f0) / h
        if not np.isfinite(fj):
            fj = value(x - e)
            n += 1
            g[j] = (f0 - fj) / h
            ok = ok and np.isfinite(fj)
    return g, n, ok


def maximize_twin(twin, x0, objective="posterior", difference=False, gtol=1e-5, ftol=0.0, max_iter=None):
    """tda_user_maximize for one start, statement by statement: dict(x, logprior, loglike, value, grad_norm, iterations, evaluations, status)"""
    x = np.array(x0, dtype=float)
    d = x.shape[0]
    max_iter = 200 * d if max_iter is None else max_iter
    value = lambda z: twin.value(z, objective)
    evals = [1]

    def grad(z, fz):
        if not difference:
            return twin.gradient(z, objective), True
        g, n, ok = difference_gradient(value, z, fz)
        evals[0] += n
        return g, ok

    f = value(x)
    status, g, gmax, gain, gamma, pairs, iters = -1, np.zeros(d), np.nan, 0.0, 1.0, [], 0
    if not np.isfinite(f):
        status = INFEASIBLE_START
    else:
        g, ok = grad(x, f)
        gmax = np.max(np.abs(g)) if np.all(np.isfinite(g)) else np.nan
        if not ok or not np.all(np.isfinite(g)):
            status = NONFINITE_GRADIENT
    for it in range(max_iter + 1):
        if status >= 0:
            break
        if gmax <= gtol:
            status = CONVERGED_GRADIENT
            break
        if it > 0 and ftol > 0.0 and gain <= ftol * max(1.0, abs(f)):
            status = CONVERGED_VALUE
            break
        if it == max_iter:
            status = MAX_ITER
            break
        p, al = g.copy(), []
        for s, y, rho in reversed(pairs):
            a = rho * np.dot(s, p)
            al.append(a)
            p = p - a * y
        if pairs:
            p = p * gamma
        for (s, y, rho), a in zip(pairs, reversed(al)):
            p = p + s * (a - rho * np.dot(y, p))
        gtp = np.dot(g, p)
        if pairs and not (gtp > 0.0 and np.isfinite(gtp)):
            pairs = []
        accepted, gn = False, None
        for attempt in range(2):
            if accepted:
                break
            if attempt == 1:
                if not pairs:
                    break
                pairs = []
            if not pairs:
                gg = np.dot(g, g)
                scale = 1.0 / np.sqrt(gg) if gg > 1.0 else 1.0
                p, gtp = g * scale, gg * scale
            t = 1.0
            for _ in range(HALVINGS + 1):
                xn = x + t * p
                fn = value(xn)
                evals[0] += 1
                if np.isfinite(fn) and fn >= f + ARMIJO * t * gtp:
                    accepted, gn = True, None
                    break
                if np.isfinite(fn) and abs(fn - f) <= FLOOR * EPS * max(1.0, abs(f)):  # values at their rounding: the slope decides
                    gn, ok = grad(xn, fn)
                    slope = np.dot(gn, p)
                    if ok and -(1.0 - 2.0 * ARMIJO) * gtp <= slope <= 0.9 * gtp:
                        accepted = True
                        break
                    gn = None
                t *= 0.5
        if not accepted:
            status = LINESEARCH_FAILED
            continue
        if gn is None:
            gn, ok = grad(xn, fn)
        s, y = xn - x, g - gn
        sy, yy = np.dot(s, y), np.dot(y, y)
        gain, x, f, g = fn - f, xn, fn, gn
        iters += 1
        if not ok or not np.all(np.isfinite(g)):
            gmax, status = np.nan, NONFINITE_GRADIENT
            continue
        gmax = np.max(np.abs(g))
        if sy > EPS * yy:
            pairs = (pairs + [(s, y, 1.0 / sy)])[-HISTORY:]
            gamma = sy / yy
    lp, ll = twin.evaluate(x)
    return dict(x=x, logprior=lp, loglike=ll, value=f, grad_norm=gmax, iterations=iters, evaluations=evals[0], status=status)


def run_twin(case):
    """the twin over every start of a case: a list of maximize_twin's results"""
    return [maximize_twin(case["twin"], x0, case.get("objective", "posterior"), case.get("difference", False), case["gtol"]) for x0 in case["starts"]]


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def closed_form_mode(A, y, noise_var, prior_mean, prior_var):
    """mode and negative Hessian of a linear-Gaussian posterior with diagonal noise and prior: (x_hat, H)"""
    w = 1.0 / (np.zeros(A.shape[0]) + noise_var)
    H = A.T @ (w[:, None] * A) + np.diag(1.0 / np.asarray(prior_var, dtype=float))
    return np.linalg.solve(H, A.T @ (w * y) + prior_mean / prior_var), H


def gradient_test_bound(H, gtol):
    """|x - x_hat|_2 where max_j |g_j| <= gtol and g = -H (x - x_hat): |x - x_hat|_2 <= |g|_2 / lambda_min(H) <= sqrt(d) gtol / lambda_min(H)"""
    return np.sqrt(H.shape[0]) * gtol / np.linalg.eigvalsh(H)[0]


def hessian_diagonal(twin, x, objective="posterior", delta=1e-5):
    """d^2 f / d x_j^2 by central differences of the exact gradient (relative error delta^2, far below what the bound needs)"""
    out = np.empty_like(x)
    for j in range(x.shape[0]):
        e = np.zeros_like(x)
        e[j] = delta * max(1.0, abs(x[j]))
        out[j] = (twin.gradient(x + e, objective)[j] - twin.gradient(x - e, objective)[j]) / (2.0 * e[j])
    return out


def difference_bound(twin, x, gtol, objective="posterior"):
    """the exact gradient where the forward-difference gradient passed the test: its truncation h / 2 max_j |H_jj| and the rounding
    of two objective values over h, 2 eps |f| / h, with the smallest step h = 2^-26 max(1, |x_j|)"""
    h = 2.0 ** -26 * np.maximum(1.0, np.abs(x))
    return gtol + 0.5 * np.max(h) * np.max(np.abs(hessian_diagonal(twin, x, objective))) + 2.0 * EPS * abs(twin.value(x, objective)) / np.min(h)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
CLOSED_FORM_SHAPES = [(1, 1, 3), (5, 70, 19), (64, 130, 7), (65, 70, 5), (128, 64, 3)]


def closed_form_case(d, m, n, noise):
    """a linear source of the tests' own under a diagonal Gaussian prior; noise 'iso' or 'diag'"""
    import tinyda_amd as tda

    rng = np.random.default_rng(1000 * d + m)
    A = linear_matrix(m, d)
    truth = 0.5 * rng.standard_normal(d)
    var = 0.25 if noise == "iso" else 0.2 + 0.3 * rng.random(m)
    y = A @ truth + np.sqrt(var) * rng.standard_normal(m)
    pm, pv = 0.1 * np.cos(np.arange(d)), 0.5 + 0.5 * rng.random(d)
    twin = Twin(lambda x: A @ x, lambda x, s: A.T @ s, *gauss_loglike(y, var), *gauss_prior(pm, pv))
    model = tda.DeviceModel(LINEAR_SRC, m, reference=lambda x: A @ x)
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, (np.zeros(m) + var) * np.eye(m)), model)
    x_hat, H = closed_form_mode(A, y, var, pm, pv)
    return dict(posterior=post, twin=twin, starts=pm + np.sqrt(pv) * rng.standard_normal((n, d)), gtol=1e-9, x_hat=x_hat, H=H)


def fixture_posteriors():
    """the three posteriors of tests/golden/g25_map.npz with their fixed starts: name -> case (a `reference=` twin everywhere, so
    that the reference's optimiser, the host route and the device see the same posterior)"""
    import tinyda_amd as tda

    cases = {}
    # extmodel, isotropic noise, d = 5, m = 70
    d, m = 5, 70
    rng = np.random.default_rng(2501)
    truth = 0.4 * rng.standard_normal(d)
    y = xm.np_forward(truth, m)[0] + 0.1 * rng.standard_normal(m)
    pm, pv = np.zeros(d), np.ones(d)
    fwd, vjp = extmodel_parts(m)
    cases["extmodel"] = dict(
        posterior=tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, 0.01 * np.eye(m)), tda.DeviceModel(xm.source(), m, reference=fwd)),
        twin=Twin(fwd, vjp, *gauss_loglike(y, 0.01), *gauss_prior(pm, pv)), starts=truth + 0.05 * rng.standard_normal((3, d)), gtol=1e-5)
    # Poisson DeviceLogLike + family prior, d = 4
    d, m = 4, 23
    rng = np.random.default_rng(2502)
    comps = xp.components(d, ("norm", "gamma", "lognorm", "t"))
    truth = np.array([c.ppf(0.5) for c in comps])
    fwd, vjp = extmodel_parts(m)
    expo = 5.0 + 5.0 * rng.random(m)
    y = rng.poisson(expo * np.exp(fwd(truth))).astype(float)
    prior = tda.DevicePrior.from_distributions(comps)
    like = tda.DeviceLogLike(xl.POISSON_SRC, y, expo, reference=xl.poisson_terms, reference_gradient=xl.poisson_terms_grad)
    cases["poisson_families"] = dict(
        posterior=tda.Posterior(prior, like, tda.DeviceModel(xm.source(), m, reference=fwd)),
        twin=Twin(fwd, vjp, lambda F, y=y: np.sum(xl.poisson_terms(F, y, expo)), lambda F, y=y: xl.poisson_terms_grad(F, y, expo), prior.logpdf, prior.reference_gradient),
        starts=truth * (1.0 + 0.1 * rng.standard_normal((3, d))), gtol=1e-5)
    # the heat ring, d = 4, m = 16
    d, m = 4, 16
    truth, y, theta0 = xw.problem(d, m, 3, 2503)
    pm, pv = np.zeros(d), np.ones(d)
    fwd, vjp = ring_parts(m)
    cases["ring"] = dict(
        posterior=tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, 1e-4 * np.eye(m)),
                                tda.DeviceModel(xw.source(gradient="wave"), m, reference=fwd)),
        twin=Twin(fwd, vjp, *gauss_loglike(y, 1e-4), *gauss_prior(pm, pv)), starts=theta0, gtol=1e-5)
    return cases


def form_cases(d=13, m=70):
    """every form of the contract once: name -> case (source gradient everywhere)"""
    import tinyda_amd as tda

    cases = {}
    rng = np.random.default_rng(77)
    pm, pv = np.zeros(d), np.ones(d)
    mvn = st.multivariate_normal(pm, np.diag(pv))
    # wave model + tda_gradient_wave
    truth = 0.5 * rng.standard_normal(d)
    fwd, vjp = ring_parts(m)
    y = fwd(truth) + 0.01 * rng.standard_normal(m)
    cases["wave"] = dict(posterior=tda.Posterior(mvn, tda.GaussianLogLike(y, 1e-4 * np.eye(m)), tda.DeviceModel(xw.source(gradient="wave"), m)),
                         twin=Twin(fwd, vjp, *gauss_loglike(y, 1e-4), *gauss_prior(pm, pv)), starts=truth + 0.01 * rng.standard_normal((5, d)), gtol=1e-5)
    # the likelihoods and priors stand over extmodel
    fwd, vjp = extmodel_parts(m)
    truth = 0.3 * rng.standard_normal(d)
    par = 0.05 + 0.05 * rng.random(m)
    y = fwd(truth) + par * rng.standard_normal(m)
    starts = truth + 0.02 * rng.standard_normal((5, d))
    model = tda.DeviceModel(xm.source(), m)
    cases["student_t"] = dict(posterior=tda.Posterior(mvn, tda.DeviceLogLike(xl.STUDENT_T_SRC, y, par), model), starts=starts, gtol=1e-5,
                              twin=Twin(fwd, vjp, lambda F: np.sum(xl.t_terms(F, y, par)), lambda F: xl.t_terms_grad(F, y, par), *gauss_prior(pm, pv)))
    cases["ar1"] = dict(posterior=tda.Posterior(mvn, tda.DeviceLogLike(xlw.AR1_SRC, y, par), model), starts=starts, gtol=1e-5,
                        twin=Twin(fwd, vjp, lambda F: float(np.sum(xlw.ar1(F, y, par))), lambda F: np.asarray(xlw.ar1_grad(F, y, par)).reshape(m), *gauss_prior(pm, pv)))
    comps = xp.components(d, ("norm", "gamma", "lognorm", "t", "invgamma"))
    inside = np.array([c.ppf(0.6) for c in comps])
    yf = fwd(inside) + 0.1 * rng.standard_normal(m)
    prior = tda.DevicePrior.from_distributions(comps)
    cases["families"] = dict(posterior=tda.Posterior(prior, tda.GaussianLogLike(yf, 0.01 * np.eye(m)), model), gtol=1e-5,
                             starts=inside * (1.0 + 0.05 * rng.standard_normal((5, d))) + 0.02,
                             twin=Twin(fwd, vjp, *gauss_loglike(yf, 0.01), prior.logpdf, prior.reference_gradient))
    cauchy = xpw.cauchy_difference(d)
    cases["cauchy_difference"] = dict(posterior=tda.Posterior(xpw.device_prior(cauchy), tda.GaussianLogLike(y, np.diag(par ** 2)), model), starts=starts, gtol=1e-5,
                                      twin=Twin(fwd, vjp, *gauss_loglike(y, par ** 2), cauchy.logpdf, cauchy.grad))
    return cases


def difference_cases(d=5, m=23):
    """sources without a gradient: extmodel cut before its tda_gradient, and a JointPrior of families (its lowering has no gradient)"""
    import tinyda_amd as tda

    rng = np.random.default_rng(78)
    fwd, vjp = extmodel_parts(m)
    truth = 0.3 * rng.standard_normal(d)
    y = fwd(truth) + 0.1 * rng.standard_normal(m)
    pm, pv = np.zeros(d), np.ones(d)
    cases = {"extmodel": dict(
        posterior=tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, 0.01 * np.eye(m)), tda.DeviceModel(without_gradient(xm.source()), m)),
        twin=Twin(fwd, vjp, *gauss_loglike(y, 0.01), *gauss_prior(pm, pv)), starts=truth + 0.05 * rng.standard_normal((4, d)), gtol=1e-4, difference=True)}
    comps = xp.components(d, ("norm", "gamma", "lognorm", "t", "invgamma"))
    inside = np.array([c.ppf(0.6) for c in comps])
    yf = fwd(inside) + 0.1 * rng.standard_normal(m)
    joint = tda.JointPrior(comps)
    grad = tda.DevicePrior.from_distributions(comps).reference_gradient
    cases["joint_families"] = dict(posterior=tda.Posterior(joint, tda.GaussianLogLike(yf, 0.01 * np.eye(m)), tda.DeviceModel(xm.source(), m)), gtol=1e-4, difference=True,
                                   starts=inside * (1.0 + 0.05 * rng.standard_normal((4, d))) + 0.02, twin=Twin(fwd, vjp, *gauss_loglike(yf, 0.01), joint.logpdf, grad))
    return cases


def support_case(d=3, m=23):
    """gamma priors (support x > 0) with data generated at negative parameters, which pull every component towards 0 and across;
    the last start lies outside"""
    import tinyda_amd as tda

    rng = np.random.default_rng(79)
    fwd, vjp = extmodel_parts(m)
    comps = [xp.component("gamma") for _ in range(d)]
    y = fwd(-0.3 * np.ones(d)) + 0.1 * rng.standard_normal(m)
    prior = tda.DevicePrior.from_distributions(comps)
    starts = np.vstack([0.01 + 0.05 * rng.random((6, d)), np.full((1, d), 0.05)])
    starts[-1, 1] = -0.05
    return dict(posterior=tda.Posterior(prior, tda.GaussianLogLike(y, 0.01 * np.eye(m)), tda.DeviceModel(xm.source(), m)), starts=starts, gtol=1e-5,
                twin=Twin(fwd, vjp, *gauss_loglike(y, 0.01), prior.logpdf, prior.reference_gradient))


NAN_ABOVE = 0.4


def nan_case(d=3, m=23):
    """extmodel with every output NaN above theta_0 = 0.4, and data generated at theta_0 = 0.8, which pull across the threshold"""
    import tinyda_amd as tda

    rng = np.random.default_rng(80)
    fwd, vjp = extmodel_parts(m, NAN_ABOVE)
    truth = np.array([0.8, -0.2, 0.3])
    y = xm.np_forward(truth, m)[0] + 0.1 * rng.standard_normal(m)
    pm, pv = np.zeros(d), np.ones(d)
    starts = np.column_stack([0.3 * rng.random(5), 0.2 * rng.standard_normal((5, 2))])
    return dict(posterior=tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, 0.01 * np.eye(m)), tda.DeviceModel(xm.source(nan_above=NAN_ABOVE), m)),
                twin=Twin(fwd, vjp, *gauss_loglike(y, 0.01), *gauss_prior(pm, pv)), starts=starts, gtol=1e-5)


def two_modes_case(n=32):
    """F(theta) = theta_0^2 + theta_1 observed once, under a Gaussian prior shifted a little to theta_0 > 0: one mode on each side of
    theta_0 = 0, the right one higher.  `modes` are the two stationary points to rounding (Newton from the twin's ends), `H` their
    negative Hessians."""
    import tinyda_amd as tda

    y, var, pm, pv = np.array([1.0]), 0.04, np.array([0.05, 0.0]), np.ones(2)
    fwd, vjp = (lambda x: np.array([x[0] * x[0] + x[1]])), (lambda x, s: np.array([2.0 * x[0] * s[0], s[0]]))
    twin = Twin(fwd, vjp, *gauss_loglike(y, var), *gauss_prior(pm, pv))

    def neg_hessian(x):
        r = x[0] * x[0] + x[1] - y[0]
        J = np.array([2.0 * x[0], 1.0])
        return (np.outer(J, J) + r * np.diag([2.0, 0.0])) / var + np.diag(1.0 / pv)

    modes = []
    for x in (np.array([-1.0, 0.0]), np.array([1.0, 0.0])):
        x = maximize_twin(twin, x, gtol=1e-10)["x"]
        for _ in range(3):
            x = x + np.linalg.solve(neg_hessian(x), twin.gradient(x))
        modes.append(x)
    rng = np.random.default_rng(81)
    side = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)
    starts = np.column_stack([side * (0.5 + 0.8 * rng.random(n)), 0.3 * rng.standard_normal(n)])
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, var * np.eye(1)), tda.DeviceModel(TWO_MODES_SRC, 1))
    return dict(posterior=post, twin=twin, starts=starts, gtol=1e-7, modes=np.array(modes), H=[neg_hessian(x) for x in modes])
