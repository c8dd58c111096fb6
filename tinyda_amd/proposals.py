"""Transition kernels with the reference's constructor signatures and proposal protocol
(tinyDA/proposal.py:17-41): setup_proposal / adapt / make_proposal / get_acceptance / get_q.

On the device path `sample()` never calls these methods per step: `_lowering()` hands the constructor
arguments to the HIP engine, which runs propose -> evaluate -> accept -> adapt fused.  The methods exist so
that the same objects also drive the host loop for opaque Python models (BASELINE config 1), and so user
code written against tinyDA keeps working.
"""
import numpy as np
import scipy.stats as stats

from . import _lib
from .moments import RecursiveSampleMoments


class Proposal:
    is_symmetric = False

    def setup_proposal(self, **kwargs):
        pass

    def adapt(self, **kwargs):
        pass

    def make_proposal(self, link):
        pass

    def get_acceptance(self, proposal_link, previous_link):
        pass

    def get_q(self, x_link, y_link):
        pass


class IndependenceSampler(Proposal):
    """Independent proposals from a fixed distribution q with .rvs() and .logpdf() (proposal.py:65-129).  On the device
    path q must be Gaussian (a frozen scipy.stats.multivariate_normal, or any object with `mean` and `cov`)."""

    def __init__(self, q):
        self.q = q
        self.q.logpdf(self.q.rvs(1))  # the reference's interface check (proposal.py:101-105)

    def make_proposal(self, link):
        return self.q.rvs(1).flatten()

    def get_acceptance(self, proposal_link, previous_link):
        q_proposal = self.get_q(None, proposal_link)
        q_previous = self.get_q(None, previous_link)
        return np.exp(proposal_link.posterior - previous_link.posterior + q_previous - q_proposal)

    def get_q(self, x_link, y_link):
        return self.q.logpdf(y_link.parameters)

    def _lowering(self):
        mean, cov = getattr(self.q, "mean", None), getattr(self.q, "cov", None)
        if mean is None or cov is None:
            return None
        return dict(kind=_lib.PROP_INDEPENDENCE, C_=np.atleast_2d(np.asarray(cov, dtype=np.float64)),
                    q_mean=np.atleast_1d(np.asarray(mean, dtype=np.float64)))


def _require_square(C, name):
    # same checks and messages as proposal.py:189-196 / :443-450
    if not isinstance(C, np.ndarray):
        raise TypeError("%s must be a numpy array" % name)
    if C.ndim == 1:
        if C.shape[0] != 1:
            raise ValueError("%s must be an NxN array" % name)
    elif C.shape[0] != C.shape[1]:
        raise ValueError("%s must be an NxN array" % name)


class GaussianRandomWalk(Proposal):
    """theta' = theta + scaling * N(0, C), optional global scaling adaptation (proposal.py:132-258)."""

    is_symmetric = True
    alpha_star = 0.24

    def __init__(self, C, scaling=1, adaptive=False, gamma=1.01, period=100):
        _require_square(C, "C")
        self.C = C
        self.d = C.shape[0]
        self._init_scaling(scaling, adaptive, gamma, period)

    def _init_scaling(self, scaling, adaptive, gamma, period):
        self.scaling = scaling
        self.adaptive = adaptive
        self.gamma = gamma
        self.period = period
        self.k = 0  # completed scaling adaptations (diminishing adaptation)
        self.t = 0  # adapt() calls
        self._factor_of = None

    def _draw(self):
        """N(0, C) as chol(C) z.  (The reference asks NumPy, which re-runs an SVD of C on every call;
        the law is the same.)"""
        if self._factor_of is not self.C:
            self._L = np.linalg.cholesky(np.atleast_2d(self.C))
            self._factor_of = self.C
        return self._L @ np.random.standard_normal(self.d)

    def adapt(self, **kwargs):
        self.t += 1
        if self.adaptive and self.t % self.period == 0:
            rate = np.mean(kwargs["accepted"][-self.period:])
            self.scaling = np.exp(np.log(self.scaling) + self.gamma ** -self.k * (rate - self.alpha_star))
            self.k += 1

    def make_proposal(self, link):
        return link.parameters + self.scaling * self._draw()

    def get_acceptance(self, proposal_link, previous_link):
        if np.isnan(proposal_link.posterior):
            return 0
        return np.exp(proposal_link.posterior - previous_link.posterior)

    def _lowering(self):
        return dict(kind=_lib.PROP_GRW, C_=np.atleast_2d(self.C), scaling=float(self.scaling),
                    adaptive=bool(self.adaptive), gamma=float(self.gamma), period=int(self.period))


class CrankNicolson(GaussianRandomWalk):
    """pCN: theta' = sqrt(1 - beta^2) theta + beta N(0, C_prior); acceptance on the likelihood ratio
    (proposal.py:261-369).  The prior mean is ignored, as in the reference."""

    is_symmetric = False

    def __init__(self, scaling=0.1, adaptive=False, gamma=1.01, period=100):
        self._init_scaling(scaling, adaptive, gamma, period)

    def setup_proposal(self, **kwargs):
        prior = kwargs["posterior"].prior
        self.C = prior.cov if hasattr(prior, "cov") else prior.cov_object.covariance
        self.d = self.C.shape[0]

    def make_proposal(self, link):
        return np.sqrt(1 - self.scaling ** 2) * link.parameters + self.scaling * self._draw()

    def get_acceptance(self, proposal_link, previous_link):
        if np.isnan(proposal_link.posterior):
            return 0
        return np.exp(proposal_link.likelihood - previous_link.likelihood)

    def get_q(self, x_link, y_link):
        return stats.multivariate_normal.logpdf(
            y_link.parameters, mean=np.sqrt(1 - self.scaling ** 2) * x_link.parameters, cov=self.scaling ** 2 * self.C
        )

    def _lowering(self):
        return dict(kind=_lib.PROP_PCN, C_=None, scaling=float(self.scaling), adaptive=bool(self.adaptive),
                    gamma=float(self.gamma), period=int(self.period))


class OperatorWeightedCrankNicolson(CrankNicolson):
    """Operator-weighted pCN (Law 2014): theta' = sqrtm(I - scaling B) theta + sqrtm(scaling B) N(0, C_prior), acceptance on
    the likelihood ratio (proposal.py:515-605).  The operators are recomputed when the adaptive scaling changes.  On the
    device path the fixed operators are handed to the engine; with adaptive=True and a symmetric B the engine gets B's spectrum and
    works the per-chain operators out from each chain's own scaling (single-level chains, linear forward model)."""

    def __init__(self, B, scaling=1.0, adaptive=False, gamma=1.01, period=100):
        self.B = B
        super().__init__(scaling, adaptive, gamma, period)

    def _operators(self):
        from scipy.linalg import sqrtm

        d = np.atleast_2d(self.B).shape[0]
        self.state_operator = np.real(sqrtm(np.eye(d) - self.scaling * self.B))
        self.noise_operator = np.real(sqrtm(self.scaling * self.B))

    def setup_proposal(self, **kwargs):
        super().setup_proposal(**kwargs)
        self._operators()

    def adapt(self, **kwargs):
        super().adapt(**kwargs)
        if self.adaptive and self.t % self.period == 0:
            self._operators()

    def make_proposal(self, link):
        return np.dot(self.state_operator, link.parameters) + np.dot(self.noise_operator, self._draw())

    def get_q(self, x_link, y_link):
        return stats.multivariate_normal.logpdf(
            y_link.parameters, mean=np.dot(self.state_operator, x_link.parameters), cov=np.dot(self.scaling * self.B, self.C)
        )

    def _lowering(self):
        if self.adaptive:
            # per-chain operators (every chain adapts its own scaling): for a symmetric B they are functions of its spectrum,
            # which is what the engine takes (tda_engine_set_proposal_spectrum); any other B: host protocol
            B = np.atleast_2d(np.asarray(self.B, dtype=np.float64))
            if B.shape[0] != B.shape[1] or not np.allclose(B, B.T, rtol=1e-12, atol=1e-14):
                return None
            lam, V = np.linalg.eigh(0.5 * (B + B.T))
            return dict(kind=_lib.PROP_OWCN, C_=None, scaling=float(self.scaling), adaptive=True, gamma=float(self.gamma),
                        period=int(self.period), spectrum=(np.ascontiguousarray(V), np.ascontiguousarray(lam)))
        self._operators()
        return dict(kind=_lib.PROP_OWCN, C_=None, scaling=1.0, adaptive=False, gamma=float(self.gamma), period=int(self.period),
                    state_operator=np.ascontiguousarray(self.state_operator, dtype=np.float64),
                    noise_operator=np.ascontiguousarray(self.noise_operator, dtype=np.float64))


def _grad_log_prior(x, prior):
    """utils.py:273-280 for a frozen scipy multivariate normal (anything with mean / cov); the prior's own `grad_logpdf` where
    it has one (a DevicePrior with reference_gradient); finite differences otherwise."""
    own = getattr(prior, "grad_logpdf", None)
    if callable(own):
        return np.asarray(own(x), dtype=np.float64)
    cov = getattr(prior, "cov", None)
    if cov is None and hasattr(prior, "cov_object"):
        cov = prior.cov_object.covariance
    if cov is not None and hasattr(prior, "mean"):
        return np.dot(np.linalg.inv(np.atleast_2d(cov)), (prior.mean - x))
    from scipy.optimize import approx_fprime

    return approx_fprime(x, prior.logpdf)


class MALA(GaussianRandomWalk):
    """Metropolis-adjusted Langevin: theta' = theta + scaling^2/2 grad log post(theta) + scaling N(0, I), acceptance with
    the two transition densities (proposal.py:861-1005).  The gradient is exact when the model has a
    `gradient(parameters, sensitivity)` method and the likelihood a `grad_loglike`, finite differences of
    `posterior.logpdf` otherwise.  On the device path (linear model, Gaussian prior) the gradient is c - H theta with
    H = Sigma_prior^-1 + A^T Sigma_e^-1 A precomputed once: a d x d product per step instead of a second pass over the
    observations."""

    is_symmetric = False
    alpha_star = 0.57

    def __init__(self, scaling=0.1, adaptive=False, gamma=1.01, period=100):
        self._init_scaling(scaling, adaptive, gamma, period)

    def setup_proposal(self, **kwargs):
        self.posterior = kwargs["posterior"]
        self.d = np.asarray(self.posterior.prior.rvs()).size
        exact = callable(getattr(self.posterior.model, "gradient", None)) and hasattr(self.posterior.likelihood, "grad_loglike")
        self.compute_gradient = self._compute_gradient if exact else self._compute_gradient_approx

    def _compute_gradient(self, link):
        sens = self.posterior.likelihood.grad_loglike(link.model_output)
        return _grad_log_prior(link.parameters, self.posterior.prior) + self.posterior.model.gradient(link.parameters, sens)

    def _compute_gradient_approx(self, link):
        from scipy.optimize import approx_fprime

        return approx_fprime(link.parameters, self.posterior.logpdf)

    def make_proposal(self, link):
        if not hasattr(link, "gradient"):
            link.gradient = self.compute_gradient(link)
        return link.parameters + 0.5 * self.scaling ** 2 * link.gradient + self.scaling * np.random.standard_normal(self.d)

    def get_acceptance(self, proposal_link, previous_link):
        if np.isnan(proposal_link.posterior):
            return 0
        if not hasattr(proposal_link, "gradient"):
            proposal_link.gradient = self.compute_gradient(proposal_link)
        q_x_y = self.get_q(previous_link, proposal_link)
        q_y_x = self.get_q(proposal_link, previous_link)
        return np.exp(proposal_link.posterior - previous_link.posterior + q_x_y - q_y_x)

    def get_q(self, x_link, y_link):
        return -0.5 / self.scaling ** 2 * np.linalg.norm(
            x_link.parameters - y_link.parameters - 0.5 * self.scaling ** 2 * y_link.gradient) ** 2

    def _lowering(self):
        return dict(kind=_lib.PROP_MALA, C_=None, scaling=float(self.scaling), adaptive=bool(self.adaptive),
                    gamma=float(self.gamma), period=int(self.period))


def mass_windows(W, period):
    """The windows of the warm-up adaptation of the mass (include/tinyda_amd_mass.h, "Schedule"), as (first step, last step
    exclusive) with steps counted from 0: W steps of P = W / period periods; period 0 is a buffer, windows of 1, 2, 4, ...
    periods follow, and a window of L periods starting at period s with s + 3 L > P takes all the rest and is the last."""
    if int(W) != W or int(period) != period or period < 1 or W % period != 0 or W < 2 * period:
        raise ValueError("adapt_mass = %r must be a multiple of the period (%r) and at least two periods (or 0: off)" % (W, period))
    W, period = int(W), int(period)
    P, out, s, L = W // period, [], 1, 1
    while s < P:
        if s + 3 * L > P:
            L = P - s
        out.append((s * period, (s + L) * period))
        s, L = s + L, 2 * L
    return out


def _mass_pool(mean, M2, n, inv_mass):
    """The window's end of include/tinyda_amd_mass.h ("Update") over the moments mean, M2 [N, d] of N chains with n states each:
    -> (the new inverse mass, the number of entries refused).  Sums in the kernel's order: 256 strided partial sums, then a tree."""
    N = mean.shape[0]

    def pooled(x):
        part = np.zeros((256, x.shape[1]))
        for r in range(0, N, 256):
            part[:min(256, N - r)] += x[r:r + 256]
        s = 128
        while s >= 1:
            part[:s] += part[s:2 * s]
            s >>= 1
        return part[0]

    with np.errstate(all="ignore"):
        mbar = pooled(mean) / float(N)
        dm = mean - mbar[None, :]
        B, Wn = pooled(dm * dm), pooled(M2)
        T = float(n) * float(N)
        var = (Wn + float(n) * B) / (T - 1.0)
        w = var * T / (T + 5.0) + 1e-3 * 5.0 / (T + 5.0)
        ok = np.isfinite(w) & (w > 0.0)
    return np.where(ok, w, inv_mass), int(np.sum(~ok))


def _dense_mass_pool(S1, S2, n, N, chol):
    """The window's end of include/tinyda_amd_dense_mass_adaptation.h ("Update") over the sums S1 [NC, d] and S2 [NC, d, d] (the
    lower triangle is read) of NC chunks, n states of each of N chains, taken about any shift: -> (the new factor L, 0) or, where
    the regularised covariance is not finite or np.linalg.cholesky fails, (chol, 1): the whole factor is kept."""
    d = S1.shape[1]
    with np.errstate(all="ignore"):
        s1, s2 = np.zeros(d), np.zeros((d, d))
        for c in range(S1.shape[0]):  # chunks in ascending order
            s1, s2 = s1 + S1[c], s2 + S2[c]
        T = float(n) * float(N)
        m = s1 / T
        C = (s2 - (T * m)[:, None] * m[None, :]) / (T - 1.0)
        W = C * T / (T + 5.0)
        W[np.diag_indices(d)] += 1e-3 * 5.0 / (T + 5.0)
        W = np.tril(W) + np.tril(W, -1).T  # (only the lower triangle is ever formed)
        if not np.all(np.isfinite(W)):
            return chol, 1
        try:
            L = np.tril(np.linalg.cholesky(W))
        except np.linalg.LinAlgError:
            return chol, 1
        if not (np.all(np.isfinite(L)) and np.all(np.diag(L) > 0.0)):
            return chol, 1
    return L, 0


def dense_inv_mass(W):
    """A dense inverse mass of HMC / NUTS (include/tinyda_amd_dense_mass.h), validated: -> (W [d, d], its lower Cholesky factor L,
    W = L L^T).  W must be square, finite, exactly symmetric and positive definite (np.linalg.cholesky decides)."""
    W = np.array(W, dtype=np.float64)
    if W.ndim != 2 or W.shape[0] != W.shape[1] or W.shape[0] < 1:
        raise ValueError("inv_mass takes one finite, positive value per parameter, [d], or a symmetric positive definite matrix, [d, d]; not the shape %r" % (W.shape,))
    if not np.all(np.isfinite(W)):
        raise ValueError("a dense inv_mass must be finite")
    if not np.array_equal(W, W.T):
        raise ValueError("a dense inv_mass must be symmetric, W == W.T exactly: symmetrise it first, W = (W + W.T) / 2")
    try:
        L = np.linalg.cholesky(W)
    except np.linalg.LinAlgError as exc:
        raise ValueError("a dense inv_mass must be positive definite: np.linalg.cholesky failed (%s)" % (exc,)) from None
    if not (np.all(np.isfinite(L)) and np.all(np.diag(L) > 0.0)):
        raise ValueError("a dense inv_mass must be positive definite: its Cholesky factor is not finite with a positive diagonal")
    return W, np.tril(L)


class _Metric:
    """The arithmetic that the mass enters, for the host classes below: a diagonal inverse mass w on the momentum p, or a dense one
    W = L L^T on the whitened momentum q = L^T p (include/tinyda_amd_dense_mass.h); `p` below is p or q accordingly."""

    def __init__(self, w, L):
        self.w, self.L = w, L

    def draw(self, z):  # the momentum of the step's unit normals
        return z / np.sqrt(self.w) if self.L is None else z

    def kinetic(self, p):
        return 0.5 * np.sum(self.w * (p * p)) if self.L is None else 0.5 * np.sum(p * p)

    def force(self, g):  # what a half step adds to the momentum, per unit of step size
        return g if self.L is None else self.L.T @ g

    def velocity(self, p):
        return self.w * p if self.L is None else self.L @ p

    def dot(self, pa, rho):  # p_a^T W rho
        return np.sum((self.w * pa) * rho) if self.L is None else np.sum(pa * rho)


class HMC(MALA):
    """Hamiltonian Monte Carlo (an extension: the reference has none): per proposal a momentum p = z / sqrt(w) from d unit normals
    z, `n_leapfrog` leapfrog steps of size `scaling` under the diagonal inverse mass w = `inv_mass` (None: 1) on the log-posterior
    and the gradient that MALA uses (exact or finite differences, chosen as MALA chooses), and one accept test on the energy
    difference, alpha = exp(post' - post + K0 - K1) with K = 1/2 sum_j w_j p_j^2.  A position whose log-posterior is NaN or infinite
    ends the trajectory and rejects.  With one step and unit mass this is MALA.  `adaptive` adapts the step size towards 0.65
    acceptance.  On the device path (a single-level DeviceModel with `tda_gradient`, wherever MALA lowers) the whole trajectory
    runs in one kernel, tda_user_hmc_steps; over any other model the host protocol below runs.

    `adapt_mass` = W > 0 adapts the inverse mass during the first W steps (a multiple of `period`, at least two periods), from
    `inv_mass` as the starting mass, as include/tinyda_amd_mass.h writes it out: regularised variances of the states of windows
    that double in length (`mass_windows`), after which the mass is frozen; with `adaptive` (recommended) the step size's
    diminishing gain restarts at every update of the mass.  On the device path the variances are pooled over all chains of the
    engine, which share one mass vector.  On the host path every chain has its own copy of the proposal and adapts from its own
    window alone, on the same schedule, with the same regulariser and the same restart: pooling over chains exists only on the
    device.  `mass_updates` and `mass_refused` count the window ends applied and the entries they left unchanged.

    A two-dimensional `inv_mass` = W [d, d] is a fixed dense inverse mass (symmetric positive definite; `W == W.T` exactly), as
    include/tinyda_amd_dense_mass.h writes it out: its Cholesky factor is computed once and kept as `chol_inv_mass`, the momentum
    is held whitened, q = L^T p, and a leapfrog step is q += (e/2) L^T g; theta += e L q; q += (e/2) L^T g'.  It lowers wherever
    the diagonal mass lowers.  `adapt_mass` learns a diagonal and is refused beside it; `mass_from_samples` turns a pilot run
    into such a matrix.

    `adapt_mass` = W with `adapt_dense=True` learns the dense inverse mass during warm-up instead, on the schedule above, as
    include/tinyda_amd_dense_mass_adaptation.h writes it out: at a window's end the regularised covariance of the window's states
    and its Cholesky factor replace `inv_mass` [d, d] and `chol_inv_mass`, or, where the covariance is not finite and positive
    definite, the whole factor is kept and `mass_refused` goes up by one.  `inv_mass` (None, [d] or [d, d]) is the start.  On the
    device the covariance is pooled over all chains of the engine; a host chain adapts from its own window alone."""

    alpha_star = 0.65

    def __init__(self, scaling=0.1, n_leapfrog=8, inv_mass=None, adaptive=False, gamma=1.01, period=100, adapt_mass=0, adapt_dense=False):
        if int(n_leapfrog) != n_leapfrog or not 1 <= n_leapfrog <= 1024:
            raise ValueError("n_leapfrog must be an integer in 1 .. 1024, not %r" % (n_leapfrog,))
        self.adapt_dense = bool(adapt_dense)
        if self.adapt_dense and not adapt_mass:
            raise ValueError("adapt_dense=True needs adapt_mass > 0, the number of warm-up steps: adapt_mass = %r" % (adapt_mass,))
        self.chol_inv_mass = None
        if inv_mass is not None and np.ndim(inv_mass) >= 2:
            inv_mass, self.chol_inv_mass = dense_inv_mass(inv_mass)
            if adapt_mass and not self.adapt_dense:
                raise ValueError("adapt_mass = %r with a dense inv_mass: the warm-up adaptation learns a diagonal mass" % (adapt_mass,))
        elif inv_mass is not None:
            inv_mass = np.atleast_1d(np.asarray(inv_mass, dtype=np.float64)).copy()
            if inv_mass.ndim != 1 or not np.all(np.isfinite(inv_mass) & (inv_mass > 0)):
                raise ValueError("inv_mass takes one finite, positive value per parameter")
        self.n_leapfrog, self.inv_mass = int(n_leapfrog), inv_mass
        self._init_scaling(scaling, adaptive, gamma, period)
        if adapt_mass != 0 and (int(adapt_mass) != adapt_mass or adapt_mass < 0):
            raise ValueError("adapt_mass = %r must be a multiple of the period (%r) and at least two periods (or 0: off)" % (adapt_mass, period))
        self.adapt_mass = int(adapt_mass)
        self._mass_windows = mass_windows(self.adapt_mass, period) if self.adapt_mass else []
        self._mass_n, self._mass_mean, self._mass_M2 = 0, None, None
        self.mass_updates, self.mass_refused = 0, 0
        # the start of a dense adaptation, as the plan carries it: (the diagonal [d] or None, the factor [d, d] or None)
        self._mass_start = (None if inv_mass is None or self.chol_inv_mass is not None else inv_mass.copy(),
                            None if self.chol_inv_mass is None else self.chol_inv_mass.copy())
        self._mass_shift = None

    def setup_proposal(self, **kwargs):
        super().setup_proposal(**kwargs)
        if self.inv_mass is not None and self.inv_mass.shape != ((self.d,) if self.chol_inv_mass is None else (self.d, self.d)):
            raise ValueError("inv_mass has %d entries for %d parameters" % (self.inv_mass.shape[0], self.d))
        if self.adapt_mass and self.inv_mass is None:
            self.inv_mass = np.ones(self.d)
        if self.adapt_dense and self.chol_inv_mass is None:  # a diagonal start: L = diag(sqrt(w)), W = L L^T
            self.chol_inv_mass = np.diag(np.sqrt(self.inv_mass))
            self.inv_mass = self.chol_inv_mass @ self.chol_inv_mass.T

    def _adapt_dense_mass(self, x):
        """_adapt_mass under adapt_dense (include/tinyda_amd_dense_mass_adaptation.h with N = 1, one chunk): the state before a
        window's first step is its shift; the sums of y = x - a and of y y^T over the window; at its end the new factor"""
        s = self.t - 1
        if s >= self.adapt_mass:
            return
        x = np.asarray(x, dtype=np.float64)
        for first, end in self._mass_windows:
            if first <= s < end:
                y = x - self._mass_shift
                self._mass_n += 1
                self._mass_mean = self._mass_mean + y  # (S1 and S2 of the text)
                self._mass_M2 = self._mass_M2 + y[:, None] * y[None, :]
                if s + 1 == end:
                    self.chol_inv_mass, refused = _dense_mass_pool(self._mass_mean[None, :], self._mass_M2[None, :, :], self._mass_n, 1, self.chol_inv_mass)
                    self.inv_mass = self.chol_inv_mass @ self.chol_inv_mass.T
                    self.mass_refused += refused
                    self.mass_updates += 1
                    self._mass_n = 0
                    if self.adaptive:
                        self.k = 0  # the step-size rule's gain is full again under the new metric
                break
        if any(s + 1 == first for first, _ in self._mass_windows):  # x is the state before the next window's first step
            self._mass_shift = x.copy()
            self._mass_n, self._mass_mean, self._mass_M2 = 0, np.zeros(self.d), np.zeros((self.d, self.d))

    def _adapt_mass(self, x):
        """fold the state of step self.t - 1 (steps counted from 0) into its window; at the window's end the new mass"""
        if self.adapt_dense:
            return self._adapt_dense_mass(x)
        s = self.t - 1
        if s >= self.adapt_mass:
            return
        for first, end in self._mass_windows:
            if first <= s < end:
                x = np.asarray(x, dtype=np.float64)
                if self._mass_n == 0:
                    self._mass_mean, self._mass_M2 = np.zeros(self.d), np.zeros(self.d)
                self._mass_n += 1
                delta = x - self._mass_mean
                self._mass_mean = self._mass_mean + delta / float(self._mass_n)
                self._mass_M2 = self._mass_M2 + delta * (x - self._mass_mean)
                if s + 1 == end:
                    self.inv_mass, refused = _mass_pool(self._mass_mean[None, :], self._mass_M2[None, :], self._mass_n, self.inv_mass)
                    self.mass_refused += refused
                    self.mass_updates += 1
                    self._mass_n = 0
                    if self.adaptive:
                        self.k = 0  # the step-size rule's gain is full again under the new metric

    def adapt(self, **kwargs):
        super().adapt(**kwargs)
        if self.adapt_mass:
            self._adapt_mass(kwargs["parameters"])

    def _metric(self):
        return _Metric(np.ones(self.d) if self.inv_mass is None else self.inv_mass, self.chol_inv_mass)

    def make_proposal(self, link):
        if not hasattr(link, "gradient"):
            link.gradient = self.compute_gradient(link)
        eps, M = self.scaling, self._metric()
        p = M.draw(np.random.standard_normal(self.d))
        k0 = M.kinetic(p)
        p = p + (0.5 * eps) * M.force(link.gradient)
        theta = np.asarray(link.parameters, dtype=np.float64)
        self._end = None  # (the end point, its gradient, K0 - K1): None when the trajectory ended early
        for i in range(1, self.n_leapfrog + 1):
            theta = theta + eps * M.velocity(p)
            at = self.posterior.create_link(theta)
            if not np.isfinite(at.posterior):
                return theta
            grad = self.compute_gradient(at)
            p = p + (eps if i < self.n_leapfrog else 0.5 * eps) * M.force(grad)
        self._end = (theta, grad, k0 - M.kinetic(p))
        return theta

    def get_acceptance(self, proposal_link, previous_link):
        end = getattr(self, "_end", None)
        if end is None or end[0] is not proposal_link.parameters and not np.array_equal(end[0], proposal_link.parameters):
            return 0
        if np.isnan(proposal_link.posterior):
            return 0
        proposal_link.gradient = end[1]
        return np.exp((proposal_link.posterior - previous_link.posterior) + end[2])

    def get_q(self, x_link, y_link):  # (the momentum is not part of a link: the energy difference is inside get_acceptance)
        return 0.0

    def _lowered_mass(self, low):
        """the mass in a plan: `inv_mass` [d] or None, and under a dense mass `dense_mass`, its factor [d, d] (the key is there only then)"""
        if self.adapt_dense:  # the start as it was given (a host run may have moved inv_mass since), and the switch
            w, L = self._mass_start
            low = dict(low, inv_mass=None if w is None else w.copy(), adapt_mass=self.adapt_mass, adapt_dense=True)
            return low if L is None else dict(low, dense_mass=L.copy())
        if self.chol_inv_mass is not None:
            return dict(low, inv_mass=None, dense_mass=self.chol_inv_mass.copy())
        low = dict(low, inv_mass=None if self.inv_mass is None else self.inv_mass.copy())
        return dict(low, adapt_mass=self.adapt_mass) if self.adapt_mass else low  # (off: the plan is what it was)

    def _lowering(self):
        return self._lowered_mass(dict(kind=_lib.PROP_HMC, C_=None, scaling=float(self.scaling), adaptive=bool(self.adaptive), gamma=float(self.gamma),
                                       period=int(self.period), n_leapfrog=self.n_leapfrog))


def _logaddexp(a, b):
    hi, lo = (a, b) if a > b else (b, a)
    return hi + np.log1p(np.exp(lo - hi))


class NUTS(HMC):
    """The no-U-turn sampler (an extension: the reference has none): HMC whose trajectory length is chosen per step.  Multinomial
    NUTS with the diagonal inverse mass w = `inv_mass` (None: 1) in iterative form, as include/tinyda_amd_nuts.h writes it out: a
    tree of leapfrog steps of size `scaling` doubles forwards or backwards at random, at most `max_depth` times, until its ends
    turn towards each other (or one inside the newest subtree does, or a leaf diverges: its energy error exceeds 1000 or its
    log-posterior is not finite); the new state is drawn from the tree's leaves with weights exp(-energy error), biased towards
    the newest subtree.  `accepted` is whether the state moved.  `adaptive` adapts the step size at the period boundary towards
    `target_accept` in the mean of the leaves' min(1, exp(-energy error)).  On the device path (wherever HMC lowers) a whole tree
    runs in one kernel, tda_user_nuts_steps; over any other model the host protocol below builds the same tree in NumPy, with the
    momentum from np.random.standard_normal, the direction of a doubling from np.random.randint(2) and then its merge uniform
    from np.random.random, and one np.random.random per leaf of a subtree after its first.  `totals` counts what the device's
    proposal_state reports: n_leapfrog, n_divergent, n_max_depth, depth_sum.  `adapt_mass` is HMC's: warm-up adaptation of the
    inverse mass, pooled over all chains on the device and per chain on the host, and with `adapt_dense=True` of a dense one.  A two-dimensional `inv_mass` is HMC's fixed
    dense inverse mass (include/tinyda_amd_dense_mass.h): the edges, the momentum sums and the checkpoints then hold the whitened
    momentum q = L^T p, and the U-turn test is a plain dot product of q's."""

    def __init__(self, scaling=0.1, max_depth=8, inv_mass=None, adaptive=False, target_accept=0.8, gamma=1.01, period=100, adapt_mass=0, adapt_dense=False):
        if int(max_depth) != max_depth or not 1 <= max_depth <= 10:
            raise ValueError("max_depth must be an integer in 1 .. 10, not %r" % (max_depth,))
        if not 0.0 < target_accept < 1.0:
            raise ValueError("target_accept must lie in (0, 1), not %r" % (target_accept,))
        super().__init__(scaling, 1, inv_mass, adaptive, gamma, period, adapt_mass, adapt_dense)
        self.n_leapfrog = None  # (chosen per step)
        self.max_depth, self.target_accept = int(max_depth), float(target_accept)
        self.alpha_star = self.target_accept
        self.totals = dict(n_leapfrog=0, n_divergent=0, n_max_depth=0, depth_sum=0)
        self._stat, self._stat_sum = 0.0, 0.0

    def make_proposal(self, link):
        if not hasattr(link, "gradient"):
            link.gradient = self.compute_gradient(link)
        eps, M = self.scaling, self._metric()
        theta0 = np.asarray(link.parameters, dtype=np.float64)
        p0 = M.draw(np.random.standard_normal(self.d))
        h0 = -link.posterior + M.kinetic(p0)
        left = right = (theta0, p0, np.asarray(link.gradient, dtype=np.float64))
        rho, LW = p0, 0.0
        cand = (theta0, left[2], 0)  # (position, gradient, the number of the leaf in this step; 0: the initial state)
        asum, nleaf, depth, stop = 0.0, 0, 0, None
        with np.errstate(all="ignore"):
            for j in range(self.max_depth):
                fwd, uj = int(np.random.randint(2)), np.random.random()
                e = eps if fwd else -eps
                theta, p, g = right if fwd else left
                ck, sub, LWs, rs = {}, None, 0.0, None
                for n in range(1 << j):
                    p = p + (0.5 * e) * M.force(g)
                    theta = theta + e * M.velocity(p)
                    at = self.posterior.create_link(theta)
                    nleaf += 1
                    if not np.isfinite(at.posterior):
                        stop = "divergent"
                        break
                    g = np.asarray(self.compute_gradient(at), dtype=np.float64)
                    p = p + (0.5 * e) * M.force(g)
                    h = -at.posterior + M.kinetic(p)
                    if np.isnan(h) or h - h0 > 1000.0:
                        stop = "divergent"
                        break
                    lw = h0 - h
                    asum += min(1.0, np.exp(lw))
                    if n == 0:
                        LWs, rs, sub = lw, p, (theta, g, nleaf)
                    else:
                        LWs, rs = _logaddexp(LWs, lw), rs + p
                        if np.random.random() < np.exp(lw - LWs):
                            sub = (theta, g, nleaf)
                    top = bin(n >> 1).count("1")
                    if n % 2 == 0:
                        ck[top] = (p, rs)
                    else:
                        ones, turn = (n ^ (n + 1)).bit_length() - 1, False  # trailing one bits of n
                        for k in range(top, top - ones, -1):
                            pa, ra = ck[k]
                            rr = (rs - ra) + pa
                            if not (M.dot(pa, rr) > 0.0 and M.dot(p, rr) > 0.0):
                                turn = True
                        if turn:
                            stop = "uturn_subtree"
                            break
                if stop:
                    break
                if uj < np.exp(LWs - LW):
                    cand = sub
                LW, rho = _logaddexp(LW, LWs), rho + rs
                if fwd:
                    right = (theta, p, g)
                else:
                    left = (theta, p, g)
                depth = j + 1
                if not (M.dot(left[1], rho) > 0.0 and M.dot(right[1], rho) > 0.0):
                    stop = "uturn_tree"
                    break
        self._stat = asum / nleaf
        self._end = cand
        self.last_tree = dict(stop=stop or "max_depth", depth=depth, n_leapfrog=nleaf, selected=cand[2], stat=self._stat)
        self.totals["n_leapfrog"] += nleaf
        self.totals["n_divergent"] += stop == "divergent"
        self.totals["n_max_depth"] += stop is None
        self.totals["depth_sum"] += depth
        return cand[0]

    def get_acceptance(self, proposal_link, previous_link):
        end = getattr(self, "_end", None)
        if end is None or end[2] == 0 or (end[0] is not proposal_link.parameters and not np.array_equal(end[0], proposal_link.parameters)):
            return 0.0
        proposal_link.gradient = end[1]
        return 1.0

    def adapt(self, **kwargs):
        self.t += 1
        self._stat_sum += self._stat
        if self.t % self.period == 0:
            if self.adaptive:
                self.scaling = np.exp(np.log(self.scaling) + self.gamma ** -self.k * (self._stat_sum / self.period - self.alpha_star))
                self.k += 1
            self._stat_sum = 0.0
        if self.adapt_mass:
            self._adapt_mass(kwargs["parameters"])

    def _lowering(self):
        return self._lowered_mass(dict(kind=_lib.PROP_NUTS, C_=None, scaling=float(self.scaling), adaptive=bool(self.adaptive), gamma=float(self.gamma),
                                       period=int(self.period), max_depth=self.max_depth, target_accept=self.target_accept))


class AdaptiveMetropolis(GaussianRandomWalk):
    """Haario et al. (2001): proposal covariance <- running sample covariance every `period` adapt calls
    once t >= t0 (proposal.py:372-512).

    `block_moments` (extension, device path only, default off): update the running covariance once per block of steps
    in closed form on the matrix cores instead of following RecursiveSampleMoments.update operation for operation --
    algebraically identical, ~8x cheaper, differs from the reference recursion by that recursion's rounding error."""

    def __init__(self, C0, sd=None, epsilon=1e-6, t0=0, period=100, adaptive=False, gamma=1.01, block_moments=False):
        _require_square(C0, "C0")
        self.block_moments = bool(block_moments)
        self.C = C0
        self.d = C0.shape[0]
        self._init_scaling(1, adaptive, gamma, period)
        self.sd = sd if sd is not None else min(1, 2.4 ** 2 / self.d)
        self.epsilon = epsilon
        self.t0 = t0

    def setup_proposal(self, **kwargs):
        self.AM_recursor = RecursiveSampleMoments(
            kwargs["parameters"], np.zeros((self.d, self.d)), sd=self.sd, epsilon=self.epsilon
        )

    def adapt(self, **kwargs):
        super().adapt(**kwargs)
        self.AM_recursor.update(kwargs["parameters"])
        if self.t >= self.t0 and self.t % self.period == 0:
            self.C = self.AM_recursor.get_sigma()

    def _lowering(self):
        return dict(kind=_lib.PROP_AM, C_=np.atleast_2d(self.C), adaptive=bool(self.adaptive), gamma=float(self.gamma),
                    period=int(self.period), sd=float(self.sd), epsilon=float(self.epsilon), t0=int(self.t0),
                    block_moments=self.block_moments)


class DREAMZ(GaussianRandomWalk):
    """DREAM(Z): differential-evolution jumps from an archive of past states (proposal.py:608-852).
    Host protocol = reference semantics (per-chain archive, np.random global stream); on the device path the
    constructor arguments are lowered and the archive lives in HBM."""

    def __init__(self, M0, delta=1, b=5e-2, b_star=1e-6, Z_method="random", nCR=3, adaptive=False, gamma=1.01, period=100):
        self.M = M0
        self.M0 = M0
        self._init_scaling(1, adaptive, gamma, period)
        self.delta, self.b, self.b_star = delta, b, b_star
        self.Z_method = Z_method
        self.nCR = nCR
        self.mCR = None
        self.pCR = np.array(nCR * [1 / nCR])

    def setup_proposal(self, **kwargs):
        prior = kwargs["posterior"].prior
        self.d = prior.rvs().size
        if self.adaptive:
            self.LCR = np.zeros(self.nCR)
            self.DeltaCR = np.ones(self.nCR)
        if self.Z_method == "lhs":
            import scipy.stats as st

            u = st.qmc.LatinHypercube(d=self.d).random(n=self.M)
            if hasattr(prior, "ppf"):
                self.Z = prior.ppf(u)
                return
            if hasattr(prior, "mean") and (hasattr(prior, "cov") or hasattr(prior, "cov_object")):
                cov = prior.cov if hasattr(prior, "cov") else prior.cov_object.covariance
                self.Z = st.norm(loc=np.asarray(prior.mean), scale=np.sqrt(np.diag(cov))).ppf(u)
                return
        self.Z = prior.rvs(self.M)

    def adapt(self, **kwargs):
        GaussianRandomWalk.adapt(self, **kwargs)
        self.Z = np.vstack((self.Z, kwargs["parameters"]))
        self.M = self.Z.shape[0]
        if self.adaptive and self.t % self.period == 0:
            jump = kwargs["parameters"] - kwargs["parameters_previous"]
            self.DeltaCR[self.mCR] += (jump ** 2 / np.var(self.Z, axis=0)).sum()
            self.LCR[self.mCR] += 1
            if np.all(self.LCR > 0):
                mean = self.DeltaCR / self.LCR
                self.pCR = mean / mean.sum()

    def make_proposal(self, link, Z=None):
        Z = self.Z if Z is None else Z
        M = Z.shape[0]
        up, down = np.zeros(self.d), np.zeros(self.d)
        for _ in range(self.delta):
            r1, r2 = np.random.choice(M, 2, replace=False)
            up += Z[r1]
            down += Z[r2]
        self.mCR = np.random.choice(self.nCR, p=self.pCR)
        mask = (np.random.uniform(size=self.d) < (self.mCR + 1) / self.nCR).astype(float)
        if mask.sum() == 0:
            mask[np.random.choice(self.d)] = 1
        gamma = self.scaling * 2.38 / np.sqrt(2 * self.delta * mask.sum())
        e = np.random.uniform(-self.b, self.b, size=self.d)
        eps = np.random.normal(0, self.b_star, size=self.d)
        return link.parameters + mask * ((1 + e) * gamma * (up - down) + eps)

    _shared = False

    def _lowering(self):
        if self.Z_method not in ("random", "lhs"):
            return None
        return dict(kind=_lib.PROP_DREAMZ, Z_method=self.Z_method, M0=int(self.M0), delta=int(self.delta), b=float(self.b), b_star=float(self.b_star),
                    nCR=int(self.nCR), adaptive=bool(self.adaptive), gamma=float(self.gamma), period=int(self.period),
                    shared=self._shared)


class DREAM(DREAMZ):
    """DREAM with one archive shared by all chains (proposal.py:1627-1656; ray.py:365-384 ArchiveManager).
    The reference pushes rows to a Ray actor fire-and-forget, so what a proposal sees is timing dependent; the
    device engine synchronises the archive at block boundaries (RCCL all-gather across GPUs)."""

    _shared = True
