"""One composer for every form of a source-defined posterior: the sources and NumPy twins of tests/ext*.py put together from
independent choices, as tinyda_amd/_contract.py lets a user put them together, and the list of combined cases that the three
kernels over the gradient share (tda_user_mala_steps, tda_user_hmc_steps, tda_user_maximize).

The axes and their forms (what the program of csrc/tda_user_program.hip selects between):

    forward     per_output (tda_forward)  |  wave (tda_forward_wave)
    gradient    per_parameter (tda_gradient)  |  wave (tda_gradient_wave)
    likelihood  iso  |  diag  |  term (tda_loglike_term + _grad)  |  wave (tda_loglike_wave + tda_loglike_grad_wave)
    prior       gauss (diagonal Gaussian)  |  term (tda_logprior_term + _grad)  |  wave (tda_logprior_wave + tda_logprior_grad)

and the kinds that fill a form:

    model       extmodel (per_output / per_parameter), the ring of extwave in its four combinations
    likelihood  iso, diag; t, poisson (term); ar1, marginal, softmax (wave)
    prior       gauss; lognormal, families (term); cauchy, tv, hierarchical, ordered (wave)

A case is built from parts: `Composed` is the oracle level (evaluate / grad_logpost: the oracle's MALA and exthmc.run_hmc read
it), `twin()` the same posterior for one parameter vector as extoptimize.Twin (maximize_twin reads it), `make_engine()` the
engine over the concatenated sources and `posterior()` the tda.Posterior of the same case for tda.maximize.  The step sizes are
data: tests/golden/forms_sweep.json, chosen by tests/golden/gen_forms_sweep.py and verified by tests/test_forms_sweep_cases.py."""
import json
import os

import numpy as np

from oracle import tinyda_oracle as orc

from . import exthmc as xh
from . import extloglike as xl
from . import extloglikewave as xlw
from . import extmodel as xm
from . import extoptimize as xo
from . import extprior as xp
from . import extpriorgrad as xg
from . import extpriorwave as xpw
from . import extwave as xw
from .extengine import NOISE_SOURCE, PRIOR_SOURCE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forms_sweep.json")
SEED, CHAIN_OFFSET = xh.SEED, xh.CHAIN_OFFSET
N_FORMS = 24
MAX_CHAINS, MAX_EVALUATIONS = 17, 480  # per case: chains, model evaluations per chain (T L for HMC, T for MALA)
N_STARTS = 3  # of tda.maximize: the first chains' starts
GTOL = 1e-5
# Admission (tests/golden/gen_forms_sweep.py, tests/test_forms_sweep_cases.py): beside exthmc's rule, one ulp on every gradient
# moves no state by more than a hundredth of the bar the states are compared at.  The device's gradient and NumPy's are sums of up
# to 2048 + 128 terms in another order over exp / log that may differ by an ulp: tens of ulps apart, not one, so a case is compared
# only where a hundred of them still fit the bar.  (exthmc's rule looks at the log-posteriors alone, which a drift of the states
# of 1e-9 does not move by 1e-11.)
STATE_SHARE = 1e-2

# ---- the axes ---------------------------------------------------------------------------------------------------------------------------
MODELS = {  # kind -> (forward form, gradient form)
    "extmodel": ("per_output", "per_parameter"),
    "ring_ww": ("wave", "wave"), "ring_wp": ("wave", "per_parameter"), "ring_pw": ("per_output", "wave"), "ring_pp": ("per_output", "per_parameter"),
}
LIKELIHOODS = {"iso": "iso", "diag": "diag", "t": "term", "poisson": "term", "ar1": "wave", "marginal": "wave", "softmax": "wave"}  # kind -> form
PRIORS = {"gauss": "gauss", "lognormal": "term", "families": "term", "cauchy": "wave", "tv": "wave", "hierarchical": "wave", "ordered": "wave"}
FAMILIES = ("norm", "gamma", "lognorm", "t", "invgamma")  # smooth inside their supports; three of them with an edge at 0
AXES = ("forward", "gradient", "likelihood", "prior")
DEFAULT_FORMS = {"forward": "per_output", "gradient": "per_parameter", "likelihood": "iso", "prior": "gauss"}
D_VALUES, M_VALUES = (1, 63, 64, 65, 127, 128), (1, 63, 64, 65, 129, 2048)


def forms_of(c):
    """the form of a case on each axis"""
    return dict(forward=MODELS[c["model"]][0], gradient=MODELS[c["model"]][1], likelihood=LIKELIHOODS[c["like"]], prior=PRIORS[c["prior"]])


def switches_of(c):
    """the -D switches that select a case's forms in the program (the order of the engine's option list is of no account here)"""
    f = forms_of(c)
    return ((["TDA_LOGLIKE_SOURCE"] if f["likelihood"] in ("term", "wave") else []) + (["TDA_LOGLIKE_WAVE"] if f["likelihood"] == "wave" else [])
            + (["TDA_PRIOR_SOURCE"] if f["prior"] != "gauss" else []) + (["TDA_PRIOR_WAVE"] if f["prior"] == "wave" else [])
            + (["TDA_FORWARD_WAVE"] if f["forward"] == "wave" else []) + (["TDA_GRADIENT_WAVE"] if f["gradient"] == "wave" else []))


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
# model, likelihood, prior, d, m.  The per-output ring repeats its solve for every output (m <= 129 keeps a step short).  The wave
# forward beside the per-parameter gradient holds the trajectory and 32 KiB of tangents in LDS of its own: with the 48 steps of
# the other forms that is 57 KiB, which the step programs take and the optimiser, with its ring of pairs, does not (75 KiB of the 64);
# it runs the 12 steps of h = 0.4 (the coarsest fidelity of extwave) in all three kernels.
RING_WP_KSTEPS = 12
FIXED = [
    ("ring_ww", "ar1", "cauchy", 128, 2048),      # the all-wave program, two parameters per lane, the LDS edge
    ("ring_ww", "softmax", "hierarchical", 64, 64),
    ("ring_ww", "t", "lognormal", 65, 65),
    ("ring_ww", "iso", "gauss", 127, 64),
    ("ring_ww", "diag", "families", 64, 2048),
    ("ring_pw", "t", "lognormal", 128, 64),       # the combination that takes scratch memory under HMC
    ("ring_pw", "marginal", "tv", 65, 65),
    ("ring_pw", "diag", "gauss", 64, 129),
    ("ring_pw", "iso", "cauchy", 63, 63),
    ("ring_wp", "poisson", "families", 64, 65),
    ("ring_wp", "ar1", "gauss", 65, 64),
    ("ring_wp", "iso", "ordered", 63, 129),
    ("ring_wp", "diag", "hierarchical", 127, 1),
    ("ring_pp", "marginal", "lognormal", 64, 64),
    ("ring_pp", "iso", "tv", 65, 65),
    ("extmodel", "ar1", "cauchy", 65, 129),       # a coupled likelihood with m across a multiple of 64 beside a coupled prior
    ("extmodel", "marginal", "families", 64, 2048),
    ("extmodel", "softmax", "families", 128, 65),
    ("extmodel", "poisson", "cauchy", 65, 2048),
    ("extmodel", "t", "cauchy", 64, 65),
    ("extmodel", "iso", "lognormal", 1, 2048),
    ("extmodel", "diag", "ordered", 63, 64),
    ("extmodel", "diag", "lognormal", 65, 65),
    ("extmodel", "t", "gauss", 63, 64),
]
WRAPPED_RING_CASE = 3  # a wave gradient at d >= 64 on which every start of maximize takes more than HISTORY iterations
MAP_STATIC_LDS = 45152  # static LDS of tda_user_maximize in the all-wave program of case 0, bytes (the offline compile's figure)
MAP_M_MAX = (64 * 1024 - MAP_STATIC_LDS) // 16  # the outputs (and their sensitivities) that fit beside it: 1274
MAXIMIZE_M = {0: MAP_M_MAX}  # case -> m under maximize: the step programs of case 0 fit at m = 2048, the optimiser's ring of pairs does not


def _variants(i, c):
    """by rotation: adaptive step size, non-unit inverse mass (HMC), block_steps, checkpoint resume, thinning.  maximize takes
    objective='likelihood' wherever the log-prior leaves a gradient test no stationary point within reach: the kinks of the
    total-variation prior, the flat box of the ordered one, the funnel of the hierarchical one (whose mode lies at log tau = 1 - d).
    The total-variation and hierarchical priors stand over the ring: the likelihood alone hardly determines extmodel's parameters
    (its weights take 11 patterns), and the optimiser needs thousands of iterations there."""
    return dict(adaptive=i % 2 == 1, mass=i % 3 != 1, block_steps=(0, 7, 16)[i % 3], resume=i % 5 == 0, thin=3 if i % 4 == 2 else 1,
                ml=c["prior"] in ("tv", "ordered", "hierarchical"))


def form_case(i):
    """case i of the list.  All 24 are fixed: the coverage that tests/test_forms_sweep_cases.py asks of the list leaves a seeded fill
    no room (a fill over the same axes would begin at i = len(FIXED))"""
    model, like, prior, d, m = FIXED[i]
    c = dict(i=i, model=model, like=like, prior=prior, d=d, m=m)
    c.update(_variants(i, c))
    c["name"] = "%02d_%s_%s_%s_d%d_m%d" % (i, model, like, prior, d, m)
    return c


def stored():
    """tests/golden/forms_sweep.json: per case its name, the seed of its problem and the step sizes"""
    with open(GOLDEN) as fh:
        return json.load(fh)


# ---- the parts ----------------------------------------------------------------------------------------------------------------------------
class _Like:
    """log L(F[N, m]) -> [N] and d log L / d F -> [N, m], with what the engine is given: the source, the noise kind, its parameters"""

    def __init__(self, kind, y, par):
        self.kind, self.y, self.par = kind, np.asarray(y, dtype=float), np.asarray(par, dtype=float)
        if kind in ("iso", "diag"):
            self.gauss = orc.make_loglike(kind, self.y, float(self.par[0]) if kind == "iso" else self.par)
            self.source, self.noise_kind = "", 0 if kind == "iso" else 1
        else:
            self.source = xl.KINDS[kind][0] if LIKELIHOODS[kind] == "term" else xlw.KINDS[kind][0]
            self.noise_kind = NOISE_SOURCE

    def loglike(self, F):
        F = np.atleast_2d(F)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if self.kind in ("iso", "diag"):
                return self.gauss(F)
            if LIKELIHOODS[self.kind] == "term":
                return np.sum(xl.KINDS[self.kind][1](F, self.y, self.par), axis=1)
            return np.asarray(xlw.KINDS[self.kind][1](F, self.y, self.par), dtype=float)

    def grad(self, F):
        F = np.atleast_2d(F)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if self.kind in ("iso", "diag"):
                return self.gauss.grad(F)
            return np.asarray((xl.KINDS if LIKELIHOODS[self.kind] == "term" else xlw.KINDS)[self.kind][2](F, self.y, self.par), dtype=float)


class _GaussPrior(orc.MVNPrior):
    """the oracle's diagonal Gaussian with the gradient as the levels of tests/extmodel.py compute it"""

    source = ""

    def __init__(self, mean, cov):
        super().__init__(mean, cov)
        self.precision_t = np.linalg.inv(self.cov).T

    def grad(self, theta):
        return (self.mean[None, :] - np.atleast_2d(theta)) @ self.precision_t


def _prior(kind, d):
    """-> the twin (logpdf, grad, source; p and q unless Gaussian)"""
    if kind == "gauss":
        return _GaussPrior(0.1 * np.ones(d), np.diag(0.5 + 0.01 * np.arange(d)))
    if kind == "lognormal":
        prior = xh.LognormalGradPrior(np.log(0.3) * np.ones(d), 0.5 * np.ones(d))
        prior.source = xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC
        return prior
    if kind == "families":
        prior = xg.FamilyGradPrior(xp.components(d, FAMILIES))
        prior.p, prior.q, prior.source = xg.family_source(prior.comps)
        return prior
    return {"cauchy": xpw.cauchy_difference, "tv": xpw.total_variation, "hierarchical": xpw.hierarchical, "ordered": xpw.ordered}[kind](d)


def _truth_and_starts(kind, prior, d, N, rng, ring):
    """a point the data are generated at and N starts around it, inside every support"""
    if kind == "gauss":
        truth = (0.5 if ring else 0.3) * rng.standard_normal(d)
        return truth, truth + 0.01 * rng.standard_normal((N, d))
    if kind == "lognormal":
        truth = 0.3 * np.exp(0.2 * rng.standard_normal(d))
        return truth, truth * np.exp(0.02 * rng.standard_normal((N, d)))
    if kind == "families":
        return xg.starts_inside(prior.comps, N, rng)
    return xpw.starts(prior, N, rng)


class Composed:
    """the oracle level of a case: evaluate(theta[N, d]) -> (lp, ll, F), grad_logpost(theta, F) -> [N, d]"""

    def __init__(self, forward, vjp, like, prior):
        self.fn, self.vjp, self.like, self.prior = forward, vjp, like, prior

    def forward(self, theta):
        return np.asarray(self.fn(np.atleast_2d(theta)), dtype=float)

    def evaluate(self, theta):
        F = self.forward(theta)
        return self.prior.logpdf(theta), self.like.loglike(F), F

    def grad_logpost(self, theta, F):
        with np.errstate(all="ignore"):
            return self.prior.grad(theta) + self.vjp(theta, self.like.grad(F))

    def twin(self):
        """the same posterior for one parameter vector (extoptimize.maximize_twin)"""
        like, prior = self.like, self.prior
        return xo.Twin(lambda x: self.forward(x[None, :])[0], lambda x, s: self.vjp(x[None, :], s[None, :])[0], lambda F: like.loglike(F[None, :])[0],
                       lambda F: like.grad(F[None, :])[0], lambda x: prior.logpdf(x[None, :])[0], lambda x: np.atleast_2d(prior.grad(x[None, :]))[0])


def build(c, seed=None, N=13):
    """a case with its problem: the model's source, the data, the starts, the oracle level (c["level"])"""
    c = dict(c)
    d, m, ring = c["d"], c["m"], c["model"] != "extmodel"
    rng = np.random.default_rng(1000 * d + m + 7 * c["i"] if seed is None else seed)
    prior = _prior(c["prior"], d)
    truth, theta0 = _truth_and_starts(c["prior"], prior, d, N, rng, ring)
    if ring:
        fwd, grad = MODELS[c["model"]]
        ks = RING_WP_KSTEPS if c["model"] == "ring_wp" else 48
        src = xw.source(fwd, grad, m=m, ksteps=ks)
        forward, vjp = (lambda th: xw.np_forward(th, m, ks)), (lambda th, s: xw.np_vjp(th, s, ks))
    else:
        src = xm.source()
        forward, vjp = (lambda th: xm.np_forward(th, m)), (lambda th, s: xm.np_vjp(th, s))
    F = forward(truth[None, :])[0]
    sd = 0.01 if ring else 0.1
    spread = sd * (1.0 + 0.1 * np.arange(m) / m)
    if c["like"] == "iso":
        y, par = F + sd * rng.standard_normal(m), np.array([sd ** 2])
    elif c["like"] == "diag":
        y, par = F + spread * rng.standard_normal(m), spread ** 2
    elif c["like"] == "poisson":
        par = 5.0 + 5.0 * rng.random(m)
        y = rng.poisson(par * np.exp(F)).astype(float)
    elif c["like"] == "softmax":
        pr = np.exp(F - F.max())
        y, par = rng.multinomial(40 * m, pr / pr.sum()).astype(float), np.ones(m)
    else:  # t, ar1, marginal: noise of scale p_o
        y, par = F + spread * rng.standard_normal(m), spread
    like = _Like(c["like"], y, par)
    c.update(N=N, theta0=theta0, truth=truth, model_source=src, like_twin=like, prior_twin=prior, level=Composed(forward, vjp, like, prior))
    c["source"] = src + like.source + "\n" + prior.source
    return c


def budget(c):
    """(T of MALA, T and L of HMC) within MAX_EVALUATIONS model evaluations per chain; the per-output ring repeats its solve per
    output and per parameter, so it runs a quarter of the budget"""
    slow = MODELS[c["model"]][0] == "per_output" and c["model"] != "extmodel"
    L = (2, 3, 4)[c["i"] % 3]
    evals = MAX_EVALUATIONS // (4 if slow else 1)
    return min(120, evals), min(120, evals // L), L


def proposal(c, kind, scaling):
    T_mala, T_hmc, L = budget(c)
    if kind == "mala":
        return dict(kind="mala", scaling=scaling, adaptive=c["adaptive"], gamma=1.01, period=20), T_mala
    return xh.hmc(scaling, L, c["adaptive"], xh.MASS(c["d"]) if c["mass"] else None), T_hmc


def mala_as_hmc(prop):
    """the oracle's description of MALA as the twin's of HMC with one leapfrog step under unit mass, adapted towards MALA's 0.57"""
    return dict(xh.hmc(prop["scaling"], 1, prop["adaptive"]), gamma=prop["gamma"], period=prop["period"], alpha_star=0.57)


def make_engine(c, prop):
    """the engine of a built case under `prop` (the oracle's description of MALA, or exthmc.hmc's of HMC); not initialised"""
    from tinyda_amd.engine import Engine

    prior, like, d = c["prior_twin"], c["like_twin"], c["d"]
    e = Engine(c["N"], d, seed=SEED, chain_offset=CHAIN_OFFSET, block_steps=c["block_steps"])
    if c["prior"] == "gauss":
        e.set_prior(prior.mean, prior.cov)
    else:
        e.set_prior_joint(np.full(d, PRIOR_SOURCE), prior.p, prior.q)
    e.set_level_source(0, c["source"], like.y, like.noise_kind, like.par)
    if prop["kind"] == "hmc":
        xh.set_proposal(e, prop)
    else:
        e.set_proposal(6, None, **{k: v for k, v in prop.items() if k != "kind"})
    if c["thin"] > 1:
        e.set_record_thinning(c["thin"])
    return e


def posterior(c):
    """the tda.Posterior of a built case"""
    import scipy.stats as st

    import tinyda_amd as tda

    prior, like, m = c["prior_twin"], c["like_twin"], c["m"]
    if c["prior"] == "gauss":
        pr = st.multivariate_normal(prior.mean, prior.cov)
    elif c["prior"] == "lognormal":
        pr = tda.DevicePrior(prior.source, c["d"], prior.p, prior.q)
    elif c["prior"] == "families":
        pr = tda.DevicePrior.from_distributions(prior.comps)
    else:
        pr = xpw.device_prior(prior, reference=False)
    if c["like"] in ("iso", "diag"):
        lk = tda.GaussianLogLike(like.y, np.diag(np.zeros(m) + like.par))
    else:
        lk = tda.DeviceLogLike(like.source, like.y, like.par)
    return tda.Posterior(pr, lk, tda.DeviceModel(c["model_source"], m))


def build_for_maximize(case, seed=None):
    """the case as maximize runs it: the same problem, with the outputs that fit beside the ring of pairs"""
    return build(dict(case, m=MAXIMIZE_M.get(case["i"], case["m"])), seed=seed)


def maximize_case(c):
    """the case as tests/test_gpu_optimize.py reads one: posterior (built on demand), twin, starts, gtol, objective"""
    return dict(twin=c["level"].twin(), starts=c["theta0"][:N_STARTS], gtol=GTOL, objective="likelihood" if c["ml"] else "posterior")


def thinned(ref, thin, T):
    """a trace of T steps as the engine records it under thinning: the initial link, then the steps with (t + 1) % thin == 0"""
    if thin == 1:
        return ref
    keep = np.concatenate([[0], np.arange(thin, T + 1, thin)])
    return {k: (v[:, keep] if np.ndim(v) >= 2 and v.shape[1] == T + 1 else v) for k, v in ref.items()}
