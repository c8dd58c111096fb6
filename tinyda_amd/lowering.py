"""The lowering pass: which problems sample() runs on the HIP engine, and why the others are not.

`lower()` reads each posterior's description (Posterior._lowering) and returns a plan (level descriptions, proposal description)
or the reason of the first rule that refuses the problem; backend='hip' raises with that reason, backend='auto' warns with it.
The rules are plain functions that return a reason or nothing, and ORDER IS BEHAVIOUR, because the first reason is what the user
reads: `lower()`, `_level()` and `_hierarchy()` spell the order out.  tda_engine_init refuses the same cases; they are refused
here so that backend='auto' falls back with its warning.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from ._contract import SIG
from .likelihoods import _is_diagonal
from .proposals import (DREAM, DREAMZ, HMC, MALA, NUTS, AdaptiveMetropolis, CrankNicolson, GaussianRandomWalk, IndependenceSampler,
                        OperatorWeightedCrankNicolson)

_GRW_PCN_AM = (GaussianRandomWalk, CrankNicolson, AdaptiveMetropolis)
_DEVICE_PROPOSALS = _GRW_PCN_AM + (DREAMZ, DREAM, IndependenceSampler, OperatorWeightedCrankNicolson, MALA, HMC, NUTS)

MAX_LEVELS = 6  # (0.5; five and six levels: no error model, no dense observation covariance, at most 64 parameters -- MAX_LEVELS_FULL otherwise)
MAX_LEVELS_FULL = 4
MAX_PARAMETERS = 128  # (more than 64: GRW / pCN / AdaptiveMetropolis, see _above_64_parameters)
MAX_AEM_OUTPUTS = 256  # dense error model (0.5: 129 .. 256 on k_aem_refresh_big); hierarchies sequenced by the host: MAX_AEM_OUTPUTS_HOST_SEQUENCED
MAX_AEM_OUTPUTS_HOST_SEQUENCED = 256  # (the same since k_ext_aem_*<256>)

_ISO_DIAG = (_lib.NOISE_ISO, _lib.NOISE_DIAG)

# the run's options: sample()'s adaptive_error_model after its own validation (None / 'state-independent' / 'state-dependent'),
# whether it is the diagonal extension, randomize_subchain_length, and whether the chains are sharded over processes
Run = namedtuple("Run", "n_levels proposal error_model diagonal_error_model randomize distributed")


def lower(posteriors, proposal, diagonal_error_model=False, error_model=None, randomize=False, distributed=False):
    """-> ((level descriptions, proposal description), None), or (None, the first reason why not)"""
    run = Run(len(posteriors), proposal, error_model, diagonal_error_model, randomize, distributed)
    why = _mass_adaptation(run) or _hierarchy_size(run)
    lows = []
    for post in posteriors:
        if why is None:
            low = getattr(post, "_lowering", lambda: None)()
            why = _level(low, run)
        if why is None:
            if diagonal_error_model and low["noise_kind"] == _lib.NOISE_ADAPTIVE:
                low = _with_diagonal_noise(low)
            why = _adaptive_likelihood(low, run) or _dense_noise(low, run)
            lows.append(low)
    why = why or _hierarchy(lows, run)
    if why is not None:
        return None, why
    prop = proposal._lowering()
    if prop is None:  # an option of a lowerable proposal class that the engine does not know: host protocol under 'auto'
        return None, "an option of %s the engine does not implement" % type(proposal).__name__
    return (lows, prop), None


# adapt_mass of HMC / NUTS pools the variances over the chains of ONE engine (include/tinyda_amd_mass.h): under
# distributed=True every rank would learn a mass of its own, and the union over ranks would no longer be a single-process run
def _mass_adaptation(run):
    if run.distributed and getattr(run.proposal, "adapt_mass", 0):
        return ("adapt_mass = %d of %s under distributed=True: the mass is pooled over the chains of one process only"
                % (run.proposal.adapt_mass, type(run.proposal).__name__))


# (A dense inverse mass of HMC / NUTS -- inv_mass [d, d], include/tinyda_amd_dense_mass.h -- needs no rule of its own: it is a
# key of the proposal's description, `dense_mass`, and lowers or is refused with its sampler by the rules below.  Its warm-up
# adaptation -- adapt_dense, include/tinyda_amd_dense_mass_adaptation.h -- is one more such key, and falls under the adapt_mass rule above.)
def _hierarchy_size(run):
    if not 1 <= run.n_levels <= MAX_LEVELS or type(run.proposal) not in _DEVICE_PROPOSALS:
        return "more than %d levels (or none), or a proposal class the engine has no kernel for (%s)" % (MAX_LEVELS, type(run.proposal).__name__)
    if run.n_levels > MAX_LEVELS_FULL and (run.error_model is not None or isinstance(run.proposal, DREAMZ)):
        return "more than %d levels are lowered without error model, under GaussianRandomWalk / CrankNicolson / AdaptiveMetropolis" % MAX_LEVELS_FULL


# ---- one level -----------------------------------------------------------------------------------------------------------------
def _level(low, run):
    if low is None:
        return ("a posterior the engine cannot lower (an opaque Python model, a prior other than scipy's multivariate normal / JointPrior of the "
                "scipy families of csrc/tda_prior_families.h / DevicePrior, a likelihood outside GaussianLogLike's classes)")
    if low["prior_mean"].shape[0] > MAX_PARAMETERS:
        return "more than %d parameters" % MAX_PARAMETERS
    return (("prior_source" in low and _prior_source(low, run)) or (low["noise_kind"] == _lib.NOISE_SOURCE and _loglike_source(low, run))
            or (low["prior_mean"].shape[0] > 64 and _above_64_parameters(low, run)) or _diagonal_error_model_covariance(low, run) or None)


# the proposals on the gradient of the log-posterior, MALA and HMC (a subclass: one kernel family, tda_user_mala_steps /
# tda_user_hmc_steps, one set of rules).  Every rule below that speaks of them takes the name from here
def _gradient_name(run):
    return type(run.proposal).__name__ if isinstance(run.proposal, MALA) else None


# the rules that a source-defined prior and a DeviceLogLike share: both exist inside the program compiled with a DeviceModel only,
# so the routes on which the engine's own kernels evaluate the prior or a level's likelihood are closed to them.  `who` is the label
def _level_cap(who, run):
    return "%s: hierarchies of at most %d levels" % (who, MAX_LEVELS_FULL) if run.n_levels > MAX_LEVELS_FULL else None


def _under_dreamz(who, run):
    return "%s is not lowered under DREAM(Z)" % who if isinstance(run.proposal, DREAMZ) else None


def _under_independence(who, run):
    return "%s is not lowered under IndependenceSampler" % who if isinstance(run.proposal, IndependenceSampler) else None


def _with_error_model(who, run):
    return "%s is not lowered together with an adaptive error model" % who if run.error_model is not None else None


def _with_randomize(who, run):
    return "%s is not lowered with randomize_subchain_length" % who if run.randomize else None


# mala: 'MALA', or '<who> under MALA' beside a source-defined prior
def _missing_loglike_gradient(mala, low):
    if low["noise_kind"] == _lib.NOISE_SOURCE and not low.get("loglike_has_gradient"):
        which, sig = (" that couples outputs", "tda_loglike_grad_wave") if low.get("loglike_coupled") else ("", "tda_loglike_term_grad")
        return "%s with a DeviceLogLike%s needs %s in the likelihood source" % (mala, which, SIG[sig])


# a source-defined prior (DevicePrior, or a JointPrior of scipy families beyond norm / uniform): the shared rules, and every
# route that needs a Gaussian prior
def _prior_source(low, run):
    who = low["prior_source"]["label"]
    return (_prior_source_models(who, low) or _level_cap(who, run) or _under_dreamz(who, run) or _prior_source_gaussian_proposals(who, run)
            or (_gradient_name(run) and _prior_source_mala(who, low, run)) or _under_independence(who, run) or _with_error_model(who, run) or _with_randomize(who, run))


def _prior_source_models(who, low):
    if "source" not in low or low["noise_kind"] not in _ISO_DIAG + (_lib.NOISE_SOURCE,):
        return "%s is compiled into the programs of the levels' models, which must be DeviceModels with isotropic / diagonal noise or a DeviceLogLike" % who


def _prior_source_gaussian_proposals(who, run):
    if isinstance(run.proposal, (CrankNicolson, OperatorWeightedCrankNicolson)):
        return "%s is not lowered under %s (it needs a Gaussian prior)" % (who, type(run.proposal).__name__)


# tda_user_mala_steps (HMC: tda_user_hmc_steps) takes the prior's gradient from the source: a DevicePrior that defines tda_logprior_term_grad
# (DevicePrior.from_distributions for scipy families), single level, over a model with its own gradient
def _prior_source_mala(who, low, run):
    mala = _gradient_name(run)
    if not low["prior_source"]["has_gradient"]:
        if low["prior_source"].get("coupled"):
            return "%s is not lowered under %s: a prior that couples parameters needs %s in its source" % (who, mala, SIG["tda_logprior_grad"])
        return ("%s is not lowered under %s: it needs a DevicePrior whose source defines %s (DevicePrior.from_distributions for scipy families)"
                % (who, mala, SIG["tda_logprior_term_grad"]))
    if run.n_levels != 1:
        return "%s under %s: single level only" % (who, mala)
    if not low["has_gradient"]:
        return "%s under %s needs %s (or tda_gradient_wave) in the model source" % (who, mala, SIG["tda_gradient"])
    if np.asarray(low["data"]).shape[0] > 2048:
        return "%s under %s over a source-defined model: at most 2048 outputs" % (who, mala)
    return _missing_loglike_gradient("%s under %s" % (who, mala), low)


# a DeviceLogLike: the shared rules, and MALA last
def _loglike_source(low, run):
    who = "DeviceLogLike"
    if "loglike_source" not in low:
        return "DeviceLogLike is compiled into the program of its level's model, which must be a DeviceModel"
    return (_level_cap(who, run) or _under_dreamz(who, run) or _loglike_source_owcn(run) or _under_independence(who, run)
            or _with_error_model(who, run) or _with_randomize(who, run) or (_gradient_name(run) and _loglike_source_mala(low, run)))


def _loglike_source_owcn(run):
    return "DeviceLogLike is not lowered under OperatorWeightedCrankNicolson" if isinstance(run.proposal, OperatorWeightedCrankNicolson) else None


def _loglike_source_mala(low, run):
    if run.n_levels != 1 or ("prior_joint" in low and "prior_source" not in low) or not _is_diagonal(low["prior_cov"]):
        return "%s with a DeviceLogLike: single level, multivariate normal prior with diagonal covariance or a DevicePrior with its gradient" % _gradient_name(run)
    return _missing_loglike_gradient(_gradient_name(run), low)


# 65 .. 128 parameters (0.5, tda_kernels_wide.h): single-level chains, Delayed Acceptance and MLDA (up to four levels), linear,
# source-defined and batched host models with isotropic / diagonal noise, Gaussian priors (diagonal or dense covariance) and
# JointPrior, GaussianRandomWalk / CrankNicolson / AdaptiveMetropolis
def _above_64_parameters(low, run):
    n, prop = run.n_levels, type(run.proposal)
    external = "batched" in low or "source" in low
    diagonal_error_model = n >= 2 and run.error_model is not None and run.diagonal_error_model
    mala_on_source_gradient = prop in (MALA, HMC, NUTS) and n == 1 and low.get("has_gradient")  # (a source-defined model's tda_gradient)
    other_proposal = prop not in _GRW_PCN_AM and not mala_on_source_gradient
    other_model = (low.get("A") is None and not external) or "rosenbrock" in low  # (linear, source-defined and batched host models)
    dense_prior_of_external = external and not _is_diagonal(low["prior_cov"])  # (external models: diagonal prior covariance, as at any width)
    third_noise = (_lib.NOISE_ADAPTIVE if run.error_model is not None and not run.diagonal_error_model  # (the dense error model)
                   else _lib.NOISE_DENSE if n == 1 and low.get("A") is not None else _lib.NOISE_SOURCE)  # (NOISE_SOURCE: checked by _loglike_source)
    if (diagonal_error_model or n > MAX_LEVELS_FULL or other_proposal or other_model or getattr(run.proposal, "block_moments", False)
            or dense_prior_of_external or low["noise_kind"] not in _ISO_DIAG + (third_noise,)):
        return ("more than 64 parameters are lowered for single-level chains, Delayed Acceptance and MLDA of linear, source-defined and batched host models with "
                "isotropic / diagonal noise, GaussianRandomWalk / CrankNicolson / AdaptiveMetropolis (error models: the dense one)")


def _diagonal_error_model_covariance(low, run):
    if run.diagonal_error_model and low["noise_kind"] == _lib.NOISE_ADAPTIVE and not _is_diagonal(np.asarray(low["noise"], dtype=np.float64)):
        return "error_model_covariance='diagonal' needs diagonal covariances in the adaptive likelihoods"


# diagonal error model: the adaptive likelihood's (diagonal) covariance travels as its diagonal
def _with_diagonal_noise(low):
    dg = np.diag(np.asarray(low["noise"], dtype=np.float64)).copy()
    iso = np.all(dg == dg[0])
    return dict(low, noise_kind=_lib.NOISE_ISO if iso else _lib.NOISE_DIAG, noise=dg[:1].copy() if iso else dg)


def _adaptive_likelihood(low, run):
    if low["noise_kind"] == _lib.NOISE_ADAPTIVE and (run.n_levels < 2 or np.asarray(low["data"]).shape[0] > MAX_AEM_OUTPUTS):
        return "AdaptiveGaussianLogLike on the device: coarse levels of a hierarchy with at most %d outputs" % MAX_AEM_OUTPUTS


def _dense_noise(low, run):
    if low["noise_kind"] != _lib.NOISE_DENSE:
        return None
    if run.n_levels > MAX_LEVELS_FULL:
        return "a dense observation covariance in a hierarchy: at most %d levels" % MAX_LEVELS_FULL
    if low["A"] is None:  # callback / source-defined model: any sampler they run under, m <= 2048
        if np.asarray(low["data"]).shape[0] > 2048:
            return "a dense observation covariance beside a callback / source-defined model: at most 2048 outputs"
    elif low["A"].shape[0] > 1024 or (run.n_levels != 1 and type(run.proposal) not in _GRW_PCN_AM):
        # linear model, m <= 1024 (MFMA quadratic form): single level under GRW / pCN / AM / DREAM(Z), and since 0.4 any level
        # of a Delayed Acceptance / MLDA hierarchy of linear levels under GRW / pCN / AM
        return ("a dense observation covariance with a linear model is lowered for at most 1024 outputs, single level (any proposal the engine knows) "
                "or a hierarchy of linear levels under GaussianRandomWalk / CrankNicolson / AdaptiveMetropolis")


# ---- the hierarchy as a whole --------------------------------------------------------------------------------------------------
def _hierarchy(lows, run):
    return (_diagonal_error_model_noise(lows, run) or _dense_error_model(lows, run) or _shared_archive(run) or _rosenbrock(lows, run)
            or _joint_prior(lows, run) or _external_models(lows, run) or (_gradient_name(run) and _mala(lows, run))
            or (isinstance(run.proposal, OperatorWeightedCrankNicolson) and _owcn(lows, run)) or _independence(lows, run) or _one_prior(lows))


def _diagonal_error_model_noise(lows, run):
    if run.diagonal_error_model and any(lw["noise_kind"] not in _ISO_DIAG for lw in lows):
        return "the diagonal error model takes its Sigma_e from isotropic / diagonal level noise"


# tda_host_init.inc, "adaptive error model set-up": adaptive likelihoods below an ISOTROPIC finest level
def _dense_error_model(lows, run):
    if run.error_model is None or run.diagonal_error_model or len(lows) <= 1:
        return None
    if lows[-1]["noise_kind"] != _lib.NOISE_ISO or any(lw["noise_kind"] == _lib.NOISE_DENSE for lw in lows):
        return "dense error model: the finest level must have an isotropic likelihood on the device (and no level a dense observation covariance)"
    if any(lw["noise_kind"] != _lib.NOISE_ADAPTIVE for lw in lows[:-1]):
        return "dense error model: every level below the finest needs an AdaptiveGaussianLogLike"
    if np.asarray(lows[0]["data"]).shape[0] > MAX_AEM_OUTPUTS_HOST_SEQUENCED and (isinstance(run.proposal, DREAMZ) or any("source" in lw or "batched" in lw for lw in lows)):
        return ("dense error model with more than %d outputs: hierarchies of linear levels under GaussianRandomWalk / CrankNicolson / AdaptiveMetropolis"
                % MAX_AEM_OUTPUTS_HOST_SEQUENCED)


def _shared_archive(run):
    if isinstance(run.proposal, DREAMZ) and run.n_levels != 1 and run.proposal._shared:
        return "DREAM's shared archive is single-level on the device (below a hierarchy: DREAMZ's per-chain archives)"


def _rosenbrock(lows, run):
    if any("rosenbrock" in low for low in lows) and not isinstance(run.proposal, DREAMZ):
        return "the Rosenbrock model is fused into the DREAM(Z) kernel only"


# JointPrior: GRW / AM / DREAM(Z), single level or hierarchy, every model kind but the Rosenbrock example; the kernels that
# evaluate the prior test the support bounds (proposals outside are rejected)
def _joint_prior(lows, run):
    if not any("prior_joint" in low for low in lows):
        return None
    if isinstance(run.proposal, CrankNicolson) or any("rosenbrock" in lw for lw in lows):
        return "JointPrior: not with CrankNicolson or the Rosenbrock model"
    if any(lw["noise_kind"] == _lib.NOISE_DENSE for lw in lows):
        return "JointPrior: not with a dense observation covariance"


# source-defined and batched host models: single level, or a whole hierarchy of them (Delayed Acceptance / MLDA with
# host-sequenced level actions: GRW / pCN / AM / DREAMZ).  iso / diag noise, diagonal prior.
def _external_models(lows, run):
    if not any("source" in low or "batched" in low for low in lows):
        return None
    if run.n_levels > MAX_LEVELS_FULL:
        return "hierarchies of callback / source-defined models: at most %d levels" % MAX_LEVELS_FULL
    if run.n_levels > 1 and (any("rosenbrock" in low for low in lows) or type(run.proposal) not in _GRW_PCN_AM + (DREAMZ,)):
        return "hierarchies of callback / source-defined models run under GaussianRandomWalk / CrankNicolson / AdaptiveMetropolis / DREAMZ"
    for i, low in enumerate(lows):
        ok_noise = (low["noise_kind"] in _ISO_DIAG + (_lib.NOISE_SOURCE,) or (low["noise_kind"] == _lib.NOISE_DENSE and low["A"] is None)
                    or (low["noise_kind"] == _lib.NOISE_ADAPTIVE and i < len(lows) - 1))
        if not ok_noise or not _is_diagonal(low["prior_cov"]):
            return "callback / source-defined models need isotropic / diagonal noise (dense: top level only) and a diagonal prior covariance"


# exact gradient: of a linear-Gaussian posterior (single level, linear model, Gaussian prior), or from a source-defined
# model's own tda_gradient (single level, iso / diag noise, diagonal Gaussian prior or a DevicePrior with its gradient:
# tda_user_mala_steps)
def _mala(lows, run):
    low, mala = lows[0], _gradient_name(run)
    if run.n_levels == 1 and "source" in low and ("prior_joint" not in low or "prior_source" in low):  # (a source-defined prior: checked by _prior_source)
        if not low["has_gradient"]:
            return "%s over a source-defined model needs %s in the model source" % (mala, SIG["tda_gradient"])
        if low["noise_kind"] not in _ISO_DIAG + (_lib.NOISE_SOURCE,) or np.asarray(low["data"]).shape[0] > 2048:
            return "%s over a source-defined model: isotropic or diagonal noise, at most 2048 outputs" % mala
    elif isinstance(run.proposal, HMC):  # (the engine's linear-model MALA, k_mh_steps with its closed-form gradient, has no leapfrog loop)
        return "%s: single level, a DeviceModel with tda_gradient, Gaussian prior with diagonal covariance or a DevicePrior with its gradient" % mala
    elif run.n_levels != 1 or "source" in low or "batched" in low or "rosenbrock" in low or "prior_joint" in low:
        return "MALA: single level, linear model, Gaussian prior"


# single level; fixed operators: linear, callback or source-defined model
def _owcn(lows, run):
    if run.n_levels != 1 or run.proposal._lowering() is None or "rosenbrock" in lows[0] or "prior_joint" in lows[0]:
        return "OperatorWeightedCrankNicolson: single level, operators the engine can lower"
    if run.proposal.adaptive and ("source" in lows[0] or "batched" in lows[0]):
        return "adaptive OperatorWeightedCrankNicolson (per-chain operators) is lowered for linear models"


# Gaussian q, single level; linear, callback or source-defined model
def _independence(lows, run):
    if isinstance(run.proposal, IndependenceSampler) and (run.n_levels != 1 or run.proposal._lowering() is None or "rosenbrock" in lows[0]):
        return "IndependenceSampler: single level, Gaussian q"


# one prior for the hierarchy (every tinyDA example shares it across levels)
def _one_prior(lows):
    ps0 = lows[0].get("prior_source")
    for low in lows[1:]:
        ps = low.get("prior_source")
        same_source = (ps is None) == (ps0 is None) and (ps is None or (
            ps["source"] == ps0["source"] and np.array_equal(ps["p"], ps0["p"]) and np.array_equal(ps["q"], ps0["q"])))
        if not (np.array_equal(low["prior_mean"], lows[0]["prior_mean"]) and np.array_equal(low["prior_cov"], lows[0]["prior_cov"]) and same_source):
            return "the levels of a hierarchy must share one prior"


def _wrap_opaque_models(posteriors):
    """Posteriors whose model is a plain callable -> copies with a BatchedModel looping over the chains (models returning the
    reference's (output, qoi) tuples included: the engine takes the output, the quantity of interest is produced again when a
    Link of the result is materialised); None if a likelihood has no data vector."""
    from .models import BatchedModel, DeviceModel, LinearModel, Rosenbrock
    from .target import Posterior

    out = []
    for post in posteriors:
        if isinstance(post.model, (LinearModel, Rosenbrock, DeviceModel, BatchedModel)):
            out.append(post)
            continue
        data = getattr(post.likelihood, "data", None)
        if not callable(post.model) or data is None:
            return None
        m = int(np.atleast_1d(np.asarray(data)).shape[0])
        fn = post.model

        def batch(thetas, fn=fn, m=m):
            res = np.empty((thetas.shape[0], m))
            for i in range(thetas.shape[0]):
                f = fn(thetas[i])
                if isinstance(f, tuple):  # posterior.py:97-101
                    f = f[0]
                if not isinstance(f, np.ndarray):
                    raise TypeError("Model output must be a numpy array!")
                res[i] = np.asarray(f, dtype=np.float64).reshape(m)
            return res

        bm = BatchedModel(batch, m)
        bm.single = fn  # one parameter vector -> the user's own return value (output or (output, qoi))
        out.append(Posterior(post.prior, post.likelihood, bm))
    return out
