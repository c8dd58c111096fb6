"""Generate lowering_matrix.json: what the lowering pass decides for a matrix of problems -- lowered or not, the first refusal
reason verbatim, and for lowered problems a description of the plan (the proposal description; per level its keys, noise_kind,
array shapes and the prior_source sub-dict).  Run it AT THE COMMIT WHOSE DECISIONS ARE TO BE KEPT (the parent of a change to the
pass); tests/test_lowering_matrix.py replays the file against the code under test through the same `cases()` and `outcome()`.

The axes: model x likelihood x prior x proposal at a single level, homogeneous hierarchies of 2 .. 7 levels
and hierarchies with adaptive likelihoods below the finest level x error model x randomize (all thinned by a checksum of the
case's name, so the selection is fixed), two-level hierarchies mixed from a list of levels, and a list of single cases for the rules
that only a particular size reaches.  The user sources are those of tests/ext*.py.  Only data is stored, everything once:
key sets, level descriptions, proposal descriptions and outcomes in tables of their own (a plan is [proposal, [levels]] by
number), the cases as numbers of outcomes in the order of `cases()`, a checksum of the case names, and per refusal site the
number of cases whose first reason it is ("sites").  `load()` reads the file back with the outcomes written out.

    python tests/golden/gen_lowering_matrix.py            # writes the file, prints how many cases reach each refusal site
"""
import hashlib
import itertools
import json
import os
import re
import subprocess
import sys
import zlib
from functools import lru_cache

import numpy as np
import scipy.stats as st

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import tinyda_amd as tda  # noqa: E402
from tinyda_amd import api  # noqa: E402
from tests import extloglike as xl  # noqa: E402
from tests import extloglikewave as xlw  # noqa: E402
from tests import extmodel as xm  # noqa: E402
from tests import extprior as xp  # noqa: E402
from tests import extpriorgrad as xg  # noqa: E402
from tests import extpriorwave as xpw  # noqa: E402
from tests import extwave as xwv  # noqa: E402

PATH = os.path.join(HERE, "lowering_matrix.json")

# ---- the axes --------------------------------------------------------------------------------------------------------------------
MODEL_DIM = {"lin4": 4, "lin100": 100, "lin129": 129, "callable": 4, "wrapped": 4, "batched": 4, "batched100": 100, "rosen": 4, "rosen100": 100,
             "dev": 4, "dev100": 100, "dev_nograd": 4, "dev_wave": 4, "dev_wave_gradwave": 4, "dev_gradwave": 4}
LIKE_OUTPUTS = {"iso": 3, "diag": 3, "dense": 3, "adaptive": 3, "adaptive_dense": 3, "adaptive257": 257, "ll_term": 3, "ll_term_nograd": 3,
                "ll_wave": 3, "ll_wave_nograd": 3, "iso2049": 2049, "ll_term2049": 2049, "dense1025": 1025, "dense2049": 2049}
PRIORS = ("mvn", "mvn_dense", "mvn_shifted", "joint", "joint_families", "dp_term", "dp_term_grad", "dp_wave", "dp_wave_nograd",
          "dp_families", "dp_term_other", "scalar")
PROPOSALS = ("grw", "grw_adaptive", "pcn", "am", "am_block", "dreamz", "dreamz_lhs", "dreamz_other", "dream", "indep", "indep_other",
             "owcn", "owcn_adaptive", "owcn_adaptive_other", "mala", "hmc", "subclass")
ERROR_MODELS = ("-", "si", "sd", "diag")  # none, state-independent, state-dependent, state-independent with the diagonal covariance


class _Subclass(tda.GaussianRandomWalk):
    pass


class _OtherQ:
    """a proposal density for IndependenceSampler that is not Gaussian (no mean / cov)"""

    def rvs(self, n=1):
        return np.zeros((n, 4))

    def logpdf(self, x):
        return 0.0


@lru_cache(maxsize=None)
def model(name, m):
    d = MODEL_DIM[name]
    if name.startswith("lin"):
        return tda.LinearModel(np.ones((m, d)) + np.arange(m)[:, None])
    if name == "callable":
        return lambda th: xm.np_forward(th, m)[0]
    if name.startswith("batched"):
        return tda.BatchedModel(lambda th: xm.np_forward(th, m), m)
    if name.startswith("rosen"):
        return tda.Rosenbrock()
    if name.startswith("dev_") and name != "dev_nograd":
        return tda.DeviceModel(xwv.source("per_output" if name == "dev_gradwave" else "wave", None if name == "dev_wave" else "wave", m=m), m)
    return tda.DeviceModel(xm.source().split("__device__ double tda_gradient")[0] if name == "dev_nograd" else xm.source(), m)


@lru_cache(maxsize=None)
def likelihood(name, m):
    y = 0.1 * np.arange(m)
    if name.startswith("iso"):
        return tda.GaussianLogLike(y, 0.04 * np.eye(m))
    if name == "diag":
        return tda.GaussianLogLike(y, np.diag(0.04 * (1.0 + np.arange(m))))
    if name.startswith("dense"):
        return tda.GaussianLogLike(y, 0.04 * np.eye(m) + 0.01 * np.ones((m, m)))
    if name in ("adaptive", "adaptive257"):
        return tda.AdaptiveGaussianLogLike(y, 0.04 * np.eye(m))
    if name == "adaptive_dense":
        return tda.AdaptiveGaussianLogLike(y, 0.04 * np.eye(m) + 0.01 * np.ones((m, m)))
    if name.startswith("ll_term"):
        return tda.DeviceLogLike(xl.TERM_ONLY_SRC if name == "ll_term_nograd" else xl.STUDENT_T_SRC, y)
    return xlw.device_loglike("ar1", y, np.ones(m), source=xlw.without_grad(xlw.AR1_SRC) if name == "ll_wave_nograd" else None)


@lru_cache(maxsize=None)
def prior(name, d):
    if name == "mvn":
        return st.multivariate_normal(np.zeros(d), np.diag(1.0 + 0.5 * np.arange(d)))
    if name == "mvn_dense":
        return st.multivariate_normal(np.zeros(d), np.eye(d) + 0.1 * np.ones((d, d)))
    if name == "mvn_shifted":
        return st.multivariate_normal(np.ones(d), np.diag(1.0 + 0.5 * np.arange(d)))
    if name == "joint":
        return tda.JointPrior([st.norm(0.5, 2.0), st.uniform(-1.0, 3.0)] * (d // 2) + [st.norm(0.0, 1.0)] * (d % 2))
    if name == "joint_families":
        return tda.JointPrior(xp.components(d))
    if name == "dp_term":
        return tda.DevicePrior(xp.LOGNORMAL_SRC, d)
    if name == "dp_term_other":
        return tda.DevicePrior(xp.LOGNORMAL_SRC, d, p=0.5 * np.ones(d))
    if name == "dp_term_grad":
        return tda.DevicePrior(xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, d)
    if name == "dp_wave":
        return xpw.device_prior(xpw.cauchy_difference(d))
    if name == "dp_wave_nograd":
        return xpw.device_prior(xpw.cauchy_difference(d), source=xpw.CAUCHY_DIFF_SRC.split("__device__ double tda_logprior_grad")[0])
    if name == "dp_families":
        return tda.DevicePrior.from_distributions(xp.components(d))
    return st.norm()  # "scalar": a frozen scalar scipy distribution


@lru_cache(maxsize=None)
def proposal(name, d):
    if name == "grw":
        return tda.GaussianRandomWalk(np.eye(d))
    if name == "grw_adaptive":
        return tda.GaussianRandomWalk(np.eye(d), adaptive=True)
    if name == "pcn":
        return tda.CrankNicolson(0.1)
    if name == "am":
        return tda.AdaptiveMetropolis(np.eye(d))
    if name == "am_block":
        return tda.AdaptiveMetropolis(np.eye(d), block_moments=True)
    if name == "dreamz":
        return tda.DREAMZ(M0=10)
    if name == "dreamz_lhs":
        return tda.DREAMZ(M0=10, Z_method="lhs")
    if name == "dreamz_other":
        return tda.DREAMZ(M0=10, Z_method="sobol")
    if name == "dream":
        return tda.DREAM(M0=10)
    if name == "indep":
        return tda.IndependenceSampler(st.multivariate_normal(np.zeros(d), np.eye(d)))
    if name == "indep_other":
        return tda.IndependenceSampler(_OtherQ())
    if name == "owcn":
        return tda.OperatorWeightedCrankNicolson(0.5 * np.eye(d), scaling=0.5)
    if name == "owcn_adaptive":
        return tda.OperatorWeightedCrankNicolson(0.5 * np.eye(d), scaling=0.5, adaptive=True)
    if name == "owcn_adaptive_other":
        return tda.OperatorWeightedCrankNicolson(0.5 * np.eye(d) + np.triu(0.1 * np.ones((d, d)), 1), scaling=0.5, adaptive=True)
    if name == "mala":
        return tda.MALA(0.05)
    if name == "hmc":
        return tda.HMC(0.05, n_leapfrog=3)
    return _Subclass(np.eye(d))


@lru_cache(maxsize=None)
def posterior(level):
    mdl, like, pri = level
    m = 1 if mdl.startswith("rosen") else LIKE_OUTPUTS[like]
    post = tda.Posterior(prior(pri, MODEL_DIM[mdl]), likelihood(like, m), model("callable" if mdl == "wrapped" else mdl, m))
    return api._wrap_opaque_models([post])[0] if mdl == "wrapped" else post


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def name_of(levels, prop, em, randomize):
    return "%s|%s|%s|r%d" % (",".join("/".join(lv) for lv in levels), prop, em, randomize)


def _kept(name, one_in):
    return zlib.crc32(name.encode()) % one_in == 0


SINGLE_MODELS = ("lin4", "lin100", "callable", "wrapped", "batched", "batched100", "rosen", "dev", "dev100", "dev_nograd", "dev_wave",
                 "dev_wave_gradwave", "dev_gradwave")
SINGLE_LIKES = ("iso", "diag", "dense", "adaptive", "ll_term", "ll_term_nograd", "ll_wave", "ll_wave_nograd", "iso2049", "ll_term2049")
SINGLE_PRIORS = tuple(p for p in PRIORS if p not in ("mvn_shifted", "dp_term_other"))
HIER_MODELS = ("lin4", "lin100", "wrapped", "batched", "dev", "dev100", "dev_wave_gradwave")
HIER_LIKES = ("iso", "diag", "dense", "ll_term", "ll_wave_nograd")
HIER_PRIORS = ("mvn", "mvn_dense", "joint", "joint_families", "dp_term_grad", "dp_wave", "dp_families")
HIER_PROPOSALS = ("grw", "grw_adaptive", "pcn", "am", "am_block", "dreamz", "dream", "indep", "owcn", "mala", "hmc", "subclass")
HIER_THINNING = {2: 24, 3: 48, 4: 96, 5: 48, 6: 96, 7: 192}  # one case in ... of the product
# levels of the mixed two-level hierarchies (the mixtures the other tests build: adaptive coarse under isotropic fine, batched
# plus linear, Gaussian coarse plus DeviceLogLike fine, levels with different priors)
MIXED_LEVELS = (("lin4", "iso", "mvn"), ("lin4", "adaptive", "mvn"), ("lin4", "dense", "mvn"), ("lin4", "diag", "mvn_shifted"),
                ("batched", "iso", "mvn"), ("wrapped", "adaptive", "mvn"), ("dev", "iso", "mvn"), ("dev", "ll_term", "mvn"), ("dev", "ll_wave", "mvn"),
                ("dev", "iso", "dp_term"), ("dev", "ll_term", "dp_term"), ("dev", "diag", "dp_term_other"), ("dev_wave", "iso", "dp_wave"),
                ("dev", "adaptive", "joint"), ("lin4", "iso", "joint"), ("rosen", "iso", "mvn"))
MIXED_PROPOSALS = ("grw", "pcn", "am", "dreamz", "dream", "mala", "hmc")
# single cases: the rules that only a particular size, or a particular pair of levels, reaches
_L, _A = ("lin4", "iso", "mvn"), ("lin4", "adaptive", "mvn")
EXTRA = (
    ((("lin129", "iso", "mvn"),), "am", "-", 0),
    ((("lin4", "dense1025", "mvn"),), "grw", "-", 0),
    ((("batched", "dense2049", "mvn"),), "grw", "-", 0),
    ((("dev", "dense2049", "mvn"),), "am", "-", 0),
    ((("dev", "dense", "mvn"),), "mala", "-", 0),
    ((("lin4", "adaptive257", "mvn"), ("lin4", "iso", "mvn")), "grw", "si", 0),
    ((("lin4", "adaptive257", "mvn"), ("lin4", "iso", "mvn")), "dreamz", "si", 0),
    ((("batched", "adaptive257", "mvn"), ("lin4", "iso", "mvn")), "grw", "si", 0),
    ((("lin4", "adaptive_dense", "mvn"), _L), "grw", "diag", 0),
    ((("lin4", "adaptive_dense", "mvn"), _L), "grw", "si", 0),
    ((_A, _A, _A, _A, _L), "grw", "si", 0),
    ((_A, _A, _A, _L), "grw", "si", 0),
    ((_A, _A, _L), "dreamz", "si", 0),
    ((_A, _A, _L), "dreamz", "diag", 0),
    ((_A, _L, _L), "grw", "si", 0),
    ((_A, _L), "grw", "si", 1),
    ((_L, ("lin4", "dense", "mvn")), "dreamz", "-", 0),
    ((("rosen", "iso", "joint"),), "dreamz", "-", 0),
    ((("rosen100", "iso", "mvn"),), "dreamz", "-", 0),
    ((("rosen100", "iso", "mvn"),), "grw", "-", 0),
    ((("dev", "ll_term_nograd", "dp_term_grad"),), "mala", "-", 0),
    ((("dev", "ll_wave_nograd", "dp_term_grad"),), "mala", "-", 0),
    ((("dev", "ll_term_nograd", "mvn"),), "mala", "-", 0),
    ((("dev", "ll_wave_nograd", "mvn"),), "mala", "-", 0),
    ((("dev", "iso2049", "mvn"),), "mala", "-", 0),
    ((("lin4", "iso", "mvn"),), "owcn_adaptive_other", "-", 0),
    ((("lin100", "adaptive", "mvn"), ("lin100", "iso", "mvn")), "pcn", "diag", 0),
    ((("lin100", "adaptive", "mvn"), ("lin100", "iso", "mvn")), "pcn", "si", 0),
)


def cases():
    """(name, levels, proposal, error model, randomize) in a fixed order; a level is (model, likelihood, prior)"""
    out = []
    for lv in itertools.product(SINGLE_MODELS, SINGLE_LIKES, SINGLE_PRIORS):
        for prop in PROPOSALS:
            if _kept(name_of((lv,), prop, "-", 0), 6):
                out.append(((lv,), prop, "-", 0))
    for n in (2, 3, 4, 5, 6, 7):
        for lv in itertools.product(HIER_MODELS, HIER_LIKES, HIER_PRIORS):
            below = (lv[0], "adaptive", lv[2])
            for levels in ((lv,) * n, (below,) * (n - 1) + (lv,)):
                for prop, em, rnd in itertools.product(HIER_PROPOSALS, ERROR_MODELS, (0, 1)):
                    if rnd and n != 2:  # (sample(): a Delayed Acceptance option)
                        continue
                    if _kept(name_of(levels, prop, em, rnd), HIER_THINNING[n]):
                        out.append((levels, prop, em, rnd))
    for coarse, fine in itertools.product(MIXED_LEVELS, MIXED_LEVELS):
        for prop, em in itertools.product(MIXED_PROPOSALS, ERROR_MODELS):
            if _kept(name_of((coarse, fine), prop, em, 0), 6):
                out.append(((coarse, fine), prop, em, 0))
    out.extend(EXTRA)
    seen, unique = set(), []
    for c in out:
        nm = name_of(*c)
        if nm not in seen:
            seen.add(nm)
            unique.append((nm,) + c)
    return unique


# ---- one case's outcome ------------------------------------------------------------------------------------------------------------
def _digest(data):
    return hashlib.sha1(data).hexdigest()[:16]


def _describe(v):
    if isinstance(v, np.ndarray):
        return {"shape": list(v.shape)}
    if isinstance(v, (tuple, list)):
        return [_describe(x) for x in v]
    if isinstance(v, dict):
        return {k: _describe(x) for k, x in v.items()}
    if isinstance(v, (np.integer, np.floating, np.bool_)):
        return v.item()
    return v


def _describe_level(low):
    out = {"keys": sorted(low), "noise_kind": int(low["noise_kind"]),
           "shapes": {k: list(v.shape) for k, v in sorted(low.items()) if isinstance(v, np.ndarray)}}
    ps = low.get("prior_source")
    if ps is not None:
        out["prior_source"] = dict({k: _describe(v) for k, v in ps.items() if k not in ("source", "p", "q")}, keys=sorted(ps),
                                   source=[len(ps["source"]), _digest(ps["source"].encode())],
                                   p=_digest(np.ascontiguousarray(ps["p"], dtype=np.float64).tobytes()),
                                   q=_digest(np.ascontiguousarray(ps["q"], dtype=np.float64).tobytes()))
    return out


def outcome(levels, prop, em, randomize):
    """the first refusal reason (a string), or the description of the plan (a dict)"""
    posts = [posterior(lv) for lv in levels]
    plan = api._device_plan(posts, proposal(prop, MODEL_DIM[levels[0][0]]), em == "diag",
                            {"-": None, "si": "state-independent", "sd": "state-dependent", "diag": "state-independent"}[em], bool(randomize))
    if plan is None:
        return api._refusal[0]
    return {"proposal": _describe(plan[1]), "levels": [_describe_level(low) for low in plan[0]]}


def names_digest(names):
    return _digest("\n".join(names).encode())


# ---- the refusal sites of the pass, in the order of the code; each is recognised by its text ------------------------------------
_WHO = r"(DevicePrior|JointPrior of scipy families \(source-defined prior\))"
_GRAD = r"(MALA|HMC)"  # the proposals on the gradient of the log-posterior share their rules, each worded with its own name
SITES = (
    ("levels or proposal class", r"more than 6 levels \(or none\), or a proposal class"),
    ("five / six levels: error model, DREAM(Z)", r"more than 4 levels are lowered without error model"),
    ("posterior without a lowering", r"a posterior the engine cannot lower"),
    ("more than 128 parameters", r"more than 128 parameters$"),
    ("prior: models / noise", _WHO + r" is compiled into the programs of the levels' models"),
    ("prior: level cap", _WHO + r": hierarchies of at most 4 levels"),
    ("prior: DREAM(Z)", _WHO + r" is not lowered under DREAM\(Z\)"),
    ("prior: pCN / OWCN", _WHO + r" is not lowered under \w+ \(it needs a Gaussian prior\)"),
    ("prior: MALA, coupled without gradient", _WHO + r" is not lowered under " + _GRAD + r": a prior that couples parameters needs"),
    ("prior: MALA, term without gradient", _WHO + r" is not lowered under " + _GRAD + r": it needs a DevicePrior whose source defines"),
    ("prior: MALA, single level", _WHO + r" under " + _GRAD + r": single level only"),
    ("prior: MALA, model gradient", _WHO + r" under " + _GRAD + r" needs __device__ double tda_gradient"),
    ("prior: MALA, 2048 outputs", _WHO + r" under " + _GRAD + r" over a source-defined model: at most 2048 outputs"),
    ("prior: MALA, coupled likelihood gradient", _WHO + r" under " + _GRAD + r" with a DeviceLogLike that couples outputs needs"),
    ("prior: MALA, likelihood term gradient", _WHO + r" under " + _GRAD + r" with a DeviceLogLike needs"),
    ("prior: IndependenceSampler", _WHO + r" is not lowered under IndependenceSampler"),
    ("prior: error model", _WHO + r" is not lowered together with an adaptive error model"),
    ("prior: randomize", _WHO + r" is not lowered with randomize_subchain_length"),
    ("likelihood: model", r"DeviceLogLike is compiled into the program of its level's model"),
    ("likelihood: level cap", r"DeviceLogLike: hierarchies of at most 4 levels"),
    ("likelihood: DREAM(Z)", r"DeviceLogLike is not lowered under DREAM\(Z\)"),
    ("likelihood: OWCN", r"DeviceLogLike is not lowered under OperatorWeightedCrankNicolson"),
    ("likelihood: IndependenceSampler", r"DeviceLogLike is not lowered under IndependenceSampler"),
    ("likelihood: error model", r"DeviceLogLike is not lowered together with an adaptive error model"),
    ("likelihood: randomize", r"DeviceLogLike is not lowered with randomize_subchain_length"),
    ("likelihood: MALA, level / prior", _GRAD + r" with a DeviceLogLike: single level, multivariate normal prior"),
    ("likelihood: MALA, coupled gradient", _GRAD + r" with a DeviceLogLike that couples outputs needs"),
    ("likelihood: MALA, term gradient", _GRAD + r" with a DeviceLogLike needs"),
    ("more than 64 parameters", r"more than 64 parameters are lowered for"),
    ("diagonal error model: adaptive covariances", r"error_model_covariance='diagonal' needs diagonal covariances"),
    ("adaptive likelihood: hierarchy, outputs", r"AdaptiveGaussianLogLike on the device: coarse levels"),
    ("dense noise: level cap", r"a dense observation covariance in a hierarchy: at most 4 levels"),
    ("dense noise: callback / source, 2048 outputs", r"a dense observation covariance beside a callback / source-defined model"),
    ("dense noise: linear", r"a dense observation covariance with a linear model is lowered for"),
    ("diagonal error model: level noise", r"the diagonal error model takes its Sigma_e from"),
    ("dense error model: finest level", r"dense error model: the finest level must have an isotropic likelihood"),
    ("dense error model: levels below", r"dense error model: every level below the finest needs"),
    ("dense error model: more than 256 outputs", r"dense error model with more than 256 outputs"),
    ("DREAM's shared archive", r"DREAM's shared archive is single-level"),
    ("Rosenbrock", r"the Rosenbrock model is fused into the DREAM\(Z\) kernel only"),
    ("JointPrior: pCN / Rosenbrock", r"JointPrior: not with CrankNicolson or the Rosenbrock model"),
    ("JointPrior: dense noise", r"JointPrior: not with a dense observation covariance"),
    ("external models: level cap", r"hierarchies of callback / source-defined models: at most 4 levels"),
    ("external models: proposals of a hierarchy", r"hierarchies of callback / source-defined models run under"),
    ("external models: noise / prior covariance", r"callback / source-defined models need isotropic / diagonal noise"),
    ("MALA: model gradient", _GRAD + r" over a source-defined model needs"),
    ("MALA: source-defined model, noise / outputs", _GRAD + r" over a source-defined model: isotropic or diagonal noise"),
    ("HMC: otherwise", r"HMC: single level, a DeviceModel with tda_gradient"),
    ("MALA: otherwise", r"MALA: single level, linear model, Gaussian prior"),
    ("OWCN: level / operators", r"OperatorWeightedCrankNicolson: single level, operators"),
    ("OWCN: adaptive", r"adaptive OperatorWeightedCrankNicolson \(per-chain operators\)"),
    ("IndependenceSampler", r"IndependenceSampler: single level, Gaussian q"),
    ("one prior for the hierarchy", r"the levels of a hierarchy must share one prior"),
    ("option of a proposal", r"an option of \w+ the engine does not implement"),
)


def site_of(reason):
    hits = [name for name, pattern in SITES if re.match(pattern, reason)]
    assert len(hits) == 1, (reason, hits)
    return hits[0]


class _Table:
    """values once, in the order of their first use"""

    def __init__(self):
        self.rows, self.index = [], {}

    def add(self, value):
        key = json.dumps(value, sort_keys=True)
        if key not in self.index:
            self.index[key] = len(self.rows)
            self.rows.append(value)
        return self.index[key]


def load():
    """the file with its outcomes written out again as `outcome()` returns them"""
    with open(PATH) as fh:
        m = json.load(fh)
    levels = [dict(lv, keys=m["keysets"][lv["keys"]]) for lv in m["levels"]]
    m["outcomes"] = [o if isinstance(o, str) else {"proposal": m["proposals"][o[0]], "levels": [levels[i] for i in o[1]]} for o in m["outcomes"]]
    return m


def main():
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
    keysets, levels, proposals, outcomes, picks = _Table(), _Table(), _Table(), _Table(), []
    all_cases = cases()
    reached = {name: 0 for name, _ in SITES}
    for nm, lvs, prop, em, rnd in all_cases:
        res = outcome(lvs, prop, em, rnd)
        if isinstance(res, str):
            reached[site_of(res)] += 1
        else:  # a plan: its proposal and its levels by their numbers in the tables, a level's keys likewise
            res = [proposals.add(res["proposal"]), [levels.add(dict(lv, keys=keysets.add(lv["keys"]))) for lv in res["levels"]]]
        picks.append(outcomes.add(res))
    out = {"commit": commit, "n_cases": len(all_cases), "names": names_digest([c[0] for c in all_cases]), "sites": reached, "keysets": keysets.rows,
           "levels": levels.rows, "proposals": proposals.rows, "outcomes": outcomes.rows, "cases": picks}
    with open(PATH, "w") as fh:  # one entry per line
        fh.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":"))) for k, v in out.items()) + "\n}\n")
    lowered = sum(not isinstance(outcomes.rows[i], str) for i in picks)
    print("%d cases at %s: %d lowered, %d refused, %d distinct outcomes" % (len(picks), commit[:7], lowered, len(picks) - lowered, len(outcomes.rows)))
    for name, _ in SITES:
        print("%6d  %s" % (reached[name], name))


if __name__ == "__main__":
    main()
