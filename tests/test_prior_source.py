"""Source-defined priors (DevicePrior, JointPrior of scipy families, TDA_PRIOR_SOURCE) without a device: the shipped term
library against scipy's logpdf, the host methods, the lowering rules, the host protocol and the oracle level against the
reference's own chains (tests/golden/g19_prior_families_*.npz, gen_golden_prior_source.py), and the hiprtc program
compiled offline for gfx950 with the prior switch."""
import re
import warnings

import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from . import extloglike as xl
from . import extprior as xp
from .extengine import assert_host_classes_replay, assert_oracle_replays, golden_proposal as g19_oracle_proposal  # noqa: F401 (test_gpu_prior_source)
from .extmodel import np_forward, source
from .extprior import host_library as _host_library
from .extprogram import STEP_KERNELS as KERNELS, assembly, assert_switch_is_an_option_only, assert_without_scratch, compile_program, needs_hipcc

G19 = ("g19_prior_families_grw", "g19_prior_families_am")
TERM_SIG = "__device__ double tda_logprior_term(double x, double p, double q, int j)"


def _gauss_like(m):
    import tinyda_amd as tda

    return tda.GaussianLogLike(np.zeros(m), 0.04 * np.eye(m))


def _posterior(prior, m=3, model="device", like=None):
    import tinyda_amd as tda

    d = prior.dim
    if model == "device":
        mdl = tda.DeviceModel(source(), m, reference=lambda t: np_forward(t, m)[0])
    elif model == "linear":
        mdl = tda.LinearModel(np.ones((m, d)))
    else:
        mdl = tda.BatchedModel(lambda th: np_forward(th, m), m)
    return tda.Posterior(prior, _gauss_like(m) if like is None else like, mdl)


def _family_prior(d):
    import tinyda_amd as tda

    return tda.JointPrior(xp.components(d))


def _device_prior(d, reference=True):
    import tinyda_amd as tda

    p, q = 0.1 * np.arange(d) / d, 0.5 + 0.01 * np.arange(d)
    return tda.DevicePrior(xp.LOGNORMAL_SRC, d, p, q, reference=xp.LognormalPrior(p, q) if reference else None)


# ---- 1. the shipped term library against scipy ------------------------------------------------------------------------------
def test_term_library_against_scipy_logpdf(tmp_path):
    """Every family: 2000 draws from the component, 200 wide normal points (most of them outside a bounded support) and the
    support's edges.  The -inf sets must be identical.  Bound: the term is g(z) + c, and the library and scipy each reach it
    from x by at most 8 rounded operations and libm calls (z: 2, log / log1p: 1, g: up to 4, + c: 1), each within 1 ulp of a
    result no larger than M = max(1, |logpdf|, |c|, |g|) -- g and c may cancel, and a rounding of z moves log z by eps
    absolutely, hence the 1.  So the two differ by at most 16 eps M.  The Weibull power alone is taken another way than
    scipy's pow: exp(c log z) turns the roundings of log z and of the product into a relative (|c log z| + 1) eps of z^c,
    which that family's bound adds."""
    names = xp.FAMILY_NAMES
    comps = [xp.component(n, loc=0.3, scale=1.7) for n in names]
    term, rows = _host_library(tmp_path, comps)
    rng = np.random.default_rng(0)
    eps = np.finfo(float).eps
    for j, (n, c) in enumerate(zip(names, comps)):
        lo, hi = xp.support(c)
        edges = [v for v in (lo, hi) if np.isfinite(v)]
        x = np.concatenate([c.rvs(size=2000, random_state=rng), rng.normal(0.0, 3.0, 200), edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = c.logpdf(x)
        mine = term(x, j)
        assert not np.any(np.isnan(mine)) and not np.any(mine == np.inf), n
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(mine)), (n, x[fin != np.isfinite(mine)])
        assert (~fin).sum() > 0 or not edges, n
        cj = rows[j][3]
        bound = 16 * eps * np.maximum.reduce([np.ones(fin.sum()), np.abs(ref[fin]), np.full(fin.sum(), abs(cj)), np.abs(ref[fin] - cj)])
        if n == "weibull_min":
            z, shape = (x[fin] - rows[j][4]) / rows[j][5], rows[j][1]
            bound = bound + eps * (np.abs(shape * np.log(z)) + 1.0) * z ** shape
        err = np.abs(mine[fin] - ref[fin])
        print(n, "max err / bound", np.max(err / bound), "outside", (~fin).sum())
        assert np.all(err <= bound), (n, np.max(err / bound))


def test_family_component_declines_when_scipy_helpers_are_missing(monkeypatch):
    """the lowering reads a frozen distribution through scipy's own _parse_args / _argcheck: without them the component is
    host-only, not an AttributeError"""
    import tinyda_amd as tda
    from tinyda_amd import likelihoods as lk

    comp = st.gamma(2.0, scale=3.0)
    assert lk._family_component(comp) is not None

    def gone(self):
        raise AttributeError("_argcheck")

    monkeypatch.setattr(type(comp.dist), "_argcheck", property(gone), raising=False)
    assert not hasattr(comp.dist, "_argcheck")
    assert lk._family_component(comp) is None and tda.JointPrior([comp])._source_lowering() is None


def test_family_lowering_tables_and_what_stays_host_only():
    import tinyda_amd as tda
    from tinyda_amd import _lib, likelihoods as lk

    comps = xp.components(13)
    kinds, loc, scale, src = tda.JointPrior(comps)._source_lowering()
    assert kinds.dtype == np.int32 and np.all(kinds == _lib.PRIOR_SOURCE)
    assert np.array_equal(loc, [xp.FAMILY_PARAMS[n][1] for n in xp.FAMILY_NAMES])
    assert np.array_equal(scale, [xp.FAMILY_PARAMS[n][2] for n in xp.FAMILY_NAMES])
    assert src.endswith(lk.family_library_source()) and src.startswith("#define TDA_PRIOR_DIM 13\n")
    # exact literals: the tables read back bit for bit
    for name, col in (("tda_prior_a", 1), ("tda_prior_b", 2), ("tda_prior_c", 3)):
        vals = re.search(name + r"\[13\] = \{([^}]*)\}", src).group(1).split(", ")
        assert [float(v) for v in vals] == [lk._family_component(c)[col] for c in comps]
    fam = re.search(r"tda_prior_family\[13\] = \{([^}]*)\}", src).group(1).split(", ")
    assert [lk._FAMILIES[int(f)][0] for f in fam] == list(xp.FAMILY_NAMES)
    # all-norm / uniform lists: today's three arrays
    low = tda.JointPrior([st.norm(0.5, 2.0), st.uniform(-1.0, 3.0)])._lowering()
    assert len(low) == 3 and np.array_equal(low[0], [0, 1]) and np.array_equal(low[1], [0.5, -1.0]) and np.array_equal(low[2], [2.0, 3.0])
    # anything else stays with the host protocol
    class Mine:
        def logpdf(self, x):
            return 0.0

    for other in (st.lognorm, Mine(), st.poisson(3.0), st.gumbel_r(0.0, 1.0), st.gamma(2.0, scale=-1.0)):
        assert tda.JointPrior([st.norm(0.0, 1.0), other])._source_lowering() is None
    # truncnorm far in a tail: the constant stays finite and exact
    far = st.truncnorm(8.0, 9.0)
    np.testing.assert_allclose(lk._family_component(far)[3] - 0.5 * 8.5 ** 2, far.logpdf(8.5), rtol=1e-13)


# ---- 2. DevicePrior ------------------------------------------------------------------------------------------------------
def test_device_prior_validation_and_host_methods():
    import tinyda_amd as tda

    d = 4
    pr = _device_prior(d)
    th = np.array([0.5, 1.0, 2.0, 0.1])
    ref = sum(st.lognorm(pr.q[j], scale=np.exp(pr.p[j])).logpdf(th[j]) for j in range(d))
    np.testing.assert_allclose(pr.logpdf(th), ref, rtol=1e-13)
    assert pr.logpdf(np.array([0.5, -1.0, 2.0, 0.1])) == -np.inf
    assert np.asarray(pr.rvs()).shape == (d,)
    kinds, p, q, src = pr._source_lowering()
    assert np.all(kinds == 2) and np.array_equal(p, pr.p) and np.array_equal(q, pr.q) and src == xp.LOGNORMAL_SRC
    bare = tda.DevicePrior(xp.LOGNORMAL_SRC, d)
    assert np.array_equal(bare.p, np.zeros(d)) and np.array_equal(bare.q, np.ones(d))
    with pytest.raises(TypeError, match="no host reference implementation"):
        bare.logpdf(th)
    with pytest.raises(TypeError, match="initial_parameters"):
        bare.rvs()
    with pytest.raises(ValueError):
        tda.DevicePrior(xp.LOGNORMAL_SRC, d, np.zeros(d + 1))
    with pytest.raises(ValueError):
        tda.DevicePrior(xp.LOGNORMAL_SRC, d, q=np.full(d, np.inf))
    with pytest.raises(ValueError, match="tda_logprior_term"):
        tda.DevicePrior("// " + TERM_SIG + "\n/* tda_logprior_term( */", d)
    # a JointPrior as the reference
    jp = _family_prior(5)
    dp = tda.DevicePrior(jp._source_lowering()[3], 5, jp._source_lowering()[1], jp._source_lowering()[2], reference=jp)
    u = np.random.default_rng(3).random((4, 5))
    assert np.array_equal(dp.ppf(u), jp.ppf(u)) and dp.logpdf(jp.ppf(u)[0]) == jp.logpdf(jp.ppf(u)[0])


# ---- 3. lowering ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 96, 128])
def test_device_plan_single_level(d):
    import tinyda_amd as tda
    from tinyda_amd import api

    for prior in (_family_prior(d), _device_prior(d), _device_prior(d, reference=False)):
        post = _posterior(prior)
        for prop, kind in ((tda.GaussianRandomWalk(np.eye(d)), 0), (tda.GaussianRandomWalk(np.eye(d), adaptive=True), 0),
                           (tda.AdaptiveMetropolis(np.eye(d)), 2), (tda.AdaptiveMetropolis(np.eye(d), adaptive=True), 2)):
            plan = api._device_plan([post], prop)
            assert plan is not None, api._refusal
            low = plan[0][0]
            assert plan[1]["kind"] == kind and np.all(low["prior_joint"][0] == 2)
            kinds, p, q, src = prior._source_lowering()
            assert np.array_equal(low["prior_joint"][1], p) and np.array_equal(low["prior_joint"][2], q)
            assert low["prior_source"]["source"] == src
            # one program: the model's source, then the prior's
            assert low["source"].index("tda_forward") < low["source"].index("tda_logprior_term") and low["source"].endswith(src)
    # diagonal noise, and a DeviceLogLike: model, likelihood, prior
    m = 3
    diag = tda.GaussianLogLike(np.zeros(m), np.diag(0.04 + 0.01 * np.arange(m)))
    assert api._device_plan([_posterior(_family_prior(d), like=diag)], tda.GaussianRandomWalk(np.eye(d))) is not None
    like = tda.DeviceLogLike(xl.STUDENT_T_SRC, np.zeros(m), np.ones(m))
    plan = api._device_plan([_posterior(_family_prior(d), like=like)], tda.AdaptiveMetropolis(np.eye(d)))
    assert plan is not None, api._refusal
    s = plan[0][0]["source"]
    assert s.index("tda_forward") < s.index("tda_loglike_term") < s.index("tda_logprior_term") and plan[0][0]["noise_kind"] == 4


def test_device_plan_hierarchies():
    import tinyda_amd as tda
    from tinyda_amd import api

    jp, dp = _family_prior(2), _device_prior(2)
    grw, am = tda.GaussianRandomWalk(np.eye(2)), tda.AdaptiveMetropolis(np.eye(2))
    for prior in (jp, dp):
        a, b = _posterior(prior, m=3), _posterior(prior, m=5)
        assert api._device_plan([a, b], grw) is not None, api._refusal
        assert api._device_plan([a, b, a], am) is not None, api._refusal
        assert api._device_plan([a, b, a, b], grw) is not None, api._refusal
    p96 = _posterior(_family_prior(96))
    assert api._device_plan([p96, p96], tda.GaussianRandomWalk(np.eye(96))) is not None, api._refusal
    # one prior for the hierarchy
    other = tda.JointPrior(xp.components(2, ("gamma", "lognorm")))
    assert api._device_plan([_posterior(jp), _posterior(other)], grw) is None and "share one prior" in api._refusal[0]
    mvn = st.multivariate_normal(np.zeros(2), np.eye(2))
    mvn.dim = 2
    assert api._device_plan([_posterior(mvn), _posterior(jp)], grw) is None and "share one prior" in api._refusal[0]
    dp2 = tda.DevicePrior(xp.LOGNORMAL_SRC, 2, dp.p + 1.0, dp.q)
    assert api._device_plan([_posterior(dp), _posterior(dp2)], grw) is None and "share one prior" in api._refusal[0]


def test_device_plan_refusals():
    import tinyda_amd as tda
    from tinyda_amd import api

    grw = tda.GaussianRandomWalk(np.eye(2))
    for prior, who in ((_family_prior(2), "JointPrior of scipy families"), (_device_prior(2), "DevicePrior")):
        t = _posterior(prior)

        def refused(posts, prop, *needles, **kw):
            assert api._device_plan(posts, prop, **kw) is None
            assert who in api._refusal[0], api._refusal
            for n in needles:
                assert n in api._refusal[0], api._refusal

        refused([_posterior(prior, model="linear")], grw, "DeviceModel")
        refused([_posterior(prior, model="batched")], grw, "DeviceModel")
        refused([t, _posterior(prior, model="linear")], grw, "DeviceModel")
        refused([_posterior(prior, like=tda.GaussianLogLike(np.zeros(3), 0.04 * np.eye(3) + 0.01))], grw, "isotropic / diagonal noise")
        refused([t], tda.DREAMZ(M0=10), "DREAM(Z)")
        refused([t], tda.DREAM(M0=10), "DREAM(Z)")
        refused([t], tda.CrankNicolson(0.1), "CrankNicolson", "Gaussian prior")
        refused([t], tda.OperatorWeightedCrankNicolson(0.5 * np.eye(2), 0.5), "OperatorWeightedCrankNicolson")
        refused([t], tda.MALA(0.05), "MALA")
        refused([t], tda.IndependenceSampler(st.multivariate_normal(np.zeros(2), np.eye(2))), "IndependenceSampler")
        refused([t, t], grw, "error model", error_model="state-independent")
        refused([t, t], grw, "error model", error_model="state-independent", diagonal_error_model=True)
        refused([t, t], grw, "randomize_subchain_length", randomize=True)
        refused([t] * 5, grw, "at most 4 levels")
    # more than 128 parameters: the existing rule
    assert api._device_plan([_posterior(_family_prior(129))], tda.GaussianRandomWalk(np.eye(129))) is None
    assert "128 parameters" in api._refusal[0]
    # a component outside the table: the posterior cannot be lowered at all
    odd = tda.JointPrior([st.norm(0.0, 1.0), st.gumbel_r(0.0, 1.0)])
    odd.dim = 2
    assert api._device_plan([_posterior(odd)], grw) is None and "DevicePrior" in api._refusal[0]


def test_gaussian_priors_plan_as_before():
    import tinyda_amd as tda
    from tinyda_amd import api

    d, m = 3, 4
    joint = tda.JointPrior([st.norm(0.5, 2.0), st.uniform(-1.0, 3.0), st.norm(-0.5, 0.3)])
    for model in ("device", "linear", "batched"):
        post = _posterior(joint, m=m, model=model)
        plan = api._device_plan([post], tda.GaussianRandomWalk(np.eye(d)))
        low = plan[0][0]
        assert "prior_source" not in low and len(low["prior_joint"]) == 3
        assert np.array_equal(low["prior_joint"][0], [0, 1, 0]) and low["prior_joint"][0].dtype == np.int32
        assert np.array_equal(low["prior_mean"], [0.5, 0.5, -0.5]) and np.array_equal(low["prior_cov"], np.diag([4.0, 0.75, 0.09]))
        if model == "device":
            assert low["source"] == post.model.source
        assert api._device_plan([post], tda.DREAMZ(M0=10)) is not None
        assert api._device_plan([post], tda.CrankNicolson(0.1)) is None and "JointPrior: not with CrankNicolson" in api._refusal[0]
    mvn = st.multivariate_normal(np.arange(d) * 0.1, np.diag([1.0, 2.0, 3.0]))
    mvn.dim = d
    post = _posterior(mvn, m=m)
    for prop in (tda.GaussianRandomWalk(np.eye(d)), tda.CrankNicolson(0.1), tda.DREAMZ(M0=10), tda.MALA(0.05)):
        plan = api._device_plan([post], prop)
        assert plan is not None, api._refusal
        low = plan[0][0]
        assert "prior_source" not in low and "prior_joint" not in low and low["source"] == post.model.source
        assert np.array_equal(low["prior_mean"], mvn.mean) and np.array_equal(low["prior_cov"], mvn.cov)
    # the draws of missing initial parameters for norm / uniform priors: the generator and the arithmetic they had
    a = api._joint_rvs(joint._lowering(), 1, api._host_rng(7, api._TAG_THETA0, 3))[0]
    rng = np.random.default_rng([7, api._TAG_THETA0, 3])
    u, z = rng.random((1, d)), rng.standard_normal((1, d))
    assert np.array_equal(a, np.where(np.array([0, 1, 0]) == 0, np.array([0.5, -1.0, -0.5]) + np.array([2.0, 3.0, 0.3]) * z, np.array([0.5, -1.0, -0.5]) + np.array([2.0, 3.0, 0.3]) * u)[0])


def test_source_prior_starts_are_keyed_by_global_chain_id():
    from tinyda_amd import api

    jp = _family_prior(13)
    whole = api._source_prior_starts(jp, 6, 0, 11)
    shard = api._source_prior_starts(jp, 3, 3, 11)
    assert all(np.array_equal(a, b) for a, b in zip(whole[3:], shard))
    fp = xp.FamilyPrior(jp.distributions)
    assert np.all(fp.inside(np.stack(whole))) and not np.array_equal(whole[0], whole[1])
    assert not np.array_equal(whole[0], api._source_prior_starts(jp, 1, 0, 12)[0])
    # the draw of chain c: its own generator's uniforms through the components' quantile functions
    u = np.random.default_rng([11, api._TAG_THETA0, 4]).random(13)
    assert np.array_equal(whole[4], [c.ppf(v) for c, v in zip(jp.distributions, u)])
    # a DevicePrior draws through its reference: ppf when it has one, else rvs(random_state=generator); none: an error that says so
    import tinyda_amd as tda

    low = jp._source_lowering()
    assert np.array_equal(np.stack(api._source_prior_starts(tda.DevicePrior(low[3], 13, low[1], low[2], reference=jp), 6, 0, 11)), np.stack(whole))
    dp = _device_prior(3)
    a, b = api._source_prior_starts(dp, 2, 5, 1), api._source_prior_starts(dp, 1, 6, 1)
    assert np.array_equal(a[1], b[0]) and np.all(np.stack(a) > 0)
    with pytest.raises(TypeError, match="initial_parameters"):
        api._source_prior_starts(_device_prior(3, reference=False), 2, 0, 1)


def test_auto_backend_falls_back_with_one_warning():
    import tinyda_amd as tda
    from tinyda_amd.api import HostFallbackWarning

    jp = _family_prior(2)
    post = _posterior(jp, model="linear")
    th0 = np.array([c.ppf(0.5) for c in jp.distributions])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.GaussianRandomWalk(0.01 * np.eye(2)), 20, n_chains=2, initial_parameters=th0, seed=1, backend="auto",
                         force_sequential=True)
    fb = [x for x in w if issubclass(x.category, HostFallbackWarning)]
    assert len(fb) == 1 and "JointPrior of scipy families" in str(fb[0].message)
    assert res["backend"] == "host" and len(res["chain_0"]) == 21
    with pytest.raises(tda.EngineError, match="JointPrior of scipy families"):
        tda.sample(post, tda.GaussianRandomWalk(0.01 * np.eye(2)), 20, n_chains=2, initial_parameters=th0, seed=1, backend="hip")
    with pytest.raises(tda.EngineError, match="DevicePrior"):
        tda.sample(_posterior(_device_prior(2)), tda.MALA(0.05), 20, n_chains=2, initial_parameters=th0, seed=1, backend="hip")


# ---- 4. host protocol and oracle level against the reference's chains ---------------------------------------------------------
def _g19_components(g):
    return [xp.component(str(n), tuple(g["shapes"][j, :int(g["n_shapes"][j])]), float(g["loc"][j]), float(g["scale"][j]))
            for j, n in enumerate(g["families"])]


@pytest.mark.parametrize("name", G19)
def test_host_classes_replay_reference_chain(golden, monkeypatch, name):
    import tinyda_amd as tda

    g = golden(name)
    m = g["data"].shape[0]
    comps = _g19_components(g)
    post = tda.Posterior(tda.JointPrior(comps), tda.GaussianLogLike(g["data"], float(g["sigma2"]) * np.eye(m)),
                         tda.DeviceModel(source(), m, reference=lambda t: np_forward(t, m)[0]))
    assert post.prior._lowering() is None and len(post.prior._source_lowering()) == 4
    assert_host_classes_replay(g, post, monkeypatch)


@pytest.mark.parametrize("name", G19)
def test_oracle_level_replays_reference_chain(golden, name):
    g = golden(name)
    m = g["data"].shape[0]
    prior = xp.FamilyPrior(_g19_components(g))
    level = orc.CallableGaussianLevel(lambda t: np_forward(t, m), g["data"], "iso", float(g["sigma2"]), prior)
    assert_oracle_replays(g, level)
    assert int(g["n_outside"]) >= 1
    assert np.all(prior.inside(g["theta"].reshape(-1, prior.dim)))


# ---- 5. the hiprtc program with the prior switch, compiled offline as shipped ------------------------------------------------
@needs_hipcc
@pytest.mark.parametrize("loglike", [False, True])
def test_prior_program_compiles_for_gfx950_without_scratch(tmp_path, loglike):
    """the user source is what sample() hands over: the model (+ the likelihood), the generated 13-family prologue at d = 128,
    the shipped library"""
    prior_src = _family_prior(128)._source_lowering()[3]
    user = source() + (xl.KINDS["t"][0] if loglike else "") + "\n" + prior_src
    assert_without_scratch(tmp_path, "prior", user, ["TDA_PRIOR_SOURCE"] + (["TDA_LOGLIKE_SOURCE"] if loglike else []), KERNELS)


@needs_hipcc
def test_handwritten_prior_compiles_and_missing_function_names_the_signature(tmp_path):
    rc, log, usage = compile_program(tmp_path, "lognormal", source() + xp.LOGNORMAL_SRC, ["TDA_PRIOR_SOURCE"])
    assert rc == 0 and usage["tda_user_steps"]["ScratchSize [bytes/lane]"] == 0, log[-2000:]
    rc, log, _ = compile_program(tmp_path, "no_term", source(), ["TDA_PRIOR_SOURCE"])
    assert rc != 0 and "tda_logprior_term_missing" in log and TERM_SIG in log
    # the MALA program does not take the switch
    rc, log, _ = compile_program(tmp_path, "mala", source() + xp.LOGNORMAL_SRC, ["TDA_PRIOR_SOURCE", "TDA_USER_MALA"])
    assert rc != 0 and "TDA_PRIOR_SOURCE" in log


def test_program_text_never_defines_the_prior_switch():
    """without -DTDA_PRIOR_SOURCE the programs are what they were: the file and its headers never define the switch (the host's
    option list: tests/test_user_build.py)"""
    header = assert_switch_is_an_option_only("TDA_PRIOR_SOURCE", ("tda_prior_families.h",))
    assert re.search(r"TDA_PRIOR_SOURCE\s*=\s*2", header) and TERM_SIG in header


@needs_hipcc
def test_gaussian_prior_program_does_not_see_a_prior_in_the_source(tmp_path):
    """the prior's code sits behind the switch: without it the step program's instructions are the same whether or not the
    source holds a tda_logprior_term"""
    assert assembly(tmp_path, "with_term", source() + xp.LOGNORMAL_SRC, []) == assembly(tmp_path, "without", source(), [])
