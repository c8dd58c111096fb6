"""NUTS without a GPU: the NumPy twin (tests/extnuts.py) tied to HMC's twin at max_depth = 1, its balance on a closed-form
target, the anatomy of a recorded tree against a brute-force check, the host class against the twin, the lowering pass and the
constructor, the NUTS program compiled offline, and the admission of every case that tests/test_gpu_nuts.py runs."""
import os
import re
import warnings

import numpy as np
import pytest
import scipy.stats as st

from . import exthmc as xh
from . import extloglike as xl
from . import extloglikewave as xlw
from . import extmodel as xm
from . import extnuts as xn
from . import extprior as xp
from . import extpriorgrad as xg
from . import extpriorwave as xpw
from . import extwave as xw
from .extprogram import ROOT, assert_switch_is_an_option_only, assert_without_scratch, compile_program, needs_hipcc
from .test_mala_source import FORWARD_ONLY_SRC

NUTS_KERNELS = ("tda_user_nuts_steps", "tda_user_mala_grad0")
NUTS = ["TDA_USER_MALA", "TDA_USER_NUTS"]


class ConstantDraws:
    """every doubling in one direction with one merge uniform, every leaf with one selection uniform"""

    def __init__(self, N, fwd, u=0.0, leaf_u=0.0):
        self.N, self.fwd, self.u, self.leaf_u = N, fwd, u, leaf_u

    def doubling(self, s, j):
        return np.full(self.N, self.fwd, dtype=bool), np.full(self.N, self.u)

    def leaf(self, s, l):
        return np.full(self.N, self.leaf_u)


# ---- 1. max_depth = 1 is one leapfrog step of HMC's twin ----------------------------------------------------------------------------
def test_one_leaf_is_one_leapfrog_step_of_hmcs_twin():
    """forward: the leaf equals exthmc.leapfrog at L = 1 (position, momentum, gradient, log-prior, log-likelihood and with them the
    energy) at 1e-12; backward: the leaf of p with -eps is the forward leaf of -p with the momentum negated; and a whole step
    at max_depth = 1 ends at the start or at that leaf"""
    d, m, N = 5, 23, 9
    _, theta0, _, _, _, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    rng = np.random.default_rng(11)
    w, eps = xh.MASS(d), np.full(N, 0.04)
    p0 = rng.standard_normal((N, d)) / np.sqrt(w)
    lp0, ll0, F = level.evaluate(theta0)
    g0 = level.grad_logpost(theta0, F)
    on = np.ones(N, dtype=bool)
    th, p, g, lp, ll, fin = xn.leaf_step(level, theta0, p0, g0, eps, w, on)
    th_h, p_h, (lp_h, ll_h, g_h), ended = xh.leapfrog(level, theta0, p0, g0, eps, w, 1)
    assert fin.all() and not ended.any()
    for got, want in ((th, th_h), (p, p_h), (g, g_h), (lp, lp_h), (ll, ll_h)):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0.0)
    energy = lambda lp, ll, p: -(lp + ll) + 0.5 * np.sum(w * (p * p), axis=1)  # noqa: E731
    np.testing.assert_allclose(energy(lp, ll, p), energy(lp_h, ll_h, p_h), rtol=1e-12)
    th_b, p_b, g_b, lp_b, ll_b, _ = xn.leaf_step(level, theta0, p0, g0, -eps, w, on)
    th_f, p_f, g_f, lp_f, ll_f, _ = xn.leaf_step(level, theta0, -p0, g0, eps, w, on)
    np.testing.assert_allclose(th_b, th_f, rtol=1e-12)
    np.testing.assert_allclose(p_b, -p_f, rtol=1e-12)
    np.testing.assert_allclose(lp_b + ll_b, lp_f + ll_f, rtol=1e-12)
    # the whole step: u_0 = 0 always takes the leaf, u_0 close to 1 takes it iff the energy fell
    z = (p0 * np.sqrt(w))[:, None, :]
    for fwd, want in ((True, th), (False, th_b)):
        ref = xn.run_nuts(level, xn.nuts(0.04, 1, inv_mass=w), theta0, z, ConstantDraws(N, fwd, u=0.0))
        np.testing.assert_allclose(ref["theta"][:, 1], want, rtol=1e-12)
        assert ref["accepted"][:, 1].all() and np.all(ref["depth"] == 1) and np.all(ref["n_leaf"] == 1)
    ref = xn.run_nuts(level, xn.nuts(0.04, 1, inv_mass=w), theta0, z, ConstantDraws(N, True, u=1.0 - 1e-16))
    fell = energy(lp, ll, p) < energy(lp0, ll0, p0)
    assert np.array_equal(ref["accepted"][:, 1].astype(bool), fell) and 0 < fell.sum() < N
    assert np.array_equal(ref["theta"][~fell, 1], theta0[~fell])


# ---- 2. balance on a closed form ------------------------------------------------------------------------------------------------------
class GaussianLevel:
    """N(mean, cov) as a level: evaluate -> (log-prior 0, log-density, None), grad_logpost"""

    def __init__(self, mean, cov):
        self.mean, self.P = mean, np.linalg.inv(cov)

    def evaluate(self, theta):
        r = theta - self.mean
        return np.zeros(len(theta)), -0.5 * np.einsum("ni,ij,nj->n", r, self.P, r), None

    def grad_logpost(self, theta, F):
        return -(theta - self.mean) @ self.P


def test_twin_leaves_a_gaussian_invariant():
    """2000 independent starts drawn from a correlated 2-d Gaussian, 50 steps each: the pooled mean and covariance of the ends
    stay the target's, within the Monte Carlo error formula of test_gpu_hmc's test_sample_api_ill_conditioned_gaussian_posterior
    (the mean within 5 standard errors, here of independent draws; the covariance within 5 % of the largest scale)"""
    N, T, d, D = 2000, 50, 2, 5
    mean, cov = np.array([0.5, -1.0]), np.array([[1.0, 0.9], [0.9, 2.0]])
    rng = np.random.default_rng(2)
    theta0 = rng.multivariate_normal(mean, cov, size=N)
    draws = xn.ArrayDraws(rng.integers(0, 2, (N, T, D)).astype(bool), rng.random((N, T, D)), rng.random((N, T, 1 << D)))
    ref = xn.run_nuts(GaussianLevel(mean, cov), xn.nuts(0.35, D), theta0, rng.standard_normal((N, T, d)), draws)
    print("stops", {xn.STOP_NAMES[k]: int(np.sum(ref["stop"] == k)) for k in range(4)}, "mean depth %.2f, mean statistic %.3f, moved %.3f"
          % (ref["depth"].mean(), ref["stat"].mean(), ref["accepted"][:, 1:].mean()))
    assert np.sum(ref["stop"] == 2) > 100 and np.sum(ref["stop"] == 3) > 100 and 1.0 < ref["depth"].mean() < D
    X = ref["theta"][:, -1]
    se = np.sqrt(np.diag(cov) / N)
    assert np.all(np.abs(X.mean(axis=0) - mean) < 5 * se), (X.mean(axis=0), mean, se)
    np.testing.assert_allclose(np.cov(X.T), cov, atol=0.05 * np.sqrt(np.outer(np.diag(cov), np.diag(cov))).max())
    # and the ends are not the starts: the chains moved by about the target's own scale
    assert np.mean(np.abs(X - theta0)) > 0.5


# ---- 3. the anatomy of recorded trees --------------------------------------------------------------------------------------------------
def test_tree_anatomy_against_brute_force():
    """for the recorded trees of one chain: every U-turn check of the iterative scheme equals the check over the stored leaves of
    its aligned sub-subtree (same verdict, the momentum sum at 1e-12), every aligned sub-subtree that was completed has been
    checked exactly once, and the selection weights (1 for the initial leaf, exp(lw) per merged leaf) sum to the tree's weight"""
    d, m, N, T, D = 5, 23, 3, 40, 5
    _, theta0, _, _, _, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    z = xn.philox_normals(N, T, d)
    prop = xn.nuts(0.03, D, inv_mass=xh.MASS(d))
    w = prop["inv_mass"]
    ref = xn.run_nuts(level, prop, theta0, z, xn.PhiloxDraws(xn.SEED, xn.CHAIN_OFFSET, N), record=1)
    n_checks = n_turn = 0
    for s, tree in enumerate(ref["trees"]):
        leaves = {(lf["j"], lf["n"]): lf for lf in tree["leaves"]}
        seen = set()
        for ch in tree["checks"]:
            j, n = ch["j"], ch["n"]
            ones = (n ^ (n + 1)).bit_length() - 1
            k = bin(n >> 1).count("1") - ch["row"] + 1  # the sub-subtree has 2^k leaves
            assert 1 <= k <= ones, (s, ch)
            first = n - (1 << k) + 1
            assert first % (1 << k) == 0  # aligned
            ps = np.stack([leaves[(j, i)]["p"] for i in range(first, n + 1)])
            rho = ps.sum(axis=0)
            np.testing.assert_allclose(ch["rho"], rho, rtol=1e-12, atol=1e-13 * np.abs(ps).max())
            brute = not (np.sum((w * ps[0]) * rho) > 0.0 and np.sum((w * ps[-1]) * rho) > 0.0)
            assert brute == ch["turn"], (s, ch)
            assert (j, n, k) not in seen
            seen.add((j, n, k))
            n_checks += 1
            n_turn += brute
        # every completed aligned sub-subtree of a subtree whose leaves all exist was checked
        for (j, n) in leaves:
            if n & 1:
                for k in range(1, (n ^ (n + 1)).bit_length()):
                    assert (j, n, k) in seen, (s, j, n, k)
        merged = [lf for lf in tree["leaves"] if lf["j"] in tree["merged"]]
        assert len(merged) == (1 << tree["depth"]) - 1
        np.testing.assert_allclose(1.0 + sum(np.exp(lf["lw"]) for lf in merged), np.exp(tree["LW"]), rtol=1e-12)
        assert tree["selected"] == 0 or any(lf["l"] == tree["selected"] and lf["taken"] for lf in merged)
    print("checks %d, of them turning %d; stops %s" % (n_checks, n_turn, [int(np.sum(ref["stop"][1] == k)) for k in range(4)]))
    assert n_checks > 200 and n_turn >= 5 and np.sum(ref["stop"][1] == 2) >= 3 and np.sum(ref["stop"][1] == 3) >= 3


# ---- 4. the host class is the twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
def test_host_class_is_the_twin(adaptive, monkeypatch):
    """tda.NUTS under the host protocol on recorded draws: the selected leaf, the stop reason, the depth and `accepted` exact, the
    log-posterior 1e-10, the adapted step size 1e-12"""
    import tinyda_amd as tda

    d, m, N, T, D = 5, 23, 3, 60, 4
    y, theta0, pm, pv, nz, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((N, T, d))
    fwd, u, leaf_u = rng.integers(0, 2, (N, T, D)), rng.random((N, T, D)), rng.random((N, T, 1 << D))
    tw = xn.nuts(0.05, D, adaptive, xh.MASS(d))
    ref = xn.run_nuts(level, tw, theta0, z, xn.ArrayDraws(fwd.astype(bool), u, leaf_u))
    assert len(set(ref["stop"].ravel())) >= 3 and 0.02 < np.mean(ref["selected"] == 0) < 0.98
    model = tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0], reference_gradient=lambda t, s: xm.np_vjp(t, s)[0])
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, np.diag(nz)), model)
    for c in range(N):
        prop = tda.NUTS(scaling=0.05, max_depth=D, inv_mass=xh.MASS(d), adaptive=adaptive, gamma=1.01, period=20)
        prop.setup_proposal(parameters=theta0[c], posterior=post)
        assert prop.compute_gradient == prop._compute_gradient and prop.alpha_star == 0.8
        at = dict(s=0, j=-1, k=0)  # the position of the host class in its draws: step, doubling, leaf draws of the doubling so far

        def randint(n):
            at["j"], at["k"] = at["j"] + 1, 0
            at["merge"] = True
            return fwd[c, at["s"], at["j"]]

        def random():
            if at.pop("merge", False):
                return u[c, at["s"], at["j"]]
            at["k"] += 1  # the k-th leaf after the first of doubling j is leaf 2^j + k of its step
            return leaf_u[c, at["s"], (1 << at["j"]) + at["k"]]

        monkeypatch.setattr(np.random, "standard_normal", lambda n: z[c, at["s"]])
        monkeypatch.setattr(np.random, "randint", randint)
        monkeypatch.setattr(np.random, "random", random)
        link = post.create_link(theta0[c])
        accepted = []
        for s in range(T):
            at.update(s=s, j=-1, k=0)
            cand = post.create_link(prop.make_proposal(link))
            acc = 0.5 < prop.get_acceptance(cand, link)
            if acc:
                link = cand
            accepted.append(acc)
            prop.adapt(parameters=link.parameters, accepted=accepted)
            tree = prop.last_tree
            assert (tree["selected"], tree["stop"], tree["depth"], tree["n_leapfrog"]) == (
                ref["selected"][c, s], xn.STOP_NAMES[ref["stop"][c, s]], ref["depth"][c, s], ref["n_leaf"][c, s]), (c, s)
            assert acc == bool(ref["accepted"][c, s + 1]), (c, s)
            np.testing.assert_allclose(link.posterior, ref["logpost"][c, s + 1], rtol=1e-10)
            np.testing.assert_allclose(link.parameters, ref["theta"][c, s + 1], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(prop.scaling, ref["scaling"][c], rtol=1e-12)
        assert [prop.totals[k] for k in ("n_leapfrog", "n_divergent", "n_max_depth", "depth_sum")] == ref["totals"][c].tolist()
        assert (prop.scaling != 0.05) == adaptive


# ---- 5. lowering and the constructor ---------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    import tinyda_amd as tda

    for bad in (dict(max_depth=0), dict(max_depth=11), dict(max_depth=2.5), dict(target_accept=0.0), dict(target_accept=1.0), dict(target_accept=-0.3),
                dict(inv_mass=[1.0, 0.0]), dict(inv_mass=[np.nan, 1.0])):
        with pytest.raises(ValueError):
            tda.NUTS(0.1, **bad)
    prop = tda.NUTS()
    assert (prop.scaling, prop.max_depth, prop.inv_mass, prop.adaptive, prop.target_accept, prop.gamma, prop.period) == (0.1, 8, None, False, 0.8, 1.01, 100)
    assert isinstance(prop, tda.HMC)
    with pytest.raises(ValueError, match="inv_mass"):
        tda.NUTS(0.1, inv_mass=[1.0, 2.0, 3.0]).setup_proposal(parameters=np.zeros(2), posterior=_posterior(2, 1))


def _posterior(d, m, model=None, likelihood=None, prior=None):
    import tinyda_amd as tda

    return tda.Posterior(st.multivariate_normal(0.1 * np.ones(d), np.diag(0.5 + 0.01 * np.arange(d))) if prior is None else prior,
                         tda.GaussianLogLike(np.zeros(m), 0.01 * np.eye(m)) if likelihood is None else likelihood,
                         tda.DeviceModel(xm.source(), m) if model is None else model)


def _lower(posts, prop):
    from tinyda_amd.lowering import lower

    return lower(posts, prop)


def _forms():
    import tinyda_amd as tda

    y, par = np.zeros(23), 0.1 * np.ones(23)
    cauchy, lognormal = xpw.cauchy_difference(13), tda.DevicePrior(xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, 5, np.zeros(5), np.ones(5))
    return {
        "gaussian": _posterior(5, 23),
        "diagonal noise": _posterior(5, 23, likelihood=tda.GaussianLogLike(y, np.diag(0.01 * (1.0 + np.arange(23))))),
        "d = 128, m = 2048": _posterior(128, 2048),
        "wave forms": _posterior(5, 24, model=tda.DeviceModel(xw.source("wave", "wave"), 24)),
        "DeviceLogLike": _posterior(5, 23, likelihood=tda.DeviceLogLike(xl.KINDS["t"][0], y, par)),
        "DeviceLogLike, coupled": _posterior(5, 23, likelihood=xlw.device_loglike("ar1", y, par, reference=False)),
        "DevicePrior": _posterior(5, 23, prior=lognormal),
        "DevicePrior, coupled": _posterior(13, 23, prior=xpw.device_prior(cauchy, reference=False)),
    }


def test_lowering_plans():
    """NUTS lowers wherever HMC does, with its own kind, depth, target and mass in the plan"""
    import tinyda_amd as tda
    from tinyda_amd import _lib

    assert _lib.PROP_NUTS == 8
    w = 0.5 + np.arange(128.0)
    for name, post in _forms().items():
        d = post.prior.rvs().size if not hasattr(post.prior, "dim") else post.prior.dim
        assert _lower([post], tda.HMC(0.05))[0] is not None, name
        plan, why = _lower([post], tda.NUTS(0.05, max_depth=7, inv_mass=w[:d], adaptive=True, target_accept=0.7, period=50))
        assert plan is not None, (name, why)
        p = plan[1]
        assert (p["kind"], p["max_depth"], p["target_accept"], p["adaptive"], p["period"], p["C_"]) == (_lib.PROP_NUTS, 7, 0.7, True, 50, None)
        assert np.array_equal(p["inv_mass"], w[:d]) and plan[0][0]["has_gradient"] and "n_leapfrog" not in p
    assert _lower([_forms()["gaussian"]], tda.NUTS(0.05))[0][1]["inv_mass"] is None


def test_lowering_refusals_are_hmcs_with_the_name_nuts():
    """every posterior that HMC is refused on: NUTS is refused with the same words under its own name, and neither reason
    names another gradient proposal"""
    import tinyda_amd as tda
    from tinyda_amd._contract import SIG

    y, par = np.zeros(23), 0.1 * np.ones(23)
    post = _posterior(5, 23)
    linear = tda.Posterior(post.prior, tda.GaussianLogLike(np.zeros(3), 0.01 * np.eye(3)), tda.LinearModel(np.ones((3, 5))))
    batched = tda.Posterior(post.prior, post.likelihood, tda.BatchedModel(lambda th: np.zeros((th.shape[0], 23)), 23))
    dense = st.multivariate_normal(np.zeros(2), np.array([[1.0, 0.3], [0.3, 1.0]]))
    cases = {
        "no gradient": ([_posterior(5, 23, model=tda.DeviceModel(FORWARD_ONLY_SRC, 23))], ("NUTS over a source-defined model needs", SIG["tda_gradient"])),
        "no likelihood gradient": ([_posterior(5, 23, likelihood=tda.DeviceLogLike(xl.TERM_ONLY_SRC, y, par))], ("NUTS with a DeviceLogLike needs", SIG["tda_loglike_term_grad"])),
        "no coupled likelihood gradient": ([_posterior(5, 23, likelihood=tda.DeviceLogLike(xlw.without_grad(xlw.AR1_SRC), y, par))], ("that couples outputs", SIG["tda_loglike_grad_wave"])),
        "no prior gradient": ([_posterior(5, 23, prior=tda.DevicePrior(xp.LOGNORMAL_SRC, 5, np.zeros(5), np.ones(5)))], ("is not lowered under NUTS", SIG["tda_logprior_term_grad"])),
        "hierarchy": ([post, post], ()),
        "linear model": ([linear], ("NUTS: single level, a DeviceModel with tda_gradient",)),
        "batched model": ([batched], ("a DeviceModel with tda_gradient",)),
        "129 parameters": ([_posterior(129, 23)], ()),
        "2049 outputs": ([_posterior(5, 2049)], ("at most 2048 outputs",)),
        "joint prior": ([_posterior(2, 3, prior=tda.JointPrior([st.norm(0.0, 1.0), st.uniform(-1.0, 2.0)]))], ()),
        "dense prior": ([_posterior(2, 3, prior=dense)], ()),
    }
    for name, (posts, needles) in cases.items():
        plan_h, why_h = _lower(posts, tda.HMC(0.05))
        plan_n, why_n = _lower(posts, tda.NUTS(0.05))
        assert plan_h is None and plan_n is None, name
        assert why_n == why_h.replace("HMC", "NUTS"), (name, why_n, why_h)
        assert "MALA" not in why_n and "HMC" not in why_n, why_n
        for needle in needles:
            assert needle in why_n, (name, needle, why_n)
    assert _lower([linear], tda.MALA(0.05))[0] is not None  # (MALA keeps the engine's linear-Gaussian kernel)


def test_sample_falls_back_with_a_reason_naming_nuts():
    """backend='auto' over a LinearModel warns once and runs the host class; backend='hip' raises the same reason"""
    import tinyda_amd as tda
    from tinyda_amd.api import HostFallbackWarning

    A = np.array([[1.0, 0.5], [0.2, 1.0], [0.3, 0.3]])
    post = tda.Posterior(st.multivariate_normal(np.zeros(2), np.eye(2)), tda.GaussianLogLike(np.array([0.3, -0.2, 0.1]), 0.25 * np.eye(3)), tda.LinearModel(A))
    with pytest.raises(tda.EngineError, match="NUTS: single level, a DeviceModel with tda_gradient"):
        tda.sample(post, tda.NUTS(0.2, max_depth=3), 10, n_chains=2, backend="hip")
    np.random.seed(4)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.NUTS(0.2, max_depth=4, adaptive=True, period=10), 40, n_chains=2, backend="auto")
    fb = [x for x in w if issubclass(x.category, HostFallbackWarning)]
    assert len(fb) == 1 and "NUTS" in str(fb[0].message)
    assert res["backend"] == "host" and len(res["chain_0"]) == 41
    assert len({tuple(lk.parameters) for lk in res["chain_0"]}) > 20  # (the state moves at nearly every step)
    assert all(np.isfinite(lk.posterior) for lk in res["chain_1"])


# ---- 6. the NUTS program, compiled offline as shipped -----------------------------------------------------------------------------------
FORMS = {
    "extmodel": (lambda: xm.source(), []),
    "ring_wave_forms": (lambda: xw.source("wave", "wave"), ["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE"]),
    "ring_forward_wave": (lambda: xw.source("wave", "per_parameter"), ["TDA_FORWARD_WAVE"]),
    "student_t": (lambda: xm.source() + xl.KINDS["t"][0], ["TDA_LOGLIKE_SOURCE"]),
    "ar1_wave": (lambda: xlw.full_source("ar1"), ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE"]),
    "lognormal_prior": (lambda: xm.source() + xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, ["TDA_PRIOR_SOURCE"]),
    "cauchy_prior_wave": (lambda: xm.source() + xpw.CAUCHY_DIFF_SRC, ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"]),
}


@needs_hipcc
@pytest.mark.parametrize("form", list(FORMS))
def test_nuts_program_compiles_without_scratch(tmp_path, form):
    """tda_user_nuts_steps in place of tda_user_mala_steps, tda_user_mala_grad0 beside it, over every form of the contract: no
    scratch memory and no spilled vector registers (measured, hipcc of ROCm 7, gfx950: 207 vector registers for extmodel's
    source, 199 for the ring with both wave forms)"""
    src, switches = FORMS[form]
    assert_without_scratch(tmp_path, form, src(), NUTS + switches, NUTS_KERNELS)


@needs_hipcc
def test_the_switch_alone_selects_the_kernel(tmp_path):
    from .extprogram import MALA_KERNELS

    rc, log, usage = compile_program(tmp_path, "mala", xm.source(), ["TDA_USER_MALA"])
    assert rc == 0 and set(usage) == set(MALA_KERNELS), log[-3000:]
    rc, log, _ = compile_program(tmp_path, "no_gradient", FORWARD_ONLY_SRC, NUTS)
    assert rc != 0 and "tda_gradient_missing" in log


def test_the_switch_is_an_option_only_and_the_header():
    header = assert_switch_is_an_option_only(r"TDA_USER_NUTS\b", ("tda_usermodel.inc", "tda_user_build.h", "tda_host_nuts.inc"))
    assert "tda_engine_set_nuts" not in header and "TDA_PROP_NUTS = 8" in header and "stream 8" not in header
    nuts_header = open(os.path.join(ROOT, "include", "tinyda_amd_nuts.h")).read()
    assert re.search(r"int tda_engine_set_nuts\(tda_engine\* e, int32_t max_depth /\* 1..10 \*/, double target_accept /\* \(0,1\) \*/, const double\* inv_mass", nuts_header)
    assert "stream 8" in nuts_header


def test_nuts_symbol_table():
    """the header's functions are bound by load() through their own table, never by load_from (the CPU build has no NUTS)"""
    from tinyda_amd import _lib

    assert set(_lib.NUTS_SYMBOLS) == {"tda_engine_set_nuts", "tda_engine_get_nuts_totals"} and not set(_lib.NUTS_SYMBOLS) & set(_lib.SYMBOLS)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyda_amd_nuts.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(tda_[a-z_]+)\s*\(", text)) == set(_lib.NUTS_SYMBOLS)


# ---- 7. the cases of tests/test_gpu_nuts.py: admitted here, run there -----------------------------------------------------------------
def _admit(case, level, prop, theta0, T):
    assert T == 120 and theta0.shape[0] == 13
    z = xn.philox_normals(theta0.shape[0], T, theta0.shape[1])
    ref, dpost, dstate = xn.assert_admissible(level, prop, theta0, z, xn.PhiloxDraws(xn.SEED, xn.CHAIN_OFFSET, theta0.shape[0]))
    xn.assert_within_tolerance(case, dpost, dstate)
    return ref, xn.coverage(ref, prop["max_depth"])


@pytest.mark.parametrize("case", list(xn.FORWARD_CASES))
def test_forward_cases_are_admissible_and_cover(case):
    """on the engine's own variates (the oracle's Philox stream): one ulp up or down on every gradient leaves every tree as it is,
    ten times what it moves fits the case's tolerance, and the twin's trace holds every kind of tree"""
    level, prop, theta0, T, _ = xn.forward_case(case)
    ref, cov = _admit(case, level, prop, theta0, T)
    assert cov["uturn_subtree"] >= 10 and cov["uturn_tree_deep"] >= 10 and cov["max_depth"] >= 10 and cov["stayed"] >= 10, cov
    assert cov["forward_deep"] >= 1 and cov["backward_deep"] >= 1, cov
    assert prop["max_depth"] != 3 or cov["at_cap"] > 0.5  # (max_depth = 3: most trees hit the cap)
    assert prop["adaptive"] == bool(np.any(ref["scaling"] != prop["scaling"]))


@pytest.mark.parametrize("case", list(xn.CONTRACT_STEP))
def test_contract_cases_are_admissible(case):
    level, prop, theta0, T, _ = xn.contract_case(case)
    ref, cov = _admit(case, level, prop, theta0, T)
    assert prop["max_depth"] == 4 and cov["mean_depth"] > 1.5
    if case == "lognormal_prior_at_the_edge":
        assert cov["left_support"] >= 5 and np.all(ref["theta"] > 0.0), cov


def test_nan_region_case_is_admissible():
    level, prop, theta0, T, thr, _ = xn.nan_case()
    ref, cov = _admit("nan_region", level, prop, theta0, T)
    assert cov["divergent"] >= 5 and cov["left_support"] >= 5 and np.all(ref["theta"][:, :, 0] <= thr), cov
