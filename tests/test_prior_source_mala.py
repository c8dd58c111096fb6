"""MALA under source-defined priors (tda_logprior_term_grad) without a device: the gradient of the shipped family library
against mpmath at 80 digits (tests/golden/g22_prior_family_grads.npz; tests/extpriorgrad.py has the reference and derives the
bound), its NumPy twin and the oracle level that carries it, DevicePrior's gradient interface and from_distributions, what
lowers under MALA and why the rest does not, and the MALA programs compiled offline for gfx950 with the prior switch."""
import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from . import extfamilies as xf
from . import extloglike as xl
from . import extmodel as xm
from . import extprior as xp
from . import extpriorgrad as xg
from . import extwave as xw
from .extprogram import compile_program as _compile, needs_hipcc
from .test_prior_source import _device_prior, _posterior

MALA_KERNELS = ("tda_user_mala_steps", "tda_user_mala_grad0")


@pytest.fixture(scope="module")
def g21(golden):
    return golden(xf.GOLDEN_NAME)


@pytest.fixture(scope="module")
def g22(golden):
    return golden(xg.GOLDEN_NAME)


# ---- (a) the family gradients against mpmath -----------------------------------------------------------------------------------------
def test_fixture_is_what_mpmath_gives(g21, g22):
    pytest.importorskip("mpmath")
    again = xg.reference(g21)
    for k, v in again.items():
        assert np.array_equal(v, g22[k]), k
    inside = g22["inside"]
    assert np.array_equal(inside, np.isfinite(g21["ref"])) and inside[:, xf.REST].all() and inside.sum() >= 128 * (1 + xf.KEEP_PER_ROW) - 300
    assert not inside[:, xf.OUT_LO:].any()


@pytest.fixture(scope="module")
def host(g21, tmp_path_factory):
    rows = xf.decode_rows(g21)
    term, grad, low = xg.host_library(tmp_path_factory.mktemp("family_grads"), [xf.component(r) for r in rows])
    return rows, term, grad, low


def test_host_library_gradient_over_the_grid(g21, g22, host):
    """the shipped library compiled for the host against g'(z) / scale from mpmath at every in-support point of the g21 grid;
    the bound is 8 eps gmag + gcond + gallow, derived in the docstring of tests/extpriorgrad.py (roundings of the addends, the
    rounding of z, Weibull's power).  Largest error / bound on the host build: 0.19 (beta), 0.17 (weibull_min), every other family below 0.14."""
    rows, _, grad, _ = host
    inside, ref, tol = g22["inside"], g22["ref"], xg.bound(g22)
    got = np.zeros(ref.shape)
    for j in range(len(rows)):
        got[j, inside[j]] = grad(g21["x"][j, inside[j]], j)
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref)
    exact = inside & (tol == 0.0)  # g' = 0 with nothing to round: uniform, beta(1, 1), z = 0 of a symmetric family
    assert np.all(err[exact] == 0.0) and all(exact[i][inside[i]].all() for i, r in enumerate(rows) if r[0] == "uniform")
    ratio = np.zeros(ref.shape)
    cmp = inside & (tol > 0.0)
    ratio[cmp] = err[cmp] / tol[cmp]
    xg.report(rows, ratio, inside, "error / bound")
    bad = [(rows[i], k, g21["x"][i, k], ratio[i, k]) for i, k in zip(*np.nonzero(ratio > 1.0))]
    assert not bad, bad


# ---- (b) the NumPy twin and the oracle level -----------------------------------------------------------------------------------------
def test_numpy_twin_matches_the_library_and_scipy(g21, g22, host):
    """the twin against the compiled library (the same formulas in the same order: the bound's rounding part alone, both being
    that far from the exact value of their common z at most) and against central differences of scipy's logpdf at the rest points"""
    from tinyda_amd import likelihoods as lk

    rows, _, grad, low = host
    inside, x = g22["inside"], g21["x"]
    for k in range(xf.N_COLS):
        got = lk.family_gradient(low, np.where(inside[:, k], x[:, k], x[:, xf.REST]))
        for j in np.nonzero(inside[:, k])[0]:
            want = grad(x[j, k:k + 1], j)[0]
            assert abs(got[j] - want) <= 2 * (8 * xg.EPS * g22["gmag"][j, k] + g22["gallow"][j, k]), (rows[j], k, got[j], want)
    # batched input, and scipy by central differences (relative step 1e-6 of the scale: O(h^2) truncation, 1e-16 / h rounding)
    both = lk.family_gradient(low, np.stack([x[:, xf.REST], x[:, xf.REST]]))
    assert both.shape == (2, 128) and np.array_equal(both[0], both[1])
    checked = 0
    for j, r in enumerate(rows):
        c, h = xf.component(r), 1e-6 * r[3]
        x0 = x[j, xf.REST]
        if r[0] == "laplace" or not np.all(np.isfinite(c.logpdf([x0 - h, x0 + h]))):
            continue  # (the kink of the Laplace density is its rest point; a truncnorm window narrower than the step)
        fd = (c.logpdf(x0 + h) - c.logpdf(x0 - h)) / (2 * h)
        # (truncation: a part in 1e5 of the addends' magnitudes is generous for h = 1e-6 scale; rounding: a few eps of the two log-densities over h)
        assert abs(both[0, j] - fd) <= 1e-5 * g22["gmag"][j, xf.REST] + 8 * xg.EPS * max(1.0, abs(c.logpdf(x0))) / h, (r, both[0, j], fd)
        checked += 1
    assert checked >= 100


def test_oracle_level_gradient_is_the_gradient_of_its_own_evaluate():
    d, m = 13, 23
    comps = xp.components(d)
    rng = np.random.default_rng(4)
    truth, th = xg.starts_inside(comps, 3, rng)
    y = xm.np_forward(truth, m)[0]
    prior = xg.FamilyGradPrior(comps)
    par = 0.1 * (1.0 + 0.1 * np.arange(m) / m)
    for level in (xg.gaussian_grad_level(prior, m, y), xg.loglike_grad_level(prior, m, y, par, "t")):
        lp, ll, F = level.evaluate(th)
        g = level.grad_logpost(th, F)
        for j in range(d):
            if comps[j].dist.name == "laplace":
                continue
            h = 1e-6
            e = np.zeros(d)
            e[j] = h
            up, dn = level.evaluate(th + e), level.evaluate(th - e)
            fd = ((up[0] + up[1]) - (dn[0] + dn[1])) / (2 * h)
            np.testing.assert_allclose(g[:, j], fd, rtol=2e-6, atol=1e-6 * np.max(np.abs(lp + ll)))


@pytest.mark.parametrize("d", [128, 46])
def test_probe_chains_move_by_the_gradient_on_the_oracle(g21, g22, d):
    """the chains of the GPU test of the gradient alone (extpriorgrad.probe_chains), on the oracle with the NumPy twin: every
    point of the grid that is not on an edge is compared in exactly one chain, every chain built for a step size is accepted at
    it and stays inside the supports, and (theta_1 - theta_0) / h is the gradient within the bound of the GPU test"""
    rows = xf.decode_rows(g21)[:d]
    x, h, z, compared, ref, tol = xg.probe_chains(g21, g22, d)
    inside = g22["inside"][:d, :xf.OUT_LO]
    assert inside.sum() - 40 <= compared.sum() <= inside.sum() and np.all(z[compared] == 0.0) and h.max() <= 0.5
    prior = xg.FamilyGradPrior([xf.component(r) for r in rows])
    level = orc.CallableGaussianLevel(lambda th: np.zeros((len(th), 3)), np.zeros(3), "iso", 1.0, prior)
    level.grad_logpost = lambda th, F: prior.grad(th)
    bound = xg.probe_bound(x, h, ref, tol)
    for hv in np.unique(h):
        sel = h == hv
        with np.errstate(all="ignore"):
            res = orc.run_mh(level, dict(kind="mala", scaling=float(np.sqrt(2.0 * hv))), x[sel], z[sel][:, None, :], np.zeros((sel.sum(), 1)))
        assert res["accepted"][:, 1].all() and np.all(prior.inside(res["theta"][:, 1])), hv
        err = np.abs((res["theta"][:, 1] - x[sel]) / hv - ref[sel])
        assert np.all(err[compared[sel]] <= bound[sel][compared[sel]])
    with np.errstate(all="ignore"):
        sharp = (bound <= 1e-6 * np.abs(ref))[compared & (ref != 0.0)].mean()
    print("share of points held to 1e-6 of the gradient or better: %.3f" % sharp)
    assert sharp > 0.8


# ---- DevicePrior's interface -----------------------------------------------------------------------------------------------------------
def test_device_prior_gradient_interface():
    import tinyda_amd as tda

    d = 3
    plain = _device_prior(d)
    assert plain.has_gradient is False and not hasattr(plain, "grad_logpdf")
    commented = tda.DevicePrior(xp.LOGNORMAL_SRC + "// " + xg.GRAD_SIG + "\n/* tda_logprior_term_grad( */", d)
    assert commented.has_gradient is False
    p, q = plain.p, plain.q
    full = tda.DevicePrior(xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, d, p, q, reference=xp.LognormalPrior(p, q),
                           reference_gradient=lambda th: xg.lognormal_grad(th, p, q))
    assert full.has_gradient is True
    th = np.array([0.5, 1.0, 2.0])
    h = 1e-6
    fd = [(full.logpdf(th + h * np.eye(d)[j]) - full.logpdf(th - h * np.eye(d)[j])) / (2 * h) for j in range(d)]
    np.testing.assert_allclose(full.grad_logpdf(th), fd, rtol=1e-7)
    assert not hasattr(tda.DevicePrior(xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, d), "grad_logpdf")


def test_from_distributions():
    import tinyda_amd as tda
    from tinyda_amd import likelihoods as lk

    comps = xp.components(13)
    dp = tda.DevicePrior.from_distributions(comps)
    jp = tda.JointPrior(comps)
    _, loc, scale, src = jp._source_lowering()
    assert dp.has_gradient and dp.dim == 13 and dp.source == src and np.array_equal(dp.p, loc) and np.array_equal(dp.q, scale)
    assert isinstance(dp.reference, tda.JointPrior) and dp.reference.distributions == comps
    th = np.array([c.ppf(0.4) for c in comps])
    assert dp.logpdf(th) == jp.logpdf(th)
    assert np.array_equal(dp.grad_logpdf(th), lk.family_gradient([lk._family_component(c) for c in comps], th))
    u = np.random.default_rng(1).random((2, 13))
    assert np.array_equal(dp.ppf(u), jp.ppf(u))
    with pytest.raises(ValueError, match=r"component 1 \(gumbel_r\)"):
        tda.DevicePrior.from_distributions([st.norm(0.0, 1.0), st.gumbel_r(0.0, 1.0)])
    with pytest.raises(ValueError, match=r"component 0 \(truncnorm\)"):
        tda.DevicePrior.from_distributions([st.truncnorm(-np.inf, 1.0)])
    with pytest.raises(ValueError, match="component 2"):
        tda.DevicePrior.from_distributions([st.norm(0.0, 1.0), st.gamma(2.0), object()])


# ---- (c) lowering decisions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 13, 96])
def test_device_plan_under_mala(d):
    import tinyda_amd as tda
    from tinyda_amd import _lib, api

    prior = tda.DevicePrior.from_distributions(xp.components(d))
    for adaptive in (False, True):
        plan = api._device_plan([_posterior(prior)], tda.MALA(0.05, adaptive=adaptive))
        assert plan is not None, api._refusal
        low = plan[0][0]
        assert plan[1]["kind"] == _lib.PROP_MALA and np.all(low["prior_joint"][0] == _lib.PRIOR_SOURCE)
        assert low["prior_source"]["has_gradient"] is True and low["prior_source"]["label"] == "DevicePrior"
        assert low["source"].index("tda_gradient") < low["source"].index("tda_logprior_term_grad") and low["source"].endswith(prior.source)
    m = 3
    poisson = tda.DeviceLogLike(xl.POISSON_SRC, np.ones(m), np.ones(m))
    plan = api._device_plan([_posterior(prior, like=poisson)], tda.MALA(0.05))
    assert plan is not None, api._refusal
    assert plan[0][0]["noise_kind"] == _lib.NOISE_SOURCE and plan[0][0]["prior_source"]["has_gradient"]
    diag = tda.GaussianLogLike(np.zeros(m), np.diag(0.04 + 0.01 * np.arange(m)))
    assert api._device_plan([_posterior(prior, like=diag)], tda.MALA(0.05)) is not None, api._refusal
    # GRW and AM plan as they did, and the lowering says whether the gradient is there
    assert api._device_plan([_posterior(prior)], tda.GaussianRandomWalk(np.eye(d)))[0][0]["prior_source"]["has_gradient"] is True
    assert api._device_plan([_posterior(_device_prior(d))], tda.GaussianRandomWalk(np.eye(d)))[0][0]["prior_source"]["has_gradient"] is False
    assert api._device_plan([_posterior(tda.JointPrior(xp.components(d)))], tda.GaussianRandomWalk(np.eye(d)))[0][0]["prior_source"]["has_gradient"] is False


def test_device_plan_refusals_under_mala():
    import tinyda_amd as tda
    from tinyda_amd import api

    d, m = 2, 3
    prior = tda.DevicePrior.from_distributions(xp.components(d))
    mala = tda.MALA(0.05)

    def refused(posts, *needles):
        assert api._device_plan(posts, mala) is None
        for n in ("DevicePrior",) + needles:
            assert n in api._refusal[0], api._refusal

    refused([_posterior(_device_prior(d))], "MALA", "tda_logprior_term_grad")
    no_grad = tda.DeviceModel(xm.source().split("__device__ double tda_gradient")[0], m)
    assert not no_grad.has_gradient
    refused([tda.Posterior(prior, tda.GaussianLogLike(np.zeros(m), 0.04 * np.eye(m)), no_grad)], "MALA", "tda_gradient")
    refused([_posterior(prior), _posterior(prior)], "MALA", "single level")
    refused([_posterior(prior, like=tda.GaussianLogLike(np.zeros(m), 0.04 * np.eye(m) + 0.01))], "isotropic / diagonal noise")
    refused([_posterior(prior, like=tda.DeviceLogLike(xl.TERM_ONLY_SRC, np.zeros(m), np.ones(m)))], "MALA", "tda_loglike_term_grad")
    big = 2049
    refused([_posterior(prior, m=big, like=tda.GaussianLogLike(np.zeros(big), 0.04 * np.eye(big)))], "MALA", "2048 outputs")
    # a plain JointPrior of families stays closed under MALA, and the reason says where the route is
    assert api._device_plan([_posterior(tda.JointPrior(xp.components(d)))], mala) is None
    assert "JointPrior of scipy families" in api._refusal[0] and "from_distributions" in api._refusal[0]


def test_host_mala_takes_the_exact_prior_gradient(monkeypatch):
    """the host MALA over a DevicePrior with reference_gradient: model.gradient + grad_loglike + the prior's own grad_logpdf, no
    finite differences anywhere"""
    import scipy.optimize

    import tinyda_amd as tda

    d, m = 5, 7
    comps = xp.components(d)
    prior = tda.DevicePrior.from_distributions(comps)
    rng = np.random.default_rng(2)
    truth, th = xg.starts_inside(comps, 1, rng)
    y = xm.np_forward(truth, m)[0]
    model = tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0],
                            reference_gradient=lambda t, s: xm.np_vjp(t, s)[0])
    post = tda.Posterior(prior, tda.GaussianLogLike(y, xp.SIGMA2 * np.eye(m)), model)

    def boom(*a, **k):
        raise AssertionError("finite differences")

    monkeypatch.setattr(scipy.optimize, "approx_fprime", boom)
    prop = tda.MALA(0.01)
    prop.setup_proposal(posterior=post)
    assert prop.compute_gradient == prop._compute_gradient
    link = post.create_link(th[0])
    got = prop.compute_gradient(link)
    level = xg.gaussian_grad_level(xg.FamilyGradPrior(comps), m, y)
    np.testing.assert_allclose(got, level.grad_logpost(th, level.forward(th))[0], rtol=1e-12)
    # a prior without the attribute still differentiates logpdf numerically (and meets the patched function)
    bare = tda.Posterior(tda.JointPrior(comps), post.likelihood, model)
    prop2 = tda.MALA(0.01)
    prop2.setup_proposal(posterior=bare)
    with pytest.raises(AssertionError, match="finite differences"):
        prop2.compute_gradient(bare.create_link(th[0]))


# ---- (d) the MALA programs with the prior switch, compiled offline as shipped --------------------------------------------------------
def _family_source(d):
    import tinyda_amd as tda

    return tda.DevicePrior.from_distributions(xp.components(d)).source


MALA_PROGRAMS = {
    "families_d128": (lambda: xm.source() + "\n" + _family_source(128), []),
    "lognormal": (lambda: xm.source() + xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, []),
    "families_student_loglike": (lambda: xm.source() + xl.KINDS["t"][0] + "\n" + _family_source(128), ["TDA_LOGLIKE_SOURCE"]),
    "families_wave_model_wave_gradient": (lambda: xw.source("wave", "wave") + "\n" + _family_source(128), ["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE"]),
}


@needs_hipcc
@pytest.mark.parametrize("case", list(MALA_PROGRAMS))
def test_mala_prior_program_compiles_for_gfx950_without_scratch(tmp_path, case):
    make, switches = MALA_PROGRAMS[case]
    rc, log, usage = _compile(tmp_path, "mala_prior", make(), ["TDA_USER_MALA", "TDA_PRIOR_SOURCE"] + switches)
    assert rc == 0, log[-3000:]
    assert set(MALA_KERNELS) == set(usage), (usage, log[-2000:])
    for k in MALA_KERNELS:
        print(k, usage[k])
        assert usage[k]["ScratchSize [bytes/lane]"] == 0 and usage[k]["VGPRs Spill"] == 0, (k, usage[k])


@needs_hipcc
def test_missing_prior_gradient_names_the_signature(tmp_path):
    rc, log, _ = _compile(tmp_path, "no_grad", xm.source() + xp.LOGNORMAL_SRC, ["TDA_USER_MALA", "TDA_PRIOR_SOURCE"])
    assert rc != 0 and "tda_logprior_term_grad_missing" in log and "TDA_PRIOR_SOURCE" in log and xg.GRAD_SIG in log
    # the step program of the same source does not ask for it
    rc, log, _ = _compile(tmp_path, "step", xm.source() + xp.LOGNORMAL_SRC, ["TDA_PRIOR_SOURCE"])
    assert rc == 0, log[-2000:]
