"""get_MAP / get_ML / maximize on the device (tda_user_maximize, include/tinyda_amd_optimize.h, tinyda_amd/optimize.py).  Every case
is built by tests/extoptimize.py, where tests/test_optimize.py runs the NumPy twin of the kernel over the same starts and checks
that all of them converge (or, for the support and NaN cases, end as expected): no assertion here exempts a start.

Bounds.  Densities at the returned point against the twin's evaluate(x): 1e-10 relative, the project's density bar.  First-order
optimality: the twin's exact gradient at the returned x is at most gtol + 1e-10 (|log-prior| + |log-likelihood| + 1) -- the
kernel's own gradient passed gtol, and the two differ by the rounding of the sums they are made of.  Closed form: |x - x_hat|_2
<= sqrt(d) gtol / lambda_min(H), because g = -H (x - x_hat) (extoptimize.gradient_test_bound).  Forward differences: the bound
of extoptimize.difference_bound (truncation h / 2 max |H_jj| and rounding 2 eps |f| / h)."""
import os
import warnings

import numpy as np
import pytest

import tinyda_amd as tda

from . import extoptimize as xo

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_map.npz"))


def _run(case, **kw):
    kw.setdefault("gtol", case["gtol"])
    kw.setdefault("objective", case.get("objective", "posterior"))
    return tda.maximize(case["posterior"], initial_parameters=case["starts"], backend="hip", **kw)


def _check_densities(case, res, rows=None):
    for i in (range(res.x.shape[0]) if rows is None else rows):
        lp, ll = case["twin"].evaluate(res.x[i])
        print("start %d: status %s, iterations %d, evaluations %d, |dlp| %.1e, |dll| %.1e" % (i, res.status_names[res.status[i]], res.iterations[i], res.evaluations[i],
                                                                                           abs(res.logprior[i] - lp), abs(res.loglike[i] - ll)))
        assert abs(res.logprior[i] - lp) <= xo.DENSITY_RTOL * max(1.0, abs(lp))
        assert abs(res.loglike[i] - ll) <= xo.DENSITY_RTOL * max(1.0, abs(ll))


def _check_first_order(case, res, gtol, objective="posterior"):
    for i in range(res.x.shape[0]):
        g = np.max(np.abs(case["twin"].gradient(res.x[i], objective)))
        bound = gtol + 1e-10 * case["twin"].magnitude(res.x[i])
        print("start %d: exact gradient %.3e (kernel's %.3e), bound %.3e" % (i, g, res.grad_norm[i], bound))
        assert g <= bound


# ---- 1. closed form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["iso", "diag"])
@pytest.mark.parametrize("d,m,n", xo.CLOSED_FORM_SHAPES)
def test_closed_form_mode(d, m, n, noise):
    case = xo.closed_form_case(d, m, n, noise)
    res = _run(case, gradient="source")
    assert res.backend == "hip" and res.x.shape == (n, d)
    assert np.all(res.status == xo.CONVERGED_GRADIENT), res
    bound = xo.gradient_test_bound(case["H"], case["gtol"])
    err = np.linalg.norm(res.x - case["x_hat"], axis=1)
    print("max |x - x_hat| %.3e, bound %.3e; iterations %s" % (err.max(), bound, res.iterations))
    assert np.all(err <= bound)
    assert np.all(res.grad_norm <= case["gtol"]) and np.all(res.value == res.logprior + res.loglike)
    _check_densities(case, res)
    _check_first_order(case, res, case["gtol"])
    if d >= 64:
        assert res.iterations.min() > xo.HISTORY  # the ring of pairs wrapped


# ---- 2. the reference's own results -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["extmodel", "poisson_families", "ring"])
def test_at_least_the_references_value(name):
    case = xo.fixture_posteriors()[name]
    assert np.array_equal(case["starts"], GOLDEN[name + "_starts"])
    res = _run(case, gradient="source")
    ref = GOLDEN[name + "_logprior"] + GOLDEN[name + "_loglike"]
    print(name, "device", res.value, "reference", ref)
    assert np.all(res.status == xo.CONVERGED_GRADIENT)
    assert np.all(res.value >= ref - 1e-10 * np.abs(ref))
    _check_densities(case, res)
    if name == "extmodel":
        ml = tda.maximize(case["posterior"], initial_parameters=case["starts"], objective="likelihood", backend="hip")
        print(name, "device ML", ml.value, "reference", GOLDEN["extmodel_ml_loglike"])
        assert np.all(ml.status == xo.CONVERGED_GRADIENT)
        assert np.all(ml.value >= GOLDEN["extmodel_ml_loglike"] - 1e-10 * np.abs(GOLDEN["extmodel_ml_loglike"])) and np.all(ml.value == ml.loglike)
        x = tda.get_ML(case["posterior"], initial_parameters=case["starts"], backend="hip")
        assert np.array_equal(x, ml.x[ml.best])


# ---- 3. every form once ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wave", "student_t", "ar1", "families", "cauchy_difference"])
def test_every_form_of_the_contract(name):
    case = xo.form_cases()[name]
    res = _run(case, gradient="source")
    assert np.all(res.status == xo.CONVERGED_GRADIENT), res
    _check_densities(case, res)
    _check_first_order(case, res, case["gtol"])


# ---- 4. forward differences --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["extmodel", "joint_families"])
def test_forward_differences(name):
    case = xo.difference_cases()[name]
    res = _run(case)  # gradient='auto': neither source has every gradient function
    assert np.all(res.status == xo.CONVERGED_GRADIENT), res
    d = case["starts"].shape[1]
    assert np.all(res.evaluations >= (res.iterations + 1) * (d + 1))  # d evaluations per gradient
    _check_densities(case, res)
    for i in range(res.x.shape[0]):
        g, bound = np.max(np.abs(case["twin"].gradient(res.x[i]))), xo.difference_bound(case["twin"], res.x[i], case["gtol"])
        print("start %d: exact gradient %.3e, bound %.3e" % (i, g, bound))
        assert g <= bound
    if name == "extmodel":
        with pytest.raises(tda.EngineError) as exc:
            _run(case, gradient="source")
        assert "__device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, int n_outputs, int j)" in str(exc.value)


# ---- 5. supports and non-finite values ----------------------------------------------------------------------------------------------------
def test_iterates_stay_inside_a_support():
    case = xo.support_case()
    res = _run(case)
    inside = slice(0, -1)
    assert np.all(res.status[inside] == xo.CONVERGED_GRADIENT) and np.all(res.x[inside] > 0.0) and np.all(np.isfinite(res.value[inside]))
    _check_densities(case, res, range(res.x.shape[0] - 1))
    _check_first_order(dict(case, starts=case["starts"][inside]), tda.maximize(case["posterior"], initial_parameters=case["starts"][inside], backend="hip"), case["gtol"])
    assert res.status[-1] == xo.INFEASIBLE_START and np.array_equal(res.x[-1], case["starts"][-1]) and res.iterations[-1] == 0 and res.evaluations[-1] == 1
    assert res.best is not None and res.best < res.x.shape[0] - 1
    # the likelihood alone knows no support: the same start runs
    ml = _run(case, objective="likelihood")
    assert ml.status[-1] != xo.INFEASIBLE_START and ml.iterations[-1] > 0 and np.isfinite(ml.value[-1]) and ml.value[-1] == ml.loglike[-1]
    assert np.all(ml.status == xo.CONVERGED_GRADIENT)


def test_nan_outputs_are_failed_trials():
    case = xo.nan_case()
    res = _run(case)
    print(res, res.x)
    assert np.all(np.isfinite(res.value)) and np.all(res.x[:, 0] <= xo.NAN_ABOVE)
    assert np.all(np.isin(res.status, (xo.LINESEARCH_FAILED, xo.MAX_ITER)))  # the pull goes across the threshold: no stationary point below it
    assert np.all(res.x[:, 0] > xo.NAN_ABOVE - 1e-6)
    _check_densities(case, res)


# ---- 6. two modes ------------------------------------------------------------------------------------------------------------------------
def test_two_modes_are_both_found_and_the_higher_is_best():
    case = xo.two_modes_case()
    res = _run(case)
    assert np.all(res.status == xo.CONVERGED_GRADIENT)
    # near a mode g = -H (x - x*) up to the change of H over the distance, which the factor 2 covers many times over (the distances are 1e-7)
    bounds = [2.0 * xo.gradient_test_bound(H, case["gtol"]) for H in case["H"]]
    dist = np.linalg.norm(res.x[:, None, :] - case["modes"][None], axis=2)
    which = np.argmin(dist, axis=1)
    print("ends per mode", np.bincount(which), "largest distance %.2e, bounds %s" % (dist.min(axis=1).max(), bounds))
    assert np.all(dist[np.arange(len(which)), which] <= np.array(bounds)[which])
    assert set(which) == {0, 1}
    values = [case["twin"].value(x) for x in case["modes"]]
    assert which[res.best] == int(np.argmax(values)) and res.value[res.best] == res.value.max()


# ---- 7. the public interface -------------------------------------------------------------------------------------------------------------
def test_get_map_feeds_sample():
    import scipy.stats as st

    case = xo.fixture_posteriors()["ring"]
    post, d = case["posterior"], case["starts"].shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x = tda.get_MAP(post, n_starts=16, seed=5)
        again = tda.maximize(post, n_starts=16, seed=5)
        other = tda.maximize(post, n_starts=16, seed=6)
    assert x.shape == (d,) and again.backend == "hip" and np.array_equal(x, again.x[again.best])
    twice = tda.maximize(post, n_starts=16, seed=5)
    for field in ("x", "value", "logprior", "loglike", "grad_norm", "iterations", "evaluations", "status"):
        assert np.array_equal(getattr(again, field), getattr(twice, field), equal_nan=True), field
    assert not np.array_equal(again.x, other.x)
    # the starts in the three shapes
    one = tda.maximize(post, initial_parameters=case["starts"][0])
    many = tda.maximize(post, initial_parameters=case["starts"])
    listed = tda.maximize(post, initial_parameters=[row for row in case["starts"]])
    assert one.x.shape == (1, d) and many.x.shape == case["starts"].shape and np.array_equal(many.x, listed.x) and np.array_equal(one.x[0], many.x[0])
    with pytest.raises(TypeError, match="options"):
        tda.get_MAP(post, options={"maxiter": 3})
    # the ends of the optimiser start the chains
    res = tda.sample(post, tda.GaussianRandomWalk(1e-4 * np.eye(d)), 20, n_chains=16, initial_parameters=[row for row in again.x], backend="hip", seed=1)
    assert res["backend"] == "hip"
    first = np.stack([tda.get_samples(res, "parameters")["chain_%d" % c][0] for c in range(16)])
    assert np.array_equal(first, again.x)
    assert isinstance(post.prior, st._multivariate.multivariate_normal_frozen)


def test_lds_refusal_names_the_bytes():
    import scipy.stats as st

    from . import extwave as xw

    m = 16
    # a workspace with which the MALA program fits (56000 + 2048 + 128 bytes) and which leaves no room for the ring of pairs
    src = xw.source(gradient="wave").replace("#define TDA_WORKSPACE (WV_K * 64)", "#define TDA_WORKSPACE 7000")
    assert src != xw.source(gradient="wave")
    post = tda.Posterior(st.multivariate_normal(np.zeros(4), np.eye(4)), tda.GaussianLogLike(np.zeros(m), 1e-4 * np.eye(m)), tda.DeviceModel(src, m))
    with pytest.raises(tda.EngineError) as exc:
        tda.maximize(post, initial_parameters=np.zeros(4), backend="hip")
    text = str(exc.value)
    print(text)
    assert "at most 64 KiB of LDS per start" in text and "18528 bytes for the ring" in text and "%d bytes for its %d outputs" % (8 * m, m) in text
