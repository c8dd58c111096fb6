"""The three kernels over the gradient of a source-defined posterior -- tda_user_mala_steps, tda_user_hmc_steps and
tda_user_maximize -- over the combined forms of tests/extforms.py: two wave forms together, a wave gradient above 64
parameters, a coupled likelihood with m across a multiple of 64 beside a coupled prior, at the boundary shapes
d in {1, 63, 64, 65, 127, 128}, m in {1, 63, 64, 65, 129, 2048}.

MALA runs on the engine's own Philox stream against the oracle, HMC against the twin of tests/exthmc.py: masks exact,
log-posterior 1e-10, states 1e-9 (atol 1e-12), final step size 1e-12 (extengine.compare).  tda.maximize at the bars of
tests/test_gpu_optimize.py: both densities 1e-10, the twin's exact gradient at most gtol + 1e-10 (|log-prior| + |log-likelihood|
+ 1).  tests/test_forms_sweep_cases.py admits every case on the CPU, on the stored step sizes of tests/golden/forms_sweep.json:
no assertion here exempts a chain, a start or a case."""
from functools import lru_cache

import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extforms as xf
from . import exthmc as xh
from . import extoptimize as xo
from .extengine import assert_rate, assert_resume_bitwise, compare, run_forward

pytestmark = pytest.mark.gpu
IDS = [xf.form_case(i)["name"] for i in range(xf.N_FORMS)]


@lru_cache(maxsize=2)
def _built(i):
    row = xf.stored()[i]
    c = xf.build(xf.form_case(i), seed=row["seed"])
    assert row["name"] == c["name"]
    return c, row


def _steps(i, kind):
    """the engine on its own variates against the oracle (MALA) or the twin (HMC), and the resume check where the case has one"""
    c, row = _built(i)
    prop, T = xf.proposal(c, kind, row[kind + "_scaling"])
    params, stats, acc, scal, _, z, u = run_forward(xf.make_engine(c, prop), c["theta0"], T, prop)
    rows = T // c["thin"]
    params, stats, acc = params[:rows], stats[:rows], acc[:rows]
    zz, uu = np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1)
    with np.errstate(all="ignore"):
        ref = orc.run_mh(c["level"], prop, c["theta0"], zz, uu) if kind == "mala" else xh.run_hmc(c["level"], prop, c["theta0"], zz, uu)
    assert_rate(ref["accepted"][:, 1:])
    assert np.all(np.isfinite(stats))
    compare(params, stats, acc, xf.thinned(ref, c["thin"], T), scal)
    if c["resume"]:  # the gradient at the current states travels in the blob

        def make():
            e = xf.make_engine(dict(c, thin=1), prop)
            e.init(c["theta0"])
            return e

        assert_resume_bitwise(make, whole=T, first=T // 2 + 1)


@pytest.mark.parametrize("i", range(xf.N_FORMS), ids=IDS)
def test_mala_matches_oracle(i):
    _steps(i, "mala")


@pytest.mark.parametrize("i", range(xf.N_FORMS), ids=IDS)
def test_hmc_matches_twin(i):
    _steps(i, "hmc")


def _close(got, want):
    return got == want or abs(got - want) <= xo.DENSITY_RTOL * max(1.0, abs(want))  # (equal: both -inf, outside a support under objective='likelihood')


def _maximize(c, m_case, **kw):
    import tinyda_amd as tda

    return tda.maximize(xf.posterior(c), initial_parameters=m_case["starts"], backend="hip", gradient="source", gtol=m_case["gtol"], objective=m_case["objective"], **kw)


@pytest.mark.parametrize("i", range(xf.N_FORMS), ids=IDS)
def test_maximize_converges_to_a_stationary_point_of_the_twin(i):
    c = xf.build_for_maximize(xf.form_case(i), seed=xf.stored()[i]["seed"])
    m_case = xf.maximize_case(c)
    res = _maximize(c, m_case)
    twin, objective = m_case["twin"], m_case["objective"]
    print(res.status, res.iterations, res.evaluations)
    assert res.backend == "hip" and np.all(res.status == xo.CONVERGED_GRADIENT), res
    for k in range(res.x.shape[0]):
        lp, ll = twin.evaluate(res.x[k])
        g = np.max(np.abs(twin.gradient(res.x[k], objective)))
        bound = m_case["gtol"] + 1e-10 * ((1.0 + abs(ll)) if objective == "likelihood" and not np.isfinite(lp) else twin.magnitude(res.x[k]))
        print("start %d: iterations %d, |dlp| %.1e, |dll| %.1e, exact gradient %.3e (kernel's %.3e), bound %.3e"
              % (k, res.iterations[k], abs(res.logprior[k] - lp), abs(res.loglike[k] - ll), g, res.grad_norm[k], bound))
        assert _close(res.logprior[k], lp) and _close(res.loglike[k], ll)
        assert g <= bound


# ---- the LDS edge: the all-wave program (ring wave / wave, AR(1), Cauchy difference) at the largest m it is admitted with -------------
# The step programs hold 2 m doubles beside their static part (parameters, gradient, the ring's 24 KiB of workspace), and fit at the
# 2048 outputs the engine stops at: case 0 of the list is that run, and 2049 outputs meet the rule that names the 2048.  The optimiser
# holds the ring of L-BFGS pairs besides: extforms.MAP_STATIC_LDS bytes in all (the figure of the offline compile, which
# tests/test_forms_sweep_cases.py asserts), so that 16 m bytes more fit up to extforms.MAP_M_MAX = 1274 outputs: case 0 of the
# maximize test is that run, and one output more is refused with the bytes.
def _all_wave(m, d=128, N=5):
    c = xf.form_case(0)
    assert (c["model"], c["like"], c["prior"], c["d"], c["m"]) == ("ring_ww", "ar1", "cauchy", 128, 2048) and xf.MAXIMIZE_M == {0: xf.MAP_M_MAX}
    return xf.build(dict(c, d=d, m=m), N=N)


@pytest.mark.parametrize("kind", ["mala", "hmc"])
def test_step_programs_stop_at_2048_outputs(kind):
    from tinyda_amd import _lib

    c = _all_wave(2049)
    prop, _ = xf.proposal(c, kind, 0.01)
    e = xf.make_engine(c, prop)
    try:
        with pytest.raises(_lib.EngineError, match="%s over a source-defined model: at most 2048 outputs" % kind.upper()):
            e.init(c["theta0"])
    finally:
        e.close()


def test_maximize_refuses_the_first_m_that_does_not_fit():
    import tinyda_amd as tda

    m = xf.MAP_M_MAX + 1
    assert m == 1275
    c = _all_wave(m)
    with pytest.raises(tda.EngineError) as exc:
        _maximize(c, dict(xf.maximize_case(c), starts=c["theta0"][:2]))
    text = str(exc.value)
    print(text)
    assert "at most 64 KiB of LDS per start" in text and "this source needs %d bytes" % xf.MAP_STATIC_LDS in text
    assert "18528 bytes for the ring" in text and "%d bytes for its %d outputs" % (16 * m, m) in text
