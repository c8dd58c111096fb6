"""HMC without a GPU: the NumPy twin (tests/exthmc.py) tied to the oracle's MALA at one leapfrog step, its reversibility and the
order of its energy error, the host class against the twin, the lowering pass, the HMC program compiled offline, the build
description through a stand-alone host program (tests/hmc_build_main.cpp, also built with the address and undefined-behaviour
sanitizers), and the admission of every case that tests/test_gpu_hmc.py runs."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import scipy.stats as st

from oracle import tinyda_oracle as orc

from . import exthmc as xh
from . import extloglike as xl
from . import extloglikewave as xlw
from . import extmodel as xm
from . import extprior as xp
from . import extpriorgrad as xg
from . import extpriorwave as xpw
from . import extwave as xw
from .extprogram import CSRC, MALA_KERNELS, ROOT, assert_switch_is_an_option_only, assert_without_scratch, compile_program, needs_hipcc
from .test_gpu_mala_source import CASES as MALA_CASES
from .test_mala_source import FORWARD_ONLY_SRC

HMC_KERNELS = ("tda_user_hmc_steps", "tda_user_mala_grad0")
HMC = ["TDA_USER_MALA", "TDA_USER_HMC"]
CXX = shutil.which("g++") or shutil.which("c++")


# ---- 1. one leapfrog step under unit mass is MALA ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(MALA_CASES))
def test_one_leapfrog_step_is_the_oracles_mala(case):
    """theta + eps (z + eps / 2 g) against theta + eps^2 / 2 g + eps z, and K0 - K1 against the two transition densities: equal
    algebraically, rounded in another order.  Variates from a fixed generator (seed 20260 + d: no mask flips; a flip would be a tie
    in u < alpha and ask for another seed, not another tolerance).  The adaptive cases run the twin towards MALA's 0.57."""
    d, m, noise, adaptive, scaling, _ = MALA_CASES[case]
    N, T = 13, 120
    _, theta0, _, _, _, level = xh.gaussian_problem(d, m, noise, N, seed=d * 1000 + m)
    rng = np.random.default_rng(20260 + d)
    z, u = rng.standard_normal((N, T, d)), rng.random((N, T))
    ref = orc.run_mh(level, dict(kind="mala", scaling=scaling, adaptive=adaptive, gamma=1.01, period=20), theta0, z, u)
    got = xh.run_hmc(level, dict(xh.hmc(scaling, 1, adaptive), alpha_star=0.57), theta0, z, u)
    print(case, "acceptance %.3f, max relative difference of the log-posterior %.1e"
          % (ref["accepted"][:, 1:].mean(), np.max(np.abs(got["logpost"] / ref["logpost"] - 1.0))))
    assert np.array_equal(got["accepted"], ref["accepted"])
    np.testing.assert_allclose(got["logpost"], ref["logpost"], rtol=1e-9)
    np.testing.assert_allclose(got["scaling"], ref["scaling"], rtol=1e-12)
    assert 0.05 < ref["accepted"][:, 1:].mean() < 0.98


# ---- 2. / 3. the leapfrog map ---------------------------------------------------------------------------------------------------------
def test_trajectories_are_reversible():
    """L steps, the momentum negated, L steps again: back at the start, to 1e-10 of the scale of theta and of p"""
    d, m, L, N = 5, 23, 7, 9
    _, theta0, _, _, _, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    rng = np.random.default_rng(1)
    p0, eps, w = rng.standard_normal((N, d)), np.full(N, 0.04), xh.MASS(d)
    lp, ll, F = level.evaluate(theta0)
    th1, p1, (_, _, g1), ended = xh.leapfrog(level, theta0, p0, level.grad_logpost(theta0, F), eps, w, L)
    assert not ended.any() and np.max(np.abs(th1 - theta0)) > 0.05
    th2, p2, _, ended = xh.leapfrog(level, th1, -p1, g1, eps, w, L)
    assert not ended.any()
    print("reversibility: theta %.1e, p %.1e" % (np.max(np.abs(th2 - theta0)), np.max(np.abs(-p2 - p0))))
    assert np.max(np.abs(th2 - theta0)) <= 1e-10 * np.max(np.abs(theta0))
    assert np.max(np.abs(-p2 - p0)) <= 1e-10 * np.max(np.abs(p0))


def test_energy_error_is_second_order():
    """max |dH| over 50 trajectories of the same length in time: half the step size (and twice the steps) divides it by about 4"""
    d, m, N = 5, 23, 50
    _, theta0, _, _, _, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    rng = np.random.default_rng(2)
    z, u = rng.standard_normal((N, 1, d)), np.zeros((N, 1))
    worst = [np.max(np.abs(xh.run_hmc(level, xh.hmc(eps, L), theta0, z, u)["dH"])) for eps, L in ((0.02, 8), (0.01, 16))]
    print("max |dH|: %.3e at eps = 0.02, %.3e at eps = 0.01, ratio %.2f" % (worst[0], worst[1], worst[0] / worst[1]))
    assert 3.0 < worst[0] / worst[1] < 5.0


# ---- 4. the host class is the twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
def test_host_class_is_the_twin(adaptive, monkeypatch):
    """tda.HMC under the host protocol on recorded variates: masks exact, log-posteriors 1e-10, the adapted step size 1e-12"""
    import tinyda_amd as tda

    d, m, N, T, L = 5, 23, 3, 60, 4
    y, theta0, pm, pv, nz, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    rng = np.random.default_rng(3)
    z, u = rng.standard_normal((N, T, d)), rng.random((N, T))
    tw = xh.hmc(0.05, L, adaptive, xh.MASS(d))
    ref = xh.run_hmc(level, tw, theta0, z, u)
    assert 0.1 <= ref["accepted"][:, 1:].mean() <= 0.9
    model = tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0], reference_gradient=lambda t, s: xm.np_vjp(t, s)[0])
    post = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, np.diag(nz)), model)
    for c in range(N):
        prop = tda.HMC(scaling=0.05, n_leapfrog=L, inv_mass=xh.MASS(d), adaptive=adaptive, gamma=1.01, period=20)
        prop.setup_proposal(parameters=theta0[c], posterior=post)
        assert prop.compute_gradient == prop._compute_gradient and prop.alpha_star == 0.65
        zs = iter(z[c])
        monkeypatch.setattr(np.random, "standard_normal", lambda n: next(zs))
        link = post.create_link(theta0[c])
        accepted = []
        with np.errstate(over="ignore"):
            for s in range(T):
                cand = post.create_link(prop.make_proposal(link))
                acc = u[c, s] < prop.get_acceptance(cand, link)
                if acc:
                    link = cand
                accepted.append(acc)
                prop.adapt(parameters=link.parameters, accepted=accepted)
                assert acc == bool(ref["accepted"][c, s + 1]), (c, s)
                np.testing.assert_allclose(link.posterior, ref["logpost"][c, s + 1], rtol=1e-10)
        np.testing.assert_allclose(prop.scaling, ref["scaling"][c], rtol=1e-12)


def test_constructor_refuses_bad_trajectories():
    import tinyda_amd as tda

    for bad in (dict(n_leapfrog=0), dict(n_leapfrog=1025), dict(n_leapfrog=2.5), dict(inv_mass=[1.0, 0.0]), dict(inv_mass=[1.0, -2.0]),
                dict(inv_mass=[np.nan, 1.0])):
        with pytest.raises(ValueError):
            tda.HMC(0.1, **bad)
    prop = tda.HMC(0.1, inv_mass=[1.0, 2.0, 3.0])
    post = _posterior(2, 1)
    with pytest.raises(ValueError, match="inv_mass"):
        prop.setup_proposal(parameters=np.zeros(2), posterior=post)


# ---- 5. lowering ----------------------------------------------------------------------------------------------------------------------
def _posterior(d, m, model=None, likelihood=None, prior=None):
    import tinyda_amd as tda

    return tda.Posterior(st.multivariate_normal(0.1 * np.ones(d), np.diag(0.5 + 0.01 * np.arange(d))) if prior is None else prior,
                         tda.GaussianLogLike(np.zeros(m), 0.01 * np.eye(m)) if likelihood is None else likelihood,
                         tda.DeviceModel(xm.source(), m) if model is None else model)


def _lower(posts, prop):
    from tinyda_amd.lowering import lower

    return lower(posts, prop)


def test_lowering_plans():
    """HMC lowers wherever MALA over a DeviceModel does, with its own kind, trajectory length and mass in the plan"""
    import tinyda_amd as tda
    from tinyda_amd import _lib

    assert _lib.PROP_HMC == 7
    y, par = np.zeros(23), 0.1 * np.ones(23)
    cauchy, lognormal = xpw.cauchy_difference(13), tda.DevicePrior(xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, 5, np.zeros(5), np.ones(5))
    forms = {
        "gaussian": _posterior(5, 23),
        "diagonal noise": _posterior(5, 23, likelihood=tda.GaussianLogLike(y, np.diag(0.01 * (1.0 + np.arange(23))))),
        "d = 128, m = 2048": _posterior(128, 2048),
        "wave forms": _posterior(5, 24, model=tda.DeviceModel(xw.source("wave", "wave"), 24)),
        "DeviceLogLike": _posterior(5, 23, likelihood=tda.DeviceLogLike(xl.KINDS["t"][0], y, par)),
        "DeviceLogLike, coupled": _posterior(5, 23, likelihood=xlw.device_loglike("ar1", y, par, reference=False)),
        "DevicePrior": _posterior(5, 23, prior=lognormal),
        "DevicePrior, coupled": _posterior(13, 23, prior=xpw.device_prior(cauchy, reference=False)),
    }
    w = 0.5 + np.arange(128.0)
    for name, post in forms.items():
        d = post.prior.rvs().size if not hasattr(post.prior, "dim") else post.prior.dim
        for cls, kind in ((tda.MALA, _lib.PROP_MALA), (tda.HMC, _lib.PROP_HMC)):
            plan, why = _lower([post], cls(0.05, adaptive=True, period=50))
            assert plan is not None, (name, cls.__name__, why)
            assert plan[1]["kind"] == kind and plan[1]["adaptive"] and plan[1]["period"] == 50 and plan[0][0]["has_gradient"]
        plan, why = _lower([post], tda.HMC(0.05, n_leapfrog=11, inv_mass=w[:d]))
        assert plan is not None and plan[1]["n_leapfrog"] == 11 and np.array_equal(plan[1]["inv_mass"], w[:d]) and plan[1]["C_"] is None, (name, why)
    assert _lower([forms["gaussian"]], tda.HMC(0.05))[0][1]["inv_mass"] is None


def test_lowering_refusals():
    """every refusal of HMC: MALA's rule and MALA's words with the proposal's own name"""
    import tinyda_amd as tda
    from tinyda_amd._contract import SIG

    y, par = np.zeros(23), 0.1 * np.ones(23)
    hmc = tda.HMC(0.05)

    def refused(posts, *needles):
        plan, why = _lower(posts, hmc)
        assert plan is None, needles
        assert "MALA" not in why, why
        for n in ("HMC",) + needles:
            assert n in why, (n, why)
        return why

    # a missing gradient in each of the three sources
    refused([_posterior(5, 23, model=tda.DeviceModel(FORWARD_ONLY_SRC, 23))], "HMC over a source-defined model needs", SIG["tda_gradient"])
    refused([_posterior(5, 23, likelihood=tda.DeviceLogLike(xl.TERM_ONLY_SRC, y, par))], "HMC with a DeviceLogLike needs", SIG["tda_loglike_term_grad"])
    refused([_posterior(5, 23, likelihood=tda.DeviceLogLike(xlw.without_grad(xlw.AR1_SRC), y, par))], "that couples outputs", SIG["tda_loglike_grad_wave"])
    refused([_posterior(5, 23, prior=tda.DevicePrior(xp.LOGNORMAL_SRC, 5, np.zeros(5), np.ones(5)))], "is not lowered under HMC", SIG["tda_logprior_term_grad"])
    # a hierarchy, the built-in linear model, the Rosenbrock example, a batched host model
    post = _posterior(5, 23)
    plan, why = _lower([post, post], hmc)
    assert plan is None and "hierarchies" in why
    linear = tda.Posterior(post.prior, tda.GaussianLogLike(np.zeros(3), 0.01 * np.eye(3)), tda.LinearModel(np.ones((3, 5))))
    assert refused([linear]).startswith("HMC: single level, a DeviceModel with tda_gradient")
    assert _lower([linear], tda.MALA(0.05))[0] is not None  # (MALA keeps the engine's linear-Gaussian kernel)
    batched = tda.Posterior(post.prior, post.likelihood, tda.BatchedModel(lambda th: np.zeros((th.shape[0], 23)), 23))
    refused([batched], "a DeviceModel with tda_gradient")
    # the sizes: 129 parameters, 2049 outputs
    plan, why = _lower([_posterior(129, 23)], hmc)
    assert plan is None and why == "more than 128 parameters"
    refused([_posterior(5, 2049)], "at most 2048 outputs")
    # a JointPrior of norm / uniform components and a dense prior covariance
    refused([_posterior(2, 3, prior=tda.JointPrior([st.norm(0.0, 1.0), st.uniform(-1.0, 2.0)]))])
    dense = st.multivariate_normal(np.zeros(2), np.array([[1.0, 0.3], [0.3, 1.0]]))
    plan, why = _lower([_posterior(2, 3, prior=dense)], hmc)
    assert plan is None


def test_sample_falls_back_with_a_reason_naming_hmc():
    """backend='auto' over a LinearModel warns once and runs the host class; backend='hip' raises the same reason"""
    import tinyda_amd as tda
    from tinyda_amd.api import HostFallbackWarning

    A = np.array([[1.0, 0.5], [0.2, 1.0], [0.3, 0.3]])
    post = tda.Posterior(st.multivariate_normal(np.zeros(2), np.eye(2)), tda.GaussianLogLike(np.array([0.3, -0.2, 0.1]), 0.25 * np.eye(3)), tda.LinearModel(A))
    with pytest.raises(tda.EngineError, match="HMC: single level, a DeviceModel with tda_gradient"):
        tda.sample(post, tda.HMC(0.2, n_leapfrog=3), 10, n_chains=2, backend="hip")
    np.random.seed(4)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.HMC(0.2, n_leapfrog=3), 40, n_chains=2, backend="auto")
    fb = [x for x in w if issubclass(x.category, HostFallbackWarning)]
    assert len(fb) == 1 and "HMC" in str(fb[0].message)
    assert res["backend"] == "host" and len(res["chain_0"]) == 41
    assert len({tuple(lk.parameters) for lk in res["chain_0"]}) > 12  # (proposals were accepted: the chain moved)
    assert all(np.isfinite(lk.posterior) for lk in res["chain_1"])


# ---- 6. the HMC program, compiled offline as shipped ----------------------------------------------------------------------------------
@needs_hipcc
def test_hmc_program_compiles_without_scratch(tmp_path):
    """tda_user_hmc_steps in place of tda_user_mala_steps, tda_user_mala_grad0 beside it; no scratch memory and no spilled vector
    registers for extmodel's source and for the ring with both wave forms (measured, hipcc of ROCm 7, gfx950: 141 and 125 vector
    registers in tda_user_hmc_steps, 131 and 114 in tda_user_mala_steps of the same sources)"""
    assert_without_scratch(tmp_path, "extmodel", xm.source(), HMC, HMC_KERNELS)
    ring = HMC + ["TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE"]
    rc, log, usage = compile_program(tmp_path, "ring", xw.source("wave", "wave"), ring)
    assert rc == 0 and set(usage) == set(HMC_KERNELS), log[-3000:]
    print("ring", usage["tda_user_hmc_steps"])
    assert usage["tda_user_hmc_steps"]["ScratchSize [bytes/lane]"] == 0 and usage["tda_user_hmc_steps"]["VGPRs Spill"] == 0
    # the switch alone selects the kernel: without it the program is the MALA program
    rc, log, usage = compile_program(tmp_path, "mala", xm.source(), ["TDA_USER_MALA"])
    assert rc == 0 and set(usage) == set(MALA_KERNELS), log[-3000:]


@needs_hipcc
@pytest.mark.parametrize("form", ["student_t", "ar1_wave", "lognormal_prior", "cauchy_prior_wave"])
def test_hmc_program_compiles_under_every_form(tmp_path, form):
    src, switches = {
        "student_t": (xm.source() + xl.KINDS["t"][0], ["TDA_LOGLIKE_SOURCE"]),
        "ar1_wave": (xlw.full_source("ar1"), ["TDA_LOGLIKE_SOURCE", "TDA_LOGLIKE_WAVE"]),
        "lognormal_prior": (xm.source() + xp.LOGNORMAL_SRC + xg.LOGNORMAL_GRAD_SRC, ["TDA_PRIOR_SOURCE"]),
        "cauchy_prior_wave": (xm.source() + xpw.CAUCHY_DIFF_SRC, ["TDA_PRIOR_SOURCE", "TDA_PRIOR_WAVE"]),
    }[form]
    assert_without_scratch(tmp_path, form, src, HMC + switches, HMC_KERNELS)


def test_the_switch_is_an_option_only():
    header = assert_switch_is_an_option_only(r"TDA_USER_HMC\b", ("tda_usermodel.inc", "tda_user_build.h", "tda_host_hmc.inc"))
    assert "tda_engine_set_hmc" not in header and "TDA_PROP_HMC = 7" in header
    hmc_header = open(os.path.join(ROOT, "include", "tinyda_amd_hmc.h")).read()
    assert re.search(r"int tda_engine_set_hmc\(tda_engine\* e, int32_t n_leapfrog, const double\* inv_mass", hmc_header)


@needs_hipcc
def test_source_without_gradient_names_the_signature(tmp_path):
    from tinyda_amd._contract import SIG

    rc, log, _ = compile_program(tmp_path, "no_gradient", FORWARD_ONLY_SRC, HMC)
    assert rc != 0 and "tda_gradient_missing" in log and SIG["tda_gradient"] in log


def test_hmc_symbol_table():
    """the third header's one function is bound by load() through its own table, never by load_from (the CPU build has no HMC)"""
    from tinyda_amd import _lib

    assert set(_lib.HMC_SYMBOLS) == {"tda_engine_set_hmc"} and not set(_lib.HMC_SYMBOLS) & set(_lib.SYMBOLS)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyda_amd_hmc.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(tda_[a-z_]+)\s*\(", text)) == set(_lib.HMC_SYMBOLS)


# ---- 7. the build description ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def build_tool(request, tmp_path_factory):
    """tests/hmc_build_main.cpp, built once as it is and once with -fsanitize=address,undefined (a stand-alone program: the
    sanitizers' runtimes are linked in, nothing is preloaded); a sanitizer report ends the program with a non-zero status"""
    if CXX is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("hmc_build_" + request.param)
    exe = str(work / "tool")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    r = subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "hmc_build_main.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and request.param == "sanitized" and re.search(r"cannot find.*(asan|ubsan)", r.stdout):
        pytest.skip("the sanitizers' runtime libraries are not installed")
    assert r.returncode == 0, r.stdout[-3000:]

    def run(*args, text=None):
        if text is not None:
            path = work / "input"
            path.write_bytes(text.encode())
            args += (str(path),)
        return subprocess.run([exe] + [str(a) for a in args], check=True, stdout=subprocess.PIPE, text=True).stdout

    return run


@pytest.mark.parametrize("forms", [(0, 0, 0, 0), (1, 1, 0, 0), (0, 0, 1, 1), (1, 1, 2, 2)], ids=lambda f: "fw%d_gw%d_ll%d_pr%d" % f)
def test_build_key_and_options(build_tool, forms):
    """an HMC program never comes out of the cache for a MALA request of the same source, or the reverse: the keys differ, and
    the options differ by exactly -DTDA_USER_HMC"""
    key, mala, hmc = build_tool("options", *forms).splitlines()
    assert key == "101"
    mala, hmc = mala.split(), hmc.split()
    assert "-DTDA_USER_MALA" in mala and "-DTDA_USER_HMC" not in mala
    assert sorted(hmc) == sorted(mala + ["-DTDA_USER_HMC"])
    assert [o for o in hmc if o != "-DTDA_USER_HMC"] == mala  # (the order of the others as it was)


def test_build_diagnosis_and_lds(build_tool):
    log = "error: static assertion failed: tda_gradient_missing: MALA needs ..."
    code, msg = build_tool("diagnose", 1, text=log).split("\n", 1)
    assert int(code) == -1 and msg.startswith("HMC needs what MALA needs -- ") and "tda_gradient" in msg
    code, msg = build_tool("diagnose", 0, text=log).split("\n", 1)
    assert int(code) == -1 and msg.startswith("MALA on a source-defined model")
    assert "with the HMC kernels" in build_tool("diagnose", 1, text="some other error")
    assert build_tool("lds", 0, 300).split() == ["2400", "2400", "2400"]  # the LDS per chain is the MALA program's
    assert build_tool("lds", 1, 300).split() == ["4800", "4800", "4800"]


# ---- the cases of tests/test_gpu_hmc.py: admitted here, run there --------------------------------------------------------------------
@pytest.mark.parametrize("case", list(xh.FORWARD_CASES) + list(xh.CONTRACT_CASES))
def test_gpu_cases_are_admissible(case):
    """on the engine's own variates (the oracle's Philox stream): one ulp on every gradient leaves the masks as they are and the
    log-posteriors within 1e-11, and the twin accepts between 10 % and 90 % of its proposals"""
    level, prop, theta0, T, _ = xh.forward_case(case) if case in xh.FORWARD_CASES else xh.contract_case(case)
    assert T * prop["n_leapfrog"] <= 480 and theta0.shape[0] == 13
    z, u = xh.philox_variates(xh.SEED, xh.CHAIN_OFFSET, theta0.shape[0], T, theta0.shape[1])
    ref = xh.assert_admissible(level, prop, theta0, z, u)
    if case == "lognormal_prior_at_the_edge":
        inside = (ref["ended"] > 0) & (ref["ended"] < prop["n_leapfrog"])
        print("trajectories that left the support at an interior leapfrog step: %d" % inside.sum())
        assert inside.sum() >= 10 and not np.any(ref["accepted"][:, 1:][ref["ended"] > 0])


def test_nan_region_case_is_admissible():
    level, free, prop, theta0, T, _, _ = xh.nan_case()
    z, u = xh.philox_variates(xh.SEED, xh.CHAIN_OFFSET, theta0.shape[0], T, theta0.shape[1])
    ref = xh.assert_admissible(level, prop, theta0, z, u)
    assert np.count_nonzero(ref["ended"]) >= 10 and not np.array_equal(xh.run_hmc(free, prop, theta0, z, u)["accepted"], ref["accepted"])
