"""Dense inverse masses of HMC / NUTS without a GPU (include/tinyda_amd_dense_mass.h): the NumPy twins of tests/extdense.py tied
bit for bit to the diagonal twins at W = I and W = diag(powers of 4), and by a change of variables to the unit-mass twins on the
whitened posterior; the host classes against the twins; the constructors' validation and the lowering; mass_from_samples against
np.cov; the dense programs compiled offline; the admission of every case that tests/test_gpu_dense_mass.py runs; and the
end-to-end conditions of that file met by the host class alone."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import scipy.stats as st

from . import extdense as xd
from . import exthmc as xh
from . import extmodel as xm
from . import extnuts as xn
from . import extwave as xw
from .extprogram import CSRC, ROOT, assert_without_scratch, needs_hipcc

TRACE_KEYS = ("theta", "logprior", "loglike", "logpost", "accepted", "scaling")
NUTS_KEYS = TRACE_KEYS + ("stop", "depth", "selected", "n_leaf", "stat", "totals")


def _problem(kind, N=5, T=40):
    """a forward case of exthmc / extnuts (d = 5, m = 23, adaptive) on variates of a fixed generator"""
    d, m = 5, 23
    y, theta0, pm, pv, nz, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    rng = np.random.default_rng(17)
    z = rng.standard_normal((N, T, d))
    if kind == "hmc":
        return level, theta0, z, rng.random((N, T)), xh.hmc(0.05, 4, True)
    D = 4
    draws = xn.ArrayDraws(rng.integers(0, 2, (N, T, D)).astype(bool), rng.random((N, T, D)), rng.random((N, T, 1 << D)))
    return level, theta0, z, draws, xn.nuts(0.05, D, True)


def _run(kind, level, prop, theta0, z, draws):
    dense = "chol" in prop
    run = (xd.run_hmc if dense else xh.run_hmc) if kind == "hmc" else (xd.run_nuts if dense else xn.run_nuts)
    return run(level, prop, theta0, z, draws)


# ---- 1, 2. the dense twin at a diagonal W is the diagonal twin, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hmc", "nuts"])
@pytest.mark.parametrize("mass", ["unit", "spread"])
def test_twin_at_a_diagonal_mass_is_the_diagonal_twin(kind, mass):
    """W = I against inv_mass=None, and W = diag(MASS_SPREAD) against MASS_SPREAD: powers of 4, so the square roots and every
    scaling are exact, and the terms outside the triangle add exact zeros"""
    level, theta0, z, draws, prop = _problem(kind)
    d = theta0.shape[1]
    w = None if mass == "unit" else xn.MASS_SPREAD(d)
    W = np.eye(d) if w is None else np.diag(w)
    chol = np.linalg.cholesky(W)
    assert np.array_equal(chol @ chol.T, W)
    ref = _run(kind, level, dict(prop, inv_mass=w), theta0, z, draws)
    got = _run(kind, level, dict(prop, chol=chol), theta0, z, draws)
    assert np.any(ref["scaling"] != prop["scaling"])
    assert 0.05 < ref["accepted"][:, 1:].mean() < 0.98 if kind == "hmc" else len(set(ref["stop"].ravel())) >= 2
    for key in NUTS_KEYS if kind == "nuts" else TRACE_KEYS:
        assert np.array_equal(got[key], ref[key]), key


# ---- 3. change of variables -----------------------------------------------------------------------------------------------------------
class _Whitened:
    """xi -> level at theta = L xi: the log-posterior of xi up to a constant, its gradient L^T g"""

    def __init__(self, level, chol):
        self.level, self.chol = level, chol

    def evaluate(self, xi):
        return self.level.evaluate(xi @ self.chol.T)

    def grad_logpost(self, xi, F):
        return np.asarray(self.level.grad_logpost(xi @ self.chol.T, F), dtype=float) @ self.chol


@pytest.mark.parametrize("case", ["hmc_d5_m23", "nuts_d5_m23", "hmc_d65_m23", "nuts_d2_m1"])
def test_dense_twin_is_the_unit_twin_on_the_whitened_posterior(case):
    """theta = L xi: HMC / NUTS under W = L L^T on theta is HMC / NUTS under unit mass on xi, with the same variates.  Masks and tree
    decisions exact, log-posterior 1e-10, states (mapped back by L) at the bar of the GPU tests, on admitted cases"""
    level, prop, theta0, T, _ = xd.forward_case(case)
    N, d = theta0.shape
    z, u = xd.variates(N, T, d)
    chol, kind = prop["chol"], prop["kind"]
    draws = u if kind == "hmc" else xn.PhiloxDraws(xd.SEED, xd.CHAIN_OFFSET, N)
    ref = xd.assert_admissible(level, prop, theta0, z, draws)[0]
    unit = dict({k: v for k, v in prop.items() if k != "chol"}, inv_mass=None)
    xi0 = np.linalg.solve(chol, theta0.T).T
    white = (xh.run_hmc if kind == "hmc" else xn.run_nuts)(_Whitened(level, chol), unit, xi0, z, draws)
    assert np.array_equal(white["accepted"], ref["accepted"])
    if kind == "nuts":
        for key in ("stop", "depth", "selected", "n_leaf"):
            assert np.array_equal(white[key], ref[key]), key
    np.testing.assert_allclose(white["logpost"], ref["logpost"], rtol=1e-10)
    np.testing.assert_allclose(white["theta"] @ chol.T, ref["theta"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(white["scaling"], ref["scaling"], rtol=1e-12)


# ---- 4. the host classes ----------------------------------------------------------------------------------------------------------------
def _host_posterior(d, m, y, pm, pv, nz):
    import tinyda_amd as tda

    model = tda.DeviceModel(xm.source(), m, reference=lambda t: xm.np_forward(t, m)[0], reference_gradient=lambda t, s: xm.np_vjp(t, s)[0])
    return tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, np.diag(nz)), model)


@pytest.mark.parametrize("adaptive", [False, True])
def test_host_hmc_is_the_twin(adaptive, monkeypatch):
    """tda.HMC(inv_mass=W) under the host protocol on recorded variates: masks exact, log-posteriors 1e-10, states 1e-9, the adapted
    step size 1e-12 (as tests/test_hmc.py ties the diagonal class)"""
    import tinyda_amd as tda

    d, m, N, T, L = 5, 23, 3, 60, 4
    y, theta0, pm, pv, nz, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    rng = np.random.default_rng(3)
    z, u = rng.standard_normal((N, T, d)), rng.random((N, T))
    W = xd.DENSE(d)
    post = _host_posterior(d, m, y, pm, pv, nz)
    first = tda.HMC(scaling=0.07, n_leapfrog=L, inv_mass=W, adaptive=adaptive, gamma=1.01, period=20)
    ref = xd.run_hmc(level, dict(xh.hmc(0.07, L, adaptive), chol=first.chol_inv_mass), theta0, z, u)
    assert 0.1 <= ref["accepted"][:, 1:].mean() <= 0.9
    for c in range(N):
        prop = tda.HMC(scaling=0.07, n_leapfrog=L, inv_mass=W, adaptive=adaptive, gamma=1.01, period=20)
        prop.setup_proposal(parameters=theta0[c], posterior=post)
        assert np.array_equal(prop.chol_inv_mass, first.chol_inv_mass) and np.array_equal(prop.inv_mass, W)
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
                np.testing.assert_allclose(link.parameters, ref["theta"][c, s + 1], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(prop.scaling, ref["scaling"][c], rtol=1e-12)
        assert (prop.scaling != 0.07) == adaptive


@pytest.mark.parametrize("adaptive", [False, True])
def test_host_nuts_is_the_twin(adaptive, monkeypatch):
    """tda.NUTS(inv_mass=W) on recorded draws: the selected leaf, the stop reason, the depth and `accepted` exact, the log-posterior
    1e-10, the states 1e-9, the adapted step size 1e-12 (as tests/test_nuts.py ties the diagonal class)"""
    import tinyda_amd as tda

    d, m, N, T, D = 5, 23, 3, 60, 4
    y, theta0, pm, pv, nz, level = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((N, T, d))
    fwd, u, leaf_u = rng.integers(0, 2, (N, T, D)), rng.random((N, T, D)), rng.random((N, T, 1 << D))
    W = xd.DENSE(d)
    chol = tda.NUTS(inv_mass=W).chol_inv_mass
    ref = xd.run_nuts(level, dict(xn.nuts(0.03, D, adaptive), chol=chol), theta0, z, xn.ArrayDraws(fwd.astype(bool), u, leaf_u))
    assert len(set(ref["stop"].ravel())) >= 2
    post = _host_posterior(d, m, y, pm, pv, nz)
    for c in range(N):
        prop = tda.NUTS(scaling=0.03, max_depth=D, inv_mass=W, adaptive=adaptive, gamma=1.01, period=20)
        prop.setup_proposal(parameters=theta0[c], posterior=post)
        at = dict(s=0, j=-1, k=0)

        def randint(n):
            at["j"], at["k"] = at["j"] + 1, 0
            at["merge"] = True
            return fwd[c, at["s"], at["j"]]

        def random():
            if at.pop("merge", False):
                return u[c, at["s"], at["j"]]
            at["k"] += 1
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


# ---- 5. validation and lowering ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["HMC", "NUTS"])
def test_constructor_validation(cls):
    import tinyda_amd as tda

    make = getattr(tda, cls)
    W = xd.DENSE(4)
    prop = make(inv_mass=W)
    assert np.array_equal(prop.inv_mass, W) and np.array_equal(prop.chol_inv_mass, np.linalg.cholesky(W))
    assert np.array_equal(prop.chol_inv_mass, np.tril(prop.chol_inv_mass))
    with pytest.raises(ValueError, match=r"not the shape \(3, 4\)"):
        make(inv_mass=W[:3])
    with pytest.raises(ValueError, match=r"not the shape \(2, 2, 2\)"):
        make(inv_mass=np.ones((2, 2, 2)))
    skew = W.copy()
    skew[0, 1] = np.nextafter(skew[0, 1], np.inf)
    with pytest.raises(ValueError, match=r"symmetric, W == W.T exactly: symmetrise it first"):
        make(inv_mass=skew)
    with pytest.raises(ValueError, match="positive definite: np.linalg.cholesky failed"):
        make(inv_mass=np.diag([1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="positive definite"):
        make(inv_mass=np.ones((3, 3)))
    bad = W.copy()
    bad[2, 2] = np.nan
    with pytest.raises(ValueError, match="must be finite"):
        make(inv_mass=bad)
    with pytest.raises(ValueError, match="adapt_mass = 200 with a dense inv_mass: the warm-up adaptation learns a diagonal mass"):
        make(inv_mass=W, adapt_mass=200)
    assert make(inv_mass=np.ones(4)).chol_inv_mass is None and make().chol_inv_mass is None
    post = types.SimpleNamespace(prior=st.multivariate_normal(np.zeros(3), np.eye(3)), model=None, likelihood=None)
    with pytest.raises(ValueError, match="inv_mass has 4 entries for 3 parameters"):
        prop.setup_proposal(parameters=np.zeros(3), posterior=post)


@pytest.mark.parametrize("cls", ["HMC", "NUTS"])
def test_lowering_carries_the_factor(cls):
    """a dense mass lowers where the diagonal one does: the plan differs by the key `dense_mass` (the factor) alone, and a plan
    without a dense mass has the keys it had"""
    import tinyda_amd as tda
    from tinyda_amd.lowering import lower

    d, m, N = 5, 23, 2
    y, theta0, pm, pv, nz, _ = xh.gaussian_problem(d, m, "diag", N, seed=5023)
    post = _host_posterior(d, m, y, pm, pv, nz)
    make = getattr(tda, cls)
    W = xd.DENSE(d)
    (_, diag), why = lower([post], make(inv_mass=np.diag(W).copy()))
    assert why is None and "dense_mass" not in diag and "adapt_mass" not in diag
    (_, dense), why = lower([post], make(inv_mass=W))
    assert why is None and set(dense) == set(diag) | {"dense_mass"} and dense["inv_mass"] is None
    assert np.array_equal(dense["dense_mass"], np.linalg.cholesky(W))
    assert {k: v for k, v in dense.items() if k not in ("dense_mass", "inv_mass")} == {k: v for k, v in diag.items() if k != "inv_mass"}
    # refused in the same places with the same reasons
    lin = tda.Posterior(st.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(y, np.diag(nz)), tda.LinearModel(np.ones((m, d))))
    assert lower([lin], make(inv_mass=W))[1] == lower([lin], make(inv_mass=np.diag(W).copy()))[1] is not None
    assert lower([post, post], make(inv_mass=W))[1] == lower([post, post], make(inv_mass=np.diag(W).copy()))[1] is not None


def test_symbols_and_header():
    """the two functions belong to the new header and their own symbol table; the switch is an option only"""
    from tinyda_amd import _lib

    assert set(_lib.DENSE_MASS_SYMBOLS) == {"tda_engine_set_dense_mass", "tda_engine_get_dense_mass"}
    assert not set(_lib.DENSE_MASS_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.MASS_SYMBOLS) | set(_lib.NUTS_SYMBOLS) | set(_lib.HMC_SYMBOLS))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tinyda_amd_dense_mass.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(tda_[a-z_]+)\s*\(", text)) == set(_lib.DENSE_MASS_SYMBOLS)
    assert "dense_mass" not in open(os.path.join(ROOT, "include", "tinyda_amd.h")).read()
    for f in ("tda_user_program.hip", "tda_user_args.h", "tda_usermodel.inc", "tda_user_build.h", "tda_host_dense_mass.inc"):
        assert not re.search(r"#\s*(define|undef)\s+TDA_DENSE_MASS\b", open(os.path.join(CSRC, f)).read()), f
    assert '"-DTDA_DENSE_MASS"' in open(os.path.join(CSRC, "tda_user_build.h")).read()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def build_tool(request, tmp_path_factory):
    """tests/dense_build_main.cpp, built once as it is and once with -fsanitize=address,undefined (a stand-alone program: the
    sanitizers' runtimes are linked in, nothing is preloaded)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    work = tmp_path_factory.mktemp("dense_build_" + request.param)
    exe = str(work / "tool")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "dense_build_main.cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and request.param == "sanitized" and re.search(r"cannot find.*(asan|ubsan)", r.stdout):
        pytest.skip("the sanitizers' runtime libraries are not installed")
    assert r.returncode == 0, r.stdout[-3000:]
    return lambda *args: subprocess.run([exe] + [str(a) for a in args], check=True, stdout=subprocess.PIPE, text=True).stdout


@pytest.mark.parametrize("kind", ["hmc", "nuts", "mala"])
def test_build_key_and_options(build_tool, kind):
    """a dense program never comes out of the cache for a diagonal request of the same source, or the reverse: the keys differ, and
    the options of an HMC / NUTS program differ by exactly -DTDA_DENSE_MASS; a MALA program takes no such option"""
    key, plain, dense = build_tool("options", kind).splitlines()
    assert key == "101"
    plain, dense = plain.split(), dense.split()
    assert "-DTDA_DENSE_MASS" not in plain and "-ffp-contract=off" in plain
    assert sorted(dense) == sorted(plain + (["-DTDA_DENSE_MASS"] if kind != "mala" else []))
    assert [o for o in dense if o != "-DTDA_DENSE_MASS"] == plain  # (the order of the others as it was)
    assert build_tool("lds").split() == ["1024"]


DENSE_FORMS = {
    "hmc": (lambda: xm.source(), ["TDA_USER_MALA", "TDA_USER_HMC", "TDA_DENSE_MASS"], ("tda_user_hmc_steps", "tda_user_mala_grad0")),
    "nuts": (lambda: xm.source(), ["TDA_USER_MALA", "TDA_USER_NUTS", "TDA_DENSE_MASS"], ("tda_user_nuts_steps", "tda_user_mala_grad0")),
    "nuts_ring_wave": (lambda: xw.source("wave", "wave"), ["TDA_USER_MALA", "TDA_USER_NUTS", "TDA_DENSE_MASS", "TDA_FORWARD_WAVE", "TDA_GRADIENT_WAVE"],
                       ("tda_user_nuts_steps", "tda_user_mala_grad0")),
}


@needs_hipcc
@pytest.mark.parametrize("form", list(DENSE_FORMS))
def test_dense_programs_compile_without_scratch(tmp_path, form):
    """-DTDA_DENSE_MASS beside -DTDA_USER_HMC / -DTDA_USER_NUTS: no scratch memory, no spilled vector registers (measured, hipcc of
    ROCm 7, gfx950, extmodel's source: 146 vector registers for HMC against 141 without the switch, 212 for NUTS against 207)"""
    src, switches, kernels = DENSE_FORMS[form]
    assert_without_scratch(tmp_path, form, src(), switches, kernels)


# ---- 6. mass_from_samples ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("records", ["arrays", "links"])
def test_mass_from_samples_is_the_regularised_pooled_covariance(records):
    import tinyda_amd as tda
    from tinyda_amd.records import DeviceChain, DeviceRecords, Link

    R, N, d, burn = 700, 5, 6, 100  # (more rows than one chunk of 256)
    rng = np.random.default_rng(8)
    P = (rng.standard_normal((R, N, d)) @ rng.standard_normal((d, d))) * np.logspace(-1, 1, d) + 3.0
    if records == "arrays":
        recs = DeviceRecords(P, np.zeros((R, N, 3)), np.ones((R, N), dtype=np.uint8))
        result = dict(sampler="MH", n_chains=N, **{"chain_%d" % i: DeviceChain(recs, i, None) for i in range(N)})
    else:
        result = dict(sampler="MH", n_chains=N, **{"chain_%d" % i: [Link(P[r, i], 0.0, None, 0.0) for r in range(R)] for i in range(N)})
    pooled = P[burn:].reshape(-1, d)
    T = pooled.shape[0]
    cov = np.cov(pooled, rowvar=False)
    W = tda.mass_from_samples(result, burnin=burn)
    assert isinstance(W, np.ndarray) and W.shape == (d, d) and np.array_equal(W, W.T)
    np.testing.assert_allclose(W, cov * T / (T + 5.0) + 1e-3 * 5.0 / (T + 5.0) * np.eye(d), rtol=1e-11, atol=1e-13)
    w = tda.mass_from_samples(result, burnin=burn, dense=False)
    assert w.shape == (d,)
    np.testing.assert_allclose(w, np.var(pooled, axis=0, ddof=1) * T / (T + 5.0) + 1e-3 * 5.0 / (T + 5.0), rtol=1e-11)
    np.testing.assert_allclose(tda.mass_from_samples(result, burnin=burn, chunk_rows=7), W, rtol=1e-11, atol=1e-13)
    assert tda.NUTS(inv_mass=W).chol_inv_mass.shape == (d, d) and tda.HMC(inv_mass=w).chol_inv_mass is None
    with pytest.raises(ValueError, match="at least two recorded states"):
        tda.mass_from_samples(result, burnin=R)


# ---- 7. the cases of tests/test_gpu_dense_mass.py: admitted here, run there --------------------------------------------------------------
def _admit(level, prop, theta0, T):
    N, d = theta0.shape
    z, u = xd.variates(N, T, d)
    draws = u if prop["kind"] == "hmc" else xn.PhiloxDraws(xd.SEED, xd.CHAIN_OFFSET, N)
    ref, dpost, dstate = xd.assert_admissible(level, prop, theta0, z, draws)
    # ten times what the perturbation moves fits the default bars: what is left for the device is summation order
    assert 10.0 * dpost <= 10.0 * xd.DEFAULT_TOLERANCE[0] and 10.0 * dstate <= 10.0 * xd.DEFAULT_TOLERANCE[1], (dpost, dstate)
    return ref


@pytest.mark.parametrize("case", list(xd.FORWARD_CASES))
def test_forward_cases_are_admissible(case):
    """on the engine's variates (the oracle's Philox stream): one ulp on every gradient and d 2^-52 on every product leave every mask
    and every tree as it is"""
    level, prop, theta0, T, _ = xd.forward_case(case)
    assert theta0.shape[0] == 13 and np.all(np.tril(prop["chol"], -1)[np.tril_indices(theta0.shape[1], -1)] != 0.0)
    ref = _admit(level, prop, theta0, T)
    assert prop["adaptive"] == bool(np.any(ref["scaling"] != prop["scaling"]))
    if prop["kind"] == "nuts":
        assert xn.coverage(ref, 4)["mean_depth"] > 1.5


@pytest.mark.parametrize("case,kind", list(xd.CONTRACT_STEP))
def test_contract_cases_are_admissible(case, kind):
    level, prop, theta0, T, _ = xd.contract_case(case, kind, xd.CONTRACT_STEP[(case, kind)])
    _admit(level, prop, theta0, T)


# ---- the end-to-end conditions of tests/test_gpu_dense_mass.py, met by the host class ---------------------------------------------------
END_TO_END = dict(sd=np.logspace(-1.0, 1.0, 8), N=256, T=400, scaling=0.1, period=20, seed=4)


def end_to_end_sigma(cfg=END_TO_END):
    """Sigma = Q diag(sd^2) Q^T with Q seeded, exactly symmetric, and Q"""
    sd = cfg["sd"]
    Q = np.linalg.qr(np.random.default_rng(cfg["seed"]).standard_normal((sd.shape[0], sd.shape[0])))[0]
    S = (Q * sd[None, :] ** 2) @ Q.T
    return 0.5 * (S + S.T), Q


def whitened_eigenvalues(C, Sigma):
    """the eigenvalues of Sigma^-1/2 C Sigma^-1/2"""
    lam, V = np.linalg.eigh(Sigma)
    R = (V / np.sqrt(lam)[None, :]) @ V.T
    return np.linalg.eigvalsh(R @ C @ R)


def test_end_to_end_reference_meets_its_conditions():
    """what tests/test_gpu_dense_mass.py asserts of sample() on the device, asserted of tda.NUTS under the host protocol on the same
    posterior N(0, Sigma) in closed form, with fewer chains (which makes the bounds harder to meet, not easier): a lower mean tree
    depth over the last 100 steps with inv_mass = Sigma than with its diagonal, finite records, the pooled covariance of the
    last 200 steps with every eigenvalue of Sigma^-1/2 C Sigma^-1/2 in [0.5, 2], and mass_from_samples of the run likewise"""
    import tinyda_amd as tda
    from tinyda_amd.records import DeviceChain, Link

    cfg = dict(END_TO_END, N=4)
    Sigma, _ = end_to_end_sigma(cfg)
    d, N, T = Sigma.shape[0], cfg["N"], cfg["T"]
    P = np.linalg.inv(Sigma)
    post = types.SimpleNamespace(prior=st.multivariate_normal(np.zeros(d), np.eye(d)), model=None, likelihood=None,
                                 create_link=lambda th: Link(th, 0.0, None, -0.5 * float(th @ (P @ th))))
    starts = np.random.default_rng(5).standard_normal((N, d)) @ np.linalg.cholesky(Sigma).T
    depth, chains = {}, {}
    rng_state = np.random.get_state()
    try:
        for name, mass in (("dense", Sigma), ("diag", np.diag(Sigma).copy())):
            np.random.seed(21)
            rows, depths = np.empty((T + 1, N, d)), np.empty((T, N))
            for c in range(N):
                prop = tda.NUTS(scaling=cfg["scaling"], adaptive=True, period=cfg["period"], inv_mass=mass)
                prop.setup_proposal(parameters=starts[c], posterior=post)
                prop.compute_gradient = lambda link: -(P @ link.parameters)
                link = post.create_link(starts[c])
                rows[0, c] = starts[c]
                for s in range(T):
                    cand = post.create_link(prop.make_proposal(link))
                    if 0.5 < prop.get_acceptance(cand, link):
                        link = cand
                    prop.adapt(parameters=link.parameters, accepted=[True])
                    rows[s + 1, c], depths[s, c] = link.parameters, prop.last_tree["depth"]
            depth[name], chains[name] = depths[-100:].mean(), rows
    finally:
        np.random.set_state(rng_state)
    print("mean tree depth of the last 100 steps: %.2f under Sigma, %.2f under its diagonal" % (depth["dense"], depth["diag"]))
    assert depth["dense"] < depth["diag"]
    assert np.all(np.isfinite(chains["dense"])) and np.all(np.isfinite(chains["diag"]))
    ev = whitened_eigenvalues(np.cov(chains["dense"][-200:].reshape(-1, d), rowvar=False), Sigma)
    result = dict(sampler="MH", n_chains=N, **{"chain_%d" % i: DeviceChain(chains["dense"][:, i], np.zeros((T + 1, 3)), np.ones(T + 1), None) for i in range(N)})
    ev_mass = whitened_eigenvalues(tda.mass_from_samples(result, burnin=T + 1 - 200), Sigma)
    print("eigenvalues of Sigma^-1/2 C Sigma^-1/2: %.2f .. %.2f; of mass_from_samples: %.2f .. %.2f" % (ev.min(), ev.max(), ev_mass.min(), ev_mass.max()))
    assert 0.5 <= ev.min() and ev.max() <= 2.0 and 0.5 <= ev_mass.min() and ev_mass.max() <= 2.0
