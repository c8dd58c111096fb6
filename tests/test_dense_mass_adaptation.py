"""Warm-up adaptation of a dense mass of HMC / NUTS (include/tinyda_amd_dense_mass_adaptation.h), without a GPU: the twin of the
three kernels (tests/extdensemass.py) against a two-pass covariance in np.longdouble, the refusal rule, a constant parameter, the
constructors and the lowering pass, the header and its symbol table, the offline build of csrc/tda_kernels_dense_mass.h, the host
classes on their own windows, and the reference of the end-to-end GPU test.  The C entry points need an engine, which needs a
device: tests/test_gpu_dense_mass_adaptation.py has them."""
import os
import re

import numpy as np
import pytest
import scipy.stats as st

from . import extdensemass as xdm
from . import extmass as xms
from . import extmodel as xm
from .extprogram import ROOT, compile_program, needs_hipcc


# ---- 1. the twin against two passes in extended precision --------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 70, 300])
@pytest.mark.parametrize("n", [20, 120])
def test_twin_matches_two_pass_covariance(N, n):
    """d = 7, standard deviations over six decades, correlated neighbours, the shift at the origin so that |delta| reaches 10: the
    twin's L L^T against the two-pass regularised covariance within the bound of the header's test plan, entry by entry; the
    same with the shift taken from the first state; the twin over the window cut at any points is bitwise the twin over the
    whole window"""
    d = 7
    X = xdm.inputs(n, N, d, seed=1000 * N + n)
    ref, mean, sd = xdm.reference(X)
    assert np.abs(mean / sd).max() > 9.9 and np.abs(np.corrcoef(X.reshape(-1, d), rowvar=False)[0, 1]) > 0.3
    for a in (np.zeros(d), None):
        L, refused, a_used = xdm.window_factor(X, np.eye(d), a)
        tol = xdm.tolerance(n, N, d, mean, sd, a_used, ref)
        err = np.abs(xdm.gram(L) - ref).astype(np.float64) / tol
        rel = tol / np.sqrt(np.outer(np.diag(ref), np.diag(ref))).astype(np.float64)
        print("N = %d, n = %d, shift %s: error %.4f of the bound; the bound is %.1e .. %.1e of sqrt(W_ii W_jj)"
              % (N, n, "0" if a is not None else "of the first state", err.max(), rel.min(), rel.max()))
        assert refused == 0 and np.all(err <= 1.0), err
        assert np.array_equal(L, np.tril(L)) and np.all(np.diag(L) > 0.0)
        cut, r2, _ = xdm.window_factor(X, np.eye(d), a, cuts=(3, 4, n - 5))
        assert r2 == 0 and np.array_equal(cut, L)
    assert np.array_equal(xdm.shift(X[0]), np.array([xms._pooled_sum(X[0][:, j]) / N for j in range(d)]))


# ---- 2. the refusal rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 70, 300])
def test_refusal_keeps_the_whole_factor(N):
    """one NaN state, or an indefinite W, refuses the whole factor: the count goes up by one and the factor is the one before,
    on the twin and on the package's own pooling (what the host classes call)"""
    from tinyda_amd.proposals import _dense_mass_pool

    rng = np.random.default_rng(N)
    n, d = 20, 4
    before = np.linalg.cholesky(np.diag([2.0, 3.0, 4.0, 5.0]) + 0.5)
    X = rng.standard_normal((n, N, d))
    good, refused, a = xdm.window_factor(X, before)
    assert refused == 0 and not np.array_equal(good, before)
    S1, S2 = xdm.accumulate(*xdm.zeros(N, d), a, X)
    own, own_refused = _dense_mass_pool(S1, S2, n, N, before)
    assert own_refused == 0 and np.allclose(own @ own.T, good @ good.T, rtol=1e-12, atol=0.0)
    # a NaN in one state of one chain
    bad = X.copy()
    bad[7, N // 2, 1] = np.nan
    got, refused, _ = xdm.window_factor(bad, before, a)
    assert refused == 1 and np.array_equal(got, before)
    S1, S2 = xdm.accumulate(*xdm.zeros(N, d), a, bad)
    own, own_refused = _dense_mass_pool(S1, S2, n, N, before)
    assert own_refused == 1 and own is before
    # an indefinite W: sums that no states give (a negative second moment), and a shift so far from the states that the raw
    # moments cancel to rounding noise of either sign
    S1, S2 = xdm.zeros(N, d)
    S2[0] = -np.eye(d)
    for pool in (xdm.update, _dense_mass_pool):
        got, refused = pool(S1, S2, n, N, before)
        assert refused == 1 and np.array_equal(got, before)
    far, refused, _ = xdm.window_factor(rng.standard_normal((20, 13, 8)), np.eye(8), a=1e9 * np.ones(8))
    assert refused == 1 and np.array_equal(far, np.eye(8))


# ---- 3. a parameter that does not move ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 70, 300])
def test_constant_parameter(N):
    """a parameter at 0.375 in every state: y is exactly 0, so L_jj = sqrt(1e-3 * 5 / (T + 5)) exactly, its row and its column are
    exact zeros, and nothing is refused"""
    n, d = 20, 5
    X = np.random.default_rng(3 * N).standard_normal((n, N, d))
    X[:, :, 2] = 0.375
    L, refused, a = xdm.window_factor(X, np.eye(d))
    T = float(n * N)
    assert refused == 0 and a[2] == 0.375
    assert L[2, 2] == np.sqrt(1e-3 * 5.0 / (T + 5.0))
    assert np.all(L[2, :2] == 0.0) and np.all(L[3:, 2] == 0.0) and np.all(np.isfinite(L)) and np.all(np.diag(L) > 0.0)


# ---- 4. constructors, lowering, interface ---------------------------------------------------------------------------------------------
def test_constructors():
    import tinyda_amd as tda

    W = np.array([[2.0, 0.5], [0.5, 1.0]])
    for cls in (tda.HMC, tda.NUTS):
        with pytest.raises(ValueError, match="adapt_dense=True needs adapt_mass > 0"):
            cls(0.1, period=20, adapt_dense=True)
        with pytest.raises(ValueError, match="adapt_dense=True needs adapt_mass > 0"):
            cls(0.1, period=20, adapt_mass=0, adapt_dense=True)
        for bad in (30, 20, 50, -40):
            with pytest.raises(ValueError, match="multiple of the period .* at least two periods"):
                cls(0.1, period=20, adapt_mass=bad, adapt_dense=True)
        with pytest.raises(ValueError, match="adapt_mass = 160 with a dense inv_mass: the warm-up adaptation learns a diagonal mass"):
            cls(0.1, period=20, adapt_mass=160, inv_mass=W)  # (without the switch: refused as before)
        for start in (None, np.array([4.0, 0.25]), W):
            prop = cls(0.1, period=20, adapt_mass=160, adapt_dense=True, inv_mass=start)
            assert prop.adapt_dense and prop.adapt_mass == 160 and prop.mass_updates == 0 and prop.mass_refused == 0
        assert not cls(0.1).adapt_dense and not cls(0.1, period=20, adapt_mass=160).adapt_dense


def _device_posterior(d=5, m=23):
    import tinyda_amd as tda

    return tda.Posterior(st.multivariate_normal(0.1 * np.ones(d), np.diag(0.5 + 0.01 * np.arange(d))), tda.GaussianLogLike(np.zeros(m), 0.01 * np.eye(m)),
                         tda.DeviceModel(xm.source(), m))


@pytest.mark.parametrize("cls", ["HMC", "NUTS"])
def test_lowering(cls):
    """the plan carries adapt_dense only when it is on; the start goes where it went: a diagonal one as inv_mass, a dense one as
    dense_mass; every key is a keyword of Engine.set_proposal; it lowers where the dense mass lowers and distributed=True is
    refused by the adapt_mass rule"""
    import inspect

    import tinyda_amd as tda
    from tinyda_amd.engine import Engine
    from tinyda_amd.lowering import lower

    make = getattr(tda, cls)
    post, d = _device_posterior(), 5
    W = np.diag(np.linspace(1.0, 2.0, d)) + 0.1
    plain = lower([post], make(0.05, adaptive=True, period=20))[0][1]
    diag = lower([post], make(0.05, adaptive=True, period=20, adapt_mass=160))[0][1]
    fixed = lower([post], make(0.05, adaptive=True, period=20, inv_mass=W))[0][1]
    assert "adapt_dense" not in plain and "adapt_dense" not in diag and "adapt_dense" not in fixed
    assert set(diag) == set(plain) | {"adapt_mass"} and set(fixed) == set(plain) | {"dense_mass"}
    names = set(inspect.signature(Engine.set_proposal).parameters)
    for start in (None, np.linspace(1.0, 2.0, d), W):
        prop = make(0.05, adaptive=True, period=20, adapt_mass=160, adapt_dense=True, inv_mass=start)
        (_, low), why = lower([post], prop)
        assert why is None and low["adapt_dense"] is True and low["adapt_mass"] == 160 and set(low) <= names
        if start is not None and np.ndim(start) == 2:
            assert set(low) == set(plain) | {"adapt_mass", "adapt_dense", "dense_mass"} and low["inv_mass"] is None
            assert np.array_equal(low["dense_mass"], np.linalg.cholesky(W))
        else:
            assert set(low) == set(plain) | {"adapt_mass", "adapt_dense"}
            assert low["inv_mass"] is None if start is None else np.array_equal(low["inv_mass"], start)
        plan, why = lower([post], prop, distributed=True)
        assert plan is None and "adapt_mass = 160" in why and "distributed=True" in why
        with pytest.raises(ValueError, match="adapt_mass = 160 of %s under distributed=True" % cls):
            tda.sample(post, prop, 10, n_chains=4, seed=1, distributed=True)
        # refused where the fixed dense mass is refused, with the same reason
        lin = tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(np.zeros(3), np.eye(3)), tda.LinearModel(np.ones((3, d))))
        assert lower([lin], prop)[1] == lower([lin], make(0.05, adaptive=True, period=20, inv_mass=W))[1] is not None


def test_header_and_symbol_table():
    """the header's three functions are bound by load() through their own table, disjoint from the older ones; the older headers
    and tinyda_amd.h keep their symbol sets; the text states the refusals that the GPU tests exercise"""
    from tinyda_amd import _lib

    want = {"tda_engine_set_dense_mass_adaptation", "tda_engine_get_dense_mass_adaptation", "tda_dense_mass_window"}
    assert set(_lib.DENSE_MASS_ADAPT_SYMBOLS) == want
    for other in (_lib.SYMBOLS, _lib.MASS_SYMBOLS, _lib.DENSE_MASS_SYMBOLS, _lib.NUTS_SYMBOLS, _lib.HMC_SYMBOLS):
        assert not want & set(other)
    header = open(os.path.join(ROOT, "include", "tinyda_amd_dense_mass_adaptation.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(tda_[a-z_]+)\s*\(", text)) == want
    for word in ("Schedule.", "Shift (k_dense_mass_shift", "Accumulation (k_dense_mass_accumulate", "Update (k_dense_mass_update", "TDA_ERR_STATE", "TDA_ERR_INVALID",
                 "WHOLE factor keeps its value", "v_mfma_f64_16x16x4"):
        assert word in header, word
    for name in ("tinyda_amd.h", "tinyda_amd_mass.h", "tinyda_amd_dense_mass.h"):
        assert "dense_mass_adaptation" not in open(os.path.join(ROOT, "include", name)).read()
    csrc = os.path.join(ROOT, "tinyda_amd", "csrc")
    assert "k_dense_mass" not in open(os.path.join(csrc, "tda_kernels_mass.h")).read()
    assert 'list(DENSE_MASS_ADAPT_SYMBOLS.items())' in open(os.path.join(ROOT, "tinyda_amd", "_lib.py")).read()


# ---- 5. the three kernels, compiled offline --------------------------------------------------------------------------------------------
@needs_hipcc
def test_dense_mass_kernels_compile_without_scratch(tmp_path):
    """csrc/tda_kernels_dense_mass.h alone, for gfx950: exactly the three kernels, no scratch memory, no spilled registers"""
    rc, log, usage = compile_program(tmp_path, "dense_mass", "", [], program_text='#include "tda_kernels_dense_mass.h"\n')
    assert rc == 0, log[-3000:]
    names = {re.search(r"k_dense_mass_[a-z]+?(?=E|$)", fn).group(0): fn for fn in usage}  # (the symbols are mangled: namespace tda)
    assert set(names) == {"k_dense_mass_shift", "k_dense_mass_accumulate", "k_dense_mass_update"} and len(usage) == 3, (usage, log[-2000:])
    for k, use in usage.items():
        print(k, use)
        assert use["ScratchSize [bytes/lane]"] == 0 and use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0, (k, use)


# ---- 6. the host classes ------------------------------------------------------------------------------------------------------------------
def _correlated_posterior():
    import tinyda_amd as tda

    d = 4
    sd = np.logspace(-1.0, 1.0, d)
    R = np.linalg.qr(np.random.default_rng(4).standard_normal((d, d)))[0]
    pv = 1e4
    nv = 1.0 / (1.0 / sd ** 2 - 1.0 / pv)  # F = R^T theta under the prior N(0, pv I): the posterior is N(., R diag(sd^2) R^T)
    y = np.array([0.02, -0.1, 1.0, -5.0])
    return tda.Posterior(st.multivariate_normal(np.zeros(d), pv * np.eye(d)), tda.GaussianLogLike(y, np.diag(nv)), tda.LinearModel(R.T.copy())), sd, R


@pytest.mark.parametrize("kind", ["HMC", "NUTS"])
@pytest.mark.parametrize("adaptive", [True, False])
def test_host_class_adapts_from_its_own_windows(kind, adaptive):
    """over a LinearModel posterior the host protocol runs: nothing differs from adapt_mass = 0 before the end of the first
    window; after each window the factor is the twin's with N = 1 over that chain's own states about the state at the window's
    start (L L^T within the bound: the host class factors with np.linalg.cholesky), inv_mass = L L^T; k restarts at each update"""
    import tinyda_amd as tda
    from tinyda_amd.hostloop import Chain

    post, sd, R = _correlated_posterior()
    d, period, W, T = 4, 10, 80, 100
    make = {"HMC": lambda am: tda.HMC(0.05, n_leapfrog=4, adaptive=adaptive, period=period, adapt_mass=am, adapt_dense=bool(am)),
            "NUTS": lambda am: tda.NUTS(0.05, max_depth=4, adaptive=adaptive, period=period, adapt_mass=am, adapt_dense=bool(am))}[kind]
    theta0 = R @ (0.5 * sd)

    def run(am, steps):
        np.random.seed(11)
        res = tda.sample(post, make(am), steps, n_chains=1, initial_parameters=[theta0], backend="host")
        return np.stack([lk.parameters for lk in res["chain_0"]])

    wins = xms.windows(W, period)
    assert wins == [(10, 20), (20, 40), (40, 80)]
    plain, adapted = run(0, T), run(W, T)
    first_end = wins[0][1]
    assert np.array_equal(plain[:first_end + 1], adapted[:first_end + 1]) and not np.array_equal(plain, adapted)

    np.random.seed(11)
    prop = make(W)
    chain = Chain(post, prop, theta0)
    ends = {end: first for first, end in wins}
    L, k_seen = np.eye(d), []
    for s in range(T):
        k_before = prop.k
        chain.sample(1, progressbar=False)
        states = np.stack([lk.parameters for lk in chain.chain])  # states[s + 1] is the state after step s
        assert np.array_equal(states, adapted[:s + 2])
        if s + 1 in ends:
            first = ends[s + 1]
            X = states[first + 1:s + 2][:, None, :]
            want = xdm.assert_window(X, prop.chol_inv_mass, L, states[first], "%s host, window [%d, %d):" % (kind, first, s + 1))
            assert not np.array_equal(prop.chol_inv_mass, L) and want.shape == (d, d)
            assert prop.inv_mass.shape == (d, d) and np.array_equal(prop.inv_mass, prop.chol_inv_mass @ prop.chol_inv_mass.T)
            assert prop.k == 0 and (k_before > 0) == adaptive
            L = prop.chol_inv_mass
            k_seen.append(k_before)
        else:
            assert np.array_equal(prop.chol_inv_mass, L)
            boundary = adaptive and (s + 1) % period == 0
            assert prop.k == k_before + (1 if boundary else 0)
    assert prop.mass_updates == 3 and prop.mass_refused == 0
    assert k_seen == ([1, 1, 3] if adaptive else [0, 0, 0])
    Sigma = (R * sd ** 2) @ R.T
    print(kind, "eigenvalues of the learnt W whitened by the covariance:", np.linalg.eigvalsh(np.linalg.solve(np.linalg.cholesky(Sigma), np.linalg.solve(np.linalg.cholesky(Sigma), prop.inv_mass).T)))


def test_host_class_refuses_the_whole_factor():
    """a window in which the chain did not move gives the regulariser alone, which is accepted; a window with a NaN state keeps
    the factor and counts one refusal"""
    import types

    import tinyda_amd as tda

    prop = tda.HMC(0.1, period=2, adapt_mass=4, adapt_dense=True, inv_mass=np.array([4.0, 0.25]))
    post = types.SimpleNamespace(prior=st.multivariate_normal(np.zeros(2), np.eye(2)), model=None, likelihood=None)
    prop.setup_proposal(parameters=np.zeros(2), posterior=post)
    assert np.array_equal(prop.chol_inv_mass, np.diag([2.0, 0.5])) and np.array_equal(prop.inv_mass, np.diag([4.0, 0.25]))
    start = prop.chol_inv_mass
    for s, x in enumerate(([0.0, 0.0], [1.0, 2.0], [np.nan, 1.0], [2.0, 1.0])):
        prop.t = s + 1
        prop._adapt_mass(np.array(x))
    assert prop.mass_updates == 1 and prop.mass_refused == 1 and prop.chol_inv_mass is start


# ---- 7. the reference of the end-to-end GPU test --------------------------------------------------------------------------------------------
END_TO_END = dict(sd=np.logspace(-1.5, 1.5, 8), rotation_seed=8, N=256, T=400, scaling=0.05, period=20, adapt_mass=160)


def whitened_eigenvalues(W, Sigma):
    """the eigenvalues of Sigma^-1/2 W Sigma^-1/2 (through the factor of Sigma)"""
    Ls = np.linalg.cholesky(Sigma)
    M = np.linalg.solve(Ls, np.linalg.solve(Ls, W).T)
    return np.linalg.eigvalsh(0.5 * (M + M.T))


def test_end_to_end_reference_meets_its_conditions():
    """what tests/test_gpu_dense_mass_adaptation.py asserts of sample() on the device, asserted of the NumPy reference alone with
    48 chains (fewer pooled states: harder, not easier): the eigenvalues of the learnt W whitened by the true covariance in
    [0.5, 2], three updates, none refused, and a lower mean tree depth over the last 100 steps than the diagonal adaptation"""
    cfg = END_TO_END
    R, Sigma = xdm.rotated_problem(cfg["sd"], cfg["rotation_seed"])
    kw = dict(sd=cfg["sd"], R=R, N=48, T=cfg["T"], scaling=cfg["scaling"], period=cfg["period"], adapt_mass=cfg["adapt_mass"], seed=5)
    on = xdm.pooled_nuts_reference(adapt_dense=True, **kw)
    off = xdm.pooled_nuts_reference(adapt_dense=False, **kw)
    ev = whitened_eigenvalues(on["chol"] @ on["chol"].T, Sigma)
    d_on, d_off = on["depth"][-100:].mean(), off["depth"][-100:].mean()
    print("whitened eigenvalues %.2f .. %.2f; mean tree depth of the last 100 steps %.2f dense, %.2f diagonal" % (ev.min(), ev.max(), d_on, d_off))
    assert 0.5 <= ev.min() and ev.max() <= 2.0
    assert on["updates"] == 3 and on["refused"] == 0 and off["updates"] == 3
    assert d_on < d_off
