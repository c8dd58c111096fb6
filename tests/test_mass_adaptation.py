"""Warm-up adaptation of the diagonal mass of HMC / NUTS (include/tinyda_amd_mass.h), without a GPU: the schedule, the twin of the
two kernels (tests/extmass.py) against a two-pass variance in np.longdouble, the host classes on their own windows, the lowering
pass, the offline build of csrc/tda_kernels_mass.h, and the reference of the end-to-end GPU test.  The refusals of the C entry
points need an engine, which needs a device: tests/test_gpu_mass_adaptation.py has them."""
import os
import re
import warnings

import numpy as np
import pytest
import scipy.stats as st

from . import exthmc as xh
from . import extmass as xms
from . import extmodel as xm
from .extprogram import ROOT, compile_program, needs_hipcc


# ---- 1. the schedule ---------------------------------------------------------------------------------------------------------------
def test_mass_windows_examples_and_shape():
    from tinyda_amd.proposals import mass_windows

    per = 20
    assert mass_windows(2 * per, per) == [(20, 40)]
    assert mass_windows(8 * per, per) == [(20, 40), (40, 80), (80, 160)]
    assert mass_windows(10 * per, per) == [(20, 40), (40, 80), (80, 200)]
    for P in range(2, 41):
        for period in (1, 7):
            win = mass_windows(P * period, period)
            assert win == xms.windows(P * period, period)
            assert all(a % period == 0 and b % period == 0 for a, b in win)
            w = [(a // period, b // period) for a, b in win]
            assert w[0][0] == 1 and w[-1][1] == P
            assert all(w[i][1] == w[i + 1][0] for i in range(len(w) - 1))  # contiguous
            lengths = [b - a for a, b in w]
            assert lengths[:-1] == [1 << i for i in range(len(lengths) - 1)]  # 1, 2, 4, .. before the last
            assert len(lengths) == 1 or lengths[-1] >= lengths[-2]
            # the last window is the first after which the next one (twice as long) would not fit whole
            s, L = w[-1][0], 1 << (len(w) - 1)
            assert s + 3 * L > P and all(a + 3 * (b - a) <= P for a, b in w[:-1])


def test_constructor_refusals():
    import tinyda_amd as tda
    from tinyda_amd.proposals import mass_windows

    for cls in (tda.HMC, tda.NUTS):
        for bad in (30, 20, 50, -40, 40.5):  # not a multiple of the period, shorter than two periods, negative, not an integer
            with pytest.raises(ValueError, match="multiple of the period .* at least two periods"):
                cls(0.1, period=20, adapt_mass=bad)
        prop = cls(0.1, period=20, adapt_mass=160)
        assert prop.adapt_mass == 160 and prop._lowering()["adapt_mass"] == 160 and prop.mass_updates == 0 and prop.mass_refused == 0
        assert cls(0.1).adapt_mass == 0 and "adapt_mass" not in cls(0.1)._lowering()  # (off: the plan is what it was)
    for bad in ((30, 20), (20, 20), (0, 20), (40, 0)):
        with pytest.raises(ValueError):
            mass_windows(*bad)


def test_header_and_symbol_table():
    """the header's two functions are bound by load() through their own table; tinyda_amd.h keeps its symbol set; the text states
    the refusals that tests/test_gpu_mass_adaptation.py exercises"""
    from tinyda_amd import _lib

    assert set(_lib.MASS_SYMBOLS) == {"tda_engine_set_mass_adaptation", "tda_engine_get_mass"} and not set(_lib.MASS_SYMBOLS) & set(_lib.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "tinyda_amd_mass.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert set(re.findall(r"\b(tda_[a-z_]+)\s*\(", text)) == set(_lib.MASS_SYMBOLS)
    assert "TDA_ERR_STATE for any other proposal kind" in header and "TDA_ERR_INVALID for a warmup_steps" in header
    assert "tda_engine_set_mass_adaptation" not in open(os.path.join(ROOT, "include", "tinyda_amd.h")).read()


# ---- 2. the twin against two passes in extended precision --------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 70, 300])
@pytest.mark.parametrize("n", [20, 120])
def test_twin_matches_two_pass_variance(N, n):
    """|mean| / sd up to 10 and standard deviations over six decades: the twin's regularised variance against the two-pass value,
    within 8 (n + N / 256 + 16) 2^-53 (1 + (mean / sd)^2) of it; the twin over the window cut into blocks of any length is
    bitwise the twin over the whole window"""
    rng = np.random.default_rng(1000 * N + n)
    d = 7
    sd = np.logspace(-3.0, 3.0, d)
    ratio = np.array([0.0, 0.3, -1.0, 3.0, -10.0, 10.0, 7.0])
    Z = rng.standard_normal((n, N, d))
    Z = (Z - Z.mean(axis=(0, 1))) / Z.std(axis=(0, 1), ddof=1)  # (the sample's own mean / sd is the ratio chosen, at any n N)
    X = (ratio * sd)[None, None, :] + sd[None, None, :] * Z
    got, refused = xms.window_mass(X, np.ones(d))
    ref, mean, s = xms.reference(X)
    assert refused == 0 and np.all(np.abs(mean / s) <= 10.0 + 1e-9) and np.abs(mean / s).max() > 9.9
    tol = xms.tolerance(n, N, mean.astype(np.float64), s.astype(np.float64))
    err = np.abs((got.astype(np.longdouble) - ref) / ref).astype(np.float64)
    print("N = %d, n = %d: error / tolerance %s" % (N, n, np.array2string(err / tol, precision=3)))
    assert np.all(err <= tol), (err, tol)
    assert np.all(tol < 1e-10)
    mean_b, M2_b, k = np.zeros((N, d)), np.zeros((N, d)), 0
    for lo, hi in ((0, 3), (3, 4), (4, n - 5), (n - 5, n)):
        mean_b, M2_b, k = xms.accumulate(mean_b, M2_b, k, X[lo:hi])
    assert k == n and np.array_equal(xms.pool(mean_b, M2_b, k, np.ones(d))[0], got)


@pytest.mark.parametrize("N", [1, 70, 300])
def test_twin_refusal_rule(N):
    """a parameter that is NaN in one chain keeps its entry and counts once; a constant parameter gets the regulariser's floor,
    finite and positive, and is not refused"""
    from tinyda_amd.proposals import _mass_pool

    rng = np.random.default_rng(N)
    n, d = 20, 4
    X = rng.standard_normal((n, N, d))
    X[7, N // 2, 1] = np.nan
    X[:, :, 2] = 0.375
    before = np.array([2.0, 3.0, 4.0, 5.0])
    got, refused = xms.window_mass(X, before)
    T = float(n * N)
    assert refused == 1 and got[1] == 3.0
    assert got[2] == 1e-3 * 5.0 / (T + 5.0) and np.isfinite(got[2]) and got[2] > 0.0
    assert np.all(np.isfinite(got)) and got[0] != 2.0 and got[3] != 5.0
    # the package's own pooling (what the host classes call): the same numbers from the same moments
    mean, M2, k = xms.accumulate(np.zeros((N, d)), np.zeros((N, d)), 0, X)
    own, own_refused = _mass_pool(mean, M2, k, before)
    assert own_refused == 1 and np.array_equal(own, got)


# ---- 3. the host classes ------------------------------------------------------------------------------------------------------------
def _linear_posterior():
    import tinyda_amd as tda

    d = 4
    sd = np.logspace(-1.5, 1.5, d)  # standard deviations spanning 10^3
    A = np.eye(d)
    pv = 1e4
    nv = 1.0 / (1.0 / sd ** 2 - 1.0 / pv)  # prior N(0, pv I): the posterior is N(., diag(sd^2))
    y = np.array([0.02, -0.1, 1.0, -5.0])
    return tda.Posterior(st.multivariate_normal(np.zeros(d), pv * np.eye(d)), tda.GaussianLogLike(y, np.diag(nv)), tda.LinearModel(A)), sd


@pytest.mark.parametrize("kind", ["HMC", "NUTS"])
@pytest.mark.parametrize("adaptive", [True, False])
def test_host_class_adapts_from_its_own_windows(kind, adaptive):
    """over a LinearModel posterior the host protocol runs: nothing differs from adapt_mass = 0 before the end of the first
    window; the mass after each window is the twin's with N = 1 over that chain's own states; k restarts at each update"""
    import tinyda_amd as tda

    post, sd = _linear_posterior()
    period, W, T = 10, 80, 100
    make = {"HMC": lambda am: tda.HMC(0.02, n_leapfrog=4, adaptive=adaptive, period=period, adapt_mass=am),
            "NUTS": lambda am: tda.NUTS(0.02, max_depth=4, adaptive=adaptive, period=period, adapt_mass=am)}[kind]
    theta0 = 0.5 * sd

    def run(am, steps):
        np.random.seed(11)
        prop = make(am)
        res = tda.sample(post, prop, steps, n_chains=1, initial_parameters=[theta0], backend="host")
        return np.stack([lk.parameters for lk in res["chain_0"]])

    wins = xms.windows(W, period)
    assert wins == [(10, 20), (20, 40), (40, 80)]
    plain, adapted = run(0, T), run(W, T)
    first_end = wins[0][1]
    assert np.array_equal(plain[:first_end + 1], adapted[:first_end + 1]) and not np.array_equal(plain, adapted)

    # the same run step by step, looking at the proposal after every adapt()
    from tinyda_amd.hostloop import Chain

    np.random.seed(11)
    prop = make(W)
    chain = Chain(post, prop, theta0)
    ends = {end: first for first, end in wins}
    w, k_seen = np.ones(4), []
    for s in range(T):
        k_before = prop.k
        chain.sample(1, progressbar=False)
        states = np.stack([lk.parameters for lk in chain.chain])
        assert np.array_equal(states, adapted[:s + 2])
        if s + 1 in ends:
            X = states[1:][ends[s + 1]:s + 1][:, None, :]  # state s is the one after step s
            want, refused = xms.window_mass(X, w)
            assert refused == 0 and np.array_equal(prop.inv_mass, want), (s, prop.inv_mass, want)
            assert prop.k == 0 and (k_before > 0) == adaptive
            w = want
            k_seen.append(k_before)
        else:
            assert np.array_equal(prop.inv_mass, w)
            boundary = adaptive and (s + 1) % period == 0
            assert prop.k == k_before + (1 if boundary else 0)
    assert prop.mass_updates == 3 and prop.mass_refused == 0
    assert k_seen == ([1, 1, 3] if adaptive else [0, 0, 0])  # (the period boundaries since the update before)
    print(kind, "inverse mass / variance after warm-up:", prop.inv_mass / sd ** 2)


# ---- 4. lowering ---------------------------------------------------------------------------------------------------------------------
def _device_posterior(d=5, m=23):
    import tinyda_amd as tda

    return tda.Posterior(st.multivariate_normal(0.1 * np.ones(d), np.diag(0.5 + 0.01 * np.arange(d))), tda.GaussianLogLike(np.zeros(m), 0.01 * np.eye(m)),
                         tda.DeviceModel(xm.source(), m))


def test_lowering_carries_adapt_mass_and_refuses_distributed():
    import tinyda_amd as tda
    from tinyda_amd.lowering import lower

    post = _device_posterior()
    for prop in (tda.HMC(0.05, adaptive=True, period=20, adapt_mass=160), tda.NUTS(0.05, adaptive=True, period=20, adapt_mass=160)):
        plan, why = lower([post], prop)
        assert plan is not None and plan[1]["adapt_mass"] == 160 and plan[1]["period"] == 20, why
        plan, why = lower([post], prop, distributed=True)
        assert plan is None and "adapt_mass = 160" in why and "distributed=True" in why and type(prop).__name__ in why
        with pytest.raises(ValueError, match="adapt_mass = 160 of %s under distributed=True" % type(prop).__name__):
            tda.sample(post, prop, 10, n_chains=4, seed=1, distributed=True)
    for prop in (tda.HMC(0.05), tda.NUTS(0.05)):  # off: the plan says so, and distributed runs lower as before
        assert "adapt_mass" not in lower([post], prop)[0][1] and lower([post], prop, distributed=True)[0] is not None


def test_engine_set_proposal_takes_the_plan():
    """every key of the lowered proposal is a keyword of Engine.set_proposal (sample() passes the plan's dict as it is)"""
    import inspect

    import tinyda_amd as tda
    from tinyda_amd.engine import Engine

    names = set(inspect.signature(Engine.set_proposal).parameters)
    for prop in (tda.HMC(0.05, period=20, adapt_mass=40), tda.NUTS(0.05, period=20, adapt_mass=40)):
        assert set(prop._lowering()) <= names


def test_backend_hip_fails_loudly_without_a_device():
    """backend='hip' over a posterior that lowers: on a box without a GPU the engine refuses to exist; nothing falls back"""
    import torch

    import tinyda_amd as tda

    if not torch.cuda.is_available():  # (with a GPU this very call runs: tests/test_gpu_mass_adaptation.py)
        with pytest.raises(tda.EngineError):
            tda.sample(_device_posterior(), tda.NUTS(0.05, adaptive=True, period=20, adapt_mass=40), 60, n_chains=4, seed=1, backend="hip")
    # over a model that does not lower, 'hip' raises with the rule's reason and 'auto' warns and adapts per chain on the host
    post, _ = _linear_posterior()
    with pytest.raises(tda.EngineError, match="NUTS: single level, a DeviceModel with tda_gradient"):
        tda.sample(post, tda.NUTS(0.05, period=20, adapt_mass=40), 10, n_chains=2, backend="hip")
    from tinyda_amd.api import HostFallbackWarning

    np.random.seed(2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = tda.sample(post, tda.NUTS(0.02, max_depth=3, adaptive=True, period=10, adapt_mass=20), 25, n_chains=2, backend="auto")
    assert len([x for x in w if issubclass(x.category, HostFallbackWarning)]) == 1 and res["backend"] == "host"


# ---- 5. the two kernels, compiled offline ------------------------------------------------------------------------------------------
@needs_hipcc
def test_mass_kernels_compile_without_scratch(tmp_path):
    """csrc/tda_kernels_mass.h alone, for gfx950: exactly the two kernels, no scratch memory, no spilled vector registers"""
    rc, log, usage = compile_program(tmp_path, "mass", "", [], program_text='#include "tda_kernels_mass.h"\n')
    assert rc == 0, log[-3000:]
    names = {re.search(r"k_mass_[a-z]+?(?=E|$)", fn).group(0): fn for fn in usage}  # (the symbols are mangled: namespace tda)
    assert set(names) == {"k_mass_accumulate", "k_mass_update"} and len(usage) == 2, (usage, log[-2000:])
    for k, use in usage.items():
        print(k, use)
        assert use["ScratchSize [bytes/lane]"] == 0 and use["VGPRs Spill"] == 0 and use["SGPRs Spill"] == 0, (k, use)


# ---- 6. the reference of the end-to-end GPU test -------------------------------------------------------------------------------------
END_TO_END = dict(sd=np.logspace(-1.5, 1.5, 8), N=256, T=400, scaling=0.05, period=20, adapt_mass=160)


def test_end_to_end_reference_meets_its_conditions():
    """what tests/test_gpu_mass_adaptation.py asserts of sample() on the device, asserted of the NumPy reference alone (the
    engine's problem with fewer chains, so that it stays quick: the pooled estimate then rests on fewer states, which makes the
    bounds harder to meet, not easier): inv_mass / true variance in [0.5, 2], three updates, and a lower mean tree depth over the
    last 100 steps than without the adaptation"""
    cfg = dict(END_TO_END, N=48)
    on = xms.pooled_nuts_reference(seed=5, **cfg)
    off = xms.pooled_nuts_reference(seed=5, **dict(cfg, adapt_mass=0))
    ratio = on["inv_mass"] / cfg["sd"] ** 2
    d_on, d_off = on["depth"][-100:].mean(), off["depth"][-100:].mean()
    print("inv_mass / variance %s; mean tree depth of the last 100 steps %.2f adapted, %.2f unit mass" % (np.array2string(ratio, precision=2), d_on, d_off))
    assert np.all(ratio >= 0.5) and np.all(ratio <= 2.0)
    assert on["updates"] == 3 and off["updates"] == 0 and np.all(off["inv_mass"] == 1.0)
    assert d_on < d_off
