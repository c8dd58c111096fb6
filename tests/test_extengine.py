"""The shared harness of the engine-against-oracle tests (tests/extengine.py) against inputs that must fail: a reference
trace made with the oracle alone stands in for the engine's outputs, exact and with one entry off by a little more, or a
little less, than each bar; the checkpoint checks run against a fake engine whose outputs are a counter."""
import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extengine as xe

D, M, N, T = 5, 7, 4, 40


@pytest.fixture(scope="module")
def trace():
    """run_mh's trace of a small linear Gaussian problem under an adaptive random walk, read-only"""
    rng = np.random.default_rng(0)
    A = rng.standard_normal((M, D)) / np.sqrt(M)
    truth = 0.3 * rng.standard_normal(D)
    y = A @ truth + 0.05 * rng.standard_normal(M)
    theta0 = truth + 0.05 * rng.standard_normal((N, D))
    z, u = rng.standard_normal((T, N, D)), rng.random((T, N))  # (in the layout in which the engine exports them)
    level = orc.LinearGaussianLevel(A, y, "iso", 0.05 ** 2, orc.MVNPrior(np.zeros(D), np.eye(D)))
    prop = dict(kind="grw", C=1e-3 * np.eye(D), scaling=1.0, adaptive=True, gamma=1.01, period=20)
    ref = orc.run_mh(level, prop, theta0, np.swapaxes(z, 0, 1), np.swapaxes(u, 0, 1))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def engine_outputs(ref):
    """params[T, N, d], stats[T, N, 3] (log-prior, log-likelihood, log-posterior), acc[T, N], scal[N]: fresh copies"""
    stats = np.stack([np.swapaxes(ref[k][:, 1:], 0, 1) for k in ("logprior", "loglike", "logpost")], axis=-1)
    return np.swapaxes(ref["theta"][:, 1:], 0, 1).copy(), stats, np.swapaxes(ref["accepted"][:, 1:], 0, 1).copy(), ref["scaling"].copy()


def fails(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def test_the_trace_is_a_fair_one(trace):
    assert trace["accepted"][:, 1:].mean() == 0.575
    xe.assert_rate(trace["accepted"][:, 1:])
    fails(xe.assert_rate, np.zeros((4, 25)) + (np.arange(25) < 2))  # 0.08
    fails(xe.assert_rate, np.zeros((4, 25)) + (np.arange(25) < 23))  # 0.92


@pytest.mark.parametrize("span_form", [False, True])
def test_compare_holds_masks_densities_and_scaling(trace, span_form):
    params, stats, acc, scal = engine_outputs(trace)
    xe.compare(params, stats, acc, trace, span_form=span_form)
    xe.compare(params, stats, acc, trace, scal, span_form=span_form)
    flipped = acc.copy()
    flipped[17, 2] ^= 1
    fails(xe.compare, params, stats, flipped, trace, span_form=span_form)
    for factor, passes in ((1 + 3e-10, False), (1 + 3e-11, True)):
        off = stats.copy()
        off[23, 1, 2] *= factor
        if passes:
            xe.compare(params, off, acc, trace, span_form=span_form)
        else:
            fails(xe.compare, params, off, acc, trace, span_form=span_form)
    fails(xe.compare, params, stats, acc, trace, scal * (1 + 1e-11), span_form=span_form)


def test_compare_holds_states_in_both_forms(trace):
    params, stats, acc, _ = engine_outputs(trace)
    big, small = (np.unravel_index(f(np.abs(params)), params.shape) for f in (np.argmax, np.argmin))
    off = params.copy()
    off[big] *= 1 + 3e-9
    fails(xe.compare, off, stats, acc, trace)
    fails(xe.compare, off, stats, acc, trace, span_form=True)
    # an entry close to zero of a component that is not: atol = 1e-12 of the plain form against 1e-9 of the component's span
    assert abs(params[small]) < 1e-3 < 1e-2 < np.max(np.abs(trace["theta"][:, :, small[2]]))
    off = params.copy()
    off[small] += 5e-12
    fails(xe.compare, off, stats, acc, trace)
    xe.compare(off, stats, acc, trace, span_form=True)


class MagnitudePrior:
    """the trace's log-prior with the magnitude() that assert_logprior measures against: here |log-prior| itself"""

    def __init__(self, prior):
        self.prior = prior

    def magnitude(self, theta):
        return np.abs(self.prior.logpdf(theta))


def test_compare_holds_the_log_prior(trace):
    params, stats, acc, _ = engine_outputs(trace)
    prior = MagnitudePrior(orc.MVNPrior(np.zeros(D), np.eye(D)))
    xe.compare(params, stats, acc, trace, prior=prior)
    off = stats.copy()
    off[5, 3, 0] *= 1 + 3e-10
    fails(xe.compare, params, off, acc, trace, prior=prior)
    xe.compare(params, off, acc, trace)


def level_outputs(trace):
    """two levels from the one trace: the coarse level's outputs carry every row, the finest's drop the initial link"""
    return [(np.swapaxes(trace["theta"][:, sk], 0, 1).copy(), np.stack([trace[k][:, sk].T for k in ("logprior", "loglike", "logpost")], axis=-1),
             trace["accepted"][:, sk].T.copy()) for sk in (slice(None), slice(1, None))]


@pytest.mark.parametrize("level", [0, 1])
def test_compare_levels(trace, level):
    res = [trace, trace]
    priors = [MagnitudePrior(orc.MVNPrior(np.zeros(D), np.eye(D)))] * 2
    outs = level_outputs(trace)
    xe.compare_levels(outs, res)
    xe.compare_levels(outs, res, states=False, logprior_of=priors)
    outs[level][2][11, 1] ^= 1
    fails(xe.compare_levels, outs, res, states=False)
    outs = level_outputs(trace)
    outs[level][1][11, 1, 2] *= 1 + 3e-10
    fails(xe.compare_levels, outs, res, states=False)
    outs = level_outputs(trace)
    outs[level][0][11, 1, 0] *= 1 + 3e-9
    fails(xe.compare_levels, outs, res)
    xe.compare_levels(outs, res, states=False)
    outs = level_outputs(trace)
    outs[level][1][11, 1, 0] *= 1 + 3e-10
    xe.compare_levels(outs, res)
    fails(xe.compare_levels, outs, res, logprior_of=priors)


def test_compare_replay(trace):
    params, stats, acc, scal = engine_outputs(trace)
    g = {k: trace[k] for k in ("theta", "logprior", "loglike", "logpost", "accepted", "scaling_hist", "C_hist")}
    C = trace["C"].copy()
    every = dict(C=C, scaling=scal, logprior=True, loglike=True)
    xe.compare_replay(params, stats, acc, g)
    xe.compare_replay(params, stats, acc, g, **every)
    flipped = acc.copy()
    flipped[0, 0] ^= 1
    fails(xe.compare_replay, params, stats, flipped, g)
    for col, kw in ((2, {}), (0, dict(logprior=True)), (1, dict(loglike=True))):
        off = stats.copy()
        off[39, 3, col] *= 1 + 3e-10
        fails(xe.compare_replay, params, off, acc, g, **kw)
        if kw:
            xe.compare_replay(params, off, acc, g)
    off = params.copy()
    off[np.unravel_index(np.argmax(np.abs(params)), params.shape)] *= 1 + 3e-10
    xe.compare_replay(off, stats, acc, g)
    fails(xe.compare_replay, off, stats, acc, g, params_rtol=1e-10)
    fails(xe.compare_replay, params, stats, acc, g, scaling=scal * (1 + 1e-11))
    fails(xe.compare_replay, params, stats, acc, g, C=C * (1 + 3e-9))


class CounterEngine:
    """run_host / run_levels_host hand out consecutive integers; get_state / set_state save and restore the counter"""

    def __init__(self, set_state_works=True, get_state_advances=False):
        self.n, self.set_state_works, self.get_state_advances = 0, set_state_works, get_state_advances

    def run_host(self, steps):
        self.n += steps
        return tuple(np.arange(self.n - steps, self.n) * k for k in (1.0, 2.0, 3.0))

    def run_levels_host(self, steps):
        return [self.run_host(steps), self.run_host(2 * steps)]

    def get_state(self):
        self.n += self.get_state_advances
        return self.n - self.get_state_advances

    def set_state(self, blob):
        if self.set_state_works:
            self.n = blob

    def close(self):
        pass


def test_resume_checks_against_a_counter():
    xe.assert_resume_bitwise(CounterEngine)
    out = xe.assert_levels_resume_bitwise(CounterEngine())
    assert len(out) == 2 and out[0][0][0] == 21 and len(out[1][0]) == 18
    with pytest.raises(AssertionError, match="resumed engine"):
        xe.assert_resume_bitwise(lambda: CounterEngine(set_state_works=False))
    fails(xe.assert_levels_resume_bitwise, CounterEngine(set_state_works=False))
    # a get_state that disturbs its own engine: the resumed engine is right, only the continuation shows it
    with pytest.raises(AssertionError, match="produced the blob"):
        xe.assert_resume_bitwise(lambda: CounterEngine(get_state_advances=True))
