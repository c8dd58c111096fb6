"""Generate g23_prior_coupled_grw.npz and g23_prior_coupled_am.npz by RUNNING THE REFERENCE (tinyDA) itself -- the golden vectors
of chains whose prior couples parameters (tinyDA's Posterior takes any object with logpdf / rvs as prior): the Cauchy-difference
prior of tests/extpriorwave.py at d = 5 under an adaptive GaussianRandomWalk, and the ordered box-uniform prior at d = 7 under
AdaptiveMetropolis, whose proposals leave the support by breaking the order; both over the non-linear model of
tests/extmodel.py, m = 23, isotropic noise, 4 chains x 200 iterations.  The reference is handed the NumPy twin as it is.  Only
data is stored: the prior's name and its p / q, the variates, the traces.

Run in the build container only (needs the reference, like gen_golden.py):

    python tests/golden/gen_golden_prior_coupled.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_golden import run_mh, save, tda  # noqa: E402
from tests import extpriorwave as xw  # noqa: E402
from tests.extmodel import np_forward  # noqa: E402

M, N_CHAINS, ITERS, SIGMA2 = 23, 4, 200, 0.01


class CountingPrior:
    """the twin, counting the evaluations that fall outside the support"""
    outside = 0

    def __init__(self, twin):
        self.twin = twin

    def logpdf(self, x):
        v = self.twin.logpdf(x)
        if v == -np.inf:
            CountingPrior.outside += 1
        return v

    def rvs(self, *a, **k):
        return self.twin.rvs(*a, **k)


def _model(theta):
    return np_forward(theta, M)[0]


def _setup(seed, name, twin):
    rng = np.random.default_rng(seed)
    truth, theta0 = xw.starts(twin, N_CHAINS, rng)
    data = _model(truth) + np.sqrt(SIGMA2) * rng.standard_normal(M)
    CountingPrior.outside = 0
    post = tda.Posterior(CountingPrior(twin), tda.GaussianLogLike(data, SIGMA2 * np.eye(M)), _model)
    return post, dict(prior=np.array(name), p=twin.p, q=twin.q, data=data, sigma2=np.array(SIGMA2), theta0=theta0)


def _check(res, need_outside):
    rate = res["accepted"][:, 1:].mean()
    assert 0.1 <= rate <= 0.9, rate
    assert CountingPrior.outside >= need_outside, "no proposal left the support"
    print("acceptance %.3f, %d proposals outside the support" % (rate, CountingPrior.outside))


def g23_prior_coupled_grw():
    d = 5
    post, meta = _setup(2301, "cauchy", xw.cauchy_difference(d))
    C, period = 2e-3 * np.eye(d), 40
    prop = tda.GaussianRandomWalk(C=C, scaling=1.0, adaptive=True, gamma=1.01, period=period)
    res, snaps = run_mh(post, prop, meta["theta0"], ITERS, N_CHAINS, seed=2310, snapshot={"period": period, "fn": lambda p: float(p.scaling)})
    _check(res, 0)
    save("g23_prior_coupled_grw", C=C, scaling0=np.array(1.0), adaptive=np.array(True), gamma=np.array(1.01), period=np.array(period),
         scaling_hist=np.array(snaps), n_outside=np.array(CountingPrior.outside), **meta, **res)


def g23_prior_coupled_am():
    d = 7
    post, meta = _setup(2302, "ordered", xw.ordered(d))
    C0, t0, period = 1.5e-3 * np.eye(d), 40, 40
    prop = tda.AdaptiveMetropolis(C0=C0, sd=None, epsilon=1e-6, t0=t0, period=period, adaptive=False, gamma=1.01)
    res, snaps = run_mh(post, prop, meta["theta0"], ITERS, N_CHAINS, seed=2320, snapshot={"period": period, "fn": lambda p: p.C.copy()})
    _check(res, 1)
    save("g23_prior_coupled_am", C0=C0, sd=np.array(prop.sd), epsilon=np.array(1e-6), t0=np.array(t0), period=np.array(period),
         C_hist=np.array(snaps), n_outside=np.array(CountingPrior.outside), **meta, **res)


if __name__ == "__main__":
    g23_prior_coupled_grw()
    g23_prior_coupled_am()
