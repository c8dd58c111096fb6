"""Generate g19_prior_families_grw.npz and g19_prior_families_am.npz by RUNNING THE REFERENCE (tinyDA) itself -- the golden
vectors of chains whose prior is a JointPrior of scipy.stats families beyond norm / uniform ("typically each a
scipy.stats.rv_continuous", distributions.py:8-56): d = 5 with [lognorm, gamma, beta, norm, uniform] under an adaptive
GaussianRandomWalk, and d = 13 with one component of each of the 13 families of tests/extprior.py under AdaptiveMetropolis;
both over the non-linear model of tests/extmodel.py, m = 23, isotropic noise, 4 chains x 300 iterations, started at low
quantiles of the components so that proposals leave the supports.  Only data is stored: the components as family names
and numbers, the variates, the traces.

Run in the build container only (needs the reference, like gen_golden.py):

    python tests/golden/gen_golden_prior_source.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_golden import run_mh, save, tda  # noqa: E402
from tests.extmodel import np_forward  # noqa: E402
from tests.extprior import FAMILY_NAMES, FAMILY_PARAMS, components, starts_near_lower_edges  # noqa: E402

M, N_CHAINS, ITERS, SIGMA2 = 23, 4, 300, 0.01


class CountingPrior:
    """the reference's JointPrior, counting the evaluations that fall outside a component's support"""
    outside = 0

    def __init__(self, comps):
        self.joint = tda.JointPrior(comps)

    def logpdf(self, x):
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.joint.logpdf(x)
        if v == -np.inf:
            CountingPrior.outside += 1
        return v

    def rvs(self, *a, **k):
        return self.joint.rvs(*a, **k)


def _model(theta):
    return np_forward(theta, M)[0]


def _setup(seed, names):
    rng = np.random.default_rng(seed)
    comps = components(len(names), names)
    truth, theta0 = starts_near_lower_edges(comps, N_CHAINS, rng)
    data = _model(truth) + np.sqrt(SIGMA2) * rng.standard_normal(M)
    CountingPrior.outside = 0
    post = tda.Posterior(CountingPrior(comps), tda.GaussianLogLike(data, SIGMA2 * np.eye(M)), _model)
    meta = dict(families=np.array(names), shapes=np.array([(FAMILY_PARAMS[n][0] + (0.0, 0.0))[:2] for n in names]),
                n_shapes=np.array([len(FAMILY_PARAMS[n][0]) for n in names]), loc=np.array([FAMILY_PARAMS[n][1] for n in names]),
                scale=np.array([FAMILY_PARAMS[n][2] for n in names]), data=data, sigma2=np.array(SIGMA2), theta0=theta0)
    return post, meta


def _check(res):
    rate = res["accepted"][:, 1:].mean()
    assert 0.1 <= rate <= 0.9, rate
    assert CountingPrior.outside >= 1, "no proposal left a support"
    print("acceptance %.3f, %d proposals outside a support" % (rate, CountingPrior.outside))


def g19_prior_families_grw():
    names = ("lognorm", "gamma", "beta", "norm", "uniform")
    post, meta = _setup(1901, names)
    C, period = 4e-3 * np.eye(len(names)), 50
    prop = tda.GaussianRandomWalk(C=C, scaling=1.0, adaptive=True, gamma=1.01, period=period)
    res, snaps = run_mh(post, prop, meta["theta0"], ITERS, N_CHAINS, seed=1910, snapshot={"period": period, "fn": lambda p: float(p.scaling)})
    _check(res)
    save("g19_prior_families_grw", C=C, scaling0=np.array(1.0), adaptive=np.array(True), gamma=np.array(1.01), period=np.array(period),
         scaling_hist=np.array(snaps), n_outside=np.array(CountingPrior.outside), **meta, **res)


def g19_prior_families_am():
    names = FAMILY_NAMES
    post, meta = _setup(1902, names)
    d = len(names)
    C0, t0, period = 5e-4 * np.eye(d), 50, 50
    prop = tda.AdaptiveMetropolis(C0=C0, sd=None, epsilon=1e-6, t0=t0, period=period, adaptive=False, gamma=1.01)
    res, snaps = run_mh(post, prop, meta["theta0"], ITERS, N_CHAINS, seed=1920, snapshot={"period": period, "fn": lambda p: p.C.copy()})
    _check(res)
    save("g19_prior_families_am", C0=C0, sd=np.array(prop.sd), epsilon=np.array(1e-6), t0=np.array(t0), period=np.array(period),
         C_hist=np.array(snaps), n_outside=np.array(CountingPrior.outside), **meta, **res)


if __name__ == "__main__":
    g19_prior_families_grw()
    g19_prior_families_am()
