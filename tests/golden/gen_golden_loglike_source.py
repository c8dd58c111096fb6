"""Generate g18_loglike_student_grw.npz and g18_loglike_poisson_am.npz by RUNNING THE REFERENCE (tinyDA) itself -- the
golden vectors of chains whose likelihood is not Gaussian.  The reference takes any object with `loglike(model_output)`
(posterior.py: "scipy.stats.rv_continuous or tinyDA.LogLike"); here it is a plain Python class that sums the per-output
terms of tests/extloglike.py (Student-t with nu = 4 and a per-output scale; Poisson counts with log link and a per-output
exposure) over the non-linear model of tests/extmodel.py, d = 5, m = 23, 4 chains x 300 iterations, under an adaptive
GaussianRandomWalk and under AdaptiveMetropolis.

Run in the build container only (needs the reference, like gen_golden.py):

    python tests/golden/gen_golden_loglike_source.py
"""
import os
import sys

import numpy as np
import scipy.stats as stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_golden import run_mh, save, tda  # noqa: E402
from tests.extloglike import poisson_terms, t_terms  # noqa: E402
from tests.extmodel import np_forward  # noqa: E402

D, M, N_CHAINS, ITERS = 5, 23, 4, 300


class SeparableLogLike:
    """the reference's likelihood protocol: loglike(model_output) -> float"""

    def __init__(self, terms, data, par):
        self.terms, self.data, self.par = terms, data, par

    def loglike(self, x):
        return np.sum(self.terms(x, self.data, self.par))


def _model(theta):
    return np_forward(theta, M)[0]


def _setup(seed, kind):
    rng = np.random.default_rng(seed)
    truth = 0.3 * rng.standard_normal(D)
    F = _model(truth)
    if kind == "t":
        par = 0.1 * (1.0 + 0.1 * np.arange(M) / M)
        data = F + par * rng.standard_t(4, M)
    else:
        par = 20.0 + np.arange(M) % 7
        data = rng.poisson(par * np.exp(F)).astype(float)
    pm, pv = 0.1 * np.ones(D), 0.5 + 0.01 * np.arange(D)
    theta0 = truth + 0.01 * rng.standard_normal((N_CHAINS, D))
    return data, par, pm, pv, theta0


def g18_loglike_student_grw():
    data, par, pm, pv, theta0 = _setup(1801, "t")
    post = tda.Posterior(stats.multivariate_normal(pm, np.diag(pv)), SeparableLogLike(t_terms, data, par), _model)
    C, period = 1e-3 * np.eye(D), 50
    prop = tda.GaussianRandomWalk(C=C, scaling=1.0, adaptive=True, gamma=1.01, period=period)
    res, snaps = run_mh(post, prop, theta0, ITERS, N_CHAINS, seed=1810, snapshot={"period": period, "fn": lambda p: float(p.scaling)})
    save("g18_loglike_student_grw", kind=np.array("t"), data=data, par=par, prior_mean=pm, prior_cov=np.diag(pv), C=C,
         scaling0=np.array(1.0), adaptive=np.array(True), gamma=np.array(1.01), period=np.array(period), theta0=theta0,
         scaling_hist=np.array(snaps), **res)


def g18_loglike_poisson_am():
    data, par, pm, pv, theta0 = _setup(1802, "poisson")
    post = tda.Posterior(stats.multivariate_normal(pm, np.diag(pv)), SeparableLogLike(poisson_terms, data, par), _model)
    C0, t0, period = 1e-3 * np.eye(D), 50, 50
    prop = tda.AdaptiveMetropolis(C0=C0, sd=None, epsilon=1e-6, t0=t0, period=period, adaptive=False, gamma=1.01)
    res, snaps = run_mh(post, prop, theta0, ITERS, N_CHAINS, seed=1820, snapshot={"period": period, "fn": lambda p: p.C.copy()})
    save("g18_loglike_poisson_am", kind=np.array("poisson"), data=data, par=par, prior_mean=pm, prior_cov=np.diag(pv), C0=C0,
         sd=np.array(prop.sd), epsilon=np.array(1e-6), t0=np.array(t0), period=np.array(period), theta0=theta0,
         C_hist=np.array(snaps), **res)


if __name__ == "__main__":
    g18_loglike_student_grw()
    g18_loglike_poisson_am()
