"""Generate g24_loglike_coupled_grw.npz and g24_loglike_coupled_am.npz by RUNNING THE REFERENCE (tinyDA) itself -- the golden
vectors of chains whose likelihood couples the model's outputs.  The reference takes any object with `loglike(model_output)`;
here it is a plain Python class around the AR(1) twin of tests/extloglikewave.py (rho = 0.6, a per-output scale) over the
non-linear model of tests/extmodel.py, d = 5, m = 23, 4 chains x 160 iterations, under an adaptive GaussianRandomWalk and under
AdaptiveMetropolis.  Only data is stored: the likelihood's name, the data and scales, the prior's moments, the variates, the traces.

Run in the build container only (needs the reference, like gen_golden.py):

    python tests/golden/gen_golden_loglike_coupled.py
"""
import os
import sys

import numpy as np
import scipy.stats as stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_golden import run_mh, save, tda  # noqa: E402
from tests import extloglikewave as xlw  # noqa: E402
from tests.extmodel import np_forward  # noqa: E402

D, M, N_CHAINS, ITERS = 5, 23, 4, 160


class CoupledLogLike:
    """the reference's likelihood protocol: loglike(model_output) -> float"""

    def __init__(self, fn, data, par):
        self.fn, self.data, self.par = fn, data, par

    def loglike(self, x):
        return float(self.fn(x, self.data, self.par)[0])


def _model(theta):
    return np_forward(theta, M)[0]


def _setup(seed):
    data, par, theta0, pm, pv = xlw.problem(D, M, "ar1", N_CHAINS, seed)
    post = tda.Posterior(stats.multivariate_normal(pm, np.diag(pv)), CoupledLogLike(xlw.ar1, data, par), _model)
    return post, dict(kind=np.array("ar1"), data=data, par=par, prior_mean=pm, prior_cov=np.diag(pv), theta0=theta0)


def _check(res):
    rate = res["accepted"][:, 1:].mean()
    assert 0.1 <= rate <= 0.9, rate
    print("acceptance %.3f" % rate)


def g24_loglike_coupled_grw():
    post, meta = _setup(2401)
    C, period = 1e-3 * np.eye(D), 40
    prop = tda.GaussianRandomWalk(C=C, scaling=1.0, adaptive=True, gamma=1.01, period=period)
    res, snaps = run_mh(post, prop, meta["theta0"], ITERS, N_CHAINS, seed=2410, snapshot={"period": period, "fn": lambda p: float(p.scaling)})
    _check(res)
    save("g24_loglike_coupled_grw", C=C, scaling0=np.array(1.0), adaptive=np.array(True), gamma=np.array(1.01), period=np.array(period),
         scaling_hist=np.array(snaps), **meta, **res)


def g24_loglike_coupled_am():
    post, meta = _setup(2402)
    C0, t0, period = 1e-3 * np.eye(D), 40, 40
    prop = tda.AdaptiveMetropolis(C0=C0, sd=None, epsilon=1e-6, t0=t0, period=period, adaptive=False, gamma=1.01)
    res, snaps = run_mh(post, prop, meta["theta0"], ITERS, N_CHAINS, seed=2420, snapshot={"period": period, "fn": lambda p: p.C.copy()})
    _check(res)
    save("g24_loglike_coupled_am", C0=C0, sd=np.array(prop.sd), epsilon=np.array(1e-6), t0=np.array(t0), period=np.array(period),
         C_hist=np.array(snaps), **meta, **res)


if __name__ == "__main__":
    g24_loglike_coupled_grw()
    g24_loglike_coupled_am()
