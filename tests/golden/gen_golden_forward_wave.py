"""Generate g20_wave_grw.npz and g20_wave_am.npz by RUNNING THE REFERENCE (tinyDA) itself over the NumPy twin of the
wave-cooperative test model (tests/extwave.py: a reaction-diffusion ring, 48 explicit Euler steps, all outputs from one
solve): 4 chains x 300 iterations, isotropic Gaussian noise sigma = 0.01, starts at truth + 0.01 N(0, I),
  g20_wave_grw  d = 5, m = 23, adaptive GaussianRandomWalk, period 50
  g20_wave_am   d = 13, m = 100, AdaptiveMetropolis, t0 = period = 50

Run in the build container only (needs the reference, like gen_golden.py):

    python tests/golden/gen_golden_forward_wave.py
"""
import os
import sys

import numpy as np
import scipy.stats as stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_golden import run_mh, save, tda  # noqa: E402
from tests.extwave import np_forward, problem  # noqa: E402

N_CHAINS, ITERS, SIGMA = 4, 300, 0.01


def _check(name, res):
    rate = res["accepted"][:, 1:].mean()
    print("%s: acceptance %.3f" % (name, rate))
    assert 0.1 <= rate <= 0.9, (name, rate)


def _posterior(d, m, seed):
    _, data, theta0 = problem(d, m, N_CHAINS, seed, sigma=SIGMA)
    pm, pv = np.zeros(d), np.ones(d)
    post = tda.Posterior(stats.multivariate_normal(pm, np.diag(pv)), tda.GaussianLogLike(data, SIGMA ** 2 * np.eye(m)),
                         lambda theta: np_forward(theta, m)[0])
    return post, dict(data=data, sigma2=np.array(SIGMA ** 2), prior_mean=pm, prior_cov=np.diag(pv), theta0=theta0)


def g20_wave_grw():
    d, m = 5, 23
    post, common = _posterior(d, m, 2001)
    C, period = 1e-3 * np.eye(d), 50
    prop = tda.GaussianRandomWalk(C=C, scaling=1.0, adaptive=True, gamma=1.01, period=period)
    res, snaps = run_mh(post, prop, common["theta0"], ITERS, N_CHAINS, seed=2010, snapshot={"period": period, "fn": lambda p: float(p.scaling)})
    _check("g20_wave_grw", res)
    save("g20_wave_grw", C=C, scaling0=np.array(1.0), adaptive=np.array(True), gamma=np.array(1.01), period=np.array(period),
         scaling_hist=np.array(snaps), **common, **res)


def g20_wave_am():
    d, m = 13, 100
    post, common = _posterior(d, m, 2002)
    C0, t0, period = 1e-4 * np.eye(d), 50, 50
    prop = tda.AdaptiveMetropolis(C0=C0, sd=None, epsilon=1e-6, t0=t0, period=period, adaptive=False, gamma=1.01)
    res, snaps = run_mh(post, prop, common["theta0"], ITERS, N_CHAINS, seed=2020, snapshot={"period": period, "fn": lambda p: p.C.copy()})
    _check("g20_wave_am", res)
    save("g20_wave_am", C0=C0, sd=np.array(prop.sd), epsilon=np.array(1e-6), t0=np.array(t0), period=np.array(period),
         C_hist=np.array(snaps), **common, **res)


if __name__ == "__main__":
    g20_wave_grw()
    g20_wave_am()
