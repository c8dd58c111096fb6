"""Generate g17_mala_rosenbrock.npz by RUNNING THE REFERENCE (tinyDA) itself -- the golden vector of MALA over a
non-linear model with a `gradient(parameters, sensitivity)` method, the set-up of the reference's MALA example
(examples/MALA Rosenbrock.ipynb): the 2-parameter Rosenbrock function with a = 1, b = 10 as a one-output forward model,
prior N(0, I), data [0], unit noise, MALA(scaling=0.01, adaptive=True) with the default period (100) and gamma (1.01).

Run in the build container only (needs the reference, like gen_golden.py):

    python tests/golden/gen_golden_mala_source.py
"""
import os
import sys

import numpy as np
import scipy.stats as stats

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import run_mh, save, tda  # noqa: E402


class RosenbrockWithGradient:
    """F(x, y) = (a - x)^2 + b (y - x^2)^2 as a one-element output; gradient(theta, s) = J(theta)^T s."""

    def __init__(self, a=1.0, b=10.0):
        self.a, self.b = a, b

    def __call__(self, theta):
        x, y = theta
        return np.array([(self.a - x) ** 2 + self.b * (y - x ** 2) ** 2])

    def gradient(self, theta, sensitivity):
        x, y = theta
        J = np.array([[-2.0 * (self.a - x) - 4.0 * self.b * x * (y - x ** 2), 2.0 * self.b * (y - x ** 2)]])
        return J.T @ np.asarray(sensitivity)


def g17_mala_rosenbrock():
    n_chains, iters, period = 4, 400, 100
    prior = stats.multivariate_normal(np.zeros(2), np.eye(2))
    post = tda.Posterior(prior, tda.GaussianLogLike(np.array([0.0]), np.eye(1)), RosenbrockWithGradient())
    prop = tda.MALA(scaling=0.01, adaptive=True)
    theta0 = np.random.default_rng(1701).standard_normal((n_chains, 2))
    res, snaps = run_mh(post, prop, theta0, iters, n_chains, seed=1710, zkind="normal01",
                        snapshot={"period": period, "fn": lambda p: float(p.scaling)})
    save("g17_mala_rosenbrock", a=np.array(1.0), b=np.array(10.0), data=np.array([0.0]), noise_var=np.array(1.0),
         prior_mean=np.zeros(2), prior_cov=np.eye(2), scaling0=np.array(0.01), adaptive=np.array(True), gamma=np.array(1.01),
         period=np.array(period), theta0=theta0, scaling_hist=np.array(snaps), **res)


if __name__ == "__main__":
    g17_mala_rosenbrock()
