"""MALA over a source-defined forward model (DeviceModel with tda_gradient): lowering rules, and the host protocol against
the reference's own MALA on the Rosenbrock example (tests/golden/g17_mala_rosenbrock.npz, gen_golden_mala_source.py)."""
import numpy as np
import pytest
import scipy.stats as st

ROSEN_SRC = r"""
// F(x, y) = (a - x)^2 + b (y - x^2)^2, a = 1, b = 10 (one output)
__device__ double tda_forward(const double* theta, int dim, int o) {
  const double x = theta[0], y = theta[1];
  return (1.0 - x) * (1.0 - x) + 10.0 * ((y - x * x) * (y - x * x));
}
__device__ double tda_gradient(const double* theta, int dim, const double* sensitivity, int n_outputs, int j) {
  const double x = theta[0], y = theta[1];
  const double dF = j == 0 ? -2.0 * (1.0 - x) - 4.0 * 10.0 * x * (y - x * x) : 2.0 * 10.0 * (y - x * x);
  return dF * sensitivity[0];
}
"""

FORWARD_ONLY_SRC = r"""
__device__ double tda_forward(const double* theta, int dim, int o) { return theta[o % dim]; }
// tda_gradient is not defined here: a mention in a comment does not count
/* nor here: __device__ double tda_gradient(const double*, int, const double*, int, int); */
"""


def rosen_forward(theta):
    x, y = theta
    return np.array([(1.0 - x) ** 2 + 10.0 * (y - x ** 2) ** 2])


def rosen_gradient(theta, sensitivity):
    x, y = theta
    J = np.array([[-2.0 * (1.0 - x) - 4.0 * 10.0 * x * (y - x ** 2), 2.0 * 10.0 * (y - x ** 2)]])
    return J.T @ sensitivity


def _posterior(model, d=2, m=1, noise=None, prior=None):
    import tinyda_amd as tda

    prior = st.multivariate_normal(np.zeros(d), np.eye(d)) if prior is None else prior
    return tda.Posterior(prior, tda.GaussianLogLike(np.zeros(m), np.eye(m) if noise is None else noise), model)


def test_has_gradient_ignores_comments():
    import tinyda_amd as tda

    assert tda.DeviceModel(ROSEN_SRC, 1).has_gradient
    assert not tda.DeviceModel(FORWARD_ONLY_SRC, 1).has_gradient
    m = tda.DeviceModel(FORWARD_ONLY_SRC, 1)
    assert not hasattr(m, "gradient")  # host MALA: finite differences
    m = tda.DeviceModel(ROSEN_SRC, 1, reference=rosen_forward, reference_gradient=rosen_gradient)
    np.testing.assert_array_equal(m.gradient(np.array([0.3, -0.2]), np.array([2.0])), rosen_gradient(np.array([0.3, -0.2]), np.array([2.0])))


def test_device_plan():
    import tinyda_amd as tda
    from tinyda_amd import api

    post = _posterior(tda.DeviceModel(ROSEN_SRC, 1))
    plan = api._device_plan([post], tda.MALA(0.05, adaptive=True, period=50))
    assert plan is not None and plan[1]["kind"] == 6 and plan[1]["adaptive"] and plan[1]["period"] == 50
    assert plan[0][0]["has_gradient"]
    # 65 .. 128 parameters
    src96 = ROSEN_SRC.replace("const double x = theta[0], y = theta[1];", "const double x = theta[0], y = theta[dim - 1];")
    plan = api._device_plan([_posterior(tda.DeviceModel(src96, 1), d=96)], tda.MALA(0.05))
    assert plan is not None and plan[1]["kind"] == 6
    assert api._device_plan([_posterior(tda.DeviceModel(src96, 1), d=128)], tda.MALA(0.05)) is not None

    # refusals: no tda_gradient, two levels, JointPrior, dense noise
    assert api._device_plan([_posterior(tda.DeviceModel(FORWARD_ONLY_SRC, 1))], tda.MALA(0.05)) is None
    assert "tda_gradient" in api._refusal[0]
    assert api._device_plan([_posterior(tda.DeviceModel(FORWARD_ONLY_SRC, 1), d=96)], tda.MALA(0.05)) is None
    assert api._device_plan([post, post], tda.MALA(0.05)) is None
    joint = tda.JointPrior([st.norm(0.0, 1.0), st.norm(0.0, 1.0)])
    assert api._device_plan([_posterior(tda.DeviceModel(ROSEN_SRC, 1), prior=joint)], tda.MALA(0.05)) is None
    assert api._refusal[0] == "MALA: single level, linear model, Gaussian prior"
    dense = np.array([[1.0, 0.3], [0.3, 1.0]])
    assert api._device_plan([_posterior(tda.DeviceModel(ROSEN_SRC, 2), m=2, noise=dense)], tda.MALA(0.05)) is None
    # (the other samplers over the same model are lowered as before)
    assert api._device_plan([post], tda.GaussianRandomWalk(np.eye(2))) is not None


def test_host_class_replays_reference_chain(golden, monkeypatch):
    """The host MALA over DeviceModel(reference=..., reference_gradient=...) takes the exact-gradient branch and replays
    the reference's chain (g17: the MALA Rosenbrock example, adaptive, 4 chains x 400 iterations)."""
    import tinyda_amd as tda

    g = golden("g17_mala_rosenbrock")
    model = tda.DeviceModel(ROSEN_SRC, 1, reference=rosen_forward, reference_gradient=rosen_gradient)
    post = tda.Posterior(st.multivariate_normal(g["prior_mean"], g["prior_cov"]),
                         tda.GaussianLogLike(g["data"], float(g["noise_var"]) * np.eye(1)), model)
    for c in range(g["theta0"].shape[0]):
        prop = tda.MALA(scaling=float(g["scaling0"]), adaptive=bool(g["adaptive"]), gamma=float(g["gamma"]), period=int(g["period"]))
        prop.setup_proposal(parameters=g["theta0"][c], posterior=post)
        assert prop.compute_gradient == prop._compute_gradient
        zs = iter(g["z"][c])
        monkeypatch.setattr(np.random, "standard_normal", lambda n: next(zs))
        link = post.create_link(g["theta0"][c])
        accepted = []
        with np.errstate(over="ignore"):
            for s in range(g["z"].shape[1]):
                cand = post.create_link(prop.make_proposal(link))
                acc = g["u"][c, s] < prop.get_acceptance(cand, link)
                if acc:
                    link = cand
                accepted.append(acc)
                prop.adapt(parameters=link.parameters, accepted=accepted)
                assert acc == bool(g["accepted"][c, s + 1]), (c, s)
                np.testing.assert_allclose(link.posterior, g["logpost"][c, s + 1], rtol=1e-10)
        np.testing.assert_allclose(prop.scaling, g["scaling_hist"][c, -1], rtol=1e-12)
