"""What the tests of MALA under source-defined priors share (tda_logprior_term_grad): the gradient functions of extprior's
hand-written priors, the shipped family library compiled for the host with its gradient, the reference g'(z) / scale in
mpmath at 80 digits on the in-support points of the g21 grid with the bound of the comparison (recorded as
tests/golden/g22_prior_family_grads.npz by tests/golden/gen_golden_prior_family_grads.py), the oracle levels that carry the
exact prior gradient, and the engine over extmodel's forward model under MALA with such a prior.

The bound.  With z = (x - loc) / scale the library returns g'(z) / scale, g' from the table of tda_prior_families.h.  At every
point

    |got - ref| <= 8 eps gmag + gcond + gallow,        eps = 2^-52

  gmag   = the sum of the magnitudes of the addends of g'(z), over scale.  Every addend is built from at most five rounded
           operations (a shape minus one, a product, a quotient, the one logarithm or the square it holds, the final division by
           scale) and the addends are summed once; a correctly rounded operation is within eps / 2 and the device's log and exp
           within one eps, so eight eps of the addends' magnitudes cover them with room for a library function that is an ulp off.
  gcond  = |g'(z (1 + eps)) - g'(z (1 - eps))| / scale.  z itself comes from x by one subtraction and one division, each within
           eps / 2, and the library can know no better z.  For an addend k / z this is a relative eps of the addend (inside
           gmag already); where g' holds log z (lognorm) it is the absolute eps / s^2 that the rounding of z puts into the
           logarithm; for beta's (b - 1) / (1 - z) it is eps z / (1 - z) of the addend, which near the upper edge is the whole
           error.  The same term is in the bound of the log-densities (extfamilies: cond).
  gallow = Weibull alone: exp(c log z) turns the roundings of log z and of the product into a relative (|c log z| + 1) eps of
           z^c, which enters g' as c z^c / z.

Nothing in the bound is measured on the code under test."""
import ctypes
import os
import subprocess

import numpy as np

from oracle import tinyda_oracle as orc

from . import extfamilies as xf
from . import extmodel as xm
from . import extprior as xp
from .extengine import PRIOR_SOURCE, set_proposal

GOLDEN_NAME = "g22_prior_family_grads"
EPS = 2.0 ** -52
GRAD_SIG = "__device__ double tda_logprior_term_grad(double x, double p, double q, int j)"

# d term / d x of extprior.LOGNORMAL_SRC and extprior.NORMAL_SRC
LOGNORMAL_GRAD_SRC = r"""
__device__ double tda_logprior_term_grad(double x, double p, double q, int j) {
  return (-1.0 - (log(x) - p) / (q * q)) / x;
}
"""
NORMAL_GRAD_SRC = r"""
__device__ double tda_logprior_term_grad(double x, double p, double q, int j) {
  return (p - x) / (q * q);
}
"""


def lognormal_grad(theta, p, q):
    theta = np.asarray(theta, dtype=float)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (-1.0 - (np.log(theta) - p) / (q * q)) / theta


# ---- the reference (mpmath) ----------------------------------------------------------------------------------------------------------
def _grad_addends(mp, name, s, z):
    """the addends of g'(z), as the table of tda_prior_families.h splits it"""
    if name in ("norm", "halfnorm", "truncnorm"):
        return [-z]
    if name == "uniform":
        return [mp.mpf(0)]
    if name == "lognorm":
        return [-1 / z, -mp.log(z) / (s[0] ** 2 * z)]
    if name == "gamma":
        return [(s[0] - 1) / z, mp.mpf(-1)]
    if name == "invgamma":
        return [-(s[0] + 1) / z, 1 / (z * z)]
    if name == "beta":
        return [(s[0] - 1) / z, -(s[1] - 1) / (1 - z)]
    if name == "expon":
        return [mp.mpf(-1)]
    if name == "laplace":
        return [-mp.sign(z)]
    if name == "cauchy":
        return [-2 * z / (1 + z * z)]
    if name == "t":
        return [-(s[0] + 1) * z / (s[0] + z * z)]
    assert name == "weibull_min", name
    return [(s[0] - 1) / z, -s[0] * mp.exp(s[0] * mp.log(z)) / z]


def reference(g21):
    """dict of [128, 14] arrays over the points of the g21 fixture: `inside` (the rest points and the kept probes inside the
    supports: where the gradient is compared), and there ref = g'(z) / scale, gmag, gcond, gallow of the module's docstring
    (0 elsewhere)"""
    mp = xf._mp()
    rows = xf.decode_rows(g21)
    x = g21["x"]
    out = {k: np.zeros(x.shape) for k in ("ref", "gmag", "gcond", "gallow")}
    out["inside"] = np.isfinite(g21["ref"])
    for i, (name, shapes, loc, scale) in enumerate(rows):
        s = [mp.mpf(v) for v in shapes]
        q = mp.mpf(scale)
        for k in np.nonzero(out["inside"][i])[0]:
            z = (mp.mpf(float(x[i, k])) - mp.mpf(loc)) / q
            add = _grad_addends(mp, name, s, z)
            out["ref"][i, k] = float(sum(add) / q)
            out["gmag"][i, k] = float(sum(abs(a) for a in add) / q)
            lo, hi, _, _ = xf.z_support(name, shapes)
            zs = [min(max(z * (1 + sg * mp.mpf(EPS)), mp.mpf(lo)), mp.mpf(hi)) for sg in (1, -1)]
            out["gcond"][i, k] = float(abs(sum(_grad_addends(mp, name, s, zs[0])) - sum(_grad_addends(mp, name, s, zs[1]))) / q)
            if name == "weibull_min":
                out["gallow"][i, k] = float(mp.mpf(EPS) * (abs(s[0] * mp.log(z)) + 1) * s[0] * mp.exp(s[0] * mp.log(z)) / (z * q))
    assert all(np.all(np.isfinite(v)) for v in out.values())
    return out


def fixture_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN_NAME + ".npz")


def bound(g22):
    """[128, 14] the bound of the module's docstring (0 where nothing is compared)"""
    return 8 * EPS * g22["gmag"] + g22["gcond"] + g22["gallow"]


def report(rows, ratio, inside, what):
    """largest error / bound per family, printed; -> the lines"""
    lines = []
    for name in xf.FAMILY_NAMES:
        mine = np.array([r[0] == name for r in rows])
        lines.append("%-12s largest %s %.3e over %d points" % (name, what, ratio[mine].max(), inside[mine].sum()))
    print("\n".join(lines))
    return lines


# ---- the shipped library on the host -------------------------------------------------------------------------------------------------
def host_library(tmp_path, comps):
    """extprior.host_library with `terms` extended to the gradient: -> term(x, j), grad(x, j), rows"""
    from tinyda_amd import likelihoods as lk

    rows = [lk._family_component(c) for c in comps]
    assert all(r is not None for r in rows)
    src = ("#include <cmath>\nusing std::log; using std::log1p; using std::exp; using std::fabs;\n#define __device__\n"
           + lk._family_prologue(rows) + lk.family_library_source()
           + "\nextern \"C\" void terms(const double* x, const double* p, const double* q, int j, int n, double* out, double* grad) {\n"
             "  for (int i = 0; i < n; ++i) {\n    out[i] = tda_logprior_term(x[i], p[j], q[j], j);\n"
             "    grad[i] = tda_logprior_term_grad(x[i], p[j], q[j], j);\n  }\n}\n")
    cpp, so = tmp_path / "libgrad.cpp", tmp_path / "libgrad.so"
    cpp.write_text(src)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(cpp)], check=True)
    lib = ctypes.CDLL(str(so))
    p, q = np.array([r[4] for r in rows]), np.array([r[5] for r in rows])
    dp = ctypes.POINTER(ctypes.c_double)

    def both(x, j):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out, grad = np.empty_like(x), np.empty_like(x)
        lib.terms(x.ctypes.data_as(dp), p.ctypes.data_as(dp), q.ctypes.data_as(dp), ctypes.c_int(j), ctypes.c_int(x.size), out.ctypes.data_as(dp),
                  grad.ctypes.data_as(dp))
        return out, grad

    return (lambda x, j: both(x, j)[0]), (lambda x, j: both(x, j)[1]), rows


# ---- oracle levels with the exact prior gradient -----------------------------------------------------------------------------------
class FamilyGradPrior(xp.FamilyPrior):
    """FamilyPrior (scipy's own logpdf) plus the exact gradient of the components (NaN or anything outside a support)"""

    def __init__(self, comps):
        from tinyda_amd import likelihoods as lk

        super().__init__(comps)
        self.rows = [lk._family_component(c) for c in self.comps]

    def grad(self, theta):
        from tinyda_amd import likelihoods as lk

        return lk.family_gradient(self.rows, np.atleast_2d(theta))


def gaussian_grad_level(prior, m, y, noise=("iso", xp.SIGMA2)):
    """extmodel's model, Gaussian noise, `prior` with logpdf / grad: the level orc.run_mh needs under MALA"""
    level = orc.CallableGaussianLevel(lambda th: xm.np_forward(th, m), y, noise[0], noise[1], prior)
    level.grad_logpost = lambda theta, F: prior.grad(theta) + xm.np_vjp(theta, level.loglike.grad(F))
    return level


def loglike_grad_level(prior, m, y, par, kind):
    """extmodel's model under a DeviceLogLike of extloglike.KINDS"""
    from . import extloglike as xl

    level = xl.LogLikeLevel(lambda th: xm.np_forward(th, m), y, par, xl.KINDS[kind][1], prior)
    dterm = xl.KINDS[kind][2]
    level.grad_logpost = lambda theta, F: prior.grad(theta) + xm.np_vjp(theta, dterm(F, y, par))
    return level


def mala_proposals_outside(ref, prior, level, z, prop):
    """[N, T] True where the MALA proposal of step t left a support, from the oracle's trace (fixed scaling): theta + s^2 / 2 grad + s z"""
    sg = prop["scaling"]
    N, T1, d = ref["theta"].shape
    cur = ref["theta"][:, :-1].reshape(-1, d)
    grad = level.grad_logpost(cur, level.forward(cur)).reshape(N, T1 - 1, d)
    props = ref["theta"][:, :-1] + 0.5 * sg ** 2 * grad + sg * z
    return ~prior.inside(props.reshape(-1, d)).reshape(N, T1 - 1)


def starts_inside(comps, n, rng, q0=0.35):
    """n starting points well inside the supports, around the components' quantiles q0, q0 + 0.1, q0 + 0.2 (MALA's drift diverges at
    the edges: chains started there reject every step)"""
    truth = np.array([c.ppf(q0 + 0.1 * (j % 3)) for j, c in enumerate(comps)])
    spread = np.array([min(0.02, 0.1 * (c.ppf(0.6) - c.ppf(0.3))) for c in comps])
    return truth, truth[None, :] + spread * rng.standard_normal((n, len(comps)))


def make_engine(psrc, p, q, N, level, prop, bs=0, seed=93, chain_offset=5):
    """single-level engine under a source-defined prior; level = (model (+ likelihood) source, data, noise kind, noise)"""
    from tinyda_amd.engine import Engine

    d = len(p)
    e = Engine(N, d, seed=seed, chain_offset=chain_offset, block_steps=bs)
    e.set_prior_joint(np.full(d, PRIOR_SOURCE), p, q)
    src, y, kind, noise = level
    e.set_level_source(0, src + "\n" + psrc, y, kind, noise)
    set_proposal(e, prop)
    return e


def family_source(comps):
    """(p, q, HIP source with the gradient) exactly as sample() hands them over for DevicePrior.from_distributions"""
    import tinyda_amd as tda

    dp = tda.DevicePrior.from_distributions(comps)
    return dp.p, dp.q, dp.source


# ---- the prior's gradient alone, through one MALA step -------------------------------------------------------------------------------
# a model with constant outputs and a zero vector-Jacobian product: the log-posterior's gradient is the prior's
ZERO_MODEL = r"""
__device__ double tda_forward(const double* theta, int dim, int o) { return 0.0; }
__device__ double tda_gradient(const double* theta, int dim, const double* sens, int m, int j) { return 0.0; }
"""


def probe_chains(g21, g22, d):
    """Chains that put every in-support point of the first d rows of the g21 grid under one MALA step whose outcome is the
    device's tda_logprior_term_grad at that point: with a zero normal in parameter j the kernel computes theta_1 = theta_0 + h
    grad (h = s^2 / 2 a power of two, so h grad rounds nothing away), and (theta_1 - theta_0) / h is the gradient up to the
    rounding of that one sum, eps / 2 |theta_1|.

    A point (row j, column k) admits a step of dist / (4 |grad|) at most (dist: the distance to the nearest edge of its
    support, or scale max(1, |z|) where that is less), so that the move stays inside and z changes by a quarter at most.  A chain has one step size, so the points of a column are split into buckets by
    the step they admit (a factor 256 each) and a chain holds the points of one bucket with h = 2^(8 b - 1), s = 2^(4 b).
    Every other row of the chain is held at one of its own points: its normal is z = -h grad / s (grad from the fixture), which
    cancels its drift up to the rounding delta = eps h |grad| of the sum.  A held row limits h twice over: delta must stay far
    inside its distance to an edge, and the change delta |grad| / dist that delta makes to its gradient must not show in the
    acceptance, whose exponent holds h |grad| |grad' - grad| / 2 of it: eps h^2 |grad|^3 / (2 dist) <= 2^-8.  Each row is held
    at the point of its own that allows the largest h, and a chain's b is lowered to what its held rows allow.
    Points on a closed edge of their support are left out (the gradient may point outside).  A point within a few ulps of an
    edge admits no step that the sum theta_0 + h grad could resolve: eps |theta| / h exceeds its gradient, probe_bound() is
    vacuous there and the point is in effect unchecked on the device (about 15 % of the points are held to less than 1e-6 of
    their gradient; the host comparison holds every point to the full bound).
    -> x[C, d], h[C], z[C, d], compared[C, d], ref[C, d], tol[C, d] (tol: bound() of the host comparison)"""
    rows = xf.decode_rows(g21)[:d]
    inside = g22["inside"][:d, :xf.OUT_LO]
    xs, refs, tols = g21["x"][:d, :xf.OUT_LO], g22["ref"][:d, :xf.OUT_LO], bound(g22)[:d, :xf.OUT_LO]
    dist = np.full(xs.shape, np.inf)
    for j, r in enumerate(rows):
        lo, hi = xp.support(xf.component(r))
        dist[j] = np.minimum(xs[j] - lo, hi - xs[j])
    inside = inside & (dist > 0.0)
    # (far from any edge the length that counts is the component's own: scale max(1, |z|))
    loc, scale = np.array([r[2] for r in rows])[:, None], np.array([r[3] for r in rows])[:, None]
    dist = np.minimum(dist, scale * np.maximum(1.0, np.abs((xs - loc) / scale)))
    ar = np.abs(refs)
    with np.errstate(all="ignore"):
        want = np.where(inside & (refs != 0.0), dist / (4.0 * ar), 1.0)  # [d, 12]
        held = np.where(inside, np.where(refs != 0.0, np.minimum(2.0 ** -10 * dist / (EPS * ar), np.sqrt(2.0 ** -7 * dist / (EPS * ar ** 3))), 1.0), 0.0)
    with np.errstate(all="ignore"):
        bucket = np.floor(np.log2(np.minimum(want, 1.0)) / 8.0)
    hold = np.argmax(held, axis=1)  # [d] the column a row is held at
    cap = np.minimum(held[np.arange(d), hold], 1.0)
    out = []
    for k in range(xs.shape[1]):
        for b in np.unique(bucket[inside[:, k], k]):
            mine = inside[:, k] & (bucket[:, k] == b)
            col = np.where(mine, k, hold)
            take = lambda a: a[np.arange(d), col]  # noqa: E731
            b = min(b, np.floor((np.log2(np.min(cap[~mine], initial=1.0)) + 1.0) / 8.0))
            h, sg = 2.0 ** (8 * b - 1), 2.0 ** (4 * b)
            out.append((take(xs), h, np.where(mine, 0.0, -h * take(refs) / sg), mine, take(refs), take(tols)))
    return tuple(np.array(v) for v in zip(*out))


def probe_bound(x, h, ref, tol):
    """[C, d] what (theta_1 - theta_0) / h is held to: the bound of the host comparison plus the rounding of the sum theta_0 + h grad,
    eps / 2 |theta_1| <= eps |theta_0|, over h"""
    with np.errstate(over="ignore"):
        return tol + EPS * np.abs(x) / h[:, None]
