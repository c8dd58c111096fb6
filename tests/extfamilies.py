"""What the tests of the prior family library (tinyda_amd/csrc/tda_prior_families.h) share: a grid of shapes of its 13
scipy.stats families laid out as 128 table rows, probe points from far in one tail to far in the other, a reference in
mpmath at 80 digits, and the tolerance.  tests/golden/gen_golden_prior_families.py writes all of it to
tests/golden/g21_prior_family_terms.npz, which is what the GPU tests read (they need neither mpmath nor the placing of the
points by scipy).

Rows.  Row i holds family FAMILY_NAMES[i % 13]; the k-th row of a family takes its k-th shape (cycled) and the row's
(loc, scale) is LOC_SCALE[i % 4].  128 rows are nine full rounds and eleven more, so every family sits both in lanes 0-63
and in the second parameter of a lane (rows 64-127), and no family has more than seven shapes, so every shape occurs.

Points.  Column 0 is the rest point ppf(0.5), columns 1-11 are ppf(q) for q in QUANTILES, columns 12 and 13 lie outside a
bounded support (its lower edge - 1e-3 scale, its upper edge + 1e-3 scale; NaN where the support has no such edge).  scipy
only places the points; every number below is computed from the doubles x, loc, scale and the shapes as they stand.

Dropped probes (columns 1-13 that exist): a probe that is not finite; one whose exact |z| exceeds 1e150 (z * z overflows,
and no proposal gets there); one whose exact z = (x - loc) / scale lies within 2^-50 relative of a support edge without
being on it (the two roundings of z then decide the side).  At most 3 % of all probes may go and every row keeps at least 8.

Reference.  The textbook density of each family at the exact z, minus log(scale), with mpmath at 80 digits.  The supports
are the ones the header documents: open at z = 0 (and z = 1) for gamma, invgamma, beta and weibull_min whatever the shape,
closed for uniform, expon, halfnorm and truncnorm.  Outside: -inf.

Tolerance.  |got - ref| <= 1e-11 max(1, mag) + cond (+ the Weibull allowance), with
  mag  = |c| + the sum of the magnitudes of the additive pieces of g(z) in the header's table, c being the whole constant of
         the row as the header defines it (normalising constant - log(scale)): were c split into its loggamma parts, the bar
         would hide a cancellation between them;
  cond = |ref(z (1 + 2^-52)) - ref(z (1 - 2^-52))|: z comes from x by one subtraction and one division, each within 2^-53;
  Weibull: exp(c log z) turns the roundings of log z and of the product into a relative (|c log z| + 1) eps of z^c
         (docstring of test_term_library_against_scipy_logpdf).
The 1e-11 is the bar of test_evaluate_against_scipy for "rounding alone".  Nothing here is measured on the code under test."""
import os

import numpy as np
import scipy.stats as st

from .extprior import FAMILY_NAMES

GOLDEN_NAME = "g21_prior_family_terms"
SHAPES = {
    "lognorm": [(0.01,), (0.25,), (0.7,), (3.0,)],
    "gamma": [(0.05,), (0.5,), (1.0,), (2.5,), (40.0,), (1e3,)],
    "invgamma": [(0.05,), (0.5,), (1.0,), (3.0,), (40.0,), (1e3,)],
    "beta": [(0.3, 0.4), (1.0, 1.0), (1.0, 7.0), (2.0, 3.5), (0.5, 60.0), (300.0, 500.0)],
    "t": [(0.3,), (1.0,), (4.0,), (30.0,), (1e3,), (1e5,), (1e6,)],
    "truncnorm": [(-1.0, 2.0), (-8.0, -6.0), (6.0, 8.0), (20.0, 21.0), (-30.0, 30.0), (-1e-6, 1e-6), (5.0, 5.0 + 1e-9)],
    "weibull_min": [(0.2,), (1.0,), (1.7,), (12.0,)],
}
LOC_SCALE = [(0.0, 1.0), (0.1, 0.7), (-3.0, 1e-3), (1e3, 25.0)]
QUANTILES = (1e-30, 1e-12, 1e-6, 1e-3, 0.05, 0.25, 0.75, 0.95, 1 - 1e-3, 1 - 1e-6, 1 - 1e-12)
N_ROWS, N_COLS, REST, OUT_LO, OUT_HI = 128, 14, 0, 12, 13
# beyond the grid: constants only (test_constants_beyond_the_grid)
EXTREME = [("t", (1e8,)), ("t", (1e10,)), ("t", (1e15,)), ("truncnorm", (-1e-9, 1e-9)), ("truncnorm", (0.0, 1e-12)),
           ("truncnorm", (30.0, 30.001)), ("truncnorm", (37.0, 38.0)), ("truncnorm", (100.0, 101.0)), ("gamma", (1e6,)),
           ("beta", (1e6, 1e6)), ("beta", (1e-3, 1e3))]
DROP_SHARE, KEEP_PER_ROW = 0.03, 8
EPS = 2.0 ** -52


def grid_rows():
    """[(family, shapes, loc, scale)] * 128"""
    rows = []
    for i in range(N_ROWS):
        name = FAMILY_NAMES[i % len(FAMILY_NAMES)]
        shapes = SHAPES.get(name, [()])
        rows.append((name, shapes[(i // len(FAMILY_NAMES)) % len(shapes)]) + LOC_SCALE[i % len(LOC_SCALE)])
    return rows


def component(row):
    name, shapes, loc, scale = row
    return getattr(st, name)(*shapes, loc=loc, scale=scale)


def first_row_of_each_shape(rows):
    """indices of the first row of every distinct (family, shapes): one row per shape"""
    seen, out = set(), []
    for i, r in enumerate(rows):
        if r[:2] not in seen:
            seen.add(r[:2])
            out.append(i)
    return out


def z_support(name, shapes):
    """(lower edge, upper edge, lower edge belongs to the support, upper edge does) of the standardised family, as the header's table has them"""
    inf = float("inf")
    if name in ("lognorm", "gamma", "invgamma", "weibull_min"):
        return 0.0, inf, False, False
    if name == "beta":
        return 0.0, 1.0, False, False
    if name == "uniform":
        return 0.0, 1.0, True, True
    if name in ("expon", "halfnorm"):
        return 0.0, inf, True, False
    if name == "truncnorm":
        return shapes[0], shapes[1], True, True
    return -inf, inf, False, False


def place_points(rows):
    """x[128, 14]: the rest point, the quantile probes, the two points outside (NaN: no such edge)"""
    x = np.full((len(rows), N_COLS), np.nan)
    with np.errstate(all="ignore"):
        for i, row in enumerate(rows):
            dist = component(row)
            x[i, REST] = dist.ppf(0.5)
            x[i, 1:1 + len(QUANTILES)] = dist.ppf(np.array(QUANTILES))
            lo, hi, _, _ = z_support(row[0], row[1])
            if np.isfinite(lo):
                x[i, OUT_LO] = row[2] + row[3] * lo - 1e-3 * row[3]
            if np.isfinite(hi):
                x[i, OUT_HI] = row[2] + row[3] * hi + 1e-3 * row[3]
    return x


def probe_exists(rows):
    """[128, 14] True for the columns that hold a probe (not the rest point, not the outside point of an edge that is not there)"""
    ex = np.ones((len(rows), N_COLS), dtype=bool)
    ex[:, REST] = False
    for i, row in enumerate(rows):
        lo, hi, _, _ = z_support(row[0], row[1])
        ex[i, OUT_LO], ex[i, OUT_HI] = np.isfinite(lo), np.isfinite(hi)
    return ex


# ---- the reference (mpmath; imported where it is used, so that reading the fixture needs none) ---------------------------------
def _mp():
    import mpmath

    mpmath.mp.dps = 80
    return mpmath.mp


def _gauss_mass(mp, a, b):
    """Phi(b) - Phi(a) from the tail that does not cancel: both bounds on one side are two values of erfc on that side"""
    r2 = mp.sqrt(2)
    if a > 0:
        return (mp.erfc(a / r2) - mp.erfc(b / r2)) / 2
    if b < 0:
        return (mp.erfc(-b / r2) - mp.erfc(-a / r2)) / 2
    return (mp.erf(b / r2) - mp.erf(a / r2)) / 2


def mp_constant(name, shapes):
    """the part of the textbook log-density that does not depend on z"""
    mp = _mp()
    s = [mp.mpf(v) for v in shapes]
    half_log_2pi = mp.log(2 * mp.pi) / 2
    if name == "norm":
        return -half_log_2pi
    if name == "lognorm":
        return -mp.log(s[0]) - half_log_2pi
    if name in ("gamma", "invgamma"):
        return -mp.loggamma(s[0])
    if name == "beta":
        return mp.loggamma(s[0] + s[1]) - mp.loggamma(s[0]) - mp.loggamma(s[1])
    if name == "halfnorm":
        return mp.log(2 / mp.pi) / 2
    if name == "laplace":
        return -mp.log(2)
    if name == "cauchy":
        return -mp.log(mp.pi)
    if name == "t":
        return mp.loggamma((s[0] + 1) / 2) - mp.loggamma(s[0] / 2) - mp.log(s[0] * mp.pi) / 2
    if name == "truncnorm":
        return -half_log_2pi - mp.log(_gauss_mass(mp, s[0], s[1]))
    if name == "weibull_min":
        return mp.log(s[0])
    assert name in ("uniform", "expon"), name
    return mp.mpf(0)


def _inside(name, shapes, z):
    lo, hi, lo_in, hi_in = z_support(name, shapes)
    return (z > lo or (lo_in and z == lo)) and (z < hi or (hi_in and z == hi))


def _pieces(mp, name, s, z):
    """the additive pieces of g(z), as the header's table splits it"""
    if name in ("norm", "halfnorm", "truncnorm"):
        return [-z * z / 2]
    if name == "uniform":
        return [mp.mpf(0)]
    if name == "lognorm":
        return [-mp.log(z), -(mp.log(z) / s[0]) ** 2 / 2]
    if name == "gamma":
        return [(s[0] - 1) * mp.log(z), -z]
    if name == "invgamma":
        return [-(s[0] + 1) * mp.log(z), -1 / z]
    if name == "beta":
        return [(s[0] - 1) * mp.log(z), (s[1] - 1) * mp.log1p(-z)]
    if name == "expon":
        return [-z]
    if name == "laplace":
        return [-abs(z)]
    if name == "cauchy":
        return [-mp.log1p(z * z)]
    if name == "t":
        return [-(s[0] + 1) / 2 * mp.log1p(z * z / s[0])]
    assert name == "weibull_min", name
    return [(s[0] - 1) * mp.log(z), -mp.exp(s[0] * mp.log(z))]


def _logpdf_z(mp, name, s, z):
    """log of the textbook density of the standardised family at z inside its support"""
    pi = mp.pi
    if name == "norm":
        return -z * z / 2 - mp.log(mp.sqrt(2 * pi))
    if name == "uniform":
        return mp.mpf(0)
    if name == "lognorm":
        return -mp.log(s[0] * z * mp.sqrt(2 * pi)) - mp.log(z) ** 2 / (2 * s[0] ** 2)
    if name == "gamma":
        return (s[0] - 1) * mp.log(z) - z - mp.loggamma(s[0])
    if name == "invgamma":
        return -(s[0] + 1) * mp.log(z) - 1 / z - mp.loggamma(s[0])
    if name == "beta":
        return (s[0] - 1) * mp.log(z) + (s[1] - 1) * mp.log1p(-z) + mp.loggamma(s[0] + s[1]) - mp.loggamma(s[0]) - mp.loggamma(s[1])
    if name == "expon":
        return -z
    if name == "halfnorm":
        return mp.log(2 / pi) / 2 - z * z / 2
    if name == "laplace":
        return -abs(z) - mp.log(2)
    if name == "cauchy":
        return -mp.log(pi) - mp.log1p(z * z)
    if name == "t":
        nu = s[0]
        return mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * pi) / 2 - (nu + 1) / 2 * mp.log1p(z * z / nu)
    if name == "truncnorm":
        return -z * z / 2 - mp.log(2 * pi) / 2 - mp.log(_gauss_mass(mp, s[0], s[1]))
    assert name == "weibull_min", name
    return mp.log(s[0]) + (s[0] - 1) * mp.log(z) - z ** s[0]


def reference(rows, x):
    """dict of [128, 14] arrays for the points x (and [128] for the constants):
      ref      reference log-density (-inf outside the support, NaN where x is not finite)
      mag      |c| + sum of |pieces of g(z)| (0 where ref is not finite)
      cond     |ref(z (1 + 2^-52)) - ref(z (1 - 2^-52))|, the perturbed z kept inside a support whose edge z sits on
      allow    the Weibull allowance eps (|c log z| + 1) z^c (0 for every other family)
      dropped  the probes that the module's docstring drops
      const    the whole constant of each row, c = normalising constant - log(scale)"""
    mp = _mp()
    n = len(rows)
    out = {k: np.zeros((n, N_COLS)) for k in ("ref", "mag", "cond", "allow")}
    out["dropped"] = np.zeros((n, N_COLS), dtype=bool)
    out["const"] = np.zeros(n)
    exists = probe_exists(rows)
    for i, (name, shapes, loc, scale) in enumerate(rows):
        s = [mp.mpf(v) for v in shapes]
        c = mp_constant(name, shapes) - mp.log(mp.mpf(scale))
        out["const"][i] = float(c)
        lo, hi, _, _ = z_support(name, shapes)
        edges = [mp.mpf(e) for e in (lo, hi) if np.isfinite(e)]
        for k in range(N_COLS):
            if not np.isfinite(x[i, k]):
                out["ref"][i, k] = np.nan
                out["dropped"][i, k] = exists[i, k]
                continue
            z = (mp.mpf(float(x[i, k])) - mp.mpf(loc)) / mp.mpf(scale)
            if abs(z) > mp.mpf(10) ** 150 or any(z != e and abs(z - e) <= mp.mpf(2) ** -50 * abs(e) for e in edges):
                out["dropped"][i, k] = True
                out["ref"][i, k] = np.nan
                continue
            if not _inside(name, shapes, z):
                out["ref"][i, k] = -np.inf
                continue
            out["ref"][i, k] = float(_logpdf_z(mp, name, s, z) - mp.log(mp.mpf(scale)))
            out["mag"][i, k] = float(abs(c) + sum(abs(p) for p in _pieces(mp, name, s, z)))
            zs = [z * (1 + sg * mp.mpf(EPS)) for sg in (1, -1)]
            zs = [min(max(v, mp.mpf(lo)), mp.mpf(hi)) if any(z == e for e in edges) else v for v in zs]
            out["cond"][i, k] = float(abs(_logpdf_z(mp, name, s, zs[0]) - _logpdf_z(mp, name, s, zs[1])))
            if name == "weibull_min":
                out["allow"][i, k] = float(mp.mpf(EPS) * (abs(s[0] * mp.log(z)) + 1) * z ** s[0])
        assert not out["dropped"][i, REST] and np.isfinite(out["ref"][i, REST]), (i, name, shapes)
    return out


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def encode_rows(rows):
    """the rows as arrays: family names, the two shape slots (NaN: none), loc, scale"""
    shapes = np.full((len(rows), 2), np.nan)
    for i, r in enumerate(rows):
        shapes[i, :len(r[1])] = r[1]
    return dict(families=np.array([r[0] for r in rows]), shapes=shapes, loc=np.array([r[2] for r in rows]), scale=np.array([r[3] for r in rows]))


def decode_rows(g):
    return [(str(n), tuple(float(v) for v in g["shapes"][i] if not np.isnan(v)), float(g["loc"][i]), float(g["scale"][i]))
            for i, n in enumerate(g["families"])]


def build_fixture():
    rows = grid_rows()
    x = place_points(rows)
    fx = dict(encode_rows(rows), x=x, **reference(rows, x))
    return fx


def fixture_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN_NAME + ".npz")


def tolerance(g):
    """[128, 14] the bar of the module's docstring at every point (0 where the reference is not finite)"""
    return 1e-11 * np.maximum(1.0, g["mag"]) + g["cond"] + g["allow"]


def kept_probes(g):
    """[(row, column)] of the probes that are compared, in row order"""
    keep = probe_exists(decode_rows(g)) & ~g["dropped"]
    return [(int(i), int(k)) for i, k in zip(*np.nonzero(keep))]


def assert_drop_caps(g):
    exists = probe_exists(decode_rows(g))
    dropped = g["dropped"] & exists
    print("probes %d, dropped %d (%.2f %%), fewest kept in a row %d" % (exists.sum(), dropped.sum(), 100.0 * dropped.sum() / exists.sum(),
                                                                        (exists & ~dropped).sum(axis=1).min()))
    assert dropped.sum() <= DROP_SHARE * exists.sum(), (dropped.sum(), exists.sum())
    assert np.all((exists & ~dropped).sum(axis=1) >= KEEP_PER_ROW), np.nonzero((exists & ~dropped).sum(axis=1) < KEEP_PER_ROW)
