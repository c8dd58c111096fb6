"""Generate forms_sweep.json: the step sizes of the combined-forms sweep (tests/extforms.py), chosen on the CPU with the twins alone.

The rule.  A case starts from the smallest of the step sizes that tests/exthmc.py holds for the forms it combines (START below
names them), and halves it up to six times until the case is admissible on the engine's own variates (the oracle's Philox stream):

    HMC    exthmc.assert_admissible: one ulp on every gradient moves no mask, the log-posteriors by 1e-11 at most and the states
           by extforms.STATE_SHARE of their bar at most, and the twin accepts between 10 % and 90 % of its proposals
    MALA   the oracle accepts between 10 % and 90 % of its proposals (extengine.assert_rate), and the same one-ulp rule holds for
           the twin with one leapfrog step under unit mass, which is MALA (tests/test_hmc.py ties the two): a drift theta + eps^2 / 2
           g(theta) with eps^2 / 2 times the curvature above 1 amplifies last-bit differences as an unstable leapfrog map does

A case for which no halving is admissible takes the next seed of its problem (at most MAX_SEEDS).  Only data is stored: per case
its name, the seed, the two step sizes and the halvings they took.  tests/test_forms_sweep_cases.py verifies every stored value
again and never chooses.

    python tests/golden/gen_forms_sweep.py [first case [last case]]     # writes the file (with a range: those rows of it)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import tinyda_oracle as orc  # noqa: E402
from tests import extforms as xf  # noqa: E402
from tests import exthmc as xh  # noqa: E402

HALVINGS, MAX_SEEDS = 6, 3
# the step sizes of exthmc's cases, per form: FORWARD_CASES for extmodel under Gaussian parts (one parameter: 0.3; more: the 0.06 of
# d = 5, the largest, since the halvings lead downwards to the 0.03 .. 0.004 of its larger cases and never upwards), _ring, _student_t,
# _ar1_wave, _cauchy_difference.  exthmc has no case of its own for the other kinds: they start from the model's value.
# (_lognormal_edge's 0.004 belongs to starts at 0.03, a tenth of the ones here, and is scaled by that: 0.04.)
START_EXTMODEL = ((1, 0.3), (128, 0.06))
START = {"ring": 0.12, "t": 0.075, "ar1": 0.1, "cauchy": 0.025, "lognormal": 0.04}


def start_of(c):
    values = [START["ring"] if c["model"] != "extmodel" else next(v for dmax, v in START_EXTMODEL if c["d"] <= dmax)]
    values += [START[k] for k in (c["like"], c["prior"]) if k in START]
    return min(values)


def variates(c, T):
    return xh.philox_variates(xf.SEED, xf.CHAIN_OFFSET, c["N"], T, c["d"])


def mala_admissible(c, scaling):
    prop, T = xf.proposal(c, "mala", scaling)
    z, u = variates(c, T)
    with np.errstate(all="ignore"):
        ref = orc.run_mh(c["level"], prop, c["theta0"], z, u)
    rate = float(ref["accepted"][:, 1:].mean())
    if not 0.1 <= rate <= 0.9:
        return False, "rate %.3f" % rate
    try:
        xh.assert_admissible(c["level"], xf.mala_as_hmc(prop), c["theta0"], z, u, state_share=xf.STATE_SHARE)
    except AssertionError as exc:
        return False, "rate %.3f, one ulp: %s" % (rate, str(exc)[:40])
    return True, "rate %.3f" % rate


def hmc_admissible(c, scaling):
    prop, T = xf.proposal(c, "hmc", scaling)
    z, u = variates(c, T)
    try:
        xh.assert_admissible(c["level"], prop, c["theta0"], z, u, state_share=xf.STATE_SHARE)
    except AssertionError as exc:
        return False, str(exc)[:60]
    return True, ""


def choose(c):
    """-> (halvings of MALA, halvings of HMC), None where none is admissible"""
    s0, out = start_of(c), []
    for kind in ("mala", "hmc"):
        found = None
        for k in range(HALVINGS + 1):
            ok, why = (mala_admissible if kind == "mala" else hmc_admissible)(c, s0 / 2 ** k)
            print("  %s %s %-4s %.6g: %s %s" % (c["name"], "ok " if ok else "-- ", kind, s0 / 2 ** k, why, ""), flush=True)
            if ok:
                found = k
                break
        out.append(found)
    return s0, out


def main(first=0, last=xf.N_FORMS):
    rows = []
    for i in range(first, last):
        case = xf.form_case(i)
        for attempt in range(MAX_SEEDS):
            seed = 1000 * case["d"] + case["m"] + 7 * i + 100000 * attempt
            c = xf.build(case, seed=seed)
            s0, (km, kh) = choose(c)
            if km is not None and kh is not None:
                break
        else:
            raise SystemExit("%s: no admissible step size" % case["name"])
        rows.append(dict(name=case["name"], seed=seed, start=s0, mala_halvings=km, hmc_halvings=kh, mala_scaling=s0 / 2 ** km, hmc_scaling=s0 / 2 ** kh))
        print(rows[-1], flush=True)
    if (first, last) != (0, xf.N_FORMS):  # a range: the other rows stay as the file has them
        rows = xf.stored()[:first] + rows + xf.stored()[last:]
    with open(xf.GOLDEN, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:]])
