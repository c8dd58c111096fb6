"""Generate g21_prior_family_terms.npz: the 128 table rows of tests/extfamilies.py (13 scipy.stats families over a grid of
shapes), their probe points from far in one tail to far in the other, and for every point the reference log-density in
mpmath at 80 digits, the magnitude and conditioning that the tolerance is made of, and the mask of dropped probes.  The
GPU tests read only this file; tests/test_prior_families.py recomputes it from the stored points and compares exactly.

Needs scipy (to place the points) and mpmath:

    python tests/golden/gen_golden_prior_families.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import extfamilies as xf  # noqa: E402

if __name__ == "__main__":
    fx = xf.build_fixture()
    xf.assert_drop_caps(fx)
    np.savez_compressed(xf.fixture_path(), **fx)
    print("wrote %s (%d bytes)" % (xf.fixture_path(), os.path.getsize(xf.fixture_path())))
