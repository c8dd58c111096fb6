"""Generate g22_prior_family_grads.npz: at the in-support points of g21_prior_family_terms.npz (the rest points and the kept
probes of the 128 table rows of tests/extfamilies.py) the derivative of the log-density, g'(z) / scale, in mpmath at 80
digits, with the magnitudes, the conditioning and the Weibull allowance that the bound of tests/extpriorgrad.py is made of.
The points and rows are g21's and are not stored again.  tests/test_prior_source_mala.py recomputes the arrays and compares
exactly; the GPU tests read only the two files.

Needs mpmath:

    python tests/golden/gen_golden_prior_family_grads.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import extfamilies as xf  # noqa: E402
from tests import extpriorgrad as xg  # noqa: E402

if __name__ == "__main__":
    fx = xg.reference(np.load(xf.fixture_path(), allow_pickle=False))
    np.savez_compressed(xg.fixture_path(), **fx)
    print("wrote %s (%d bytes), %d points" % (xg.fixture_path(), os.path.getsize(xg.fixture_path()), fx["inside"].sum()))
