"""Generate g25_map.npz by RUNNING THE REFERENCE's own get_MAP / get_ML (tinyDA/utils.py:204-269: scipy.optimize.minimize, BFGS
with a finite-difference gradient, over posterior.create_link) on the NumPy twins of the three posteriors of
tests/extoptimize.fixture_posteriors, from their fixed starts.  Only data is stored: per posterior the starts, the reference's
points and its log-prior and log-likelihood there; for the first posterior also get_ML's.

Run in the build container only (needs the reference, like gen_golden.py):

    python tests/golden/gen_golden_map.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _refload import load_reference  # noqa: E402
from tests import extoptimize as xo  # noqa: E402


def main():
    ref = load_reference()
    np.random.seed(25)  # (get_MAP draws a start from the prior even when one is given)
    out = {}
    for name, case in xo.fixture_posteriors().items():
        mine = case["posterior"]
        post = ref.Posterior(mine.prior, mine.likelihood, mine.model)  # the host twins behind `reference=`
        rows = []
        for x0 in case["starts"]:
            x = np.asarray(ref.get_MAP(post, initial_parameters=x0), dtype=float)
            link = post.create_link(x)
            rows.append((x, link.prior, link.likelihood))
            print(name, "MAP", x, link.prior, link.likelihood)
        out[name + "_starts"] = case["starts"]
        out[name + "_x"] = np.array([r[0] for r in rows])
        out[name + "_logprior"] = np.array([r[1] for r in rows], dtype=float)
        out[name + "_loglike"] = np.array([r[2] for r in rows], dtype=float)
        if name == "extmodel":
            rows = []
            for x0 in case["starts"]:
                x = np.asarray(ref.get_ML(post, initial_parameters=x0), dtype=float)
                rows.append((x, post.create_link(x).likelihood))
                print(name, "ML", x, rows[-1][1])
            out[name + "_ml_x"] = np.array([r[0] for r in rows])
            out[name + "_ml_loglike"] = np.array([r[1] for r in rows], dtype=float)
    np.savez(os.path.join(HERE, "g25_map.npz"), **out)


if __name__ == "__main__":
    main()
