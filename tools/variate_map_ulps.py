#!/usr/bin/env python3
"""The measured accuracy of the engine's variate map (csrc/tda_philox.h: tda_log_unit, tda_sincos_turn, normal_pair) against the
exact reference of tests/extvariate.py, written as JSON.  One run of what tests/test_gpu_variate_map.py runs:

  device.text     the header's text under hiprtc at the chosen inputs: worst error of ln, sin, cos in ulps and of a normal in units
                  of 2^-52 relative, whether sqrt was the correctly rounded root everywhere, and how many of the device's values
                  differ from the host build's of the same branch
  device.stream   per case (kernel, dimension, chain offset), every normal the library exported on the real stream: worst relative
                  error in units of 2^-52
  host            tests/variate_math_main.cpp, the same branch compiled for the host, at the chosen inputs and at random pairs

    python tools/variate_map_ulps.py --out profiles/variate_map_ulps.json
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--random", type=int, default=2_000_000, help="random pairs of the host build")
    args = ap.parse_args()

    import torch

    from tests import extvariate as xv
    from tests import test_gpu_variate_map as gv

    prop = torch.cuda.get_device_properties(0)
    res = {"device_name": prop.name, "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "reference": "np.longdouble, %d-bit significand" % (np.finfo(xv.LD).nmant + 1),
           "units": {"ln": "ulp", "sin": "ulp", "cos": "ulp", "z": "2^-52 relative"},
           "bounds": {"ln": xv.LN_ULPS, "sin": xv.SINCOS_ULPS, "cos": xv.SINCOS_ULPS, "z": xv.Z_REL}}

    u1, u2, got, (root, arg) = gv.device_probe()
    text = xv.map_errors(got, u1, u2)
    text["points"] = int(len(u1))
    text["sqrt_not_correctly_rounded"] = int((root != np.sqrt(arg)).sum())
    res["device"] = {"text": text, "stream": {}}

    with tempfile.TemporaryDirectory() as work:
        exe, why = xv.build_shim(work)
        host = xv.shim_map(exe, u1, u2)
        text["differs_from_host_build"] = {name: int((a != b).sum()) for name, a, b in zip(("ln", "sin", "cos", "z0", "z1"), got, host)}
        res["host"] = {"chosen": dict(xv.map_errors(host, u1, u2), points=int(len(u1)))}
        r1, r2 = xv.random_pairs(args.random, 20261020)
        res["host"]["random"] = dict(xv.map_errors(xv.shim_map(exe, r1, r2), r1, r2), points=int(args.random))

    for name in gv.CASES:
        worst, n = gv.stream_case(name)
        res["device"]["stream"][name] = {"z": worst, "normals": n}
    res["device"]["stream_worst_z"] = max(v["z"] for v in res["device"]["stream"].values())

    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
