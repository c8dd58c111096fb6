"""Largest relative deviation of the device's bulk ESS / R-hat (tda_diag_ess_rhat) from oracle/ess_oracle.py over the parameters of
every case of tests/extdiag.py -- the figures tests/test_gpu_diag.py prints before it asserts -- as one record.

    python tools/diag_parity.py [OUT.json]        (default: profiles/diag_parity.json)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from tests import extdiag
from tinyda_amd import summaries as sm


def run(x, burnin=0):
    dev = torch.tensor(np.ascontiguousarray(x if x.ndim == 3 else x[:, :, None]), dtype=torch.float64, device="cuda")
    return sm.ess_rhat_device(dev, burnin=burnin)


cases = {}
for name, (T, N, d, burnin) in extdiag.SHAPES.items():
    out = run(extdiag.shape_history(name), burnin)
    ess, rhat = extdiag.reference(name)
    cases[name] = dict(kind="shape", draws=T, chains=N, dim=d, burnin=burnin, ess_max_rel=extdiag.deviation(out["ess"], ess),
                       rhat_max_rel=extdiag.deviation(out["rhat"], rhat))
    print(name, cases[name], flush=True)
for name in extdiag.EDGES:
    x = extdiag.nan_replaced() if name == "nan_one_parameter" else extdiag.edges()[name]
    out = run(x)
    ess, rhat = extdiag.reference(name)
    cases[name] = dict(kind="edge", draws=x.shape[0], chains=x.shape[1], dim=1 if x.ndim == 2 else x.shape[2], burnin=0,
                       ess_max_rel=extdiag.deviation(out["ess"], ess), rhat_max_rel=extdiag.deviation(out["rhat"], rhat))
    if name == "all_constant":
        cases[name]["note"] = "device and oracle both NaN"
    if name == "nan_one_parameter":
        cases[name]["note"] = "the NaN replaced by a finite draw; with the NaN, parameter 1 is NaN on the device and in the NumPy twin"
    print(name, cases[name], flush=True)
rec = dict(what="tda_diag_ess_rhat against oracle/ess_oracle.py: largest relative deviation over the parameters of every case of tests/extdiag.py",
           device=torch.cuda.get_device_name(0), tolerance=dict(ess_rtol=1e-8, rhat_rtol=1e-10), cases=cases,
           reproduce="python tools/diag_parity.py; python -m pytest tests/test_gpu_diag.py -m gpu -s prints the same figures case by case")
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "diag_parity.json")
with open(dest, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print("worst ess %.2e rhat %.2e" % (max(c["ess_max_rel"] for c in cases.values()), max(c["rhat_max_rel"] for c in cases.values())))
