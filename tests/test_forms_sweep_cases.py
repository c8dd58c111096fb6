"""The combined-forms sweep without a GPU (tests/extforms.py; tests/test_gpu_forms_sweep.py runs it): what the list of cases covers,
the admission of every case on the engine's own variates at the stored step sizes of tests/golden/forms_sweep.json (verified
here, chosen by tests/golden/gen_forms_sweep.py), and every distinct program of the list compiled offline for gfx950 under the
MALA, HMC and maximize switch sets, with its scratch memory and spilled registers printed (not asserted: a combination may take
scratch memory that none of its forms takes alone)."""
import itertools
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np
import pytest

from oracle import tinyda_oracle as orc

from . import extforms as xf
from . import exthmc as xh
from . import extoptimize as xo
from .extengine import assert_rate
from .extprogram import MALA_KERNELS, compile_program, needs_hipcc
from .golden import gen_forms_sweep as gen

CASES = [xf.form_case(i) for i in range(xf.N_FORMS)]
IDS = [c["name"] for c in CASES]
SWITCH_SETS = {"mala": (["TDA_USER_MALA"], MALA_KERNELS), "hmc": (["TDA_USER_MALA", "TDA_USER_HMC"], ("tda_user_hmc_steps", "tda_user_mala_grad0")),
               "maximize": (["TDA_USER_MALA", "TDA_USER_MAP"], ("tda_user_maximize",))}


@lru_cache(maxsize=2)
def _built(i):
    row = xf.stored()[i]
    return xf.build(CASES[i], seed=row["seed"]), row


# ---- 1. what the list covers ----------------------------------------------------------------------------------------------------------
def test_the_list_has_its_shape():
    assert len(CASES) == xf.N_FORMS == 24 and len({c["name"] for c in CASES}) == 24 and len(xf.FIXED) <= 24
    for c in CASES:
        assert c["d"] in xf.D_VALUES and c["m"] in xf.M_VALUES and c["block_steps"] in (0, 7, 16), c
        T_mala, T_hmc, L = xf.budget(c)
        assert T_mala <= xf.MAX_EVALUATIONS and T_hmc * L <= xf.MAX_EVALUATIONS
    for key in ("adaptive", "mass", "resume", "ml"):
        assert {c[key] for c in CASES} == {False, True}, key
    assert {c["block_steps"] for c in CASES} == {0, 7, 16} and {c["thin"] for c in CASES} == {1, 3}
    for kinds, key in ((xf.MODELS, "model"), (xf.LIKELIHOODS, "like"), (xf.PRIORS, "prior")):  # every kind of every axis at least once
        assert {c[key] for c in CASES} == set(kinds), key


def test_every_pair_of_forms_from_two_axes_occurs():
    values = {"forward": ("per_output", "wave"), "gradient": ("per_parameter", "wave"), "likelihood": ("iso", "diag", "term", "wave"),
              "prior": ("gauss", "term", "wave")}
    seen = set()
    for c in CASES:
        f = xf.forms_of(c)
        seen |= {((a, f[a]), (b, f[b])) for a, b in itertools.combinations(xf.AXES, 2)}
    want = {((a, va), (b, vb)) for a, b in itertools.combinations(xf.AXES, 2) for va in values[a] for vb in values[b]}
    assert want <= seen, sorted(want - seen)


def test_forms_at_the_boundary_shapes():
    forms = [(xf.forms_of(c), c) for c in CASES]
    for axis in xf.AXES:  # every non-default form at d = 64 and at some d >= 65
        for form in {f[axis] for f, _ in forms} - {xf.DEFAULT_FORMS[axis]}:
            ds = {c["d"] for f, c in forms if f[axis] == form}
            assert 64 in ds and max(ds) >= 65, (axis, form, ds)
    for form in ("iso", "diag", "term", "wave"):  # every likelihood form at m = 64, m = 65 and one m >= 1000
        ms = {c["m"] for f, c in forms if f["likelihood"] == form}
        assert 64 in ms and 65 in ms and max(ms) >= 1000, (form, ms)
    assert any(c["d"] == 128 for f, c in forms if set(f.values()) == {"wave"})  # the all-wave program
    assert any(f["gradient"] == "wave" and c["mass"] and c["d"] >= 65 for f, c in forms)
    assert any(c["resume"] and f["prior"] == "wave" for f, c in forms)  # (one case runs under MALA and under HMC: both resume there)
    assert any(f["likelihood"] == "wave" and f["prior"] == "wave" and c["m"] > 64 and c["m"] % 64 for f, c in forms)


@pytest.mark.parametrize("i", range(xf.N_FORMS), ids=IDS)
def test_the_lowering_pass_takes_every_case(i):
    import tinyda_amd as tda
    from tinyda_amd import api

    c, row = _built(i)
    post = xf.posterior(c)
    for kind, cls in (("mala", tda.MALA), ("hmc", tda.HMC)):
        prop, _ = xf.proposal(c, kind, row[kind + "_scaling"])
        kw = dict(adaptive=prop["adaptive"], gamma=prop["gamma"], period=prop["period"])
        if kind == "hmc":
            kw.update(n_leapfrog=prop["n_leapfrog"], inv_mass=prop["inv_mass"])
        plan = api._device_plan([post], cls(prop["scaling"], **kw), False, None, False)
        assert plan is not None, (kind, api._refusal[0])
        assert plan[0][0]["has_gradient"]


# ---- 2. admission, on the engine's own variates ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(xf.N_FORMS), ids=IDS)
def test_stored_step_sizes_are_admissible(i):
    """the stored values follow the rule (the start of the case's forms, halved at most six times) and are admissible: HMC by
    exthmc.assert_admissible, MALA by the oracle's acceptance rate and by the same one-ulp rule on the twin with one leapfrog step"""
    c, row = _built(i)
    assert row["name"] == c["name"] and row["start"] == gen.start_of(c)
    for kind in ("mala", "hmc"):
        k = row[kind + "_halvings"]
        assert 0 <= k <= gen.HALVINGS and row[kind + "_scaling"] == row["start"] / 2 ** k
    prop, T = xf.proposal(c, "hmc", row["hmc_scaling"])
    z, u = xh.philox_variates(xf.SEED, xf.CHAIN_OFFSET, c["N"], T, c["d"])
    assert c["N"] <= xf.MAX_CHAINS and c["theta0"].shape == (c["N"], c["d"])
    xh.assert_admissible(c["level"], prop, c["theta0"], z, u, state_share=xf.STATE_SHARE)
    prop, T = xf.proposal(c, "mala", row["mala_scaling"])
    z, u = xh.philox_variates(xf.SEED, xf.CHAIN_OFFSET, c["N"], T, c["d"])
    with np.errstate(all="ignore"):
        ref = orc.run_mh(c["level"], prop, c["theta0"], z, u)
    assert_rate(ref["accepted"][:, 1:])
    assert np.all(np.isfinite(ref["logpost"]))
    one = xh.assert_admissible(c["level"], xf.mala_as_hmc(prop), c["theta0"], z, u, state_share=xf.STATE_SHARE)
    assert np.array_equal(one["accepted"], ref["accepted"])  # (the twin with one leapfrog step is the oracle's MALA)


@pytest.mark.parametrize("i", range(xf.N_FORMS), ids=IDS)
def test_every_start_of_the_twin_converges(i):
    case = xf.maximize_case(xf.build_for_maximize(CASES[i], seed=xf.stored()[i]["seed"]))
    c = CASES[i]
    res = xo.run_twin(case)
    print([(r["status"], r["iterations"], r["evaluations"]) for r in res])
    assert all(r["status"] == xo.CONVERGED_GRADIENT for r in res), [r["status"] for r in res]
    f = xf.forms_of(c)
    if i == xf.WRAPPED_RING_CASE:  # a wave gradient at d >= 64 whose ring of pairs wraps
        assert f["gradient"] == "wave" and c["d"] >= 64 and min(r["iterations"] for r in res) > xo.HISTORY


# ---- 3. every distinct program, compiled offline -------------------------------------------------------------------------------------
def _lds(log, kernel):
    """the static LDS of a kernel from the compiler's resource remarks"""
    import re

    at = log.index("Function Name: " + kernel)
    return int(re.search(r"LDS Size \[bytes/block\]: (\d+)", log[at:]).group(1))


@needs_hipcc
def test_every_program_of_the_list_compiles(tmp_path):
    """... and holds exactly its kernels, whose static LDS and the dynamic LDS of each case that runs the program (8 m bytes, twice
    that under a likelihood that couples outputs) fit the 64 KiB the engine admits"""
    programs, users = {}, {}
    for i in range(xf.N_FORMS):
        c, _ = _built(i)
        key = (c["source"], tuple(xf.switches_of(c)))
        programs.setdefault(key, c["name"])
        users.setdefault(key, []).append(c)
    jobs = [(key, build) for key in programs for build in SWITCH_SETS]

    def one(job):
        (src, sw), build = job
        return compile_program(tmp_path, programs[job[0]] + "_" + build, src, SWITCH_SETS[build][0] + list(sw))

    with ThreadPoolExecutor(max_workers=8) as pool:
        results = list(pool.map(one, jobs))
    print("\n%-48s %-9s %-22s %6s %8s %6s %6s" % ("program", "build", "kernel", "VGPRs", "scratch", "spill", "LDS"))
    for (key, build), (rc, log, usage) in zip(jobs, results):
        name = programs[key]
        assert rc == 0, (name, build, log[-3000:])
        assert set(usage) == set(SWITCH_SETS[build][1]), (name, build, set(usage))
        for kernel, use in sorted(usage.items()):
            lds = _lds(log, kernel)
            if kernel != "tda_user_mala_grad0":
                print("%-48s %-9s %-22s %6d %8d %6d %6d" % (name, build, kernel, use["VGPRs"], use["ScratchSize [bytes/lane]"], use["VGPRs Spill"], lds))
            for c in users[key]:
                m = xf.MAXIMIZE_M.get(c["i"], c["m"]) if build == "maximize" else c["m"]
                assert lds + (2 if xf.forms_of(c)["likelihood"] == "wave" else 1) * 8 * m <= 64 * 1024, (c["name"], build, kernel, lds)
        if name == CASES[0]["name"] and build == "maximize":  # the figure that the LDS edge of tests/test_gpu_forms_sweep.py is computed from
            assert _lds(log, "tda_user_maximize") == xf.MAP_STATIC_LDS
