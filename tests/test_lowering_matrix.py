"""The lowering pass against the recorded matrix of its decisions (tests/golden/lowering_matrix.json, written by
tests/golden/gen_lowering_matrix.py at the commit named in the file): for every case the same decision, the same first refusal
reason to the letter, and for lowered cases the same proposal description and per level the same keys, noise_kind, array shapes
and prior_source sub-dict.  And the reason of a refusal reaches the caller of sample() that was refused, whatever other threads
are doing."""
import importlib.util
import json
import os
import sys
import threading

import numpy as np
import pytest
import scipy.stats as st

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_lowering_matrix", os.path.join(GOLDEN, "gen_lowering_matrix.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

UNREACHABLE = {
    # with a dense error model every level below the finest needs an AdaptiveGaussianLogLike ("dense error model: levels below"),
    # and an adaptive likelihood with more than MAX_AEM_OUTPUTS = MAX_AEM_OUTPUTS_HOST_SEQUENCED = 256 outputs is refused while
    # its level is read ("adaptive likelihood: hierarchy, outputs"): the rule waits for the two limits to differ again
    "dense error model: more than 256 outputs",
}


@pytest.fixture(scope="module")
def matrix():
    return gen.load()


def test_every_recorded_decision(matrix):
    cases = gen.cases()
    assert len(cases) == matrix["n_cases"] == len(matrix["cases"]) and gen.names_digest([c[0] for c in cases]) == matrix["names"]
    wrong = []
    for (name, levels, prop, em, rnd), pick in zip(cases, matrix["cases"]):
        got, want = gen.outcome(levels, prop, em, rnd), matrix["outcomes"][pick]
        if isinstance(got, dict):
            got = json.loads(json.dumps(got))
        if got != want:
            wrong.append((name, got, want))
    assert not wrong, "%d of %d cases differ, the first: %r" % (len(wrong), len(cases), wrong[0])


def test_every_refusal_site_is_the_first_reason_of_a_case(matrix):
    reached = {gen.site_of(o) for o in (matrix["outcomes"][i] for i in set(matrix["cases"])) if isinstance(o, str)}
    assert {name for name, _ in gen.SITES} - reached == UNREACHABLE


def test_concurrent_refusals_keep_their_own_reason():
    """two threads, two problems refused by the pass for different reasons, a barrier before each call: each EngineError carries
    the reason of its own problem (a reason kept in a module global is cleared or overwritten by the other thread)"""
    import tinyda_amd as tda
    from tinyda_amd._lib import EngineError

    d, rounds = 4, 500
    lin = tda.Posterior(st.multivariate_normal(np.zeros(d), np.eye(d)), tda.GaussianLogLike(np.zeros(3), 0.04 * np.eye(3)), tda.LinearModel(np.ones((3, d))))
    # both are refused by late rules of the pass, so each call spends its time between the pass's start and its reason
    problems = [([lin], tda.DREAMZ(M0=10, Z_method="sobol"), "an option of DREAMZ the engine does not implement"),
                ([lin, lin], tda.MALA(0.05), "MALA: single level, linear model, Gaussian prior")]
    barrier = threading.Barrier(2)
    seen = [[], []]

    def work(k):
        posts, prop, _ = problems[k]
        for _ in range(rounds):
            barrier.wait()
            try:
                tda.sample(posts, prop, 5, backend="hip")
                seen[k].append("no error")
            except EngineError as exc:
                seen[k].append(str(exc))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    interval = sys.getswitchinterval()
    sys.setswitchinterval(1e-6)  # (the interpreter's default of 5 ms lets a whole call pass between two switches)
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        sys.setswitchinterval(interval)
    for k, (_, _, reason) in enumerate(problems):
        assert len(seen[k]) == rounds
        stray = [s for s in seen[k] if s != "this posterior / proposal combination cannot be lowered to the HIP engine: " + reason]
        assert not stray, "%d of %d calls of thread %d: %s" % (len(stray), rounds, k, stray[0])
