"""What the engine-against-oracle tests share: proposals from the oracle's description, the forward-mode run (the engine on
its own Philox stream, its variates exported for the oracle), the comparators that state the project's parity bar, the
oracle's side of a hierarchy's uniforms, and the checkpoint-resume checks.  Plain functions; the engine is whatever object
the caller built."""
import numpy as np

from oracle import tinyda_oracle as orc

PROP_KIND = {"grw": 0, "pcn": 1, "am": 2, "mala": 6}
NOISE_SOURCE, PRIOR_SOURCE = 4, 2  # the noise kind of a source-defined likelihood, the prior kind of a source-defined prior


def set_proposal(e, prop):
    """the oracle's description of a proposal (run_mh's dict), set on the engine"""
    kw = {k: v for k, v in prop.items() if k not in ("kind", "C", "C0")}
    e.set_proposal(PROP_KIND[prop["kind"]], prop.get("C", prop.get("C0")), **kw)


def golden_proposal(g):
    """the oracle's description of the proposal of a recorded reference chain (tests/golden/g18 .. g23)"""
    if "C0" in g.files:
        return dict(kind="am", C0=g["C0"], sd=float(g["sd"]), epsilon=float(g["epsilon"]), t0=int(g["t0"]), period=int(g["period"]))
    return dict(kind="grw", C=g["C"], scaling=float(g["scaling0"]), adaptive=bool(g["adaptive"]), gamma=float(g["gamma"]), period=int(g["period"]))


def assert_host_classes_replay(g, post, monkeypatch):
    """the package's host classes over the recorded variates of a reference chain: every accept decision, the log-posterior of
    every state, the adapted scaling (GaussianRandomWalk) or covariance (AdaptiveMetropolis) at the end"""
    import tinyda_amd as tda

    kw = {k: v for k, v in golden_proposal(g).items() if k != "kind"}
    for c in range(g["theta0"].shape[0]):
        prop = tda.AdaptiveMetropolis(**kw) if "C0" in kw else tda.GaussianRandomWalk(**kw)
        prop.setup_proposal(parameters=g["theta0"][c], posterior=post)
        zs = iter(g["z"][c])
        monkeypatch.setattr(np.random, "standard_normal", lambda n: next(zs))
        link = post.create_link(g["theta0"][c])
        np.testing.assert_allclose(link.posterior, g["logpost"][c, 0], rtol=1e-10)
        accepted = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for s in range(g["z"].shape[1]):
                cand = post.create_link(prop.make_proposal(link))
                acc = g["u"][c, s] < prop.get_acceptance(cand, link)
                if acc:
                    link = cand
                accepted.append(acc)
                prop.adapt(parameters=link.parameters, accepted=accepted)
                assert acc == bool(g["accepted"][c, s + 1]), (c, s)
                np.testing.assert_allclose(link.posterior, g["logpost"][c, s + 1], rtol=1e-10)
        if "C0" in kw:
            np.testing.assert_allclose(prop.C, g["C_hist"][c, -1], rtol=1e-9, atol=1e-14)
        else:
            np.testing.assert_allclose(prop.scaling, g["scaling_hist"][c, -1], rtol=1e-12)


def assert_oracle_replays(g, level):
    """the oracle over `level` on the recorded variates of a reference chain; -> its result"""
    ref = orc.run_mh(level, golden_proposal(g), g["theta0"], g["z"], g["u"])
    assert np.array_equal(ref["accepted"], g["accepted"])
    np.testing.assert_allclose(ref["logpost"], g["logpost"], rtol=1e-10)
    np.testing.assert_allclose(ref["theta"], g["theta"], rtol=1e-9, atol=1e-12)
    if "C0" in g.files:
        np.testing.assert_allclose(ref["C"], g["C_hist"][:, -1], rtol=1e-9, atol=1e-14)
    else:
        np.testing.assert_allclose(ref["scaling"], g["scaling_hist"][:, -1], rtol=1e-12)
    assert 0.1 <= g["accepted"][:, 1:].mean() <= 0.9
    return ref


def assert_rate(accepted):
    """agreement of accept masks says something only where the oracle neither accepts nor rejects nearly everything"""
    rate = accepted.mean()
    print("oracle acceptance rate %.3f" % rate)
    assert 0.1 <= rate <= 0.9, rate


# ---- single level ---------------------------------------------------------------------------------------------------------------
def run_forward(e, theta0, T, prop):
    """T steps on the engine's own Philox stream; closes the engine.  -> params, stats, acc, the final scaling, the final
    covariance (None unless AdaptiveMetropolis), and the exported normals z[T, N, d] and uniforms u[T, N]"""
    e.init(theta0)
    z, u = e.set_export(T)
    params, stats, acc = e.run_host(T)
    scal = e.proposal_state_scaling()
    C = e.proposal_state(want_am=True)["C"] if prop["kind"] == "am" else None
    e.close()
    return params, stats, acc, scal, C, z, u


def assert_logprior(got, want, theta, prior):
    """the log-prior is a sum of up to 128 terms of either sign that may cancel (it passes through zero along a chain), so
    its error is measured against the sum of the terms' magnitudes at the oracle's states: 1e-10 of that, as the log-posterior
    is held to 1e-10 of itself"""
    mag = prior.magnitude(theta.reshape(-1, theta.shape[-1])).reshape(want.shape)
    err = np.abs(got - want)
    print("log-prior: max error / magnitude %.2e" % np.max(err / mag))
    assert np.all(err <= 1e-10 * mag), np.max(err / mag)


def compare(params, stats, acc, ref, scal=None, prior=None, span_form=False):
    """Engine outputs [T, N, ...] against run_mh's traces: masks exact, log-posterior 1e-10, the log-prior by assert_logprior
    where `prior` (with a magnitude()) is given, the final scaling 1e-12 where `scal` is given.

    States are held to 1e-9 of themselves (atol 1e-12).  In the span form a state is held to 1e-9 of the larger of itself and
    the largest magnitude of its component over the oracle's trace instead.  It exists for the cases in which every step adds
    an increment that carries a relative error of its own to the state -- the 128-term proposal sum above 64 parameters, the
    factor of an adapted covariance that is close to singular -- so that a component which passes through zero keeps an
    absolute error in proportion to the distances it has moved over, not to its own value.  The caller says where it applies,
    and why."""
    assert np.array_equal(acc, np.swapaxes(ref["accepted"][:, 1:], 0, 1))
    want = np.swapaxes(ref["theta"][:, 1:], 0, 1)
    if prior is not None:
        assert_logprior(stats[:, :, 0], np.swapaxes(ref["logprior"][:, 1:], 0, 1), want, prior)
    np.testing.assert_allclose(stats[:, :, 2], np.swapaxes(ref["logpost"][:, 1:], 0, 1), rtol=1e-10)
    err = np.abs(params - want)
    print("states: max error / (1e-12 + 1e-9 |state|) %.2e, max error %.2e" % (np.max(err / (1e-12 + 1e-9 * np.abs(want))), np.max(err)))
    if span_form:
        span = np.max(np.abs(ref["theta"]), axis=(0, 1))
        print("states: max error / max(|state|, range of the component) %.2e" % np.max(err / np.maximum(np.abs(want), span)))
        assert np.all(err <= 1e-9 * np.maximum(np.abs(want), span))
    else:
        np.testing.assert_allclose(params, want, rtol=1e-9, atol=1e-12)
    if scal is not None:
        np.testing.assert_allclose(scal, ref["scaling"], rtol=1e-12)


def compare_replay(params, stats, acc, g, *, C=None, scaling=None, logprior=False, loglike=False, params_rtol=1e-9):
    """Engine outputs of a replayed golden trace `g` (the reference's own chains): masks exact, densities 1e-10, states
    `params_rtol` (atol 1e-12), the adapted covariance and the scaling against the last entry of the recorded histories"""
    assert np.array_equal(acc, np.swapaxes(g["accepted"][:, 1:], 0, 1))
    if logprior:
        np.testing.assert_allclose(stats[:, :, 0], np.swapaxes(g["logprior"][:, 1:], 0, 1), rtol=1e-10)
    np.testing.assert_allclose(stats[:, :, 2], np.swapaxes(g["logpost"][:, 1:], 0, 1), rtol=1e-10)
    if loglike:
        np.testing.assert_allclose(stats[:, :, 1], np.swapaxes(g["loglike"][:, 1:], 0, 1), rtol=1e-10)
    np.testing.assert_allclose(params, np.swapaxes(g["theta"][:, 1:], 0, 1), rtol=params_rtol, atol=1e-12)
    if C is not None:
        np.testing.assert_allclose(C, g["C_hist"][:, -1], rtol=1e-9, atol=1e-14)
    if scaling is not None:
        np.testing.assert_allclose(scaling, g["scaling_hist"][:, -1], rtol=1e-12)


# ---- hierarchies ----------------------------------------------------------------------------------------------------------------
def oracle_uniforms(seed, N, rows, sl, randomize_L=None):
    """the uniforms of every level (and the promoted index of a randomised subchain) as the engine's Philox stream draws them"""
    ps = orc.PhiloxStream(seed)
    chains = np.arange(N)
    us = [np.stack([ps.uniform(chains, t, level=k) for t in range(rows[k])], axis=1) for k in range(len(rows))]
    ridx = None
    if randomize_L:
        x0 = np.stack([ps.words(chains.astype(np.uint32), np.uint32(t), np.uint32(3), np.uint32(0))[0] for t in range(rows[1])], axis=1)
        ridx = ((x0.astype(np.uint64) * np.uint64(randomize_L)) >> np.uint64(32)).astype(np.float64) - randomize_L
    return us, ridx


def run_levels_forward(e, n_fine):
    """n_fine fine steps of an initialised hierarchy on its own Philox stream; closes the engine.  -> rows per level, the
    exported normals, the outputs per level, the final scaling"""
    rows = e.rows_per_level(n_fine)
    z, _ = e.set_export(rows[0])
    outs = e.run_levels_host(n_fine)
    scal = e.proposal_state()["scaling"]
    e.close()
    return rows, z, outs, scal


def compare_levels(outs, res, *, states=True, logprior_of=None):
    """run_levels_host's outputs against run_multilevel's traces, level by level (the finest trace carries the initial link):
    masks exact, log-posterior 1e-10, states 1e-9 (atol 1e-12) unless states=False, the log-prior by assert_logprior against
    logprior_of[level] where given"""
    nl = len(res)
    for i, ref in enumerate(res):
        sk = slice(1, None) if i == nl - 1 else slice(None)
        assert np.array_equal(outs[i][2], ref["accepted"][:, sk].T), "level %d accept masks differ" % i
        want = np.swapaxes(ref["theta"][:, sk], 0, 1)
        if logprior_of is not None:
            assert_logprior(outs[i][1][:, :, 0], ref["logprior"][:, sk].T, want, logprior_of[i])
        np.testing.assert_allclose(outs[i][1][:, :, 2], ref["logpost"][:, sk].T, rtol=1e-10)
        if states:
            np.testing.assert_allclose(outs[i][0], want, rtol=1e-9, atol=1e-12)


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------
def assert_resume_bitwise(make, whole=90, first=37):
    """make() -> an initialised engine.  get_state after `first` steps, set_state into a fresh engine: its remaining steps and
    those of the engine that produced the blob both equal the tail of an uninterrupted run"""
    a = make()
    full = a.run_host(whole)
    a.close()
    b = make()
    head = b.run_host(first)
    blob = b.get_state()
    rest_same = b.run_host(whole - first)
    b.close()
    c = make()
    c.set_state(blob)
    rest = c.run_host(whole - first)
    c.close()
    for w, f, r, r2 in zip(full, head, rest, rest_same):
        assert np.array_equal(w, np.concatenate([f, r])), "the resumed engine leaves the uninterrupted run"
        assert np.array_equal(r, r2), "the engine that produced the blob continues differently"


def assert_levels_resume_bitwise(e, first=7, rest=9):
    """an initialised hierarchy: get_state after `first` fine steps, `rest` more, set_state in place, the same `rest` again;
    closes the engine.  -> the outputs of the `rest` steps"""
    e.run_levels_host(first)
    blob = e.get_state()
    a = e.run_levels_host(rest)
    e.set_state(blob)
    b = e.run_levels_host(rest)
    e.close()
    for la, lb in zip(a, b):
        assert all(np.array_equal(x, y) for x, y in zip(la, lb))
    return a
