"""Model outputs and quantities of interest of a result on the device (tda_user_replay behind tinyda_amd/replay.py):
DeviceModel.evaluate against the NumPy twins at every lane and stride edge, the two forms of a quantity of interest, bit-identity
of the ring written per output and in the wave form, the copy-forward of repeated rows on hand-made records (bitwise against the
row-by-row evaluation, with the number of model evaluations counted), chunk invariance, sample() end to end without a host
reference (single level, thinning, burn-in, records moved to the host; Delayed Acceptance with a quantity per level), refusals.

The bar for outputs is the project's parity bar, 1e-10 max(1, |F|) against the twin.  A per-quantity QoI that is one
multiplication and one addition of doubles is compared BITWISE with its twin applied to the device's own outputs (IEEE arithmetic,
no contraction: -ffp-contract=off).  Largest deviations seen on an MI355X are entered in profiles/README.md."""
import numpy as np
import pytest
import scipy.stats as st

from . import extmodel as xm
from . import extqoi as xq
from . import extwave as xw

pytestmark = pytest.mark.gpu

SIGMA = 0.01
ROWS = 37


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def within_bar(got, want, what):
    """|got - want| <= 1e-10 max(1, |want|) entry by entry, NaN where the twin has NaN; prints the largest deviation in units of the bar"""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    dev = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    print("%s: largest deviation %.3e (bar 1e-10)" % (what, dev.max() if dev.size else 0.0))
    assert dev.size == 0 or dev.max() <= 1e-10, (what, dev.max())


def thetas(d, n=ROWS, seed=0, scale=0.5):
    return scale * np.random.default_rng(seed).standard_normal((n, d))


# ---- 1. evaluate against the twins -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(1, 1), (2, 63), (64, 64), (65, 65), (128, 130)])
def test_evaluate_per_output_model(d, m):
    import tinyda_amd as tda

    th = thetas(d, seed=d + m)
    F = tda.DeviceModel(xm.source(), m).evaluate(th)
    assert isinstance(F, np.ndarray) and F.shape == (ROWS, m)
    within_bar(F, xm.np_forward(th, m), "extmodel d=%d m=%d" % (d, m))


@pytest.mark.parametrize("d", [3, 128])
@pytest.mark.parametrize("m", [1, 23, 130])
def test_evaluate_wave_model(d, m):
    import tinyda_amd as tda

    th = thetas(d, seed=d + m)
    F = tda.DeviceModel(xw.source(), m).evaluate(th)
    within_bar(F, xw.np_forward(th, m), "ring d=%d m=%d" % (d, m))


def test_evaluate_of_no_rows_and_nan_outputs():
    import tinyda_amd as tda

    model = tda.DeviceModel(xm.source(nan_above=0.5), 5)
    assert model.evaluate(np.empty((0, 3))).shape == (0, 5)
    th = np.array([[0.1, 0.2, 0.3], [0.9, 0.2, 0.3]])
    F = model.evaluate(th)
    assert not np.isnan(F[0]).any() and np.isnan(F[1]).all()


# ---- 2. the quantity of interest, in both forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_qoi", [1, 3, 65, 130])
def test_per_quantity_form(n_qoi):
    """d = 128, m = 130: quantity k reads parameter 127 - k and output 129 - k, indices >= 64 of both for k < 64"""
    import tinyda_amd as tda

    d, m = 128, 130
    th = thetas(d, seed=n_qoi)
    F, Q = tda.DeviceModel(xm.source() + xq.PER_QUANTITY, m, n_qoi=n_qoi).evaluate(th)
    assert F.shape == (ROWS, m) and Q.shape == (ROWS, n_qoi)
    within_bar(F, xm.np_forward(th, m), "extmodel beside a quantity, n_qoi=%d" % n_qoi)
    assert same_bits(Q, xq.np_per_quantity(th, F, n_qoi))
    within_bar(Q, xq.np_per_quantity(th, xm.np_forward(th, m), n_qoi), "per-quantity form, n_qoi=%d" % n_qoi)


@pytest.mark.parametrize("forward", ["wave", "per_output"])
def test_per_quantity_form_goes_with_either_form_of_the_model(forward):
    import tinyda_amd as tda

    d, m, nq = 5, 23, 7
    th = thetas(d, seed=3)
    F, Q = tda.DeviceModel(xw.source(forward, m=m) + xq.PER_QUANTITY, m, n_qoi=nq).evaluate(th)
    within_bar(F, xw.np_forward(th, m), "ring (%s) beside a quantity" % forward)
    assert same_bits(Q, xq.np_per_quantity(th, F, nq))


def test_wave_form_reads_the_solvers_state_and_leaves_an_entry_nan():
    import tinyda_amd as tda

    d, m = 4, 16
    th = thetas(d, seed=8)
    F, Q = tda.DeviceModel(xw.source() + xq.RING_WAVE, m, n_qoi=xq.RING_WAVE_N).evaluate(th)
    within_bar(F, xw.np_forward(th, m), "ring beside the wave-form quantity")
    assert np.isnan(Q[:, 2]).all() and not np.isnan(Q[:, :2]).any()
    within_bar(Q, xq.np_ring_wave(th, m), "wave-form quantity (sum, maximum, unwritten)")
    # both forms in one source: the wave form is used (the per-quantity form would give theta * f + k / 8)
    Q2 = tda.DeviceModel(xw.source() + xq.PER_QUANTITY + xq.RING_WAVE, m, n_qoi=xq.RING_WAVE_N).evaluate(th)[1]
    assert same_bits(Q2, Q)


def test_ring_per_output_and_wave_form_give_identical_bits():
    import tinyda_amd as tda

    d, m = 5, 23
    th = thetas(d, seed=11)
    wave = tda.DeviceModel(xw.source(), m).evaluate(th)
    per_output = tda.DeviceModel(xw.source("per_output", m=m), m).evaluate(th)
    assert same_bits(wave, per_output)


# ---- 3. the copy-forward ---------------------------------------------------------------------------------------------------------------------
def hand_made_records():
    """[23, 5, 65]: chain 0 runs of 9, 8, 6 equal rows (the first straddles the boundaries of segments of 2 and of 7 rows), chain 1
    runs of 7, 5, 4, 3, 2, 1, 1; chain 2 alternates two states (a row equals the row two before it, not its predecessor); chain 3
    repeats one state whose parameter 3 is a zero that changes its sign at rows 5 and 11; chain 4 repeats one state that changes
    in parameter 64 alone at rows 4, 9 and 17"""
    R, N, d = 23, 5, 65
    rng = np.random.default_rng(2024)
    P = np.empty((R, N, d))
    for c, runs in ((0, (9, 8, 6)), (1, (7, 5, 4, 3, 2, 1, 1))):
        assert sum(runs) == R
        P[:, c] = np.repeat(0.5 * rng.standard_normal((len(runs), d)), runs, axis=0)
    two = 0.5 * rng.standard_normal((2, d))
    P[:, 2] = two[np.arange(R) % 2]
    P[:, 3] = 0.5 * rng.standard_normal(d)
    P[:, 3, 3] = 0.0
    P[5:11, 3, 3] = -0.0
    P[:, 4] = 0.5 * rng.standard_normal(d)
    for r, v in ((4, 0.25), (9, -0.75), (17, 0.25)):
        P[r:, 4, 64] = v
    assert np.signbit(P[5, 3, 3]) and not np.signbit(P[4, 3, 3]) and np.array_equal(P[4, 3], P[5, 3])  # equal as numbers, not as bits
    return P


def evaluations_expected(P, seg):
    """rows that differ bit for bit from their predecessor, plus segment starts"""
    B = bits(P)
    return sum(1 for c in range(P.shape[1]) for r in range(P.shape[0]) if r % seg == 0 or not np.array_equal(B[r, c], B[r - 1, c]))


def test_copy_forward_is_bitwise_the_row_by_row_evaluation():
    import torch

    import tinyda_amd as tda

    P = hand_made_records()
    R, N, d = P.shape
    m, nq = 70, 66
    model = tda.DeviceModel(xm.source() + xq.PER_QUANTITY, m, n_qoi=nq)
    F1, Q1 = model.evaluate(P.reshape(R * N, d))
    F1, Q1 = F1.reshape(R, N, m), Q1.reshape(R, N, nq)
    within_bar(F1.reshape(R * N, m), xm.np_forward(P.reshape(R * N, d), m), "hand-made records")
    dev = torch.from_numpy(P).cuda()
    with tda.Replay(model, d) as rp:
        for seg in (1, 2, 7, 23, 0):
            got = rp.run(dev, segment_rows=seg, count=True)
            assert same_bits(got["model_output"].cpu().numpy(), F1) and same_bits(got["qoi"].cpu().numpy(), Q1), seg
            # 0: the library's choice; 115 workgroups are far fewer than one round of resident ones, so it is one row per segment
            want = evaluations_expected(P, seg if seg else 1)
            print("segment_rows=%d: %d evaluations of %d rows" % (seg, rp.n_evaluated, R * N))
            assert rp.n_evaluated == want, (seg, rp.n_evaluated, want)
            if seg in (0, 1):
                assert rp.n_evaluated == R * N == 115
        assert evaluations_expected(P, 23) == 3 + 7 + 23 + 3 + 4  # one segment per chain: the accepted states alone
        # one destination alone
        only_q = rp.run(dev, fields=("qoi",), segment_rows=7)
        assert set(only_q) == {"qoi"} and same_bits(only_q["qoi"].cpu().numpy(), Q1)
        only_f = rp.run(dev, fields=("model_output",), segment_rows=7)
        assert set(only_f) == {"model_output"} and same_bits(only_f["model_output"].cpu().numpy(), F1)


def test_chunks_cannot_change_a_bit():
    import torch

    import tinyda_amd as tda
    from tinyda_amd.records import DeviceRecords

    P = hand_made_records()
    R, N, d = P.shape
    model = tda.DeviceModel(xm.source() + xq.PER_QUANTITY, 70, n_qoi=66)
    whole = tda.replay_records(P, model)
    by_row = tda.replay_records(P, model, budget_bytes=1, count=True)
    assert whole["model_output"].shape == (N, R, 70) and whole["qoi"].shape == (N, R, 66)
    assert same_bits(by_row["model_output"], whole["model_output"]) and same_bits(by_row["qoi"], whole["qoi"])
    assert by_row["n_evaluated"] == R * N  # every chunk starts a fresh segment
    recs = DeviceRecords(torch.from_numpy(P).cuda(), None, None)
    on_device = tda.replay_records(recs, model, ("qoi",), burnin=5, budget_bytes=3 * N * 66 * 8)
    assert set(on_device) == {"qoi"} and same_bits(on_device["qoi"], whole["qoi"][:, 5:])
    assert same_bits(np.swapaxes(whole["model_output"], 0, 1), model.evaluate(P.reshape(R * N, d))[0].reshape(R, N, 70))


# ---- 4. sample() end to end, without a host reference -------------------------------------------------------------------------------------
D, M, N_CHAINS, ITER = 4, 16, 64, 300


def ring_posterior(ksteps=48, y=None):
    import tinyda_amd as tda

    truth, y0, _ = xw.problem(D, M, 1, seed=3)
    y = y0 if y is None else y
    model = tda.DeviceModel(xw.source(ksteps=ksteps) + xq.RING_WAVE, M, n_qoi=xq.RING_WAVE_N)
    return truth, y, tda.Posterior(st.multivariate_normal(np.zeros(D), np.eye(D)), tda.GaussianLogLike(y, SIGMA ** 2 * np.eye(M)), model)


def check_result(res, y, rows, burnin=0, ksteps=48, level="fine", n_chains=N_CHAINS, seed=0):
    """the replayed outputs reproduce the recorded log-likelihood of every row of every chain, the quantities equal the twin's on
    rows 0, 1, the last and 20 random ones; layout and lengths are the reference's (diagnostics.py:114-209)"""
    import tinyda_amd as tda

    out, qoi = tda.get_samples(res, "model_output", level=level, burnin=burnin), tda.get_samples(res, "qoi", level=level, burnin=burnin)
    par, stats = tda.get_samples(res, "parameters", level=level, burnin=burnin), tda.get_samples(res, "stats", level=level, burnin=burnin)
    assert out["attribute"] == "model_output" and out["n_chains"] == n_chains and out["iterations"] == rows - burnin and out["dimension"] == M
    assert qoi["iterations"] == rows - burnin and qoi["dimension"] == xq.RING_WAVE_N
    F = np.stack([out["chain_%d" % c] for c in range(n_chains)])
    Q = np.stack([qoi["chain_%d" % c] for c in range(n_chains)])
    P = np.stack([par["chain_%d" % c] for c in range(n_chains)])
    S = np.stack([stats["chain_%d" % c] for c in range(n_chains)])
    assert F.shape == (n_chains, rows - burnin, M) and Q.shape == (n_chains, rows - burnin, xq.RING_WAVE_N)
    loglike = -0.5 * np.sum((F - y) ** 2, axis=2) / SIGMA ** 2
    rel = np.abs(loglike - S[:, :, 1]) / np.abs(S[:, :, 1])
    print("log-likelihood from the replayed outputs: largest relative deviation %.3e (bar 1e-10)" % rel.max())
    assert rel.max() <= 1e-10
    pick = np.unique(np.concatenate([[0, 1, rows - burnin - 1], np.random.default_rng(seed).integers(0, rows - burnin, 20)]))
    within_bar(Q[:, pick].reshape(-1, xq.RING_WAVE_N), xq.np_ring_wave(P[:, pick].reshape(-1, D), M, ksteps), "quantities of %d rows (%s)" % (len(pick), level))
    return F, Q


@pytest.fixture(scope="module")
def single_level():
    import tinyda_amd as tda

    truth, y, post = ring_posterior()
    assert post.model.reference is None
    res = tda.sample(post, tda.AdaptiveMetropolis(1e-3 * np.eye(D), t0=50, period=50), ITER, n_chains=N_CHAINS, initial_parameters=truth, seed=3)
    assert res["backend"] == "hip"
    return res, y, post


def test_sample_without_reference_serves_outputs_and_quantities(single_level):
    import tinyda_amd as tda

    res, y, post = single_level
    F, Q = check_result(res, y, ITER + 1)
    acc = tda.get_samples(res, "parameters")["chain_0"]
    assert 1 < len(np.unique(acc, axis=0)) < ITER + 1  # accepted and rejected steps both occur
    idata = tda.to_inference_data(res)
    assert sorted(idata.posterior_predictive) == sorted("obs_%d" % i for i in range(M))
    assert sorted(idata.qoi) == ["qoi_%d" % i for i in range(xq.RING_WAVE_N)]
    assert all(np.asarray(idata.posterior_predictive["obs_%d" % i]).shape == (N_CHAINS, ITER + 1) for i in range(M))
    assert all(np.asarray(idata.qoi[k]).shape == (N_CHAINS, ITER + 1) for k in idata.qoi)
    assert same_bits(np.asarray(idata.posterior_predictive["obs_5"]), F[:, :, 5]) and same_bits(np.asarray(idata.qoi["qoi_1"]), Q[:, :, 1])
    # one link, one chain
    link = res["chain_3"][-1]
    assert isinstance(link.qoi, np.ndarray) and isinstance(link.model_output, np.ndarray)
    assert same_bits(link.model_output, F[3, -1]) and same_bits(link.qoi, Q[3, -1])
    chain = res["chain_7"]
    assert same_bits(chain.model_output, F[7]) and same_bits(chain.qoi, Q[7])
    assert same_bits(chain[100:].qoi, Q[7, 100:])


def test_burnin_and_records_moved_to_the_host(single_level):
    import tinyda_amd as tda

    res, y, post = single_level
    whole = np.stack([tda.get_samples(res, "qoi")["chain_%d" % c] for c in range(N_CHAINS)])
    F, Q = check_result(res, y, ITER + 1, burnin=100, seed=1)
    assert same_bits(Q, whole[:, 100:])
    res["chain_0"]._records.to_host()
    assert not res["chain_0"]._records.on_device
    F2, Q2 = check_result(res, y, ITER + 1, burnin=100, seed=2)
    assert same_bits(F2, F) and same_bits(Q2, Q)


def test_thinned_records():
    import tinyda_amd as tda

    truth, y, post = ring_posterior()
    res = tda.sample(post, tda.AdaptiveMetropolis(1e-3 * np.eye(D), t0=50, period=50), ITER, n_chains=N_CHAINS, initial_parameters=truth, seed=3, thin=3)
    assert res["thin"] == 3
    check_result(res, y, 1 + ITER // 3)


def test_delayed_acceptance_each_level_with_its_own_quantity():
    import tinyda_amd as tda

    truth, y, fine = ring_posterior(48)
    _, _, coarse = ring_posterior(12, y)
    n, iters, sub = 16, 40, 3
    res = tda.sample([coarse, fine], tda.GaussianRandomWalk(1e-4 * np.eye(D)), iters, n_chains=n, initial_parameters=truth, subchain_length=sub, seed=9)
    assert res["sampler"] == "DA" and res.get("backend", "hip") != "host"
    rows_fine, rows_coarse = len(res["chain_fine_0"]), len(res["chain_coarse_0"])
    assert rows_fine == iters + 1 and rows_coarse >= iters
    Ff, Qf = check_result(res, y, rows_fine, ksteps=48, level="fine", n_chains=n)
    Fc, Qc = check_result(res, y, rows_coarse, ksteps=12, level="coarse", n_chains=n)
    assert not same_bits(Qf[:, -1], Qc[:, -1])  # (the two fidelities differ)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_lds_beyond_64_kib_names_the_quantities_share():
    import tinyda_amd as tda
    from tinyda_amd import _lib

    words, m, nq = 8000, 16, 65
    src = xw.source().replace("#define TDA_WORKSPACE (WV_K * 64)", "#define TDA_WORKSPACE %d" % words)
    assert "TDA_WORKSPACE %d" % words in src
    th = thetas(4, n=3)
    within_bar(tda.DeviceModel(src, m).evaluate(th), xw.np_forward(th, m), "ring with 8000 words of workspace")  # 1024 + 64000 + 128 bytes
    with pytest.raises(_lib.EngineError, match="64 KiB") as err:
        tda.DeviceModel(src + xq.PER_QUANTITY, m, n_qoi=nq).evaluate(th)
    msg = str(err.value)
    assert all(str(v) in msg for v in (1024 + 8 * words, 8 * (m + nq), 8 * nq)) and "quantities" in msg and "TDA_WORKSPACE" in msg, msg


def test_mis_signed_quantity_quotes_the_signature():
    import tinyda_amd as tda
    from tinyda_amd import _lib
    from tinyda_amd._contract import QOI_SIG

    bad = xq.PER_QUANTITY.replace("int n_outputs, int k)", "int n_outputs, int k, int more)")
    with pytest.raises(_lib.EngineError) as err:
        tda.DeviceModel(xm.source() + bad, 5, n_qoi=2).evaluate(thetas(3, n=2))
    assert QOI_SIG["tda_qoi"] in str(err.value)
    bad_wave = xq.RING_WAVE.replace("double* work, int lane)", "int lane)").replace("work[(WV_K - 1) * 64 + lane]", "f[0]")
    with pytest.raises(_lib.EngineError) as err:
        tda.DeviceModel(xw.source() + bad_wave, 16, n_qoi=3).evaluate(thetas(4, n=2))
    assert QOI_SIG["tda_qoi_wave"] in str(err.value)


def test_nothing_to_do_is_refused():
    import torch

    import tinyda_amd as tda
    from tinyda_amd import _lib

    model = tda.DeviceModel(xm.source(), 5)
    with tda.Replay(model, 3) as rp:
        with pytest.raises(_lib.EngineError, match="nothing to do"):
            rp.run(torch.zeros((2, 2, 3), dtype=torch.float64, device="cuda"), fields=("qoi",))
    with pytest.raises(ValueError, match="no quantity of interest"):
        tda.replay_records(np.zeros((2, 2, 3)), model, ("qoi",))
    with pytest.raises(_lib.EngineError, match="closed"):
        rp.run(torch.zeros((2, 2, 3), dtype=torch.float64, device="cuda"))
