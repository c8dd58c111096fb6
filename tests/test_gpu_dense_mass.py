"""Dense inverse masses of HMC / NUTS on the device (tda_user_hmc_steps / tda_user_nuts_steps built with -DTDA_DENSE_MASS,
include/tinyda_amd_dense_mass.h): bit for bit against the diagonal kernels at W = I and W = diag(powers of 4), Philox forward mode
against the NumPy twins of tests/extdense.py under a genuinely dense W, the source forms whose barriers meet the new ones, split
independence and checkpoint resume, the entry points' refusals, the LDS refusal, and sample(backend='hip') end to end.

tests/test_dense_mass.py ties the twins to the diagonal twins and to a change of variables, and admits every case compared here
(one ulp on every gradient and d 2^-52 on every product leave every decision as it is) on the variates the engine draws."""
import numpy as np
import pytest
import scipy.stats as st

from . import extdense as xd
from . import exthmc as xh
from . import extnuts as xn
from .extengine import assert_resume_bitwise
from .test_dense_mass import END_TO_END, end_to_end_sigma, whitened_eigenvalues

pytestmark = pytest.mark.gpu


def _records(e, theta0, T, nuts):
    e.init(theta0)
    out = e.run_host(T)
    tail = (e.proposal_state_scaling(), e.nuts_totals() if nuts else None)
    return out, tail


# ---- bitwise against the diagonal kernels ----------------------------------------------------------------------------------------------
BITWISE_STEP = {5: 0.03, 64: 0.012, 65: 0.008, 128: 0.004}


@pytest.mark.parametrize("mass", ["unit", "spread"])
@pytest.mark.parametrize("d", [5, 64, 65, 128])
@pytest.mark.parametrize("kind", ["hmc", "nuts"])
def test_diagonal_factor_is_the_diagonal_kernel_bitwise(kind, d, mass):
    """set_dense_mass(I) against unit mass, set_dense_mass(diag(sqrt(MASS_SPREAD))) against inv_mass = MASS_SPREAD (powers of 4:
    every scaling is exact): records, log-densities, accept masks, adapted step sizes and NUTS's totals with np.array_equal.
    d = 65: the second lane slot begins; d = 128: every slot is full.  Any mistake in the order of operations shows here"""
    m, N, T = 23, 13, 40
    noise = "iso" if d == 65 else "diag"
    y, theta0, pm, pv, nz, _ = xh.gaussian_problem(d, m, noise, N, seed=d * 1000 + m)
    w = None if mass == "unit" else xn.MASS_SPREAD(d)
    chol = np.eye(d) if w is None else np.diag(np.sqrt(w))
    assert np.array_equal(chol * chol, np.eye(d) if w is None else np.diag(w))
    base = xh.hmc(BITWISE_STEP[d], 4, True) if kind == "hmc" else xn.nuts(BITWISE_STEP[d], 4, True)
    got = []
    for dense in (True, False):
        e = xh.gaussian_engine(d, m, noise, N, y, pm, pv, nz, dict(kind="mala", scaling=0.1), 16 if d == 128 else 0)
        try:
            (xh if kind == "hmc" else xn).set_proposal(e, dict(base, inv_mass=None if dense else w))
            if dense:
                e.set_dense_mass(chol)
            got.append(_records(e, theta0, T, kind == "nuts"))
        finally:
            e.close()
    ((pa, sa, aa), (sca, ta)), ((pb, sb, ab), (scb, tb)) = got
    assert np.all(np.isfinite(sb)) and np.all(np.isfinite(pb)) and 0 < ab.mean() and not np.all(scb == BITWISE_STEP[d])
    assert np.array_equal(pa, pb) and np.array_equal(sa, sb) and np.array_equal(aa, ab) and np.array_equal(sca, scb)
    if kind == "nuts":
        assert np.array_equal(ta, tb) and np.all(tb[:, 0] >= T)


# ---- forward cases against the twin under DENSE(d) ---------------------------------------------------------------------------------------
def _forward(case, level, prop, theta0, T, make):
    e = make()
    try:
        e.init(theta0)
        chol = e.get_dense_mass()
        assert np.array_equal(chol, prop["chol"])
        z, u = e.set_export(T)
        params, stats, acc = e.run_host(T)
        scal = e.proposal_state_scaling()
        totals = e.nuts_totals() if prop["kind"] == "nuts" else None
    finally:
        e.close()
    twin = dict(prop, chol=chol)  # the twin takes the factor from the engine: the very bits the kernel multiplies by
    if prop["kind"] == "hmc":
        ref = xd.run_hmc(level, twin, theta0, np.swapaxes(z, 0, 1), u.T)
    else:
        ref = xd.run_nuts(level, twin, theta0, np.swapaxes(z, 0, 1), xn.PhiloxDraws(xd.SEED, xd.CHAIN_OFFSET, theta0.shape[0]))
        print("trees:", xn.coverage(ref, prop["max_depth"]))
        assert np.array_equal(totals, ref["totals"])
    xd.compare(case, params, stats, acc, ref, scal)
    assert np.all(np.isfinite(stats))


@pytest.mark.parametrize("case", list(xd.FORWARD_CASES))
def test_philox_forward_matches_twin(case):
    """masks and tree decisions exact (NUTS: the per-chain totals), log-posterior 1e-10, states 1e-9 (atol 1e-12), the final step size
    1e-12, unless extdense.TOLERANCE lists the case"""
    _forward(case, *xd.forward_case(case))


@pytest.mark.parametrize("case,kind", list(xd.CONTRACT_STEP))
def test_other_source_forms_match_twin(case, kind):
    """the ring (tda_forward_wave + tda_gradient_wave) and the Cauchy-difference prior (tda_logprior_wave + tda_logprior_grad): the
    barriers of tda_dense_product between source-defined ones, on the twin's bars"""
    _forward("%s/%s" % (case, kind), *xd.contract_case(case, kind, xd.CONTRACT_STEP[(case, kind)]))


# ---- split independence and resume -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hmc", "nuts"])
def test_splits_and_resume_are_bitwise(kind):
    """60 steps in one run, as 25 + 35, and as 25 + get_state / set_state into a fresh engine + 35 (blocks of 16 steps, periods of
    20): the same records.  The mass is configuration: the blob has the length of the diagonal engine's of the same shape"""
    d, m, noise, N = 65, 23, "diag", 11
    y, theta0, pm, pv, nz, _ = xh.gaussian_problem(d, m, noise, N, seed=7 + d)
    prop = xd.dense_proposal(kind, d, 0.01, True)
    sizes = {}

    def make(dense=True):
        e = xh.gaussian_engine(d, m, noise, N, y, pm, pv, nz, dict(kind="mala", scaling=0.1), block_steps=16)
        if dense:
            xd.set_proposal(e, prop)
        else:
            (xh if kind == "hmc" else xn).set_proposal(e, dict({k: v for k, v in prop.items() if k != "chol"}, inv_mass=xh.MASS(d)))
        e.init(theta0)
        sizes[dense] = e.get_state().size
        return e

    assert_resume_bitwise(make, whole=60, first=25)
    make(False).close()
    assert sizes[True] == sizes[False] > 0


# ---- the entry points --------------------------------------------------------------------------------------------------------------------
def test_entry_points():
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    from .test_mala_source import ROSEN_SRC

    d, N = 3, 4
    L = np.linalg.cholesky(xd.DENSE(d))
    e = Engine(N, d, seed=1)
    try:
        e.set_prior(np.zeros(d), np.eye(d))
        e.set_level_source(0, ROSEN_SRC, np.zeros(1), 0, [1.0])
        with pytest.raises(_lib.EngineError, match="TDA_PROP_HMC or TDA_PROP_NUTS must precede set_dense_mass"):
            e.set_dense_mass(L)
        e.set_proposal(6, None, scaling=0.1)  # MALA
        with pytest.raises(_lib.EngineError, match="TDA_PROP_HMC or TDA_PROP_NUTS must precede set_dense_mass"):
            e.set_dense_mass(L)
        for kind, kw in ((xh.PROP_HMC, dict(n_leapfrog=2)), (xn.PROP_NUTS, dict(max_depth=3))):
            e.set_proposal(kind, None, scaling=0.01, period=10, **kw)
            with pytest.raises(ValueError, match=r"\[dim, dim\] = \[3, 3\]"):
                e.set_dense_mass(L[:2, :2])
            bad = L.copy()
            bad[0, 2] = 1e-300
            with pytest.raises(_lib.EngineError, match=r"chol\[0\]\[2\] = 1e-300 lies above the diagonal"):
                e.set_dense_mass(bad)
            for v, word in ((0.0, "positive"), (-1.5, "positive"), (np.nan, "finite")):
                bad = L.copy()
                bad[1, 1] = v
                with pytest.raises(_lib.EngineError, match=r"chol\[1\]\[1\] = (0|-1\.5|-?nan) .*%s" % word):
                    e.set_dense_mass(bad)
            bad = L.copy()
            bad[2, 0] = np.inf
            with pytest.raises(_lib.EngineError, match=r"chol\[2\]\[0\] = inf must be finite"):
                e.set_dense_mass(bad)
            # refused in both orders with set_mass_adaptation, each naming the other call
            e.set_dense_mass(L)
            with pytest.raises(_lib.EngineError, match="set_mass_adaptation on an engine with a dense mass.*tda_engine_set_dense_mass"):
                e.set_mass_adaptation(40)
            e.set_dense_mass(None)
            e.set_mass_adaptation(40)
            with pytest.raises(_lib.EngineError, match="set_dense_mass on an engine that adapts its mass.*tda_engine_set_mass_adaptation"):
                e.set_dense_mass(L)
            e.set_mass_adaptation(0)
            e.set_dense_mass(L)
            with pytest.raises(_lib.EngineError, match="get_dense_mass applies to an initialised"):
                e.get_dense_mass()
            e.init(np.zeros((N, d)))
            assert np.array_equal(e.get_dense_mass(), L)  # bit for bit
            with pytest.raises(_lib.EngineError, match="get_mass reads a diagonal mass.*tda_engine_get_dense_mass"):
                e.get_mass()
            assert np.all(np.isfinite(e.run_host(3)[1]))
            # set_proposal clears it: the diagonal engine again
            e.set_proposal(kind, None, scaling=0.01, period=10, **kw)
            e.init(np.zeros((N, d)))
            with pytest.raises(_lib.EngineError, match="get_dense_mass applies to an initialised"):
                e.get_dense_mass()
            assert np.array_equal(e.get_mass()[0], np.ones(d))
    finally:
        e.close()


def test_device_destination_of_get_dense_mass():
    import torch

    from .test_mala_source import ROSEN_SRC
    from tinyda_amd.engine import Engine

    d, N = 5, 4
    L = np.linalg.cholesky(xd.DENSE(d))
    e = Engine(N, d, seed=1)
    try:
        e.set_prior(np.zeros(d), np.eye(d))
        e.set_level_source(0, ROSEN_SRC, np.zeros(1), 0, [1.0])
        e.set_proposal(xn.PROP_NUTS, None, scaling=0.01, max_depth=2, dense_mass=L)
        e.init(np.zeros((N, d)))
        out = e.get_dense_mass(torch.full((d, d), -1.0, dtype=torch.float64, device="cuda"))
        assert np.array_equal(out.cpu().numpy(), L)
    finally:
        e.close()


# ---- LDS ---------------------------------------------------------------------------------------------------------------------------------
def test_dense_mass_counts_in_the_lds_refusal():
    """the ring with a TDA_WORKSPACE under which the diagonal NUTS program holds exactly 64 KiB per chain (64064 bytes of static LDS,
    192 for the outputs, 1280 for the checkpoints of max_depth = 10) initialises and runs; the dense one needs 1 KiB more and is
    refused with the byte counts"""
    from tinyda_amd import _lib
    from tinyda_amd.engine import Engine

    from . import extwave as xw

    d, m, N = 5, 24, 4
    _, y, theta0 = xw.problem(d, m, N, seed=524, sigma=0.01)
    src = xw.source("wave", "wave")
    big = "#define TDA_WORKSPACE 7752\n" + "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("#define TDA_WORKSPACE"))
    assert "TDA_WORKSPACE" in src
    for dense in (False, True):
        e = Engine(N, d, seed=1)
        try:
            e.set_prior(np.zeros(d), np.eye(d))
            e.set_level_source(0, big, y, 0, [1e-4])
            e.set_proposal(xn.PROP_NUTS, None, scaling=0.05, max_depth=10, dense_mass=np.linalg.cholesky(xd.DENSE(d)) if dense else None)
            if dense:
                with pytest.raises(_lib.EngineError, match=r"NUTS over a source-defined model needs more than 64 KiB of LDS per chain: this source needs 65088 bytes "
                                                           r".*1024 bytes for the operand of the dense mass's products\) \+ 192 bytes for its 24 outputs \+ 1280 bytes "
                                                           r"for the checkpoints of max_depth = 10 over 8 padded parameters = 66560 bytes"):
                    e.init(theta0)
            else:
                e.init(theta0)
                assert np.all(np.isfinite(e.run_host(3)[1]))
        finally:
            e.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_sample_under_the_true_covariance():
    """sample(backend='hip') on N(0, Sigma), Sigma = Q diag(sd^2) Q^T with sd = logspace(-1, 1, 8), 256 chains, 400 steps of adaptive
    NUTS: under inv_mass = Sigma the mean tree depth of the last 100 steps is lower than under inv_mass = diag(Sigma); every record
    is finite; under Sigma the pooled covariance C of the last 200 steps has every eigenvalue of Sigma^-1/2 C Sigma^-1/2 in
    [0.5, 2], and so has mass_from_samples of that result (tests/test_dense_mass.py holds the host class to the same conditions)"""
    import tinyda_amd as tda

    from .test_gpu_mala_source import _linear_source

    cfg = END_TO_END
    sd, N, T = cfg["sd"], cfg["N"], cfg["T"]
    Sigma, Q = end_to_end_sigma(cfg)
    d, pv = sd.shape[0], 1e4
    nv = 1.0 / (1.0 / sd ** 2 - 1.0 / pv)  # F = Q^T theta under the prior N(0, pv I): the posterior is N(0, Q diag(sd^2) Q^T)
    post = tda.Posterior(st.multivariate_normal(np.zeros(d), pv * np.eye(d)), tda.GaussianLogLike(np.zeros(d), np.diag(nv)), tda.DeviceModel(_linear_source(Q.T.copy()), d))
    starts = list(np.random.default_rng(5).standard_normal((N, d)) @ np.linalg.cholesky(Sigma).T)
    depth = {}
    for name, mass in (("dense", Sigma), ("diag", np.diag(Sigma).copy())):
        prop = tda.NUTS(scaling=cfg["scaling"], adaptive=True, period=cfg["period"], inv_mass=mass)
        head = tda.sample(post, prop, T - 100, n_chains=N, initial_parameters=starts, seed=21, backend="hip")
        res = tda.sample(post, prop, T, n_chains=N, initial_parameters=starts, seed=21, backend="hip")
        assert res["backend"] == "hip"
        ps, ps_head = res["proposal_state"], head["proposal_state"]
        assert "inv_mass" not in ps and len(ps) == 10
        # (a run is the head of a longer one: the last 100 steps' depths are the difference of the two runs' sums)
        depth[name] = float(np.mean(np.asarray(ps["mean_tree_depth"]) * T - np.asarray(ps_head["mean_tree_depth"]) * (T - 100)) / 100.0)
        got = tda.get_samples(res)
        X = np.stack([got["chain_%d" % i] for i in range(N)])
        assert X.shape == (N, T + 1, d) and np.all(np.isfinite(X))
        for i in (0, N - 1):
            assert np.all(np.isfinite(res["chain_%d" % i].stats))
        if name == "dense":
            ev = whitened_eigenvalues(np.cov(X[:, -200:].reshape(-1, d), rowvar=False), Sigma)
            W = tda.mass_from_samples(res, burnin=T + 1 - 200)
            ev_mass = whitened_eigenvalues(W, Sigma)
            print("eigenvalues of Sigma^-1/2 C Sigma^-1/2: %.3f .. %.3f; of mass_from_samples: %.3f .. %.3f" % (ev.min(), ev.max(), ev_mass.min(), ev_mass.max()))
            assert 0.5 <= ev.min() and ev.max() <= 2.0 and 0.5 <= ev_mass.min() and ev_mass.max() <= 2.0
            assert np.array_equal(W, W.T) and tda.NUTS(inv_mass=W).chol_inv_mass.shape == (d, d)
            np.testing.assert_allclose(tda.mass_from_samples(res, burnin=T + 1 - 200, dense=False), np.diag(W), rtol=1e-12)
    print("mean tree depth of the last 100 steps: %.2f under Sigma, %.2f under its diagonal" % (depth["dense"], depth["diag"]))
    assert depth["dense"] < depth["diag"]
