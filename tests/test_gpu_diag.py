"""On-device bulk ESS / R-hat (tda_diag_ess_rhat) against oracle/ess_oracle.py, the independent restatement of Vehtari et al.
(2021) that also checks the package's NumPy implementation (tests/test_diagnostics.py)."""
import numpy as np
import pytest

from tests import extdiag
from tests.extdiag import history as _chains

pytestmark = pytest.mark.gpu

ESS_RTOL, RHAT_RTOL = 1e-8, 1e-10  # against oracle/ess_oracle.py, everywhere in this file


@pytest.mark.parametrize("T,N,d,burnin", [(400, 16, 3, 0), (257, 5, 2, 31), (1200, 64, 4, 200)])
def test_device_ess_rhat_matches_the_oracle(T, N, d, burnin):
    import torch

    from oracle import ess_oracle as eo
    from tinyda_amd import summaries as sm

    x = _chains(T, N, d, seed=T + N, rho=0.9, sticky=0.6)
    dev = torch.tensor(x, dtype=torch.float64, device="cuda")
    out = sm.ess_rhat_device(dev, burnin=burnin)
    for j in range(d):
        xs = x[burnin:, :, j].T
        np.testing.assert_allclose(out["ess"][j], eo.ess_bulk(xs), rtol=1e-8)
        np.testing.assert_allclose(out["rhat"][j], eo.rhat(xs), rtol=1e-10)
    assert out["rhat"][-1] > out["rhat"][0]


def test_device_ess_rhat_on_the_stress_cases():
    """heavy tails, antithetic chains, disagreeing chains, runs of ties with an odd number of draws (tests/test_diagnostics.py)"""
    import torch

    from oracle import ess_oracle as eo
    from tests.test_diagnostics import cases
    from tinyda_amd import summaries as sm

    for name, x in cases().items():
        if x.shape[1] < 16:
            continue
        dev = torch.tensor(np.ascontiguousarray(x.T[:, :, None]), dtype=torch.float64, device="cuda")  # [draws, chains, 1]
        out = sm.ess_rhat_device(dev)
        np.testing.assert_allclose(out["ess"][0], eo.ess_bulk(x), rtol=1e-8, err_msg=name)
        np.testing.assert_allclose(out["rhat"][0], eo.rhat(x), rtol=1e-10, err_msg=name)


def test_device_diag_rejects_host_pointers():
    from tinyda_amd import _lib, summaries as sm

    class Fake:
        shape = (100, 4, 2)

        def __init__(self):
            self.a = np.zeros(self.shape)

        def data_ptr(self):
            return self.a.ctypes.data

    with pytest.raises(_lib.EngineError):
        sm.ess_rhat_device(Fake())


# ---- the cases of tests/extdiag.py: every path of tda_diag.inc, at the benchmark's chain count and at the values where ranks go wrong ----
def _device(x):
    import torch

    return torch.tensor(np.ascontiguousarray(x if x.ndim == 3 else x[:, :, None]), dtype=torch.float64, device="cuda")


def _run(x, burnin=0, **kw):
    from tinyda_amd import summaries as sm

    return sm.ess_rhat_device(_device(x), burnin=burnin, **kw)


def _assert_same_bits(a, b):
    assert extdiag.same_bits(a["ess"], b["ess"]), (a["ess"], b["ess"])
    assert extdiag.same_bits(a["rhat"], b["rhat"]), (a["rhat"], b["rhat"])


@pytest.mark.parametrize("name", list(extdiag.SHAPES))
def test_device_matches_the_oracle_at_every_path(name):
    """block counts of the power-spectrum mean from 1 to 32 with full and short last blocks, FFT lengths at and past a power of
    two, strided centring, history stride 128, odd kept draws after a burn-in (extdiag.SHAPES); every parameter"""
    burnin = extdiag.SHAPES[name][3]
    out = _run(extdiag.shape_history(name), burnin)
    ess, rhat = extdiag.reference(name)
    print("%s: largest deviation from the oracle: ess %.2e rhat %.2e" % (name, extdiag.deviation(out["ess"], ess), extdiag.deviation(out["rhat"], rhat)))
    np.testing.assert_allclose(out["ess"], ess, rtol=ESS_RTOL)
    np.testing.assert_allclose(out["rhat"], rhat, rtol=RHAT_RTOL)


@pytest.mark.parametrize("name", [n for n in extdiag.EDGES if n != "nan_one_parameter"])
def test_device_matches_the_oracle_at_the_rank_edges(name):
    """signed zeros in one tie run, tie runs across every chain, a constant chain, no variance at all (NaN), infinities"""
    out = _run(extdiag.edges()[name])
    ess, rhat = extdiag.reference(name)
    print("%s: largest deviation from the oracle: ess %.2e rhat %.2e" % (name, extdiag.deviation(out["ess"], ess), extdiag.deviation(out["rhat"], rhat)))
    if name == "all_constant":
        assert np.isnan(ess[0]) and np.isnan(rhat[0]) and np.isnan(out["ess"][0]) and np.isnan(out["rhat"][0])
    else:
        np.testing.assert_allclose(out["ess"], ess, rtol=ESS_RTOL)
        np.testing.assert_allclose(out["rhat"], rhat, rtol=RHAT_RTOL)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_a_nan_makes_its_parameter_nan_and_no_other(sign):
    """as in the NumPy twin (tests/test_diagnostics.py); a NaN sorts to the end of the keys, one with its sign bit set to the start"""
    x = extdiag.edges()["nan_one_parameter"].copy()
    x[extdiag.NAN_AT] = np.copysign(np.nan, sign)
    j_nan = extdiag.NAN_AT[2]
    out, clean = _run(x), _run(extdiag.nan_replaced())
    ess, rhat = extdiag.reference("nan_one_parameter")
    assert np.isnan(out["ess"][j_nan]) and np.isnan(out["rhat"][j_nan])
    others = [j for j in range(x.shape[2]) if j != j_nan]
    assert extdiag.same_bits(out["ess"][others], clean["ess"][others]) and extdiag.same_bits(out["rhat"][others], clean["rhat"][others])
    print("nan_one_parameter: largest deviation from the oracle: ess %.2e rhat %.2e"
          % (extdiag.deviation(clean["ess"], ess), extdiag.deviation(clean["rhat"], rhat)))
    np.testing.assert_allclose(clean["ess"], ess, rtol=ESS_RTOL)
    np.testing.assert_allclose(clean["rhat"], rhat, rtol=RHAT_RTOL)


def test_scaling_by_a_power_of_two_changes_no_bit():
    """4 x keeps every order relation, every tie and every rounding of the median and the folded values: same ranks, same answer"""
    x = extdiag.shape_history("bench_chains")
    burnin = extdiag.SHAPES["bench_chains"][3]
    _assert_same_bits(_run(4.0 * x, burnin), _run(x, burnin))


def test_two_calls_and_another_stream_change_no_bit():
    """the two-stage sums are deterministic; a non-default stream orders the same work"""
    import torch

    from tinyda_amd import summaries as sm

    burnin = extdiag.SHAPES["long_and_wide"][3]
    dev = _device(extdiag.shape_history("long_and_wide"))
    torch.cuda.synchronize()
    first = sm.ess_rhat_device(dev, burnin=burnin)
    _assert_same_bits(sm.ess_rhat_device(dev, burnin=burnin), first)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    _assert_same_bits(sm.ess_rhat_device(dev, burnin=burnin, stream=stream.cuda_stream), first)
    torch.cuda.synchronize()


def test_burnin_is_a_slice():
    """odd remainder: 17 kept draws, the middle one dropped, whether the burn-in is an argument or cut off beforehand"""
    T, N, d, burnin = extdiag.SHAPES["three_blocks_odd_burnin"]
    assert (T - burnin) % 2 == 1
    x = extdiag.shape_history("three_blocks_odd_burnin")
    _assert_same_bits(_run(x, burnin), _run(x[burnin:]))


@pytest.mark.parametrize("what", ["seven_kept_draws", "negative_burnin", "not_contiguous"])
def test_device_diag_refuses_and_stays_usable(what):
    from tinyda_amd import _lib, summaries as sm

    x = extdiag.shape_history("second_block_two_rows")
    dev = _device(x)
    if what == "seven_kept_draws":
        with pytest.raises(_lib.EngineError):
            sm.ess_rhat_device(dev, burnin=x.shape[0] - 7)
    elif what == "negative_burnin":
        with pytest.raises(_lib.EngineError):
            sm.ess_rhat_device(dev, burnin=-1)
    else:
        with pytest.raises(ValueError):
            sm.ess_rhat_device(dev.transpose(0, 1))
    out = sm.ess_rhat_device(dev)  # a valid call right after it
    ess, rhat = extdiag.reference("second_block_two_rows")
    np.testing.assert_allclose(out["ess"], ess, rtol=ESS_RTOL)
    np.testing.assert_allclose(out["rhat"], rhat, rtol=RHAT_RTOL)
