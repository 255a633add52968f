"""The clipping searches of ppq_amd/csrc/search.hip on degenerate histograms, small and odd launch geometries and every bit width.

KL: ``CUDA.KLLosses`` against tests/search_reference.py's ``kl_contract`` -- the arithmetic the kernel documents (exact sums rounded
to float32 once, float64 divergence) -- within 2^-38 * A_j, a bound derived from the float64 round-off of the divergence alone; and
against ``oracle.kl_search`` (the reference's float32 sums in NumPy's order) within the ABSOLUTE bound that tests/test_host_search.py
measured between those two CPU references (4 x 4.18e-7).  No tolerance here comes from a kernel result.

MSE: ``CUDA.MseSearch`` against the first minimum of the oracle's candidates and float32 loss (``sorted(...)[0]`` of range.py:487,
512): ties (one occupied bin), all-NaN (empty histogram), one candidate (min_value > 0, fewer bins than levels), bins below and off
the 256-lane block, 255 levels, S == 1, the grid-stride path and 16384 bins."""
import numpy as np
import pytest
import torch

import search_reference as R
from oracle import ppq_oracle as O
from oracle.cpu_calibration import ReplayObserver

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def CUDA():
    from ppq_amd import CUDA as C
    return C


_kl_cache = {}


def _kl(CUDA, bins, bits):
    """Per (bins, bits), computed once: the families' histograms, the contract, the oracle, and the single-histogram launches."""
    if (bins, bits) not in _kl_cache:
        rows = []
        for family in R.KL_FAMILIES:
            hist = R.histogram(family, bins)
            losses, A, Z = R.kl_contract_detail(hist, bits)
            with np.errstate(all='ignore'):
                _, _, records, best = O.kl_search(hist, R.HIST_SCALE, bits, False, return_losses=True)
            got = CUDA.KLLosses(torch.from_numpy(hist).to(DEV), bits).cpu().numpy()
            assert got.shape == (1, losses.size) and got.dtype == np.float64
            rows.append((family, hist, losses, A, Z, np.array([r['kl'] for r in records]), best, got[0]))
        _kl_cache[(bins, bits)] = rows
    return _kl_cache[(bins, bits)]


@pytest.mark.parametrize('bins,bits', R.KL_CASES)
def test_kl_matches_contract(CUDA, bins, bits):
    Q = 1 << (bits - 1)
    for family, hist, want, A, Z, _, _, got in _kl(CUDA, bins, bits):
        cid = R.kl_case_id(bins, bits, family)
        assert np.array_equal(np.isnan(got), np.isnan(want)), cid
        finite = np.isfinite(want)
        err = np.abs(got[finite] - want[finite])
        assert np.all(err <= R.KL_TOL * A[finite]), (cid, float(err.max()), int(np.argmax(err - R.KL_TOL * A[finite])))
        assert np.all(got[Z] == 0.0), cid                                  # identically vanishing terms: exactly zero in any order
        if cid in R.KL_AMBIGUOUS:
            assert R.kl_ambiguous(want, A, Z)
            assert R.pick(got, Q) in [(int(j) + 1) * Q for j in R.kl_near_minimum(want, A)], cid
        else:
            assert not R.kl_ambiguous(want, A, Z)
            assert R.pick(got, Q) == R.pick(want, Q), cid


@pytest.mark.parametrize('bins,bits', R.KL_CASES)
def test_kl_within_the_measured_bound_of_the_oracle(CUDA, bins, bits):
    for family, hist, _, A, Z, oracle, best, got in _kl(CUDA, bins, bits):
        cid = R.kl_case_id(bins, bits, family)
        assert np.array_equal(np.isnan(got), np.isnan(oracle)), cid
        finite = np.isfinite(oracle)
        assert np.all(np.abs(got[finite] - oracle[finite]) <= R.ORACLE_ABS_BOUND), cid
        if cid not in R.KL_AMBIGUOUS:
            assert R.pick(got, 1 << (bits - 1)) == best, cid


@pytest.mark.parametrize('bins,bits', R.KL_CASES)
def test_kl_batched_rows_equal_single_launches(CUDA, bins, bits):
    rows = _kl(CUDA, bins, bits)
    batch = CUDA.KLLosses(torch.from_numpy(np.stack([r[1] for r in rows])).to(DEV), bits).cpu().numpy()
    assert batch.shape == (len(rows), rows[0][2].size)
    for row, (family, *_, single) in zip(batch, rows):
        assert np.array_equal(row.view(np.uint64), single.view(np.uint64)), (bins, bits, family)


# ------------------------------------------------------------------------------------------------------------------------------- MSE
_MSE_LAUNCHES = [(bins, qmin, qmax, families, mode == 's') for bins, qmin, qmax, families, modes in R.MSE_CASES for mode in modes]
_mse_cache = {}


def _mse(bins, qmin, qmax, families, symmetric):
    key = (bins, qmin, qmax, symmetric)
    if key not in _mse_cache:
        rows = R.mse_rows(bins, families, symmetric)
        _mse_cache[key] = (rows, [R.mse_first_minimum(O, h, hs, mn, qmin, qmax, symmetric)[:4] for _, h, hs, mn in rows])
    return _mse_cache[key]


def _f64(values):
    return torch.tensor(list(values), dtype=torch.float64, device=DEV)


@pytest.mark.parametrize('bins,qmin,qmax,families,symmetric', _MSE_LAUNCHES,
                         ids=[f'{b}-{lo}_{hi}-{"sym" if s else "asym"}' for b, lo, hi, _, s in _MSE_LAUNCHES])
def test_mse_search_first_minimum(CUDA, bins, qmin, qmax, families, symmetric):
    """Single launches against the oracle; then every row in ONE launch with per-row hist_scale / min_value, twice on one workspace
    that starts out zeroed (a key of 0 would win every atomicMin if the launch did not re-initialise its packed keys)."""
    from ppq_amd import _lib
    from ppq_amd.ffi import _stream
    rows, wants = _mse(bins, qmin, qmax, families, symmetric)
    singles = []
    for (name, hist, hs, mn), want in zip(rows, wants):
        got = CUDA.MseSearch(torch.from_numpy(hist).to(DEV).reshape(1, -1), _f64([hs]), _f64([mn]), qmin, qmax, symmetric).cpu().numpy()
        assert got.shape == (1, 4) and got.dtype == np.int32
        assert tuple(int(v) for v in got[0]) == want, (name, got[0], want)           # (start, end, step, cell)
        singles.append(got[0])
    hists = torch.from_numpy(np.stack([r[1] for r in rows])).to(DEV)
    hs, mn = _f64(r[2] for r in rows), _f64(r[3] for r in rows)
    batch = CUDA.MseSearch(hists, hs, mn, qmin, qmax, symmetric).cpu().numpy()
    assert np.array_equal(batch, np.stack(singles))
    ws = torch.zeros(int(_lib.lib.ppqhip_mse_search_workspace_bytes(len(rows))), dtype=torch.uint8, device=DEV)
    for _ in range(2):
        best = torch.full((len(rows), 4), -7, dtype=torch.int32, device=DEV)
        status = _lib.lib.ppqhip_mse_search(hists.data_ptr(), len(rows), bins, hs.data_ptr(), mn.data_ptr(), qmin, qmax, int(symmetric),
                                            best.data_ptr(), ws.data_ptr(), _stream())
        assert status == 0, _lib.last_error()
        assert np.array_equal(best.cpu().numpy(), batch)


def test_mse_observer_renders_16_bit_config_on_2048_bins():
    """Fewer bins than levels: the reference's step loop is empty (range.py:481, 502) and it renders the min-max candidate."""
    from ppq_amd import LinearQuantizationConfig
    from ppq_amd.observer import TensorObserverFactroy, TorchMSEObserver, render_observers
    g = torch.Generator().manual_seed(3)
    data = [torch.randn(2, 8, 9, 7, generator=g) * (1 + 0.1 * i) + 0.2 for i in range(3)]
    for sym in (True, False):
        for batched in (False, True):
            qmin, qmax = (-32768, 32767) if sym else (0, 65535)
            cfg = LinearQuantizationConfig(symmetrical=sym, quant_min=qmin, quant_max=qmax, num_of_bits=16, calibration='mse')
            ob = TensorObserverFactroy.build_observer('x', cfg)
            assert isinstance(ob, TorchMSEObserver) and ob._hist_bins == 2048
            replay = ReplayObserver('mse', qmin, qmax, 16, sym, 2048)
            for phase in (replay.phase1, replay.phase2):
                for b in data:
                    ob.observe(b.to(DEV)); phase(b.numpy())
                render_observers([ob]) if batched else ob.render_quantization_config()
                if phase == replay.phase1: replay.end_phase1()
            assert tuple(int(v) for v in ob._best) == (0, 65536, 1, 0)
            s, o = replay.render()
            assert np.float32(s) == cfg.scale.cpu().numpy() and np.float32(o) == cfg.offset.cpu().numpy(), (sym, batched)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_without_a_launch(CUDA):
    from ppq_amd import _lib
    from ppq_amd.ffi import _stream
    lib = _lib.lib

    def hist(bins, dtype=torch.int32):
        return torch.ones(2, bins, dtype=dtype, device=DEV)

    def kl_status(bins, bits):
        out = torch.full((2, 20000), -7.0, dtype=torch.float64, device=DEV)
        status = lib.ppqhip_kl_losses(hist(bins).data_ptr(), 2, bins, bits, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
        return status

    # bins > 16384, bits 1 and 12, bins no multiple of 2^(bits-1)
    for bins, bits in ((16384 + 128, 8), (2048, 1), (4096, 12), (1000, 5), (64, 8)):
        assert kl_status(bins, bits) != 0 and b'kl_losses' in lib.ppqhip_last_error(), (bins, bits)
        with pytest.raises(RuntimeError):
            CUDA.KLLosses(hist(bins), bits)

    one = _f64([0.01, 0.01])
    for bins, qmin, qmax in ((16385, 0, 255), (2048, 5, 4)):               # too many bins; no level at all
        best = torch.full((2, 4), -7, dtype=torch.int32, device=DEV)
        ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
        status = lib.ppqhip_mse_search(hist(bins).data_ptr(), 2, bins, one.data_ptr(), one.data_ptr(), qmin, qmax, 1, best.data_ptr(),
                                       ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert status != 0 and b'mse_search' in lib.ppqhip_last_error() and bool((best == -7).all()), (bins, qmin, qmax)
        with pytest.raises(RuntimeError):
            CUDA.MseSearch(hist(bins), one, one, qmin, qmax, True)

    # dtypes: the histogram is int32, hist_scale / min_value float64
    for bad in (torch.int64, torch.float32):
        with pytest.raises(RuntimeError):
            CUDA.KLLosses(hist(2048, bad), 8)
        with pytest.raises(RuntimeError):
            CUDA.MseSearch(hist(2048, bad), one, one, 0, 255, True)
    with pytest.raises(RuntimeError):
        CUDA.MseSearch(hist(2048), one.float(), one, 0, 255, True)
    with pytest.raises(RuntimeError):
        CUDA.MseSearch(hist(2048), one, one.float(), 0, 255, True)
