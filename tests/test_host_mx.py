"""MX fake quant without a GPU: the oracle (tests/mx_reference.py) against torch's own FP8 casts and the known answers, the
``use_kernels=False`` arm of ppq_amd.mx against the oracle bit for bit, the error paths, and the host-side argument checks of the
C entry points (they run before any launch, so they need no device)."""
import ctypes

import numpy as np
import pytest
import torch

import mx_reference as R
from ppq_amd import MXDelegator, MXFormat, _lib, ffi, mx_fake_quant
from ppq_amd.mx import mx_block_axis

FORMATS = R.FORMATS


def torch_arm(x: np.ndarray, fmt: str, axis: int = -1):
    t = torch.from_numpy(np.ascontiguousarray(x))
    shape = list(t.shape)
    shape[axis % t.dim()] = (shape[axis % t.dim()] + 31) // 32
    codes = torch.zeros(shape, dtype=torch.uint8)
    y = mx_fake_quant(t, fmt, axis, scale_codes=codes, use_kernels=False)
    return y.numpy(), codes.numpy()


def assert_same(got, want, what):
    (y, c), (ry, rc) = got, want
    assert y.shape == ry.shape and c.shape == rc.shape, what
    bad = np.flatnonzero(R.bits(y).ravel() != R.bits(ry).ravel())
    assert bad.size == 0, f'{what}: {bad.size} elements differ, first at {bad[:4]}: {y.ravel()[bad[:4]]} != {ry.ravel()[bad[:4]]}'
    assert np.array_equal(c, rc), f'{what}: scale codes differ'


# ---------------------------------------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize('fmt, dtype, top', [('MXFP8_E4M3', torch.float8_e4m3fn, 448.0), ('MXFP8_E5M2', torch.float8_e5m2, 57344.0)])
def test_oracle_fp8_cast_equals_torch(fmt, dtype, top):
    """Every finite float32 pattern made of each high half-word with zero low bits and with two sets of random low bits."""
    rng = np.random.default_rng(5)
    high = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    for low in (np.zeros(1 << 16, np.uint32), rng.integers(0, 1 << 16, 1 << 16).astype(np.uint32), rng.integers(0, 1 << 16, 1 << 16).astype(np.uint32)):
        x = (high | low).view(np.float32)
        x = x[np.isfinite(x)]
        assert x.size == 65280
        want = torch.from_numpy(x).clamp(-top, top).to(dtype).float().numpy()
        got = R.cast(x.astype(np.float64), fmt).astype(np.float32)
        assert np.array_equal(R.bits(got), R.bits(want))


def test_oracle_tables():
    sizes = {'MXFP8_E4M3': 127, 'MXFP8_E5M2': 124, 'MXFP6_E3M2': 32, 'MXFP6_E2M3': 32, 'MXFP4_E2M1': 8, 'MXINT8': 128}
    tops = {'MXFP8_E4M3': 448.0, 'MXFP8_E5M2': 57344.0, 'MXFP6_E3M2': 28.0, 'MXFP6_E2M3': 7.5, 'MXFP4_E2M1': 6.0, 'MXINT8': 127 / 64}
    for fmt in FORMATS:
        t = R.table(fmt)
        assert len(t) == sizes[fmt] and t[0] == 0.0 and np.all(np.diff(t) > 0)
        assert t[-1] == tops[fmt] == MXFormat[fmt].max_normal
        assert R.EMAX[fmt] == MXFormat[fmt].emax
        assert 2.0 ** R.EMAX[fmt] <= t[-1] < 2.0 ** (R.EMAX[fmt] + 1)


@pytest.mark.parametrize('fmt', list(R.KNOWN_ANSWERS))
def test_known_answers(fmt):
    code, first = R.KNOWN_ANSWERS[fmt]
    for what, (y, c) in (('oracle', R.quantize(R.KNOWN_BLOCK[None], fmt)), ('torch arm', torch_arm(R.KNOWN_BLOCK[None], fmt))):
        assert int(c[0, 0]) == code, what
        assert np.array_equal(R.bits(y[0, :8]), R.bits(np.array(first, np.float32))), (what, y[0, :8])
        assert not y[0, 8:].any(), what


# ---------------------------------------------------------------------------------------------------------- the torch arm on the CPU
@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arm_layouts(fmt):
    for k, (shape, axis) in enumerate(R.LAYOUTS + [(R.CHANNELS_LAST_SHAPE, 1)]):
        x = R.layout_input(shape, seed=k)
        assert_same(torch_arm(x, fmt, axis), R.quantize(x, fmt, axis), f'{fmt} {shape} axis {axis}')


@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arm_special_blocks(fmt):
    x = R.special_blocks(fmt)
    got, want = torch_arm(x, fmt), R.quantize(x, fmt)
    assert_same(got, want, fmt)
    y, c = want
    assert np.array_equal(R.bits(y[0]), R.bits(x[0])) and c[0, 0] == 0                   # signed zeros stay; se = -127
    assert c[1, 0] == 0 and c[5, 0] == 0                                                 # subnormal amax; no finite element
    assert c[2, 0] == 127 + 127 - R.EMAX[fmt]
    assert np.isnan(y[3, 5]) and np.isfinite(np.delete(y[3], 5)).all()
    top = np.float32(R.table(fmt)[-1]) * np.float32(2.0) ** (int(c[4, 0]) - 127)
    assert y[4, 3] == top and y[4, 17] == -top
    assert np.array_equal(np.isnan(y[5]), np.isnan(x[5])) and np.isfinite(y[5][np.isinf(x[5])]).all()
    if fmt == 'MXFP4_E2M1': assert list(y[6, 1:9]) == [1, 1, 2, 4, -1, -1, -2, -4]       # ties go to the even encoding


@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arm_gaussian_blocks_and_idempotence(fmt):
    x = R.gaussian_blocks()
    y, c = torch_arm(x, fmt)
    assert_same((y, c), R.quantize(x, fmt), fmt)
    assert_same(torch_arm(y, fmt), (y, c), fmt + ' quantised again')


@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arm_exhaustive_cast(fmt):
    x = R.exhaustive_blocks(fmt)
    got, want = torch_arm(x, fmt), R.quantize(x, fmt)
    assert (want[1] == 127).all()                                                        # X = 1 in every block
    assert_same(got, want, fmt)


def test_straight_through_gradient():
    x = torch.from_numpy(R.layout_input((3, 40), 1)).requires_grad_()
    g = torch.from_numpy(R.layout_input((3, 40), 2))
    mx_fake_quant(x, MXFormat.MXFP4_E2M1, use_kernels=False).backward(g)
    assert torch.equal(x.grad, g)


def test_formats_and_delegator():
    assert [f.name for f in MXFormat] == FORMATS and [f.value for f in MXFormat] == list(range(6))
    assert MXFormat.of('MXFP6_E2M3') is MXFormat.MXFP6_E2M3 and MXFormat.of(4) is MXFormat.MXFP4_E2M1
    assert (mx_block_axis('Conv', 0), mx_block_axis('Conv', 1), mx_block_axis('Gemm', 0), mx_block_axis('Gemm', 1)) == (1, 1, -1, -1)
    assert (mx_block_axis('MatMul', 0), mx_block_axis('MatMul', 1)) == (-1, -2)
    x = torch.from_numpy(R.layout_input((4, 35, 3, 3), 4))
    d = MXDelegator('MXFP8_E4M3', 1, use_kernels=False)
    assert_same((d(x, None).numpy(), np.zeros(0)), (R.quantize(x.numpy(), 'MXFP8_E4M3', 1)[0], np.zeros(0)), 'delegator')

    class Parked:
        from ppq_amd.core import QuantizationStates
        state = QuantizationStates.FP32
    assert d(x, Parked) is x                                                             # a dequantised operation passes through


def test_error_paths():
    x = torch.zeros(4, 64)
    with pytest.raises(ValueError, match='block size'): ffi.CUDA.MXQuantize(x, 'MXFP4_E2M1', -1, block_size=16)
    with pytest.raises(RuntimeError, match='Invalid dtype'): mx_fake_quant(x.double(), 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='Invalid dtype'): mx_fake_quant(x.half(), 'MXFP4_E2M1')
    with pytest.raises(RuntimeError, match='out of range'): mx_fake_quant(x, 'MXFP4_E2M1', axis=2, use_kernels=False)
    with pytest.raises(ValueError, match='unknown MX format'): mx_fake_quant(x, 'MXFP4_E3M0', use_kernels=False)
    with pytest.raises(ValueError, match='unknown MX format'): mx_fake_quant(x, 6, use_kernels=False)
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_fake_quant(x, 'MXFP4_E2M1')
    with pytest.raises(RuntimeError, match='not on the GPU'): ffi.MXQuantizePlan([(x, 'MXFP4_E2M1', -1)])
    with pytest.raises(RuntimeError, match='scale_codes'):
        mx_fake_quant(x, 'MXFP4_E2M1', scale_codes=torch.zeros(4, 3, dtype=torch.uint8), use_kernels=False)


def test_c_entry_points_check_arguments_without_a_device():
    """Format, sizes, null pointers, the job table and overlap are checked on the host before anything is launched."""
    lib = _lib.lib
    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data

    def single(x, y, codes, outer, length, inner, fmt):
        return lib.ppqhip_mx_fq(x, y, codes, outer, length, inner, fmt, None), _lib.last_error()
    assert single(p, p + 512, 0, 1, 64, 1, 6) == (-1, 'mx_fq: job 0: unknown MX format 6')
    assert single(p, p + 512, 0, 1, 64, 1, -1)[0] == -1
    assert single(p, p + 512, 0, -1, 64, 1, 0) == (-1, 'mx_fq: job 0: negative size')
    assert single(0, p, 0, 1, 64, 1, 0) == (-1, 'mx_fq: job 0 has a null pointer')
    assert single(p, 0, 0, 1, 64, 1, 0) == (-1, 'mx_fq: job 0 has a null pointer')
    assert single(p, p + 4, 0, 1, 64, 1, 0) == (-1, 'mx_fq: an output overlaps an input')           # shifted by one element
    assert single(p, p + 512, p + 128, 1, 64, 1, 0) == (-1, 'mx_fq: an output overlaps an input')   # the codes inside x
    assert single(p, p + 512, 0, 1 << 20, 1 << 20, 1, 0) == (-1, 'mx_fq: job 0: more than 2^31 - 1 elements')
    assert single(p, p, 0, 0, 64, 1, 0)[0] == 0                                                      # empty: nothing to launch

    jobs = np.zeros(2, dtype=ffi._MX_JOB)
    jobs[0] = (p, p + 512, 0, 1, 64, 1, 0, 0)
    jobs[1] = (p + 256, p + 512, 0, 1, 64, 1, 4, 0)
    assert lib.ppqhip_mx_fq_multi(jobs.ctypes.data, -1, None) == -1 and _lib.last_error() == 'mx_fq_multi: bad job table'
    assert lib.ppqhip_mx_fq_multi(None, 2, None) == -1 and _lib.last_error() == 'mx_fq_multi: bad job table'
    assert lib.ppqhip_mx_fq_multi(jobs.ctypes.data, 2, None) == -1 and _lib.last_error() == 'mx_fq_multi: two outputs overlap in memory'
    jobs[1]['format'] = 9
    assert lib.ppqhip_mx_fq_multi(jobs.ctypes.data, 2, None) == -1 and _lib.last_error() == 'mx_fq_multi: job 1: unknown MX format 9'
    assert lib.ppqhip_mx_fq_multi(None, 0, None) == 0
    assert ctypes.sizeof(ctypes.c_void_p) * 3 + 8 * 3 + 8 == ffi._MX_JOB.itemsize                    # the layout of ppqhip_mx_job
