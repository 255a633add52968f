"""The packed MX export without a GPU: the oracle (tests/mx_pack_reference.py) against answers worked out by hand, the
``use_kernels=False`` arm of ppq_amd.mx against the oracle byte for byte, the round trip against ``mx_fake_quant``, foreign codes,
``MXTensor`` through ``torch.save``, and the host-side argument checks of the C entry points (they run before any launch)."""
import ctypes
import io

import numpy as np
import pytest
import torch

import mx_pack_reference as P
import mx_reference as R
from ppq_amd import MXFormat, MXTensor, _lib, ffi, mx_dequantize, mx_fake_quant, mx_quantize

FORMATS = R.FORMATS


def torch_pack(x: np.ndarray, fmt: str, axis: int = -1):
    t = mx_quantize(torch.from_numpy(np.ascontiguousarray(x)), fmt, axis, use_kernels=False)
    return t.elements.numpy(), t.scales.numpy()


def assert_same(got, want, what):
    (e, s), (re_, rs) = got, want
    assert e.shape == re_.shape and s.shape == rs.shape, (what, e.shape, re_.shape, s.shape, rs.shape)
    assert e.dtype == np.uint8 and s.dtype == np.uint8, what
    assert np.array_equal(s, rs), f'{what}: scales differ'
    bad = np.flatnonzero(e.ravel() != re_.ravel())
    assert bad.size == 0, f'{what}: {bad.size} element bytes differ, first at {bad[:4]}: {e.ravel()[bad[:4]]} != {re_.ravel()[bad[:4]]}'


# ------------------------------------------------------------------------------------------------------------------ known answers
def test_known_answer_fp4():
    """R.KNOWN_BLOCK in MXFP4: X = 1; 0.5, -1.5, 3, 6, -6, 0, 0.5, 1 are the codes 1, B, 5, 7, F, 0, 1, 2; element 2i is the low nibble."""
    want = bytes([0xB1, 0x75, 0x0F, 0x21] + [0] * 12)
    for what, (e, s) in (('oracle', P.pack(R.KNOWN_BLOCK[None], 'MXFP4_E2M1')), ('torch arm', torch_pack(R.KNOWN_BLOCK[None], 'MXFP4_E2M1'))):
        assert e.shape == (1, 16) and s.shape == (1, 1), what
        assert int(s[0, 0]) == 127 and e[0].tobytes() == want, (what, e[0].tobytes().hex())


def test_known_answer_fp6():
    """R.KNOWN_BLOCK in MXFP6 E2M3 (bias 1, subnormal step 1/8): X = 1; 0.25, -1.25, 2.5, 5, -7, 0.25, 0.25, 0.75 are
    0.00.010 = 2, 1.01.010 = 42, 0.10.010 = 18, 0.11.010 = 26, 1.11.110 = 62, 2, 2, 0.00.110 = 6.  Four codes make three bytes:
    2 | 42 << 6 | 18 << 12 | 26 << 18 = 0x692A82 and 62 | 2 << 6 | 2 << 12 | 6 << 18 = 0x1820BE, least significant byte first."""
    assert R.KNOWN_ANSWERS['MXFP6_E2M3'] == (127, [0.25, -1.25, 2.5, 5, -7, 0.25, 0.25, 0.75])
    want = bytes([0x82, 0x2A, 0x69, 0xBE, 0x20, 0x18] + [0] * 18)
    for what, (e, s) in (('oracle', P.pack(R.KNOWN_BLOCK[None], 'MXFP6_E2M3')), ('torch arm', torch_pack(R.KNOWN_BLOCK[None], 'MXFP6_E2M3'))):
        assert e.shape == (1, 24) and int(s[0, 0]) == 127, what
        assert e[0].tobytes() == want, (what, e[0].tobytes().hex())


def test_oracle_fields_round_trip():
    rng = np.random.default_rng(2)
    for w in (4, 6, 8):
        c = rng.integers(0, 1 << w, (5, 3, 32)).astype(np.uint8)
        e = P.pack_fields(c, w)
        assert e.shape == (5, 3, 4 * w) and np.array_equal(P.unpack_fields(e, w), c)


# ---------------------------------------------------------------------------------------------------------- the torch arm on the CPU
@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arm_layouts(fmt):
    for k, (shape, axis) in enumerate(R.LAYOUTS + [(R.CHANNELS_LAST_SHAPE, 1)]):
        x = R.layout_input(shape, seed=k)
        want = P.pack(x, fmt, axis)
        assert_same(torch_pack(x, fmt, axis), want, f'{fmt} {shape} axis {axis}')
        lead = [d for i, d in enumerate(shape) if i != axis % len(shape)]
        nb = (shape[axis] + 31) // 32
        assert list(want[0].shape) == lead + [nb * P.BLOCK_BYTES[fmt]] and list(want[1].shape) == lead + [nb]


@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arm_special_blocks(fmt):
    x = R.special_blocks(fmt)
    e, s = want = P.pack(x, fmt)
    assert_same(torch_pack(x, fmt), want, fmt)
    B = P.BLOCK_BYTES[fmt]
    c = P.unpack_fields(e.reshape(len(x), 1, B), P.WIDTH[fmt])[:, 0]
    if fmt == 'MXINT8': assert not c[0].any()                                            # no -0 in two's complement
    else: assert np.array_equal(c[0] != 0, np.signbit(x[0])) and set(c[0]) == {0, 1 << (P.WIDTH[fmt] - 1)}      # zero keeps its sign
    if fmt in P.HAS_NAN:
        assert c[3, 5] == 0x7f | (int(np.signbit(x[3, 5])) << 7) and s[3, 0] == R.quantize(x, fmt)[1][3, 0]      # the element is NaN
        assert np.array_equal(c[5] & 0x7f == 0x7f, np.isnan(x[5])) and s[5, 0] == 0
        top = len(R.table(fmt)) - 1
        assert c[4, 3] == top and c[4, 17] == top | 0x80                                 # Inf saturates; no Inf code is written
    else:
        assert s[3, 0] == 0xff and not e[3].any() and s[5, 0] == 0xff and not e[5].any()   # the block is NaN
        assert s[4, 0] != 0xff
        top = 127 if fmt == 'MXINT8' else len(R.table(fmt)) - 1
        assert c[4, 3] == top and c[4, 17] == ((256 - 127) if fmt == 'MXINT8' else top | (1 << (P.WIDTH[fmt] - 1)))


@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arm_exhaustive_cast(fmt):
    x = R.exhaustive_blocks(fmt)
    want = P.pack(x, fmt)
    assert (want[1] == 127).all()
    assert_same(torch_pack(x, fmt), want, fmt)


# ----------------------------------------------------------------------------------------------------------------------- round trip
def round_trip(x: np.ndarray, fmt: str, axis: int = -1):
    t = torch.from_numpy(np.ascontiguousarray(x))
    got = mx_dequantize(mx_quantize(t, fmt, axis, use_kernels=False), use_kernels=False)
    want = mx_fake_quant(t, fmt, axis, use_kernels=False)
    assert got.shape == want.shape and got.is_contiguous()
    return got.numpy(), want.numpy()


@pytest.mark.parametrize('fmt', FORMATS)
def test_round_trip_equals_fake_quant(fmt):
    cases = [(R.layout_input(shape, seed=k), axis) for k, (shape, axis) in enumerate(R.LAYOUTS)]
    cases += [(R.gaussian_blocks()[:256], -1), (R.special_blocks(fmt), -1), (np.ascontiguousarray(R.special_blocks(fmt).T), 0)]
    for x, axis in cases:
        got, want = round_trip(x, fmt, axis)
        mask = P.nan_mask(x, fmt, axis)
        assert P.same_but_nan(got, want, mask, fmt), (fmt, x.shape, axis)
        assert np.array_equal(R.bits(got)[mask] & np.uint32(0x7fffffff), np.full(int(mask.sum()), 0x7fc00000, np.uint32))
        oracle = P.unpack(*P.pack(x, fmt, axis), fmt, x.shape, axis)
        assert np.array_equal(R.bits(got), R.bits(oracle)), (fmt, x.shape, axis)


def test_round_trip_corner_rules():
    x = R.special_blocks('MXINT8')
    got, want = round_trip(x, 'MXINT8')
    assert (R.bits(want[0]) == 0x80000000).any() and not R.bits(got[0]).any()            # MXINT8: -0 comes back as +0
    x = R.special_blocks('MXFP8_E4M3')
    got, want = round_trip(x, 'MXFP8_E4M3')
    assert np.isnan(got[3, 5]) and np.array_equal(R.bits(np.delete(got[3], 5)), R.bits(np.delete(want[3], 5)))   # the element alone
    x = R.special_blocks('MXFP4_E2M1')
    got, want = round_trip(x, 'MXFP4_E2M1')
    assert np.isnan(got[3]).all() and np.isfinite(np.delete(want[3], 5)).all()           # the whole block
    assert np.array_equal(R.bits(got[4]), R.bits(want[4]))                               # Inf saturates in both


# -------------------------------------------------------------------------------------------------------------------- foreign codes
@pytest.mark.parametrize('fmt', FORMATS)
def test_foreign_codes(fmt):
    """Every code under scale 127 (256, 64 or 16 of them), and under scale 0xFF; E5M2 holds Inf and NaN codes, MXINT8 -128."""
    e, s = P.foreign_codes(fmt)
    n = s.shape[-1] * 32
    want = P.unpack(e, s, fmt, (2, n))
    t = MXTensor(fmt, (2, n), 1, torch.from_numpy(e), torch.from_numpy(s))
    got = t.dequantize(use_kernels=False).numpy()
    assert np.array_equal(R.bits(got), R.bits(want))
    assert np.isnan(want[1]).all()                                                       # scale 0xFF: the whole block
    c = np.arange(1 << P.WIDTH[fmt])
    if fmt == 'MXINT8':
        assert want[0, 128] == -2.0 and want[0, 255] == -1 / 64 and want[0, 127] == 127 / 64 and not np.isnan(want[0]).any()
        assert (R.bits(want[1]) == 0x7fc00000).all()
    elif fmt == 'MXFP8_E5M2':
        assert want[0, 0x7c] == np.inf and want[0, 0xfc] == -np.inf
        assert [hex(v) for v in R.bits(want[0, [0x7d, 0x7e, 0x7f, 0xfd, 0xff]])] == ['0x7fc00000'] * 3 + ['0xffc00000'] * 2
        assert np.isfinite(want[0, :0x7c]).all() and want[0, 0x7b] == 57344.0
    elif fmt == 'MXFP8_E4M3':
        assert hex(R.bits(want[0])[0x7f]) == '0x7fc00000' and hex(R.bits(want[0])[0xff]) == '0xffc00000'
        assert np.isfinite(np.delete(want[0][:256], [0x7f, 0xff])).all() and want[0, 0x7e] == 448.0
        assert np.array_equal(R.bits(want[1][:256]) >> 31, c >> 7)                       # the element's sign bit on the NaN
    else:
        assert np.isfinite(want[0]).all() and (R.bits(want[1]) == 0x7fc00000).all()
        half = 1 << (P.WIDTH[fmt] - 1)
        assert np.array_equal(want[0, :half].astype(np.float64), R.table(fmt)) and np.array_equal(want[0, half:2 * half], -want[0, :half])


# ------------------------------------------------------------------------------------------------------------------------- MXTensor
def test_mxtensor_dict_round_trips_through_torch_save():
    x = torch.from_numpy(R.layout_input((4, 35, 3, 3), 4))
    t = mx_quantize(x, MXFormat.MXFP6_E3M2, 1, use_kernels=False)
    assert (t.format, t.shape, t.axis) == (MXFormat.MXFP6_E3M2, (4, 35, 3, 3), 1)
    assert list(t.elements.shape) == [4, 3, 3, 48] and list(t.scales.shape) == [4, 3, 3, 2] and t.nbytes == 36 * 2 * 25
    d = t.to_dict()
    assert all(isinstance(v, (torch.Tensor, int, str)) for v in d.values()) and d['format'] == 'MXFP6_E3M2'
    buf = io.BytesIO()
    torch.save(d, buf)
    buf.seek(0)
    back = MXTensor.from_dict(torch.load(buf, weights_only=True))
    assert (back.format, back.shape, back.axis) == (t.format, t.shape, t.axis)
    assert torch.equal(back.elements, t.elements) and torch.equal(back.scales, t.scales)
    assert torch.equal(mx_dequantize(back, False).view(torch.int32), mx_fake_quant(x, 'MXFP6_E3M2', 1, use_kernels=False).view(torch.int32))
    assert t.to('cpu').nbytes == t.nbytes
    with pytest.raises(ValueError, match='uint8'): MXTensor.from_dict({**d, 'elements': d['elements'].to(torch.int8)})
    with pytest.raises(ValueError, match='elements of shape'): MXTensor.from_dict({**d, 'elements': d['elements'][..., :-1]})
    with pytest.raises(ValueError, match='elements of shape'): MXTensor.from_dict({**d, 'format': 'MXFP4_E2M1'})
    with pytest.raises(ValueError, match='scales of shape'): MXTensor.from_dict({**d, 'scales': d['scales'][..., :1]})
    with pytest.raises(ValueError, match='unknown MX format'): MXTensor.from_dict({**d, 'format': 'MXFP4_E3M0'})
    with pytest.raises(ValueError, match='out of range'): MXTensor.from_dict({**d, 'axis': 4})
    with pytest.raises(ValueError, match='missing'): MXTensor.from_dict({'format': 'MXINT8'})


def test_error_paths():
    x = torch.zeros(4, 64)
    with pytest.raises(ValueError, match='block size'): ffi.CUDA.MXPack(x, 'MXFP4_E2M1', -1, block_size=16)
    with pytest.raises(RuntimeError, match='Invalid dtype'): mx_quantize(x.double(), 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='out of range'): mx_quantize(x, 'MXFP4_E2M1', axis=2, use_kernels=False)
    with pytest.raises(RuntimeError, match='Tensor is empty'): mx_quantize(x[:0], 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(ValueError, match='unknown MX format'): mx_quantize(x, 'MXFP4_E3M0', use_kernels=False)
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_quantize(x, 'MXFP4_E2M1')
    with pytest.raises(RuntimeError, match='not on the GPU'): ffi.MXPackPlan([(x, 'MXFP4_E2M1', -1)])
    t = mx_quantize(x, 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_dequantize(t)
    with pytest.raises(TypeError, match='MXTensor'): mx_dequantize(x)


# ---------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_entry_points_check_arguments_without_a_device():
    """Format, sizes, null pointers, the job table and overlap are checked on the host before anything is launched."""
    lib = _lib.lib
    buf = np.zeros(256, np.float32)                                                      # 1024 bytes
    p = buf.ctypes.data

    def pack(x, e, s, outer, length, inner, fmt):
        return lib.ppqhip_mx_pack(x, e, s, outer, length, inner, fmt, None), _lib.last_error()

    def unpack(e, s, y, outer, length, inner, fmt):
        return lib.ppqhip_mx_unpack(e, s, y, outer, length, inner, fmt, None), _lib.last_error()
    # x: 64 floats at p (256 B); elements at p + 512 (64 B); scales at p + 640 (2 B)
    assert pack(p, p + 512, p + 640, 1, 64, 1, 6) == (-1, 'mx_pack: job 0: unknown MX format 6')
    assert pack(p, p + 512, p + 640, 1, 64, 1, -1)[0] == -1
    assert pack(p, p + 512, p + 640, -1, 64, 1, 0) == (-1, 'mx_pack: job 0: negative size')
    assert pack(0, p + 512, p + 640, 1, 64, 1, 0) == (-1, 'mx_pack: job 0 has a null pointer')
    assert pack(p, 0, p + 640, 1, 64, 1, 0) == (-1, 'mx_pack: job 0 has a null pointer')
    assert pack(p, p + 512, 0, 1, 64, 1, 0) == (-1, 'mx_pack: job 0 has a null pointer')             # scales are required
    assert pack(p, p + 512, p + 640, 1 << 20, 1 << 20, 1, 0) == (-1, 'mx_pack: job 0: more than 2^31 - 1 elements')
    assert pack(p, p + 252, p + 640, 1, 64, 1, 0) == (-1, 'mx_pack: an output overlaps an input')    # elements start inside x
    assert pack(p, p + 512, p + 255, 1, 64, 1, 0) == (-1, 'mx_pack: an output overlaps an input')    # the scales' first byte is x's last
    assert pack(p, p + 512, p + 575, 1, 64, 1, 0) == (-1, 'mx_pack: two outputs overlap in memory')  # ... is the elements' last
    assert pack(p, p + 512, p + 543, 1, 64, 1, 4) == (-1, 'mx_pack: two outputs overlap in memory')  # FP4: 32 B of elements
    assert pack(p, p, p, 0, 64, 1, 0)[0] == 0                                                         # empty: nothing to launch
    assert pack(p, p, p, 1, 64, 0, 0)[0] == 0

    assert unpack(p + 512, p + 640, p, 1, 64, 1, 6) == (-1, 'mx_unpack: job 0: unknown MX format 6')
    assert unpack(p + 512, p + 640, p, 1, -64, 1, 0) == (-1, 'mx_unpack: job 0: negative size')
    assert unpack(p + 512, 0, p, 1, 64, 1, 0) == (-1, 'mx_unpack: job 0 has a null pointer')
    assert unpack(0, p + 640, p, 1, 64, 1, 0) == (-1, 'mx_unpack: job 0 has a null pointer')
    assert unpack(p + 512, p + 640, 0, 1, 64, 1, 0) == (-1, 'mx_unpack: job 0 has a null pointer')
    assert unpack(p + 512, p + 640, p, 1 << 20, 1 << 20, 1, 0) == (-1, 'mx_unpack: job 0: more than 2^31 - 1 elements')
    assert unpack(p + 252, p + 640, p, 1, 64, 1, 0) == (-1, 'mx_unpack: an output overlaps an input')
    assert unpack(p + 512, p + 255, p, 1, 64, 1, 0) == (-1, 'mx_unpack: an output overlaps an input')
    assert unpack(p, p, p, 0, 64, 1, 0)[0] == 0

    jobs = np.zeros(2, dtype=ffi._MX_PACK_JOB)
    jobs[0] = (p, p + 512, p + 640, 1, 64, 1, 0, 0)
    jobs[1] = (p + 256, p + 544, p + 648, 1, 64, 1, 4, 0)                                             # its elements inside job 0's
    assert lib.ppqhip_mx_pack_multi(jobs.ctypes.data, -1, None) == -1 and _lib.last_error() == 'mx_pack_multi: bad job table'
    assert lib.ppqhip_mx_pack_multi(None, 2, None) == -1 and _lib.last_error() == 'mx_pack_multi: bad job table'
    assert lib.ppqhip_mx_pack_multi(jobs.ctypes.data, 2, None) == -1 and _lib.last_error() == 'mx_pack_multi: two outputs overlap in memory'
    jobs[1]['elements'] = p + 128                                                                     # ... inside job 0's input
    assert lib.ppqhip_mx_pack_multi(jobs.ctypes.data, 2, None) == -1 and _lib.last_error() == 'mx_pack_multi: an output overlaps an input'
    jobs[1]['format'] = 9
    assert lib.ppqhip_mx_pack_multi(jobs.ctypes.data, 2, None) == -1 and _lib.last_error() == 'mx_pack_multi: job 1: unknown MX format 9'
    assert lib.ppqhip_mx_pack_multi(None, 0, None) == 0

    ujobs = np.zeros(2, dtype=ffi._MX_UNPACK_JOB)
    ujobs[0] = (p + 512, p + 640, p, 1, 64, 1, 0, 0)
    ujobs[1] = (p + 576, p + 648, p + 128, 1, 64, 1, 4, 0)                                            # its output inside job 0's
    assert lib.ppqhip_mx_unpack_multi(ujobs.ctypes.data, -1, None) == -1 and _lib.last_error() == 'mx_unpack_multi: bad job table'
    assert lib.ppqhip_mx_unpack_multi(None, 1, None) == -1 and _lib.last_error() == 'mx_unpack_multi: bad job table'
    assert lib.ppqhip_mx_unpack_multi(ujobs.ctypes.data, 2, None) == -1 and _lib.last_error() == 'mx_unpack_multi: two outputs overlap in memory'
    ujobs[1]['scales'] = 0
    assert lib.ppqhip_mx_unpack_multi(ujobs.ctypes.data, 2, None) == -1 and _lib.last_error() == 'mx_unpack_multi: job 1 has a null pointer'
    assert lib.ppqhip_mx_unpack_multi(None, 0, None) == 0
    for dtype in (ffi._MX_PACK_JOB, ffi._MX_UNPACK_JOB):
        assert ctypes.sizeof(ctypes.c_void_p) * 3 + 8 * 3 + 8 == dtype.itemsize                       # the layout of the job structs
