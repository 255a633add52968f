"""The contract of ppqhip_conv1x1 as tests/pointwise_conv_reference.py restates it (checked against libm's fmaf and against the
float64 result), ``harness.pointwise_eligible``, and every refusal the entry point makes on the host before it launches."""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

from pointwise_conv_reference import conv1x1_float64, conv1x1_reference, fma32, gamma

_libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _fmaf(a, b, c):
    return np.array([_libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def test_fma_emulation_matches_libm_on_random_operands():
    rng = np.random.default_rng(0)
    n = 20000
    for scale in (1.0, 1e-20, 1e19):
        a, b, c = (rng.standard_normal(n).astype(np.float32) * np.float32(scale) for _ in range(3))
        assert _same_bits(fma32(a, b, c), _fmaf(a, b, c))
    a, b = rng.standard_normal(n).astype(np.float32) * np.float32(1e-25), rng.standard_normal(n).astype(np.float32) * np.float32(1e-16)
    c = rng.standard_normal(n).astype(np.float32) * np.float32(1e-41)                # subnormal sums
    assert _same_bits(fma32(a, b, c), _fmaf(a, b, c))


def test_fma_emulation_matches_libm_next_to_float32_ties():
    """c + a b lies within 2^-70 of the midpoint of two float32 numbers: the float64 sum IS that midpoint, and only the sign of
    its rounding error says which neighbour is right (round-to-even on the float64 sum picks the wrong one half of the time)."""
    rng = np.random.default_rng(1)
    n = 4000
    c = (1.0 + rng.integers(0, 1 << 22, n) * 2.0 ** -23).astype(np.float32)              # in [1, 1.5): ulp 2^-23, odd and even
    sa, sb = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
    a = (2.0 ** -12 * (1.0 + sa * 2.0 ** -23)).astype(np.float32)
    b = (2.0 ** -12 * (1.0 + sb * rng.integers(1, 4, n) * 2.0 ** -23)).astype(np.float32)      # a b = 2^-24 (1 + O(2^-23)): half an ulp of c, off by < 2^-45
    # exact halves: a b = 2^-24 exactly (a tie, round to even) must also agree
    a[:100], b[:100] = np.float32(2.0 ** -12), np.float32(2.0 ** -12)
    for sign in (1.0, -1.0):
        bb = (b * np.float32(sign)).astype(np.float32)
        want = _fmaf(a, bb, c)
        got = fma32(a, bb, c)
        assert _same_bits(got, want)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert not _same_bits(naive, _fmaf(a, b, c)), 'the cases do not reach a double rounding: the test is vacuous'


def test_chain_is_the_scalar_fmaf_loop():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 40, 7, 7)).astype(np.float32)
    w = rng.standard_normal((70, 40)).astype(np.float32)
    bias = rng.standard_normal(70).astype(np.float32)
    for stride in (1, 2):
        y = conv1x1_reference(x, w, bias, stride)
        y0 = conv1x1_reference(x, w, None, stride)
        assert y.shape == (3, 70, (7 - 1) // stride + 1, (7 - 1) // stride + 1)
        for _ in range(200):
            n, o = int(rng.integers(3)), int(rng.integers(70))
            oh, ow = int(rng.integers(y.shape[2])), int(rng.integers(y.shape[3]))
            acc = 0.0
            for k in range(40): acc = _libm.fmaf(float(w[o, k]), float(x[n, k, oh * stride, ow * stride]), acc)
            assert np.float32(acc).view(np.int32) == y0[n, o, oh, ow].view(np.int32)
            assert (np.float32(acc) + bias[o]).view(np.int32) == y[n, o, oh, ow].view(np.int32)


@pytest.mark.parametrize('c', [40, 512])
def test_chain_within_the_recursive_summation_bound(c):
    rng = np.random.default_rng(c)
    x = rng.standard_normal((2, c, 5, 5)).astype(np.float32)
    w = rng.standard_normal((9, c)).astype(np.float32)
    y64, mag = conv1x1_float64(x, w)
    err = np.abs(conv1x1_reference(x, w).astype(np.float64) - y64)
    print(f'c = {c}: max err / bound = {float((err / (gamma(c) * mag)).max()):.3f}')
    assert np.all(err <= gamma(c) * mag)


# ---- pointwise_eligible ----------------------------------------------------------------------------------------------------------
class _T:
    """Stands in for a CUDA tensor on a box without one: the attributes pointwise_eligible reads."""
    def __init__(self, shape, dtype=torch.float32, cuda=True, contiguous=True, requires_grad=False):
        self.shape, self.dtype, self.is_cuda, self._c, self.requires_grad = torch.Size(shape), dtype, cuda, contiguous, requires_grad

    def dim(self): return len(self.shape)
    def is_contiguous(self, memory_format=torch.contiguous_format): return self._c and memory_format == torch.contiguous_format
    def numel(self): return int(np.prod(self.shape))


def test_pointwise_eligible_accepts_and_rejects(monkeypatch):
    from ppq_amd import harness
    monkeypatch.setattr(harness, 'isinstance', lambda v, t: True if type(v) is _T and t is torch.Tensor else isinstance(v, t), raising=False)
    ok = harness.pointwise_eligible
    x, w = _T((2, 64, 14, 14)), _T((96, 64, 1, 1))
    with torch.no_grad():
        assert ok(x, w, {}, 0) and ok(x, w, {'strides': 2}, 0) and ok(x, w, {'strides': [2, 2], 'pads': [0, 0, 0, 0], 'dilations': [1, 1], 'group': 1}, 0)
        work = 2.0 * 2 * 96 * 64 * 14 * 14
        assert ok(x, w, {}, work) and not ok(x, w, {}, work + 1)                      # work below min_work
        assert ok(x, w, {'strides': 2}, 2.0 * 2 * 96 * 64 * 7 * 7) and not ok(x, w, {'strides': 2}, 2.0 * 2 * 96 * 64 * 7 * 7 + 1)
        assert not ok(x, _T((96, 64, 3, 3)), {'pads': 1}, 0)                            # 3x3
        assert not ok(x, w, {'pads': 1}, 0)                                             # pad 1
        assert not ok(x, w, {'pads': [0, 0, 1, 1]}, 0)
        assert not ok(x, _T((96, 32, 1, 1)), {'group': 2}, 0)                           # groups 2
        assert not ok(x, w, {'group': 2}, 0)
        assert not ok(x, w, {'strides': 3}, 0)                                          # stride 3
        assert not ok(x, w, {'strides': [2, 1]}, 0)                                     # stride (2, 1)
        assert not ok(x, w, {'dilations': 2}, 0)
        assert not ok(_T((2, 64, 14, 14), contiguous=False), w, {}, 0)                  # channels-last / any other layout
        assert not ok(x, _T((96, 64, 1, 1), contiguous=False), {}, 0)
        assert not ok(_T((2, 64, 14, 14), dtype=torch.float64), _T((96, 64, 1, 1), dtype=torch.float64), {}, 0)     # float64
        assert not ok(_T((2, 64, 14, 14), cuda=False), w, {}, 0)                        # not on the GPU
        assert not ok(_T((2, 64, 14)), w, {}, 0)                                        # not 4-D
        assert not ok(_T((2, 64, 14, 14), requires_grad=True), w, {}, 0)                # requires_grad
        assert not ok(x, _T((96, 64, 1, 1), requires_grad=True), {}, 0)
        for key in harness.POINTWISE_KEEP_VENDOR:                                       # a class that measured slower keeps F.conv2d
            ci, co, h, wd, stride = key
            assert not ok(_T((32, ci, h, wd)), _T((co, ci, 1, 1)), {'strides': stride}, 0)
        assert ok(_T((32, 256, 14, 14)), _T((1024, 256, 1, 1)), {}, harness.POINTWISE_MIN_WORK)       # the headline's winners
        assert ok(_T((32, 256, 56, 56)), _T((512, 256, 1, 1)), {'strides': 2}, harness.POINTWISE_MIN_WORK)
        assert ok(_T((32, 512, 28, 28)), _T((128, 512, 1, 1)), {}, harness.POINTWISE_MIN_WORK)
        assert ok(_T((32, 512, 28, 28)), _T((1024, 512, 1, 1)), {'strides': 2}, harness.POINTWISE_MIN_WORK)
        assert not ok(_T((8, 256, 14, 14)), _T((1024, 256, 1, 1)), {}, harness.POINTWISE_MIN_WORK)    # batch 8 stays with MIOpen
    with torch.enable_grad():
        assert not ok(x, w, {}, 0)                                                      # grad enabled
    assert not ok(torch.zeros(2, 64, 14, 14), torch.zeros(96, 64, 1, 1), {}, 0)         # a real CPU tensor


def test_channels_last_real_tensors_are_not_eligible():
    from ppq_amd import harness
    x = torch.zeros(2, 8, 4, 4).contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous()
    with torch.no_grad(): assert not harness.pointwise_eligible(x, torch.zeros(4, 8, 1, 1), {}, 0)


# ---- host refusals of the entry point: nothing below reaches a launch, so no device is needed ---------------------------------------
def _call(x=64, w=4096, bias=0, y=8192, n=1, c=2, h=2, wd=2, o=2, stride=1):
    from ppq_amd import _lib
    return _lib.lib.ppqhip_conv1x1(x, w, bias, y, n, c, h, wd, o, stride, 0), _lib.last_error()


def test_entry_point_refusals_without_a_launch():
    from ppq_amd import _lib
    inv, uns = -1, -2
    for kw in ({'x': 0}, {'w': 0}, {'y': 0}):
        st, msg = _call(**kw)
        assert st == inv and msg == 'conv1x1: null pointer', (kw, st, msg)
    for kw in ({'n': -1}, {'c': 0}, {'h': 0}, {'wd': -3}, {'o': 0}):
        st, msg = _call(**kw)
        assert st == inv and msg == 'conv1x1: non-positive size', (kw, st, msg)
    for kw in ({'n': 1 << 20, 'c': 1 << 6, 'h': 1 << 3, 'wd': 1 << 2}, {'n': 1 << 20, 'o': 1 << 10, 'c': 1}, {'o': 1 << 16, 'c': 1 << 15, 'h': 1, 'wd': 1},
               {'n': 1 << 40}):
        st, msg = _call(**kw)
        assert st == inv and msg == 'conv1x1: more than 2^31 - 1 elements in x, w or y', (kw, st, msg)
    for stride in (0, 3, -1):
        st, msg = _call(stride=stride)
        assert st == uns and msg == 'conv1x1: stride must be 1 or 2', (stride, st, msg)
    # y [1,2,2,2] = 32 bytes, x [1,2,2,2] = 32 bytes, w [2,2] = 16 bytes, bias 8 bytes
    for kw in ({'x': 4096, 'y': 4096 + 28}, {'x': 4096 + 28, 'y': 4096}, {'w': 8192 + 28}, {'w': 8192 - 12}, {'bias': 8192 + 28}, {'bias': 8192 - 4}):
        st, msg = _call(**kw)
        assert st == inv and msg == 'conv1x1: an output overlaps an input', (kw, st, msg)
    assert _call(n=0)[0] == 0                                                           # nothing to do, nothing launched
    assert _call(n=0, x=0, w=0, y=0)[0] == 0
    for kw in ({'x': 66}, {'w': 4097}, {'y': 8195}, {'bias': 16386}):                   # no path for a pointer off the 4-byte grid
        assert _call(**kw)[0] == _lib.NOT_FUSED, kw
