"""INT4 weights of the linear INT8 layers without a GPU (ppq_amd/int8.py Int4Weight): the packed layout, the
torch arm against the NumPy oracle (tests/int8_reference.py) on the unpacked codes bit for bit, every refusal, the C entry points'
argument checks."""
import numpy as np
import pytest
import torch

import int8_reference as R
from ppq_amd import Int4Weight, Int8Tensor, _lib, int4_pack, int4_quantize_weight, int4_unpack, int8_conv2d_packed, int8_matmul, int8_quantize
from test_host_int8 import MN, SX, bits, config, pair, stored


def weights(rng, rows, k):
    """Uniform random codes over -8 .. 7 inclusive as [rows, ceil32(k)], the padding 0."""
    codes = np.zeros((rows, R.ceil32(k)), np.int8)
    codes[:, :k] = rng.integers(-8, 8, (rows, k))
    return codes


def run_gemm(dev, use_kernels, m, n, k, zx=-7, bias=True, residual=False, relu=False, out=None, out_float=None):
    """One case of the GEMM with a packed INT4 weight on ``dev`` against the oracle on the unpacked codes, on bits."""
    rng = np.random.default_rng(1000 * m + k)
    a, b, sw = R.operands(rng, m, k, zx), weights(rng, n, k), (rng.random(n) * 0.01 + 0.005).astype(np.float32)
    tb = rng.standard_normal(n).astype(np.float32) if bias else None
    tr = (rng.standard_normal((m, n)) * 40).astype(np.float32) if residual else None
    A, B = pair(dev, a, b, (m, k), (n, k), zx, sw)
    B = int4_pack(B)
    if zx == 0: B.sums = None                                                            # int8_matmul must not need them
    dv = lambda v: torch.from_numpy(v).to(dev) if v is not None else None
    got = int8_matmul(A, B, dv(tb), dv(tr), relu, out, out_float, use_kernels=use_kernels)
    _, v, q = R.layer(a, b, zx, np.float32(SX) * sw, tb, tr, relu, stored(out) if out is not None else None)
    y, p = (got, None) if out is None else (got if out_float else (None, got))
    if y is not None: assert np.array_equal(bits(y), v.view(np.int32))
    if p is not None: assert np.array_equal(p.values.cpu().numpy(), q) and (p.shape, p.axis, p.zero_point) == ((m, n), 1, stored(out)[1])


def conv_case(dev, g, zx):
    """The operands of one geometry at batch 2: (X, W as an Int8Tensor, bias, the oracle's (v, q), the output config, (oh, ow))."""
    c, h, w, kh, kw, stride, pad, dil, o = g
    rng = np.random.default_rng(c + 10 * o)
    x, wt = R.operands(rng, 2 * h * w, c, zx).reshape(2, h, w, -1), weights(rng, o * kh * kw, c).reshape(o, kh, kw, -1)
    sw, bias = (rng.random(o) * 0.01 + 0.005).astype(np.float32), rng.standard_normal(o).astype(np.float32)
    a, out_hw = R.gather(x, kh, kw, stride, pad, dil, zx)
    out = config(0.25, 131, 0, 255)
    _, v, q = R.layer(a, wt.reshape(o, -1), zx, np.float32(SX) * sw, bias, None, False, stored(out))
    X, W = pair(dev, x, wt, (2, c, h, w), (o, c, kh, kw), zx, sw)
    return X, W, torch.from_numpy(bias).to(dev), (v, q), out, out_hw


def run_conv(dev, use_kernels, g, zx=5):
    """One geometry with a packed INT4 weight on ``dev`` against the oracle: both outputs, bias."""
    X, W, bias, (v, q), out, (oh, ow) = conv_case(dev, g, zx)
    W = int4_pack(W)
    if zx == 0: W.sums = None
    y, p = int8_conv2d_packed(X, W, bias, g[5], g[6], g[7], None, False, out, True, use_kernels=use_kernels)
    assert list(y.shape) == [2, g[8], oh, ow] and np.array_equal(bits(y.permute(0, 2, 3, 1)), v.view(np.int32).reshape(2, oh, ow, -1))
    assert np.array_equal(p.values.cpu().numpy().reshape(len(q), -1), q) and (p.shape, p.axis) == ((2, g[8], oh, ow), 1)


@pytest.mark.parametrize('k', [1, 9, 40])
def test_pack_and_unpack_on_all_16_codes(k):
    codes = np.zeros((16, R.ceil32(k)), np.int8)
    codes[:, :k] = (np.arange(16)[:, None] + 5 * np.arange(k)[None, :]) % 16 - 8
    w = Int8Tensor(torch.from_numpy(codes), (16, k), 1, torch.tensor(0.5), 0, -8, 7, 0)
    p = int4_pack(w)
    assert p.values.dtype == torch.uint8 and p.values.shape == (16, R.ceil32(k) // 2) and (p.shape, p.axis, p.zero_point) == ((16, k), 1, 0)
    assert torch.equal(p.sums, w.values.sum(1, dtype=torch.int32)) and torch.equal(int4_unpack(p).values, w.values)
    assert torch.equal(p.dequantize(), w.dequantize())


def test_the_byte_layout_of_one_group():
    """Byte j of a group holds code j in bits 0 .. 3 and code 4 + j in bits 4 .. 7; the group's dword p then gives the kernel's
    fragment: (p << 4) & 0xf0f0f0f0 and p & 0xf0f0f0f0 are 16 * the codes as int8 bytes, in order."""
    group = np.array([-8, -1, 0, 7, 3, -8, 7, -2], np.int8)
    codes = np.zeros((1, 32), np.int8)
    codes[0, 8:16] = group
    v = int4_pack(Int8Tensor(torch.from_numpy(codes), (1, 32), 1, torch.tensor(1.), 0, -8, 7, 0)).values.numpy()
    assert v[0, 4:8].tolist() == [0x38, 0x8f, 0x70, 0xe7] and not v[0, :4].any() and not v[0, 8:].any()
    p = v[0, 4:8].view(np.uint32)
    frag = np.concatenate([(p << 4) & 0xf0f0f0f0, p & 0xf0f0f0f0]).view(np.int8)
    assert np.array_equal(frag, 16 * group)


@pytest.mark.parametrize('k', [1, 9, 33, 300])
def test_torch_arm_gemm_is_the_oracle(k):
    for m, n in MN: run_gemm('cpu', False, m, n, k)


@pytest.mark.parametrize('g', R.GEOMETRIES, ids=str)
def test_torch_arm_conv_is_the_oracle(g):
    run_conv('cpu', False, g)
    if g[0] == 40: run_conv('cpu', False, g, zx=0)


def test_quantize_weight_is_int8_quantize_then_pack():
    w = torch.randn(9, 40, 3, 3, generator=torch.Generator().manual_seed(5))
    for cfg in (config(w.abs().amax((1, 2, 3)) / 7, torch.zeros(9), -8, 7, channel_axis=0), config(0.3, 0, -7, 7, rounding=4)):
        got, want = int4_quantize_weight(w, cfg, 1, use_kernels=False), int4_pack(int8_quantize(w, cfg, 1, weight=True, use_kernels=False))
        assert isinstance(got, Int4Weight) and got.values.shape == (9, 3, 3, 32) and torch.equal(got.values, want.values) and torch.equal(got.sums, want.sums)
        assert (got.qmin, got.qmax, got.rounding) == (cfg.quant_min, cfg.quant_max, cfg.rounding.value) and torch.equal(got.scale, want.scale)
        assert torch.equal(got.dequantize(), int8_quantize(w, cfg, 1, weight=True, use_kernels=False).dequantize())


def test_refusals():
    w = torch.randn(8, 40)
    q = lambda cfg: int4_quantize_weight(w, cfg, 1, use_kernels=False)
    for cfg, msg in ((config(0.1, 0), 'int4_quantize_weight: the range -128 .. 127 does not lie in -8 .. 7'), (config(0.1, 0, 0, 15), 'does not lie in -8 .. 7'),
                     (config(0.1, 1, -8, 7), 'int4_quantize_weight: a weight must be symmetric'), (config(0.1, 0.5, -8, 7), 'int4_quantize_weight: the offset is not an integer'),
                     (config(torch.ones(40), torch.zeros(40), -8, 7, channel_axis=1), 'int4_quantize_weight: a weight is quantised per tensor or along axis 0')):
        with pytest.raises(RuntimeError, match=msg): q(cfg)
    W8 = int8_quantize(w, config(0.02, 0), 1, weight=True, use_kernels=False)
    X = int8_quantize(torch.randn(4, 40), config(0.03, 3), use_kernels=False)
    with pytest.raises(RuntimeError, match=r'int4_pack: the codes reach -?\d+ .. \d+: outside -8 .. 7'): int4_pack(W8)
    with pytest.raises(RuntimeError, match='int4_pack: a weight must be symmetric'): int4_pack(X)
    with pytest.raises(TypeError, match='int4_pack: expected an Int8Tensor'): int4_pack(w)
    with pytest.raises(TypeError, match='int4_unpack: expected an Int4Weight'): int4_unpack(W8)
    W = q(config(0.3, 0, -8, 7))
    big = Int4Weight(torch.zeros(1, 32768, dtype=torch.uint8), (1, 65505), 1, torch.tensor(1.), -8, 7, 0, torch.zeros(1, dtype=torch.int32))
    for call, msg in ((lambda: int8_matmul(W, W), 'x: expected an Int8Tensor'), (lambda: int8_matmul(X, w), 'w: expected an Int8Tensor or an Int4Weight'),
                      (lambda: int8_matmul(X, Int4Weight(W.values.view(torch.int8), W.shape, 1, W.scale, -8, 7, 0, W.sums)), 'w: the codes are torch.int8, not uint8'),
                      (lambda: int8_matmul(int8_quantize(torch.randn(4, 33), config(0.03, 3), use_kernels=False), W), 'K mismatch'),
                      (lambda: int8_matmul(Int8Tensor(torch.zeros(1, 65536, dtype=torch.int8), (1, 65505), 1, torch.tensor(1.), 0, -128, 127, 0), big),
                       'int8_matmul: a padded reduction length of 65536: 65536 and more could overflow int32'),
                      (lambda: int8_conv2d_packed(X, W), 'operands must be 4-d')):
        with pytest.raises((RuntimeError, TypeError), match=msg): call()


def test_c_entry_points_check_arguments_without_a_device():
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    buf = np.zeros(16384 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    # the layout of tests/test_host_int8.py; the packed weight at p + 1024 spans half of what it spans there
    def gemm(a=p, b=p + 1024, sums=p + 4096, zx=3, mul=p + 4352, res=p + 5120, c=p + 6144, q=p + 7168, grid=(1.0, 0, -128, 127, 0, 0), m=2, n=40, k=64, hw=4):
        return _lib.lib.ppqhip_int4_gemm(a, b, sums, zx, mul, p + 4608, res, 1, c, q, *grid, m, n, k, None), _lib.last_error()

    def conv(a=p, b=p + 1024, sums=p + 4096, zx=3, mul=p + 4352, res=p + 5120, c=p + 6144, q=p + 7168, grid=(1.0, 0, -128, 127, 0, 0), m=1, n=2, k=64, hw=4):
        return _lib.lib.ppqhip_int4_conv2d(a, b, sums, zx, mul, p + 4608, res, 1, c, q, *grid, m, k, hw, hw, n, 3, 3, 1, 1, 0, 0, 1, 1, None), _lib.last_error()

    for call, what, y in ((gemm, 'int4_gemm', 'c'), (conv, 'int4_conv2d', 'y')):
        assert call(c=0, q=0) == (-1, f'{what}: no output: {y} and q are both null')
        assert call(zx=128) == (-1, f'{what}: zx 128 is not an int8 zero point')
        assert call(grid=(1.0, 0, -129, 127, 0, 0))[0] == -1 and call(grid=(1.0, 0, -128, 127, 5, 0)) == (-1, f'{what}: rounding policy 5 has no tensor form (ppq_tensor_round)')
        assert call(m=-1) == (-1, f'{what}: negative size')
        assert call(a=0) == (-1, f'{what}: null pointer') == call(b=0) == call(mul=0)
        assert call(sums=0) == (-1, f'{what}: sums is required with a zero point other than 0') and call(sums=0, zx=0, m=0)[0] == 0
        assert call(a=p + 8) == (-1, f'{what}: operands, {y} and q must be 16-byte aligned') == call(b=p + 1032) == call(c=p + 6144 + 4) == call(q=p + 7168 + 8)
        for out in ({'c': p + 5120}, {'q': p + 4352}, {'q': p + 16}, {'q': p + 1024}): assert call(**out) == (-1, f'{what}: an output overlaps an input')
        assert call(q=p + 6144) == (-1, f'{what}: two outputs overlap in memory')
        assert call(m=0)[0] == 0 and call(n=0)[0] == 0                                   # nothing to launch
    assert gemm(k=65505)[1].startswith('int4_gemm: a padded reduction length of 65536') and conv(k=7296)[1].startswith('int4_conv2d: a padded reduction length of 65664')
    assert gemm(m=2 ** 31 - 1, n=2 ** 31 - 1, k=0) == (-1, 'int4_gemm: too many workgroups in one launch')
    assert conv(m=2 ** 27, n=2 ** 31 - 1, k=32, hw=3) == (-1, 'int4_conv2d: too many workgroups in one launch')
