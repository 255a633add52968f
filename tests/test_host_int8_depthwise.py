"""The depthwise linear INT8 layer without a GPU (ppq_amd/int8.py): the torch arm against the NumPy oracle
(tests/int8_depthwise_reference.py) and against the dense layer on the block-diagonal weight, bit for bit; the refusals; the C entry
point's argument checks."""
import numpy as np
import pytest
import torch

import int8_depthwise_reference as D
import int8_reference as R
from ppq_amd import (Int8DepthwiseWeight, Int8Tensor, _lib, int8_conv2d, int8_conv2d_packed, int8_depthwise_conv2d, int8_depthwise_conv2d_packed,
                     int8_depthwise_weight, int8_quantize)
from test_host_int8 import SX, bits, config, stored

C40 = D.GEOMETRIES[1]
# the C = 40 geometry again: sums null; the whole tail, codes only, on a channels-last and on a contiguous residual; one weight scale; a
# NaN and a -0.0 in bias and residual under the ReLU
VARIANTS = [dict(zx=0), dict(residual='channels_last', relu=True, out_float=False), dict(residual='contiguous', relu=True, out_float=False),
            dict(per_channel=False), dict(residual='channels_last', relu=True, plant=True)]
# the largest |I| the kernel can meet: 49 live taps of (-128) * (-128 - 127) at the centre of a 9 x 9 image, fewer towards its padding
EXTREME = ((32, 9, 9, 7, 7, (1, 1), (3, 3), (1, 1)), dict(zx=127, codes=-128))


def operands(dev, g, zx, per_channel=True, codes=None):
    """Raw codes of geometry g and their Int8Tensor / Int8DepthwiseWeight on dev: x with zero point zx and scale SX, w with the scales sw."""
    c, h, w, kh, kw = g[:5]
    rng = np.random.default_rng(c + 100 * kh)
    x, wt = R.operands(rng, 2 * h * w, c, zx).reshape(2, h, w, -1), R.operands(rng, kh * kw, c).reshape(kh, kw, -1)
    if codes is not None: x[..., :c], wt[..., :c] = codes, codes
    sw = (rng.random(c) * 0.01 + 0.005).astype(np.float32) if per_channel else np.float32(0.0075)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    sums = t(wt[..., :c].sum((0, 1), dtype=np.int32)) if zx else None                   # without a zero point the layer must not need them
    return rng, x, wt, sw, Int8Tensor(t(x), (2, c, h, w), 1, torch.tensor(SX, device=dev), zx, -128, 127, 0), \
        Int8DepthwiseWeight(t(wt), (c, 1, kh, kw), t(sw), -128, 127, 0, sums)


def run(dev, use_kernels, g, zx=5, per_channel=True, residual=None, relu=False, out_float=True, codes=None, plant=False):
    """One case on ``dev`` against the oracle, on bits: bias and the unsigned output grid always, both outputs unless out_float=False."""
    c, (stride, pad, dil) = g[0], g[5:]
    rng, x, wt, sw, X, W = operands(dev, g, zx, per_channel, codes)
    _, v0, _ = D.layer(x, wt, c, zx, np.float32(SX) * np.broadcast_to(sw, c), stride, pad, dil)
    bias = rng.standard_normal(c).astype(np.float32)
    res = (rng.standard_normal(v0.shape) * 40).astype(np.float32) if residual else None
    if plant:
        W.values[..., 3] = 0; wt[..., 3] = 0; W.sums[3] = 0                                # channel 3: I == 0, so v = (+0 + -0.0) + -0.0
        bias[1], bias[3], res[0, 0, 0, 2], res[..., 3] = np.nan, -0.0, np.nan, -0.0
    tr = torch.from_numpy(res).to(dev).permute(0, 3, 1, 2) if residual else None
    if residual == 'contiguous': tr = tr.contiguous()
    out = config(0.25, 131, 0, 255)
    got = int8_depthwise_conv2d_packed(X, W, torch.from_numpy(bias).to(dev), stride, pad, dil, tr, relu, out, out_float, use_kernels=use_kernels)
    _, v, q = D.layer(x, wt, c, zx, np.float32(SX) * np.broadcast_to(sw, c), stride, pad, dil, bias, res, relu, stored(out))
    y, p = got if out_float else (None, got)
    if y is not None: assert list(y.shape) == [2, c, *v.shape[1:3]] and np.array_equal(bits(y.permute(0, 2, 3, 1)), v.view(np.int32))
    assert np.array_equal(p.values.cpu().numpy(), q) and (p.shape, p.axis, p.zero_point) == ((2, c, *v.shape[1:3]), 1, stored(out)[1])
    if plant: assert np.isnan(v[..., 1]).all() and (q[..., 1] == -128).all() and (v[..., 3].view(np.int32) == 0).all()


@pytest.mark.parametrize('g,kw', [(g, {}) for g in D.GEOMETRIES] + [(C40, kw) for kw in VARIANTS] + [EXTREME], ids=str)
def test_torch_arm_is_the_oracle(g, kw):
    run('cpu', False, g, **kw)


def test_torch_arm_has_the_bits_of_the_dense_layer_on_the_block_diagonal_weight():
    c, _, _, kh, kw, stride, pad, dil = C40
    rng, x, wt, sw, X, W = operands('cpu', C40, 5)
    dense = np.zeros((c, kh, kw, wt.shape[-1]), np.int8)
    dense[np.arange(c), :, :, np.arange(c)] = wt[..., :c].transpose(2, 0, 1)
    B = Int8Tensor(torch.from_numpy(dense), (c, c, kh, kw), 1, W.scale, 0, -128, 127, 0, W.sums)
    bias, out = torch.from_numpy(rng.standard_normal(c).astype(np.float32)), config(0.25, 131, 0, 255)
    (y, p), (yd, pd) = (f(X, w, bias, stride, pad, dil, None, True, out, True, use_kernels=False) for f, w in ((int8_depthwise_conv2d_packed, W), (int8_conv2d_packed, B)))
    assert np.array_equal(bits(y), bits(yd)) and torch.equal(p.values, pd.values)


def test_weight_layout_refusals_and_the_two_launch_form():
    gen = torch.Generator().manual_seed(5)
    x, w = torch.randn(1, 4, 5, 5, generator=gen), torch.randn(4, 1, 3, 3, generator=gen)
    xc, wc = config(0.03, 3), config(w.abs().amax((1, 2, 3)) / 127, torch.zeros(4), -127, 127, channel_axis=0)
    W, T = int8_depthwise_weight(w, wc, use_kernels=False), int8_quantize(w, wc, 1, weight=True, use_kernels=False)
    assert W.values.shape == (3, 3, 32) and torch.equal(W.values[..., :4].permute(2, 0, 1), T.values[..., 0]) and not W.values[..., 4:].any()
    assert torch.equal(W.sums, T.sums) and W.shape == (4, 1, 3, 3) and torch.equal(W.dequantize(), T.dequantize())
    y = int8_conv2d(x, W, xc, padding=1, groups=4, use_kernels=False)
    assert torch.equal(y, int8_depthwise_conv2d(x, W, xc, padding=1, use_kernels=False))
    X = int8_quantize(x, xc, 1, use_kernels=False)
    assert torch.allclose(y, torch.nn.functional.conv2d(X.dequantize(), W.dequantize(), None, 1, 1, groups=4), rtol=1e-5, atol=1e-5)
    for call, msg in ((lambda: int8_depthwise_weight(torch.randn(4, 2, 3, 3), wc, use_kernels=False), r'expected a \[C, 1, kh, kw\] weight'),
                      (lambda: int8_conv2d(x, W, xc, groups=2, use_kernels=False), 'needs groups == 4, got 2'),
                      (lambda: int8_conv2d(x, T, xc, groups=4, use_kernels=False), 'groups must be 1, got 4'),
                      (lambda: int8_depthwise_conv2d(torch.randn(1, 5, 5, 5), W, xc, use_kernels=False), 'channel mismatch: x has 5 channels, w 4'),
                      (lambda: int8_depthwise_conv2d(x, W, xc, padding=40, dilation=40, use_kernels=False), 'stages 248960 bytes of LDS')):
        with pytest.raises(RuntimeError, match=msg): call()
    with pytest.raises(TypeError, match='expected an Int8DepthwiseWeight'): int8_depthwise_conv2d_packed(X, T)


def test_c_entry_point_checks_arguments_without_a_device():
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    buf = np.zeros(16384 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    # x [1, 4, 4, 64] at p, w [3, 3, 64] at p + 1024, sums, mul and bias from p + 4096, residual at p + 5120, y at p + 6144, q (4 x 64 B) at p + 7168
    def call(a=p, sums=p + 4096, zx=3, mul=p + 4352, res=p + 5120, c=p + 6144, q=p + 7168, grid=(1.0, 0, -128, 127, 0, 0), n=1, ch=40, dil=1, pad=0):
        return _lib.lib.ppqhip_int8_dwconv2d(a, p + 1024, sums, zx, mul, p + 4608, res, 1, c, q, *grid, n, ch, 4, 4, 3, 3, 1, 1, pad, pad, dil, dil, None), _lib.last_error()

    what = 'int8_dwconv2d'
    assert call(c=0, q=0) == (-1, f'{what}: no output: y and q are both null')
    assert call(zx=128) == (-1, f'{what}: zx 128 is not an int8 zero point')
    assert call(grid=(1.0, 0, -129, 127, 0, 0))[0] == -1 and call(grid=(1.0, 0, 5, 4, 0, 0))[0] == -1 and call(grid=(1.0, 0, 0, 127, 0, 128))[0] == -1
    assert call(grid=(1.0, 0, -128, 127, 5, 0)) == (-1, f'{what}: rounding policy 5 has no tensor form (ppq_tensor_round)')
    assert call(n=-1) == (-1, f'{what}: negative size') and call(dil=2) == (-1, f'{what}: the kernel window does not fit the padded input: no output')
    assert call(a=0) == (-1, f'{what}: null pointer') == call(mul=0)
    assert call(sums=0) == (-1, f'{what}: sums is required with a zero point other than 0') and call(sums=0, zx=0, n=0)[0] == 0
    assert call(a=p + 8) == (-1, f'{what}: operands, y and q must be 16-byte aligned') == call(c=p + 6144 + 4) == call(q=p + 7168 + 8)
    for out in ({'c': p + 5120}, {'q': p + 4352}, {'q': p + 16}): assert call(**out) == (-1, f'{what}: an output overlaps an input')
    assert call(q=p + 6144) == (-1, f'{what}: two outputs overlap in memory')
    assert call(n=0)[0] == 0 and call(ch=0)[0] == 0                                      # nothing to launch
    st, msg = call(dil=40, pad=40)
    assert st == -2 and msg.startswith(f'{what}: a 3 x 3 window at stride (1, 1) and dilation (40, 40) stages 248960 bytes of LDS')
