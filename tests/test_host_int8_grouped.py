"""The grouped linear INT8 layer without a GPU (ppq_amd/int8.py): the packing against its statement on the dense
block-diagonal weight, the torch arm against the NumPy oracle (tests/int8_grouped_reference.py) bit for bit, the refusals and the C
entry point's argument checks."""
import numpy as np
import pytest
import torch

import int8_grouped_reference as G
import int8_reference as R
from ppq_amd import (Int8GroupedWeight, Int8Tensor, _lib, int4_pack, int8_conv2d, int8_grouped_conv2d, int8_grouped_conv2d_packed, int8_grouped_weight,
                     int8_quantize)
from test_host_int8 import SX, bits, config, stored
from test_host_int8_depthwise import VARIANTS

GEOMETRIES = [g for g, _ in G.GEOMETRIES]
STRADDLE = GEOMETRIES[2]
# the largest |I| of the list: 32 * 9 products of (-128) * (-128 - 127) in the second geometry
EXTREME = (GEOMETRIES[1], dict(zx=127, codes=-128))


def operands(dev, g, zx, per_channel=True, codes=None, use_kernels=False):
    """Raw codes of geometry g, x [N, H, W, Cp] and w [O, kh, kw, C_g], with their Int8Tensor and -- packed by int8_grouped_weight from
    the codes as float32 under scale 1 -- Int8GroupedWeight on dev: x with zero point zx and scale SX, w with the scales sw."""
    groups, cg, og, n, h, w, kh, kw = g[:8]
    c, o = groups * cg, groups * og
    rng = np.random.default_rng(c + 100 * o)
    x, wt = R.operands(rng, n * h * w, c, zx).reshape(n, h, w, -1), R.operands(rng, o * kh * kw, cg).reshape(o, kh, kw, -1)[..., :cg]
    if codes is not None: x[..., :c], wt[:] = codes, codes
    sw = (rng.random(o) * 0.01 + 0.005).astype(np.float32) if per_channel else np.float32(0.0075)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    W = int8_grouped_weight(t(wt.transpose(0, 3, 1, 2).astype(np.float32)), config(1.0, 0.0), groups, use_kernels=use_kernels)
    W.scale = t(sw)
    if not zx: W.sums = None                                                             # without a zero point the layer must not need them
    return rng, x, wt, sw, Int8Tensor(t(x), (n, c, h, w), 1, torch.tensor(SX, device=dev), zx, -128, 127, 0), W


def run(dev, use_kernels, g, zx=5, per_channel=True, residual=None, relu=False, out_float=True, codes=None, plant=False):
    """One case on ``dev`` against the oracle, on bits: bias and the unsigned output grid always, both outputs unless out_float=False."""
    groups, o, (stride, pad, dil) = g[0], g[0] * g[2], g[8:]
    rng, x, wt, sw, X, W = operands(dev, g, zx, per_channel, codes, use_kernels)
    mul = np.float32(SX) * np.broadcast_to(sw, o)
    _, v0, _ = G.layer(x, wt, groups, zx, mul, stride, pad, dil)
    bias = rng.standard_normal(o).astype(np.float32)
    res = (rng.standard_normal(v0.shape) * 40).astype(np.float32) if residual else None
    if plant:
        W.values[3] = 0; wt[3] = 0; W.sums[3] = 0                                          # output 3: I == 0, so v = (+0 + -0.0) + -0.0
        bias[1], bias[3], res[0, 0, 0, 2], res[..., 3] = np.nan, -0.0, np.nan, -0.0
    tr = torch.from_numpy(res).to(dev).permute(0, 3, 1, 2) if residual else None
    if residual == 'contiguous': tr = tr.contiguous()
    out = config(0.25, 131, 0, 255)
    got = int8_grouped_conv2d_packed(X, W, torch.from_numpy(bias).to(dev), stride, pad, dil, tr, relu, out, out_float, use_kernels=use_kernels)
    _, v, q = G.layer(x, wt, groups, zx, mul, stride, pad, dil, bias, res, relu, stored(out))
    y, p = got if out_float else (None, got)
    if y is not None: assert list(y.shape) == [len(x), o, *v.shape[1:3]] and np.array_equal(bits(y.permute(0, 2, 3, 1)), v.view(np.int32))
    assert np.array_equal(p.values.cpu().numpy(), q) and (p.shape, p.axis, p.zero_point) == ((len(x), o, *v.shape[1:3]), 1, stored(out)[1])
    if plant: assert np.isnan(v[..., 1]).all() and (q[..., 1] == -128).all() and (v[..., 3].view(np.int32) == 0).all()


CASES = [(g, {}) for g in GEOMETRIES] + [(STRADDLE, kw) for kw in VARIANTS] + [EXTREME]


@pytest.mark.parametrize('g,expect', G.GEOMETRIES, ids=str)
def test_packing_is_the_block_diagonal_weight_cut_into_slices(g, expect):
    groups, cg = g[:2]
    _, _, wt, _, _, W = operands('cpu', g, 5)
    dense = G.block_diagonal(wt, groups)
    cb0, nbs = expect
    assert (W.cb0.tolist(), W.nbs, W.groups, W.shape) == (cb0, nbs, groups, (len(wt), cg, *wt.shape[1:3])) and W.cb0.dtype == torch.int32
    padded = np.concatenate([dense, np.zeros(dense.shape[:3] + (32 * nbs,), np.int8)], -1)          # blocks at or past Cp / 32: code 0
    want = np.stack([padded[row, :, :, 32 * cb0[row // 32]: 32 * (cb0[row // 32] + nbs)] for row in range(len(wt))])
    assert np.array_equal(W.values.numpy(), want) and np.array_equal(W.sums.numpy(), wt.reshape(len(wt), -1).sum(1, dtype=np.int32))
    W.scale = torch.tensor(0.5)
    assert np.array_equal(W.dequantize().numpy(), wt.transpose(0, 3, 1, 2).astype(np.float32) * np.float32(0.5))


@pytest.mark.parametrize('g,kw', CASES, ids=str)
def test_torch_arm_is_the_oracle(g, kw):
    run('cpu', False, g, **kw)


def test_refusals_and_the_two_launch_form():
    gen = torch.Generator().manual_seed(5)
    x, w = torch.randn(1, 8, 5, 5, generator=gen), torch.randn(6, 4, 3, 3, generator=gen)
    xc, wc = config(0.03, 3), config(w.abs().amax((1, 2, 3)) / 127, torch.zeros(6), -127, 127, channel_axis=0)
    W, T = int8_grouped_weight(w, wc, 2, use_kernels=False), int8_quantize(w, wc, 1, weight=True, use_kernels=False)
    assert torch.equal(W.dequantize(), T.dequantize()) and torch.equal(W.sums, T.sums)
    y = int8_conv2d(x, W, xc, padding=1, groups=2, use_kernels=False)
    assert torch.equal(y, int8_grouped_conv2d(x, W, xc, padding=1, use_kernels=False))
    X = int8_quantize(x, xc, 1, use_kernels=False)
    assert torch.allclose(y, torch.nn.functional.conv2d(X.dequantize(), W.dequantize(), None, 1, 1, groups=2), rtol=1e-5, atol=1e-5)
    W4 = int4_pack(int8_quantize(w, config(0.2, 0, -8, 7), 1, weight=True, use_kernels=False))
    dw = int8_grouped_weight(torch.randn(8, 1, 3, 3, generator=gen), config(0.01, 0), 8, use_kernels=False)          # plain depthwise: accepted
    assert int8_conv2d(x, dw, xc, groups=8, use_kernels=False).shape == (1, 8, 3, 3)
    for call, msg in ((lambda: int8_grouped_weight(w, wc, 4, use_kernels=False), '4 groups do not divide the 6 output channels'),
                      (lambda: int8_conv2d(x, W, xc, groups=1, use_kernels=False), 'a grouped weight of 2 groups needs groups == 2, got 1'),
                      (lambda: int8_conv2d(x, T, xc, groups=2, use_kernels=False), 'groups must be 1, got 2'),
                      (lambda: int8_conv2d(x, W4, xc, groups=2, use_kernels=False), 'groups must be 1, got 2'),
                      (lambda: int8_grouped_conv2d(torch.randn(1, 6, 5, 5), W, xc, use_kernels=False), 'channel mismatch: x has 6 channels, w 4 for each of 2 groups'),
                      (lambda: int8_grouped_conv2d_packed(X, Int8GroupedWeight(torch.zeros(6, 3, 3, 65536 // 9 // 32 * 32 + 32, dtype=torch.int8), (6, 4, 3, 3), 2, 228,
                                                                               W.cb0, W.scale, -127, 127, 0, W.sums), use_kernels=False),
                       'a padded reduction length of 65664: 65536 and more could overflow int32')):
        with pytest.raises(RuntimeError, match=msg): call()
    with pytest.raises(TypeError, match='expected an Int8GroupedWeight'): int8_grouped_conv2d_packed(X, T)
    for call in (lambda: int8_grouped_conv2d_packed(X, W4), lambda: int8_grouped_weight(W4, wc, 2)):
        with pytest.raises(TypeError, match='INT4 grouped weights are not supported'): call()


def test_c_entry_point_checks_arguments_without_a_device():
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    buf = np.zeros(16384 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    # x [1, 4, 4, 64] at p, w [40, 3, 3, 32] from p + 1024 ... : every refusal below comes before a pointer is followed
    def call(a=p, zx=3, mul=p + 4352, q=p + 7168, n=1, ch=40, o=40, dil=1, groups=2, nbs=1, cb0=p + 4096):
        return _lib.lib.ppqhip_int8_gconv2d(a, p + 1024, p + 4096, zx, mul, p + 4608, None, 1, None, q, 1.0, 0, -128, 127, 0, 0, n, ch, 4, 4, o, 3, 3, 1, 1, 0, 0,
                                            dil, dil, groups, nbs, cb0, None), _lib.last_error()

    what = 'int8_gconv2d'
    assert call(q=0) == (-1, f'{what}: no output: y and q are both null') and call(zx=128) == (-1, f'{what}: zx 128 is not an int8 zero point')
    assert call(n=-1) == (-1, f'{what}: negative size') == call(groups=-1) == call(nbs=-1)
    assert call(dil=2) == (-1, f'{what}: the kernel window does not fit the padded input: no output')
    assert call(groups=0) == (-1, f'{what}: groups must be at least 1, got 0') and call(nbs=0) == (-1, f'{what}: nbs must be at least 1, got 0')
    assert call(groups=3) == (-1, f'{what}: c = 40 and o = 40 must both be multiples of groups = 3')
    assert call(ch=42, groups=3) == (-1, f'{what}: c = 42 and o = 40 must both be multiples of groups = 3')
    assert call(cb0=0) == (-1, f'{what}: null pointer') == call(a=0) == call(mul=0)
    assert call(nbs=228) == (-1, f'{what}: a padded reduction length of 65664: 65536 and more could overflow int32')
    assert call(a=p + 8) == (-1, f'{what}: operands, y and q must be 16-byte aligned') and call(q=p + 16) == (-1, f'{what}: an output overlaps an input')
    assert call(n=0)[0] == 0 and call(o=0)[0] == 0                                       # nothing to launch
