"""The linear INT8 layers without a GPU (ppq_amd/int8.py): the torch arm against the NumPy oracle
(tests/int8_reference.py) bit for bit, every refusal, the C entry points' argument checks, the accuracy statement."""
import numpy as np
import pytest
import torch

import int8_reference as R
from ppq_amd import (Int8Tensor, LinearQuantizationConfig, RoundingPolicy, _lib, int8_conv2d, int8_conv2d_packed, int8_dequantize, int8_linear,
                     int8_matmul, int8_quantize)

bits = lambda t: t.contiguous().cpu().numpy().view(np.int32)
SX = 0.02


def config(scale, offset, qmin=-128, qmax=127, rounding=0, channel_axis=None):
    c = LinearQuantizationConfig(symmetrical=False, channel_axis=channel_axis, quant_min=qmin, quant_max=qmax, rounding=RoundingPolicy(rounding))
    c.scale, c.offset = torch.as_tensor(scale, dtype=torch.float32), torch.as_tensor(offset, dtype=torch.float32)
    return c


def stored(cfg):
    """out_q of the oracle for a per-tensor config: (sy, zy, qmin, qmax, rounding, q_nan) in the stored domain."""
    r = 128 if cfg.quant_max > 127 else 0
    return float(cfg.scale), int(cfg.offset) - r, cfg.quant_min - r, cfg.quant_max - r, cfg.rounding.value, -r


def pair(dev, a, b, shape_a, shape_b, zx, sw):
    """Int8Tensors of raw codes: an activation with zero point zx and scale SX, a weight with the scales sw and its sums."""
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    sums = b.reshape(len(b), -1).sum(1, dtype=np.int32)
    return (Int8Tensor(t(a), shape_a, len(shape_a) - 1 if len(shape_a) == 2 else 1, torch.tensor(SX, device=dev), zx, -128, 127, 0),
            Int8Tensor(t(b), shape_b, 1, t(sw), 0, -128, 127, 0, t(sums)))


def run_gemm(dev, use_kernels, m, n, k, zx=-7, bias=True, residual=False, relu=False, out=None, out_float=None):
    """One case of the GEMM on ``dev`` against the oracle, on bits; returns what int8_matmul returned."""
    rng = np.random.default_rng(1000 * m + k)
    a, b, sw = R.operands(rng, m, k, zx), R.operands(rng, n, k), (rng.random(n) * 0.01 + 0.005).astype(np.float32)
    tb = rng.standard_normal(n).astype(np.float32) if bias else None
    tr = (rng.standard_normal((m, n)) * 40).astype(np.float32) if residual else None
    A, B = pair(dev, a, b, (m, k), (n, k), zx, sw)
    if zx == 0: B.sums = None                                                            # int8_matmul must not need them
    dv = lambda v: torch.from_numpy(v).to(dev) if v is not None else None
    got = int8_matmul(A, B, dv(tb), dv(tr), relu, out, out_float, use_kernels=use_kernels)
    _, v, q = R.layer(a, b, zx, np.float32(SX) * sw, tb, tr, relu, stored(out) if out is not None else None)
    y, p = (got, None) if out is None else (got if out_float else (None, got))
    if y is not None: assert np.array_equal(bits(y), v.view(np.int32))
    if p is not None: assert np.array_equal(p.values.cpu().numpy(), q) and (p.shape, p.axis, p.zero_point) == ((m, n), 1, stored(out)[1])
    return got


def run_conv(dev, use_kernels, g, zx=5, tail=False):
    """One geometry on ``dev`` against the oracle: both outputs, bias; ``tail``: residual and ReLU too."""
    c, h, w, kh, kw, stride, pad, dil, o = g
    rng = np.random.default_rng(c + 10 * o)
    x = R.operands(rng, 2 * h * w, c, zx).reshape(2, h, w, -1)
    wt = R.operands(rng, o * kh * kw, c).reshape(o, kh, kw, -1)
    sw, bias = (rng.random(o) * 0.01 + 0.005).astype(np.float32), rng.standard_normal(o).astype(np.float32)
    a, (oh, ow) = R.gather(x, kh, kw, stride, pad, dil, zx)
    res = (rng.standard_normal((2, o, oh, ow)) * 40).astype(np.float32) if tail else None
    out = config(0.25, 131, 0, 255)
    X, W = pair(dev, x, wt, (2, c, h, w), (o, c, kh, kw), zx, sw)
    if zx == 0: W.sums = None
    y, p = int8_conv2d_packed(X, W, torch.from_numpy(bias).to(dev), stride, pad, dil, torch.from_numpy(res).to(dev) if tail else None, tail, out, True,
                              use_kernels=use_kernels)
    _, v, q = R.layer(a, wt.reshape(o, -1), zx, np.float32(SX) * sw, bias, res.transpose(0, 2, 3, 1).reshape(-1, o) if tail else None, tail, stored(out))
    assert list(y.shape) == [2, o, oh, ow] and np.array_equal(bits(y.permute(0, 2, 3, 1)), v.view(np.int32).reshape(2, oh, ow, o))
    assert np.array_equal(p.values.cpu().numpy().reshape(len(q), -1), q) and (p.shape, p.axis) == ((2, o, oh, ow), 1)


def accuracy_statement(dev, use_kernels):
    """int8_conv2d on quantised random data against the float64 convolution of the DEQUANTISED operands E (E0 without the bias); they
    are dequantised in float64, (code - zero point) * scale exactly: int8_dequantize's own float32 rounding is no part of the layer.
    The contract rounds at most four times: mul = sx * sw, t = float32(I), v = t * mul -- each relative 2^-24 on a value of
    magnitude |E0| -- and v + bias, 2^-24 on |E|.  So |y - E| <= 2^-24 (3 |E0| + |E|), times (1 + 2^-20) for the second-order terms."""
    gen = torch.Generator().manual_seed(11)
    x, w, bias = torch.randn(2, 40, 9, 7, generator=gen), torch.randn(70, 40, 3, 3, generator=gen) * 0.1, torch.randn(70, generator=gen)
    xc, wc = config(4 / 127, 9, 0, 255), config(w.abs().amax((1, 2, 3)) / 127, torch.zeros(70), -127, 127, channel_axis=0)
    x, w, bias = x.to(dev), w.to(dev), bias.to(dev)
    W = int8_quantize(w, wc, 1, weight=True, use_kernels=use_kernels)
    y = int8_conv2d(x, W, xc, bias, 2, 1, use_kernels=use_kernels)
    X = int8_quantize(x, xc, 1, use_kernels=use_kernels)
    exact = lambda t: (t.values[..., :40].permute(0, 3, 1, 2).double().cpu() - t.zero_point) * t.scale.double().cpu().reshape(-1, 1, 1, 1)
    assert torch.equal(exact(X).float(), int8_dequantize(X).cpu()) and torch.equal(exact(W).float(), int8_dequantize(W).cpu())
    e0 = torch.nn.functional.conv2d(exact(X), exact(W), None, 2, 1)
    e = e0 + bias.double().cpu()[None, :, None, None]
    err, bound = (y.double().cpu() - e).abs(), 2.0 ** -24 * (3 * e0.abs() + e.abs()) * (1 + 2.0 ** -20)
    print(f'accuracy: max error {err.max():.3e}, max error / bound {(err / bound).max():.3f}')
    assert bool((err <= bound).all())


MN = [(1, 1), (15, 17), (17, 63), (63, 65), (65, 130)]


@pytest.mark.parametrize('k', [1, 33, 300])
def test_torch_arm_gemm_is_the_oracle(k):
    for m, n in MN: run_gemm('cpu', False, m, n, k)
    out = config(0.25, -3, -128, 127, 4)
    run_gemm('cpu', False, 17, 63, k, residual=True, relu=True, out=out, out_float=True)
    run_gemm('cpu', False, 17, 63, k, zx=0, bias=False, out=config(0.25, 131, 0, 255), out_float=False)


@pytest.mark.parametrize('g', R.GEOMETRIES, ids=str)
def test_torch_arm_conv_is_the_oracle(g):
    run_conv('cpu', False, g, tail=g[0] == 32)
    if g[0] == 40: run_conv('cpu', False, g, zx=0)


def test_quantize_dequantize_and_the_two_launch_forms():
    gen = torch.Generator().manual_seed(3)
    x, w = torch.randn(5, 3, 40, generator=gen), torch.randn(37, 40, generator=gen)
    xc, wc = config(0.03, 120, 0, 255, 1), config(0.02, 0)
    X, W = int8_quantize(x, xc, use_kernels=False), int8_quantize(w, wc, 1, weight=True, use_kernels=False)
    want = torch.clamp(torch.floor(x / 0.03 + 0.5) + 120, 0, 255)
    assert X.values.shape == (5, 3, 64) and X.zero_point == -8 and torch.equal(X.values[..., :40].float() + 128, want) and (X.values[..., 40:] == -8).all()
    assert torch.equal(int8_dequantize(X), (want - 120) * torch.tensor(0.03)) and torch.equal(W.sums, W.values.sum(1, dtype=torch.int32))
    y = int8_linear(x, W, xc, use_kernels=False)
    assert y.shape == (5, 3, 37) and torch.equal(y, int8_matmul(X, W, use_kernels=False))
    assert torch.allclose(y, int8_dequantize(X) @ int8_dequantize(W).t(), rtol=1e-5, atol=1e-5)


def test_refusals():
    x, w = torch.randn(4, 40), torch.randn(8, 40)
    q = lambda t, c, **kw: int8_quantize(t, c, use_kernels=False, **kw)
    X, W = q(x, config(0.03, 3)), q(w, config(0.02, 0), weight=True)
    for cfg, kw, msg in ((config(0.1, 0, -129, 127), {}, 'fits neither -128 .. 127 nor 0 .. 255'), (config(0.1, 0, 0, 256), {}, 'fits neither'),
                         (config(0.1, 0.5), {}, 'the offset is not an integer'), (config(0.1, 1), {'weight': True}, 'a weight must be symmetric'),
                         (config(0.1, 0, 0, 255), {'weight': True}, 'a weight must be symmetric'), (config(0.1, 200), {}, 'lies outside the range'),
                         (config(torch.ones(4), torch.zeros(4), channel_axis=0), {}, 'an activation must be quantised per tensor'),
                         (config(torch.ones(40), torch.zeros(40), channel_axis=1), {'weight': True}, 'per tensor or along axis 0')):
        with pytest.raises(RuntimeError, match=msg): q(x, cfg, **kw)
    with pytest.raises(RuntimeError, match='expected a float32 tensor'): q(x.double(), config(0.1, 0))
    big = Int8Tensor(torch.zeros(1, 65536, dtype=torch.int8), (1, 65536), 1, torch.tensor(1.), 0, -128, 127, 0, torch.zeros(1, dtype=torch.int32))
    for call, msg in ((lambda: int8_matmul(X, X), 'w is not a weight'), (lambda: int8_matmul(X, q(torch.randn(8, 33), config(0.02, 0), weight=True)), 'K mismatch'),
                      (lambda: int8_matmul(Int8Tensor(big.values, big.shape, 1, big.scale, 0, -128, 127, 0), big), '65536 and more could overflow int32'),
                      (lambda: int8_matmul(X, W, bias=torch.zeros(8).double()), 'bias must be a float32 tensor'),
                      (lambda: int8_matmul(X, W, residual=torch.zeros(8, 4)), r'residual of shape \[8, 4\], expected \[4, 8\]'),
                      (lambda: int8_matmul(X, W, out_float=False), 'no output'), (lambda: int8_matmul(X, W, out_config=config(0.1, 0, -200, 0)), 'out_config: the range'),
                      (lambda: int8_conv2d(torch.randn(1, 4, 5, 5), W, config(0.1, 0), groups=2), 'groups must be 1'),
                      (lambda: int8_conv2d(torch.randn(4, 5, 5), W, config(0.1, 0)), 'x must be 4-d'),
                      (lambda: int8_conv2d_packed(X, W), 'operands must be 4-d')):
        with pytest.raises(RuntimeError, match=msg): call()
    with pytest.raises(TypeError, match='expected an Int8Tensor'): int8_matmul(x, W)


def test_c_entry_points_check_arguments_without_a_device():
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    buf = np.zeros(16384 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    # gemm 2 x 40 x 64 / conv x [1, 4, 4, 64], w [2, 3, 3, 64]: operands below p + 4096, sums, mul and bias there, residual at p + 5120, c / y at p + 6144,
    # q (2 x 64 B) at p + 7168
    def gemm(a=p, sums=p + 4096, zx=3, mul=p + 4352, res=p + 5120, c=p + 6144, q=p + 7168, grid=(1.0, 0, -128, 127, 0, 0), m=2, n=40, k=64):
        return _lib.lib.ppqhip_int8_gemm(a, p + 1024, sums, zx, mul, p + 4608, res, 1, c, q, *grid, m, n, k, None), _lib.last_error()

    def conv(a=p, sums=p + 4096, zx=3, mul=p + 4352, res=p + 5120, c=p + 6144, q=p + 7168, grid=(1.0, 0, -128, 127, 0, 0), m=1, n=2, k=64):
        return _lib.lib.ppqhip_int8_conv2d(a, p + 1024, sums, zx, mul, p + 4608, res, 1, c, q, *grid, m, k, 4, 4, n, 3, 3, 1, 1, 0, 0, 1, 1, None), _lib.last_error()

    for call, what, y in ((gemm, 'int8_gemm', 'c'), (conv, 'int8_conv2d', 'y')):
        assert call(c=0, q=0) == (-1, f'{what}: no output: {y} and q are both null')
        assert call(zx=128) == (-1, f'{what}: zx 128 is not an int8 zero point')
        assert call(grid=(1.0, 0, -129, 127, 0, 0))[0] == -1 and call(grid=(1.0, 0, 5, 4, 0, 0))[0] == -1 and call(grid=(1.0, 0, 0, 127, 0, 128))[0] == -1
        assert call(grid=(1.0, 0, -128, 127, 5, 0)) == (-1, f'{what}: rounding policy 5 has no tensor form (ppq_tensor_round)')
        assert call(m=-1) == (-1, f'{what}: negative size')
        assert call(a=0) == (-1, f'{what}: null pointer') == call(mul=0)
        assert call(sums=0) == (-1, f'{what}: sums is required with a zero point other than 0') and call(sums=0, zx=0, m=0)[0] == 0
        assert call(a=p + 8) == (-1, f'{what}: operands, {y} and q must be 16-byte aligned') == call(c=p + 6144 + 4) == call(q=p + 7168 + 8)
        for out in ({'c': p + 5120}, {'q': p + 4352}, {'q': p + 16}): assert call(**out) == (-1, f'{what}: an output overlaps an input')
        assert call(q=p + 6144) == (-1, f'{what}: two outputs overlap in memory')
        assert call(m=0)[0] == 0 and call(n=0)[0] == 0                                   # nothing to launch
    assert gemm(k=65505)[1].startswith('int8_gemm: a padded reduction length of 65536') and conv(k=7296)[1].startswith('int8_conv2d: a padded reduction length of 65664')


def test_accuracy_statement():
    accuracy_statement('cpu', False)
