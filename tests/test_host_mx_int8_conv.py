"""The MXINT8 convolution without a GPU: the ``use_kernels=False`` arm of ``mx_int8_conv2d_packed`` /
``mx_int8_conv2d`` against the oracle (tests/mx_int8_conv_reference.py) bit for bit, the argument checks, the host-side refusals of
the C entry point, and ``deploy_graph_mx`` of an MXINT8 x MXINT8 graph on the torch arms."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mx_conv_reference as C
import mx_int8_conv_reference as I
import mx_int8_gemm_reference as G
from ppq_amd import (MXTensor, _lib, deploy_graph_mx, harness, mx_fake_quant, mx_int8_conv2d, mx_int8_conv2d_packed, mx_quantize,
                     quantize_graph_mx)

STEM, NBC5 = C.EDGE_GEOMETRIES[2], C.EDGE_GEOMETRIES[4]          # 7 x 7 stride 2 on C = 3; nbc = 5 under a 1 x 3 kernel


def tensors(x, w, g: C.Geometry, dev='cpu'):
    X = MXTensor('MXINT8', (g.n, g.c, g.h, g.w), 1, torch.from_numpy(x[0]).to(dev), torch.from_numpy(x[1]).to(dev))
    W = MXTensor('MXINT8', (g.o, g.c, g.kh, g.kw), 1, torch.from_numpy(w[0]).to(dev), torch.from_numpy(w[1]).to(dev))
    return X, W


def packed(t: MXTensor):
    return t.elements.cpu().numpy(), t.scales.cpu().numpy()


@pytest.mark.parametrize('g,biased', [(C.FIRST, True), (STEM, False), (NBC5, False)], ids=str)
def test_torch_arm_has_the_oracles_bits(g, biased):
    assert (STEM.kh, STEM.stride, STEM.c, NBC5.nbc) == (7, (2, 2), 3, 5)
    x, w = I.raw_operands(g, range(100, 151))
    bias = np.linspace(-3.0, 5.0, g.o).astype(np.float32) if biased else None
    got = mx_int8_conv2d_packed(*tensors(x, w, g), None if bias is None else torch.from_numpy(bias), g.stride, g.pad, g.dil, use_kernels=False)
    assert got.dtype == torch.float32 and tuple(got.shape) == (g.n, g.o, g.oh, g.ow)
    assert G.same_bits(got.contiguous().numpy(), I.conv(x, w, g, bias)[0])


def test_mx_int8_conv2d_stays_within_the_derived_bound_of_float64():
    g = C.FIRST
    x, w = (torch.from_numpy(t) for t in C.random_inputs(g))
    bias = torch.linspace(-1.0, 1.0, g.o)
    W = mx_quantize(w, 'MXINT8', 1, use_kernels=False)
    X = mx_quantize(x, 'MXINT8', 1, use_kernels=False)
    y = mx_int8_conv2d(x, W, bias, 1, 1, use_kernels=False)
    assert torch.equal(y, mx_int8_conv2d_packed(X, W, bias, (1, 1), (1, 1), (1, 1), use_kernels=False))
    assert torch.equal(y, mx_int8_conv2d(x.contiguous(memory_format=torch.channels_last), W, bias, 1, 1, use_kernels=False))
    want = F.conv2d(X.dequantize(use_kernels=False).double(), W.dequantize(use_kernels=False).double(), bias.double(), 1, 1).numpy()
    _, _, s = I.conv(packed(X), packed(W), g, bias.numpy())
    assert (np.abs(y.double().numpy() - want) <= I.bound(s, g, bias.numpy())).all() and np.abs(want).max() > 1


def test_argument_checks():
    x, w = torch.randn(2, 40, 6, 5), torch.randn(7, 40, 3, 3)
    q = lambda t, f='MXINT8', axis=1: mx_quantize(t, f, axis, use_kernels=False)
    X, W = q(x), q(w)
    kw = dict(use_kernels=False)
    with pytest.raises(RuntimeError, match='x is MXFP8_E4M3, not MXINT8; mx_conv2d convolves the float formats'): mx_int8_conv2d_packed(q(x, 'MXFP8_E4M3'), W, **kw)
    with pytest.raises(RuntimeError, match='w is MXFP4_E2M1, not MXINT8'): mx_int8_conv2d_packed(X, q(w, 'MXFP4_E2M1'), **kw)
    with pytest.raises(RuntimeError, match='x .* packed along axis 3'): mx_int8_conv2d_packed(q(x, axis=3), W, **kw)
    with pytest.raises(RuntimeError, match='w must be 4-d'): mx_int8_conv2d_packed(X, q(w[:, :, :, 0]), **kw)
    with pytest.raises(RuntimeError, match='C mismatch: x has 40 channels, w has 32'): mx_int8_conv2d_packed(X, q(w[:, :32].contiguous()), **kw)
    with pytest.raises(RuntimeError, match='mx_int8_conv2d: groups must be 1'): mx_int8_conv2d(x, W, groups=2, **kw)
    with pytest.raises(RuntimeError, match='mx_int8_conv2d: x must be 4-d'): mx_int8_conv2d(x[0], W, **kw)
    with pytest.raises(RuntimeError, match='mx_int8_conv2d: a 3 x 3 kernel .* does not fit'): mx_int8_conv2d_packed(X, W, dilation=3, **kw)
    with pytest.raises(RuntimeError, match='mx_int8_conv2d: stride must be at least 1'): mx_int8_conv2d_packed(X, W, stride=0, **kw)
    with pytest.raises(RuntimeError, match=r'bias of shape \[6\], expected \[7\]'): mx_int8_conv2d_packed(X, W, torch.zeros(6), **kw)
    with pytest.raises(RuntimeError, match='bias must be a float32 tensor'): mx_int8_conv2d_packed(X, W, torch.zeros(7, dtype=torch.float64), **kw)
    with pytest.raises(TypeError, match='MXTensor'): mx_int8_conv2d_packed(x, W, **kw)
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_int8_conv2d_packed(X, W)          # the kernel arm has no CPU path
    assert mx_int8_conv2d_packed(X, W, **kw).shape == (2, 7, 4, 3)


def test_c_entry_point_checks_arguments_without_a_device():
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    buf = np.zeros(8192 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15                                                     # 16-B aligned, 8192 bytes behind it

    # x [1, 64, 4, 4]: 32 blocks, elements 1024 B at p, scales 32 B at p + 1024; w [2, 64, 3, 3]: 36 blocks, elements 1152 B at p + 2048,
    # scales 36 B at p + 3200; bias 8 B at p + 3264; y [1, 2, 2, 2]: 32 B at p + 4096
    def conv(xe=p, xs=p + 1024, we=p + 2048, ws=p + 3200, bias=p + 3264, y=p + 4096, n=1, c=64, h=4, w=4, o=2, kh=3, kw=3, sh=1, sw=1,
             ph=0, pw=0, dh=1, dw=1):
        return _lib.lib.ppqhip_mx_int8_conv2d(xe, xs, we, ws, bias, y, n, c, h, w, o, kh, kw, sh, sw, ph, pw, dh, dw, None), _lib.last_error()

    for size in ('n', 'c', 'h', 'w', 'o', 'kh', 'kw', 'sh', 'sw', 'ph', 'pw', 'dh', 'dw'):
        assert conv(**{size: -1}) == (-1, 'mx_int8_conv2d: negative size')
        assert conv(**{size: 1 << 31}) == (-1, 'mx_int8_conv2d: a size above 2^31 - 1')
    for size in ('kh', 'kw'): assert conv(**{size: 0}) == (-1, 'mx_int8_conv2d: kernel size must be at least 1')
    for size in ('sh', 'sw'): assert conv(**{size: 0}) == (-1, 'mx_int8_conv2d: stride must be at least 1')
    for size in ('dh', 'dw'): assert conv(**{size: 0}) == (-1, 'mx_int8_conv2d: dilation must be at least 1')
    no_output = 'mx_int8_conv2d: the kernel window does not fit the padded input: no output'
    assert conv(kh=5) == (-1, no_output) and conv(dw=2) == (-1, no_output) and conv(h=2) == (-1, no_output)
    assert conv(n=1 << 20, h=1 << 10, w=1 << 10) == (-1, 'mx_int8_conv2d: a size above 2^31 - 1')
    for ptr in ('xe', 'xs', 'we', 'ws', 'y'): assert conv(**{ptr: 0}) == (-1, 'mx_int8_conv2d: null pointer')
    unaligned = 'mx_int8_conv2d: elements and y must be 16-byte aligned'
    assert conv(xe=p + 8) == (-1, unaligned) and conv(we=p + 2048 + 4) == (-1, unaligned) and conv(y=p + 4096 + 4) == (-1, unaligned)
    for at in (p + 1008, p + 3184, p + 3216, p + 3248): assert conv(y=at) == (-1, 'mx_int8_conv2d: an output overlaps an input')
    assert conv(n=0)[0] == 0 and conv(o=0)[0] == 0 and conv(n=0, xe=0, y=0)[0] == 0      # nothing to launch


# --------------------------------------------------------------------------------------------------------------------- the deployment
def _int8_cnn(use_kernels=False, device='cpu'):
    g = harness.small_cnn_graph(seed=3)                                                  # Conv -> Relu -> Conv -> Add -> Relu -> GAP -> Gemm
    ex = harness.TorchExecutor(g, device)
    return g, ex, quantize_graph_mx(g, ex, 'MXINT8', 'MXINT8', use_kernels=use_kernels)


def test_deploy_graph_mx_runs_an_mxint8_graph_on_the_torch_arms():
    g, ex, d = _int8_cnn()
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2))
    simulated = ex.forward(x)[0]
    dep = deploy_graph_mx(g, ex, d, use_kernels=False)
    assert dep.deployed == ['c1', 'c2', 'fc'] and dep.skipped == {} and dep.groups == {}
    got = ex.forward(x)[0]
    assert torch.allclose(got, simulated, rtol=1e-4, atol=1e-5)
    v = lambda n: g.variables[n].value
    a = F.relu(mx_int8_conv2d(x, dep.weights['c1_w'], v('c1_b'), 1, 1, use_kernels=False))
    s = F.relu(mx_int8_conv2d(a, dep.weights['c2_w'], v('c2_b'), 1, 1, use_kernels=False) + a)
    assert torch.equal(ex.forward(x, [g.operations['add_relu'].outputs[0].name])[0], s)
    dep.remove()
    assert dep.deployed == [] and ex._overrides == {} and torch.equal(ex.forward(x)[0], simulated)
    fused = deploy_graph_mx(g, ex, d, use_kernels=False, fuse=True)                      # no fused epilogue: alone, in no group
    assert fused.deployed == ['c1', 'c2', 'fc'] and fused.groups == {} and torch.equal(ex.forward(x)[0], got)
    fused.remove()


def test_a_deployed_conv_stays_within_the_derived_bound_of_float64():
    geo = C.geometry([2, 40, 7, 5], 9, 3, (2, 1), 1, (1, 2))                             # strides, pads and dilations all pass through
    g = harness.BaseGraph('one_conv')
    x = g.create_variable('input'); g.inputs['input'] = x
    xv, wv = (torch.from_numpy(t) for t in C.random_inputs(geo))
    w = g.create_variable('w', wv, True)
    b = g.create_variable('b', torch.linspace(-1.0, 1.0, geo.o), True)
    y = g.create_operation('Conv', 'conv', [x, w, b], {'strides': geo.stride, 'pads': geo.pad, 'dilations': geo.dil})
    g.outputs[y.name] = y
    ex = harness.TorchExecutor(g, 'cpu')
    d = quantize_graph_mx(g, ex, 'MXINT8', 'MXINT8', use_kernels=False)
    dep = deploy_graph_mx(g, ex, d, use_kernels=False)
    assert dep.deployed == ['conv']
    got = ex.forward(xv)[0]
    assert tuple(got.shape) == (geo.n, geo.o, geo.oh, geo.ow)
    q = lambda t: mx_fake_quant(t, 'MXINT8', 1, use_kernels=False).double()
    want = F.conv2d(q(xv), q(wv), b.value.double(), geo.stride, geo.pad, geo.dil).numpy()
    _, _, s = I.conv(packed(mx_quantize(xv, 'MXINT8', 1, use_kernels=False)), packed(dep.weights['w']), geo, b.value.numpy())
    assert (np.abs(got.double().numpy() - want) <= I.bound(s, geo, b.value.numpy())).all() and np.abs(want).max() > 1
