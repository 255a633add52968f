"""The MXINT8 convolution on the GPU (ppq_amd/csrc/mx_int8_conv.hip): the kernel against the oracle
(tests/mx_int8_conv_reference.py) with == on the float32 bits, NaN-ness only where the oracle is NaN."""
import numpy as np
import pytest
import torch

import mx_conv_reference as C
import mx_int8_conv_reference as I
import mx_int8_gemm_reference as G
from ppq_amd import CUDA, MXTensor, deploy_graph_mx, harness, mx_int8_conv2d, mx_int8_conv2d_packed, mx_quantize, quantize_graph_mx

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# nbc = 2, 1, 4, 5; chunks that straddle taps and (nbc = 4) chunks of one tap; tails of 2 (nb' = 18 and 2), 1 (49) and 3 (15) blocks, and none (16);
# M = O = 70 (2 x 2 workgroups); stride 2, dilation 2, a 1 x 3 kernel padded along one axis only
GEOMETRIES = [C.FIRST] + C.EDGE_GEOMETRIES


def hip(x, w, g: C.Geometry, bias=None) -> np.ndarray:
    X = MXTensor('MXINT8', (g.n, g.c, g.h, g.w), 1, torch.from_numpy(x[0]).to(DEV), torch.from_numpy(x[1]).to(DEV))
    W = MXTensor('MXINT8', (g.o, g.c, g.kh, g.kw), 1, torch.from_numpy(w[0]).to(DEV), torch.from_numpy(w[1]).to(DEV))
    y = mx_int8_conv2d_packed(X, W, None if bias is None else torch.from_numpy(bias).to(DEV), g.stride, g.pad, g.dil)
    assert y.dtype == torch.float32 and tuple(y.shape) == (g.n, g.o, g.oh, g.ow) and y.permute(0, 2, 3, 1).is_contiguous()
    return y.contiguous().cpu().numpy()


@pytest.mark.parametrize('k', range(len(GEOMETRIES)), ids=lambda k: str(GEOMETRIES[k]))
def test_raw_codes_on_every_geometry(k):
    """Every block lies under its own random scale: a wrong tap, pixel, batch boundary or padding test changes the bits."""
    g = GEOMETRIES[k]
    x, w = I.raw_operands(g, range(100, 151), seed=k)
    bias = np.random.default_rng(k).standard_normal(g.o).astype(np.float32) if k % 2 == 0 else None
    want = I.conv(x, w, g, bias)[0]
    got = hip(x, w, g, bias)
    assert not np.isnan(want).any() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(hip(x, w, g, bias).view(np.uint32), got.view(np.uint32))       # two launches, identical bits


def test_extreme_scales_with_padding_inside_the_chains():
    g = C.FIRST
    x, w = I.raw_operands(g, [0, 1, 126, 127, 253, 254])
    want = I.conv(x, w, g)[0]
    assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any() and (C.tap_pixels(g) < 0).any()
    assert G.same_bits(hip(x, w, g), want)


@pytest.mark.parametrize('side', ['x', 'w'])
def test_nan_scale(side):
    g = C.NAN_GEOMETRY
    x, w = I.raw_operands(g, range(100, 151))
    clean = I.conv(x, w, g)[0]
    want_nan = np.zeros(clean.shape, bool)
    if side == 'x':
        x[1][g.n - 1, 1, g.w - 1, g.nbc - 1] = 0xff
        want_nan[:] = (C.tap_pixels(g) == ((g.n - 1) * g.h + 1) * g.w + g.w - 1).any(axis=1).reshape(g.n, 1, g.oh, g.ow)
    else:
        w[1][g.o - 2, g.kh - 1, g.kw - 1, 0] = 0xff
        want_nan[:, g.o - 2] = True
    got = hip(x, w, g)
    assert want_nan.any() and not want_nan.all() and np.array_equal(np.isnan(I.conv(x, w, g)[0]), want_nan)
    assert (got.view(np.uint32)[want_nan] == 0x7fc00000).all() and np.array_equal(got.view(np.uint32)[~want_nan], clean.view(np.uint32)[~want_nan])


@pytest.mark.parametrize('channels_last', [False, True])
def test_mx_int8_conv2d_on_float_input(channels_last):
    g = C.FIRST
    x, w = (torch.from_numpy(t).to(DEV) for t in C.random_inputs(g))
    if channels_last: x = x.contiguous(memory_format=torch.channels_last)
    bias = torch.linspace(-1.0, 1.0, g.o, device=DEV)
    W = mx_quantize(w, 'MXINT8', 1)
    y = mx_int8_conv2d(x, W, bias, 1, 1)
    assert torch.equal(y.view(torch.int32), mx_int8_conv2d(x, W, bias, 1, 1, use_kernels=False).view(torch.int32))
    X = mx_quantize(x, 'MXINT8', 1)
    _, exact, s = I.conv(*((t.elements.cpu().numpy(), t.scales.cpu().numpy()) for t in (X, W)), g, bias.cpu().numpy())
    assert (np.abs(y.cpu().numpy().astype(np.float64) - exact) <= I.bound(s, g, bias.cpu().numpy())).all() and np.abs(exact).max() > 1


@pytest.mark.parametrize('what,match', [('dtype', 'Invalid dtype'), ('shape', 'expected'), ('device', 'not on the GPU')])
def test_binding_refuses(what, match):
    X, W = (mx_quantize(torch.randn(*shape, device=DEV), 'MXINT8', 1) for shape in ((2, 40, 6, 5), (7, 40, 3, 3)))
    e, s = X.elements, X.scales
    bad = {'dtype': (e.float(), s), 'shape': (e, torch.cat([s, s], dim=3)), 'device': (e.cpu(), s)}[what]
    with pytest.raises(RuntimeError, match=match): CUDA.MXInt8Conv2d(*bad, W.elements, W.scales, 40)


def test_deployment_with_kernels_equals_the_torch_arms():
    outs = []
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    for use_kernels in (True, False):
        g = harness.small_cnn_graph(seed=3)
        ex = harness.TorchExecutor(g, DEV)
        dep = deploy_graph_mx(g, ex, quantize_graph_mx(g, ex, 'MXINT8', 'MXINT8', use_kernels=use_kernels), use_kernels=use_kernels)
        assert dep.deployed == ['c1', 'c2', 'fc']
        outs.append(ex.forward(x)[0])
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
