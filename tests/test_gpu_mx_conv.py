"""The MX convolution on the GPU: the implicit-GEMM kernel on the block-scaled MFMA (ppq_amd/csrc/mx_conv.hip) against the oracle
(tests/mx_conv_reference.py).  The layout and routing tests use data whose every partial sum is exactly representable and compare
with ``==`` on bits: a wrong tap-to-pixel map, stride, dilation, padding test, batch boundary or FP8 half-pair fails them outright.
On random data through the real exporter the kernel must have the BITS of ``mx_matmul`` on the gathered im2col operand -- the two
kernels issue the same instructions on the same register contents in the same order -- and is held to the accumulation bound
K 2^-23 sum |x| |w| against float64 (DESIGN.md sections 9.14, 9.15).  Then NaN placement, the Python API, the C entry point's edge
cases, and ``deploy_graph_mx`` on two graphs against the same layers chained by hand and against the simulation."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mx_conv_reference as C
import mx_gemm_reference as G
import mx_reference as R
from ppq_amd import (CUDA, MXFormat, MXTensor, _lib, deploy_graph_mx, harness, mx_conv2d, mx_conv2d_packed, mx_fake_quant, mx_linear,
                     mx_matmul, mx_quantize, quantize_graph_mx)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 0xA5


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tensors(x, w, fx: str, fw: str, g: C.Geometry):
    return (MXTensor(fx, (g.n, g.c, g.h, g.w), 1, dev(x[0]), dev(x[1])), MXTensor(fw, (g.o, g.c, g.kh, g.kw), 1, dev(w[0]), dev(w[1])))


def host(t: MXTensor):
    return t.elements.cpu().numpy(), t.scales.cpu().numpy()


def hip_conv(x, w, fx: str, fw: str, g: C.Geometry, bias=None) -> np.ndarray:
    X, W = tensors(x, w, fx, fw, g)
    y = mx_conv2d_packed(X, W, None if bias is None else dev(bias), g.stride, g.pad, g.dil)
    assert y.dtype == torch.float32 and tuple(y.shape) == (g.n, g.o, g.oh, g.ow)
    assert y.permute(0, 2, 3, 1).is_contiguous()                                         # [N, OH, OW, O] in storage: channels-last strides
    return y.contiguous().cpu().numpy()


def assert_bits(got: np.ndarray, want64: np.ndarray, what):
    want = want64.astype(np.float32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
    assert bad.size == 0, f'{what}: {bad.size} of {got.size} outputs differ, first at {bad[:4]}: {got.ravel()[bad[:4]]} != {want.ravel()[bad[:4]]}'


@functools.lru_cache(maxsize=None)
def exact(g, fx, fw):
    return C.exact_conv_case(g, fx, fw)


# --------------------------------------------------------------------------------------------------------------- layout: == on bits
@pytest.mark.parametrize('fx,fw', G.PAIRS)
def test_exact_all_pairs(fx, fw):
    x, w, y = exact(C.FIRST, fx, fw)
    assert_bits(hip_conv(x, w, fx, fw, C.FIRST), y, f'{fx} x {fw} {C.FIRST}')


@pytest.mark.parametrize('fx,fw', G.EDGE_PAIRS)
@pytest.mark.parametrize('g', C.EDGE_GEOMETRIES, ids=str)
def test_exact_edges(g, fx, fw):
    x, w, y = exact(g, fx, fw)
    assert_bits(hip_conv(x, w, fx, fw, g), y, f'{fx} x {fw} {g}')


@pytest.mark.parametrize('fx,fw', G.ROUTING_PAIRS)
@pytest.mark.parametrize('g', C.ROUTING_GEOMETRIES, ids=str)
def test_routing(g, fx, fw):
    """Every (tap, channel block): each output is the one term of the pixel behind the tap, or exactly +0 in the padding."""
    for tap in range(g.kh * g.kw):
        for cb in range(g.nbc):
            x, w, y = C.routing_conv_case(g, fx, fw, tap, cb)
            assert_bits(hip_conv(x, w, fx, fw, g), y, f'{fx} x {fw} {g} tap {tap} block {cb}')


# ----------------------------------------------------------------------------------------------------- random data: the two kernels tie
@functools.lru_cache(maxsize=None)
def random_on_device(g):
    x, w = C.random_inputs(g)
    return dev(x), dev(w)


@pytest.mark.parametrize('fx,fw', G.PAIRS)
def test_bits_of_mx_matmul_on_the_gathered_operand(fx, fw):
    """Random data through the real exporter, a bias, a NaN in x and one in w: ``mx_conv2d_packed`` has the bits of ``mx_matmul`` on
    ``gather_im2col(x)`` and the weight viewed as [O, K'], NaN placement included."""
    for g in C.RANDOM_GEOMETRIES:
        x, w = random_on_device(g)
        x, w = x.clone(), w.clone()
        x[g.n - 1, 5, 1, g.w - 1] = float('nan')
        w[3, g.c - 1, 0, g.kw - 1] = float('nan')
        bias = torch.linspace(-3.0, 5.0, g.o, device=DEV)
        X, W = mx_quantize(x, fx, 1), mx_quantize(w, fw, 1)
        got = mx_conv2d_packed(X, W, bias, g.stride, g.pad, g.dil)
        ae, as_ = C.gather_im2col(host(X), fx, g)
        we, ws = C.weight_operand(host(W))
        want = mx_matmul(MXTensor(fx, (g.m, g.k), 1, dev(ae), dev(as_)), MXTensor(fw, (g.o, g.k), 1, dev(we), dev(ws)), bias)
        want = want.reshape(g.n, g.oh, g.ow, g.o).permute(0, 3, 1, 2)
        nan = torch.isnan(got)
        assert nan.any() and not nan.all() and nan[:, 3].all()
        assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)), (fx, fw, str(g))


@pytest.mark.parametrize('fx,fw', G.PAIRS)
def test_random_within_the_bound(fx, fw):
    """|Y - Y_float64| <= K 2^-23 S with K = kh kw 32 nbc for every output, against the oracle on the exported bytes and against the
    simulation: mx_fake_quant of both operands convolved in float64."""
    for g in C.RANDOM_GEOMETRIES:
        x, w = random_on_device(g)
        X, W = mx_quantize(x, fx, 1), mx_quantize(w, fw, 1)
        got = mx_conv2d_packed(X, W, None, g.stride, g.pad, g.dil).contiguous().cpu().numpy().astype(np.float64)
        y, s = C.conv(host(X), host(W), fx, fw, g)
        err = np.abs(got - y)
        print(f'{fx} x {fw} {g}: max |err| / S = {(err / np.maximum(s, 1e-300)).max():.3e} (bound {g.k * 2.0 ** -23:.3e})')
        assert np.isfinite(got).all() and (err <= C.bound(s, g)).all(), (fx, fw, str(g), float((err / np.maximum(s, 1e-300)).max()))
        sim = F.conv2d(mx_fake_quant(x, fx, 1).cpu().double(), mx_fake_quant(w, fw, 1).cpu().double(), None, g.stride, g.pad, g.dil).numpy()
        assert (np.abs(got - sim) <= C.bound(s, g)).all(), (fx, fw, str(g))


# ----------------------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize('fx,fw,side,kind', C.NAN_CASES)
def test_nan_placement(fx, fw, side, kind):
    g = C.NAN_GEOMETRY
    x, w, y, nan = C.nan_conv_case(g, fx, fw, side, kind)
    bias = np.linspace(-3.0, 5.0, g.o).astype(np.float32)
    for b in (None, bias):
        got = hip_conv(x, w, fx, fw, g, b)
        assert np.array_equal(np.isnan(got), nan), np.argwhere(np.isnan(got) != nan)[:4]
        assert (R.bits(got)[nan] == 0x7fc00000).all()                                    # the quiet NaN, under a bias as well
        want = y.astype(np.float32) if b is None else y.astype(np.float32) + b[None, :, None, None]
        assert np.array_equal(R.bits(got)[~nan], R.bits(want)[~nan])


# ------------------------------------------------------------------------------------------------------------------- the Python API
def test_mx_conv2d_is_quantize_then_packed_and_takes_either_layout():
    g = C.FIRST
    x, w = random_on_device(g)
    bias = torch.linspace(-3.0, 5.0, g.o, device=DEV)
    W = mx_quantize(w, 'MXFP4_E2M1', 1)
    for fmt in ('MXFP8_E4M3', 'MXFP6_E2M3', 'MXFP4_E2M1'):
        q = mx_quantize(x, fmt, 1)
        y = mx_conv2d(x, W, fmt, bias, 1, 1)
        assert tuple(y.shape) == (g.n, g.o, g.oh, g.ow) and y.stride() == (g.oh * g.ow * g.o, 1, g.ow * g.o, g.o)
        assert y.is_contiguous(memory_format=torch.channels_last)
        bits = y.contiguous().view(torch.int32)
        assert torch.equal(bits, mx_conv2d_packed(q, W, bias, 1, 1).contiguous().view(torch.int32))
        assert torch.equal(bits, q.conv2d(W, bias, (1, 1), (1, 1), (1, 1)).contiguous().view(torch.int32))
        assert torch.equal(bits, CUDA.MXConv2d(q.elements, q.scales, q.format, W.elements, W.scales, W.format, g.c, bias, (1, 1), (1, 1)).contiguous().view(torch.int32))
        cl = x.contiguous(memory_format=torch.channels_last)
        assert not cl.is_contiguous()
        assert torch.equal(bits, mx_conv2d(cl, W, fmt, bias, 1, 1).contiguous().view(torch.int32))
        assert torch.equal(bits, (mx_conv2d(x, W, fmt, None, 1, 1) + bias.view(1, -1, 1, 1)).contiguous().view(torch.int32))    # one float32 add
    ref = mx_conv2d(x.cpu(), W.to('cpu'), 'MXFP8_E4M3', bias.cpu(), 1, 1, use_kernels=False)          # the torch arm: close, not identical
    y = mx_conv2d(x, W, 'MXFP8_E4M3', bias, 1, 1)
    assert tuple(ref.shape) == tuple(y.shape) and torch.allclose(y.cpu(), ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))


def test_misaligned_contiguous_view():
    """An image slice of a 6-bit activation with an odd nbc and an odd pixel count per image starts 8 mod 16: a valid operand, which
    the binding copies (the C entry point refuses such a pointer)."""
    g = C.geometry([2, 160, 3, 5], 33, (1, 3), 1, (0, 1))                                # 15 pixels of 120 bytes per image
    fx, fw = 'MXFP6_E3M2', 'MXFP4_E2M1'
    x, w, y = exact(g, fx, fw)
    X, W = tensors(x, w, fx, fw, g)
    e, s = X.elements[1:], X.scales[1:]
    assert e.is_contiguous() and e.data_ptr() % 16 == 8
    got = CUDA.MXConv2d(e, s, fx, W.elements, W.scales, fw, g.c, None, g.stride, g.pad, g.dil)
    assert_bits(got.contiguous().cpu().numpy(), y[1:], 'an image slice')


def test_two_calls_give_the_same_bits():
    g = C.FIRST
    x, w = random_on_device(g)
    X, W = mx_quantize(x, 'MXFP6_E3M2', 1), mx_quantize(w, 'MXFP8_E5M2', 1)
    a, b = mx_conv2d_packed(X, W, None, 1, 1), mx_conv2d_packed(X, W, None, 1, 1)
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the C entry point
def _raw(X, W, fx, fw, bias, y_ptr, g, x_off=0, **over):
    a = dict(n=g.n, c=g.c, h=g.h, w=g.w, o=g.o, kh=g.kh, kw=g.kw)
    a.update(over)
    st = _lib.lib.ppqhip_mx_conv2d(X.elements.data_ptr() + x_off, X.scales.data_ptr(), MXFormat[fx].value, W.elements.data_ptr(), W.scales.data_ptr(),
                                   MXFormat[fw].value, bias, y_ptr, a['n'], a['c'], a['h'], a['w'], a['o'], a['kh'], a['kw'], g.stride[0], g.stride[1],
                                   g.pad[0], g.pad[1], g.dil[0], g.dil[1], None)
    return st, _lib.last_error()


def test_output_outside_the_tensor_is_untouched():
    g = C.FIRST
    fx, fw = 'MXFP6_E3M2', 'MXFP8_E4M3'
    x, w, y = exact(g, fx, fw)
    X, W = tensors(x, w, fx, fw, g)
    pad, count = 8, g.m * g.o                                                            # floats: the view stays 16-B aligned
    buf = torch.full((4 * (2 * pad + count),), SENTINEL, dtype=torch.uint8, device=DEV).view(torch.float32)
    out = buf[pad:pad + count]
    assert _raw(X, W, fx, fw, None, out.data_ptr(), g)[0] == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert_bits(C.rows_to_nchw(out.cpu().numpy().reshape(g.m, g.o), g), y, 'the view')
    raw = buf.view(torch.uint8).cpu().numpy()
    assert (raw[:4 * pad] == SENTINEL).all() and (raw[4 * (pad + count):] == SENTINEL).all()


def test_c_zero_and_empty():
    """C = 0: every output is +0, or the bias's bits; N = 0 or O = 0: nothing is written.  Through the C entry point: the Python API
    refuses empty operands."""
    lib = _lib.lib
    g = C.FIRST
    E4M3, FP4 = MXFormat['MXFP8_E4M3'].value, MXFormat['MXFP4_E2M1'].value
    buf = torch.full((4 * g.m * g.o,), SENTINEL, dtype=torch.uint8, device=DEV).view(torch.float32)
    bias = torch.linspace(-2.0, 2.0, g.o, device=DEV)
    geo = (g.n, 0, g.h, g.w, g.o, g.kh, g.kw, 1, 1, 1, 1, 1, 1)
    assert lib.ppqhip_mx_conv2d(None, None, E4M3, None, None, FP4, None, buf.data_ptr(), *geo, None) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert (buf.view(torch.int32) == 0).all()
    assert lib.ppqhip_mx_conv2d(None, None, FP4, None, None, E4M3, bias.data_ptr(), buf.data_ptr(), *geo, None) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32).reshape(g.m, g.o), bias.view(torch.int32).expand(g.m, g.o))
    x, w, _ = exact(g, 'MXFP8_E4M3', 'MXFP4_E2M1')
    X, W = tensors(x, w, 'MXFP8_E4M3', 'MXFP4_E2M1', g)
    buf = torch.full((4 * g.m * g.o,), SENTINEL, dtype=torch.uint8, device=DEV)
    for over in (dict(n=0), dict(o=0), dict(n=0, o=0)):
        assert _raw(X, W, 'MXFP8_E4M3', 'MXFP4_E2M1', bias.data_ptr(), buf.data_ptr(), g, **over)[0] == 0
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


def test_refusals():
    g = C.FIRST
    fx, fw = 'MXFP8_E4M3', 'MXFP4_E2M1'
    x, w, _ = exact(g, fx, fw)
    X, W = tensors(x, w, fx, fw, g)
    out = torch.empty(g.m * g.o, device=DEV)
    xr, wr = random_on_device(g)
    with pytest.raises(RuntimeError, match='MXINT8'): mx_conv2d_packed(mx_quantize(xr, 'MXINT8', 1), W, None, 1, 1)
    with pytest.raises(RuntimeError, match='MXINT8'): mx_conv2d(xr, mx_quantize(wr, 'MXINT8', 1), 'MXFP8_E4M3', None, 1, 1)
    i8 = mx_quantize(xr, 'MXINT8', 1)
    with pytest.raises(RuntimeError, match='MXINT8 is not an operand type'):
        CUDA.MXConv2d(i8.elements, i8.scales, 'MXINT8', W.elements, W.scales, fw, g.c, None, (1, 1), (1, 1))
    with pytest.raises(RuntimeError, match='packed along axis 3'): mx_conv2d_packed(mx_quantize(xr, fx, 3), W, None, 1, 1)
    with pytest.raises(RuntimeError, match='groups must be 1'): mx_conv2d(xr, W, fx, None, 1, 1, 1, groups=2)
    with pytest.raises(RuntimeError, match='does not fit'): mx_conv2d_packed(X, W, None, 1, 0, 4)
    with pytest.raises(RuntimeError, match='expected'): CUDA.MXConv2d(X.elements, X.scales, fx, W.elements, W.scales, fw, g.c + 32)
    with pytest.raises(RuntimeError, match='at least'): CUDA.MXConv2d(X.elements, X.scales, fx, W.elements, W.scales, fw, g.c, None, (0, 1))
    with pytest.raises(RuntimeError, match='not on the GPU'): CUDA.MXConv2d(X.elements, X.scales, fx, W.elements, W.scales, fw, g.c, torch.zeros(g.o))
    unaligned = 'mx_conv2d: elements and y must be 16-byte aligned'
    assert _raw(X, W, fx, fw, None, out.data_ptr(), g, x_off=4) == (-1, unaligned)
    assert _raw(X, W, fx, fw, None, out.data_ptr() + 4, g) == (-1, unaligned)
    assert _raw(X, W, fx, fw, None, W.elements.data_ptr(), g) == (-1, 'mx_conv2d: an output overlaps an input')
    assert _raw(X, W, fx, fw, None, X.elements.data_ptr(), g) == (-1, 'mx_conv2d: an output overlaps an input')
    assert _raw(X, W, fx, fw, out.data_ptr(), out.data_ptr(), g) == (-1, 'mx_conv2d: an output overlaps an input')      # the bias
    assert _raw(X, W, fx, fw, None, out.data_ptr(), g, kh=10) == (-1, 'mx_conv2d: the kernel window does not fit the padded input: no output')
    assert _raw(X, W, fx, fw, None, out.data_ptr(), g)[0] == 0


# --------------------------------------------------------------------------------------------------------------------- the deployment
def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def test_deploy_small_cnn_has_the_bits_of_the_hand_chain():
    g = harness.small_cnn_graph(seed=3)
    ex = harness.TorchExecutor(g, DEV)
    wfmt, afmt = 'MXFP4_E2M1', 'MXFP6_E2M3'
    d = quantize_graph_mx(g, ex, wfmt, afmt)
    x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    simulated = ex.forward(x)[0]
    dep = deploy_graph_mx(g, ex, d)
    assert dep.deployed == ['c1', 'c2', 'fc'] and dep.skipped == {} and sorted(dep.weights) == ['c1_w', 'c2_w', 'fc_w']
    got = ex.forward(x)[0]
    v = lambda n: g.variables[n].value
    a = F.relu(mx_conv2d(x, dep.weights['c1_w'], afmt, v('c1_b'), 1, 1))
    b = mx_conv2d(a, dep.weights['c2_w'], afmt, v('c2_b'), 1, 1)
    f = torch.flatten(F.adaptive_avg_pool2d(F.relu(b + a), 1), 1)
    want = mx_linear(f, dep.weights['fc_w'], afmt, v('fc_b'))
    assert torch.equal(_bits(got), _bits(want))
    assert torch.allclose(got, simulated, rtol=1e-3, atol=1e-3 * float(simulated.abs().max()))
    dep.refresh()
    assert dep.deployed == ['c1', 'c2', 'fc'] and torch.equal(_bits(ex.forward(x)[0]), _bits(want))
    dep.remove()
    assert dep.deployed == [] and torch.equal(_bits(ex.forward(x)[0]), _bits(simulated))


def test_deploy_transformer_mlp_has_the_bits_of_the_hand_chain():
    g = harness.transformer_mlp_graph(seed=1)
    ex = harness.TorchExecutor(g, DEV)
    wfmt, afmt = 'MXFP4_E2M1', 'MXFP8_E4M3'
    d = quantize_graph_mx(g, ex, wfmt, afmt)
    x = torch.randn(3, 5, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    simulated = ex.forward(x)[0]
    dep = deploy_graph_mx(g, ex, d)
    assert dep.deployed == ['fc1', 'fc2'] and dep.skipped == {}
    got = ex.forward(x)[0]
    v = lambda n: g.variables[n].value
    h = F.layer_norm(x, x.shape[-1:], v('ln_w'), v('ln_b'))
    h = F.gelu(mx_linear(h, dep.weights['fc1_w'], afmt, v('fc1_b')))
    want = mx_linear(h, dep.weights['fc2_w'], afmt, v('fc2_b')) + x
    assert torch.equal(_bits(got), _bits(want))
    assert torch.allclose(got, simulated, rtol=1e-3, atol=1e-3 * float(simulated.abs().max()))
    dep.remove()
    assert torch.equal(_bits(ex.forward(x)[0]), _bits(simulated))


def test_deployed_matmul_runs_on_the_weights_own_bytes():
    g = harness.BaseGraph('mm')
    x = g.create_variable('input'); g.inputs['input'] = x
    gen = torch.Generator().manual_seed(0)
    w = g.create_variable('mm_w', torch.randn(72, 33, generator=gen), True)               # [in, out]: packed along axis 0
    m = g.create_operation('MatMul', 'mm', [x, w])
    t = g.create_operation('Transpose', 'tr', [m], {'perm': (1, 0)})
    y = g.create_operation('MatMul', 'act_act', [m, t])
    g.outputs[y.name] = y
    ex = harness.TorchExecutor(g, DEV)
    d = quantize_graph_mx(g, ex, 'MXFP6_E3M2', 'MXFP8_E4M3')
    inp = torch.randn(9, 72, generator=gen).to(DEV)
    simulated = ex.forward(inp, [m.name])[0]
    dep = deploy_graph_mx(g, ex, d)
    assert dep.deployed == ['mm'] and dep.skipped == {'act_act': 'the operands are not an activation and a parameter'}
    W = dep.weights['mm_w']
    assert W.axis == 0 and dep._operands['mm'].elements.data_ptr() == W.elements.data_ptr()
    got = ex.forward(inp, [m.name])[0]
    want = mx_linear(inp, mx_quantize(w.value.t().contiguous(), 'MXFP6_E3M2', -1), 'MXFP8_E4M3')
    assert torch.equal(_bits(got), _bits(want))
    assert torch.allclose(got, simulated, rtol=1e-3, atol=1e-3 * float(simulated.abs().max()))


def test_first_conv_against_the_simulation():
    """One layer, MXFP4 weights with MXFP6_E2M3 activations: the first Conv's output from the deployed graph and from the simulated
    graph (mx_fake_quant of both operands, float32 conv2d) differ by at most 2 K 2^-23 S -- one float32-chain allowance each for the
    scaled MFMA and for the float32 convolution around the same float64 value; S is the oracle's, on the exported bytes."""
    g = harness.small_cnn_graph(seed=3)
    ex = harness.TorchExecutor(g, DEV)
    wfmt, afmt = 'MXFP4_E2M1', 'MXFP6_E2M3'
    d = quantize_graph_mx(g, ex, wfmt, afmt)
    x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    name = g.operations['c1'].outputs[0].name
    simulated = ex.forward(x, [name])[0].contiguous().cpu().numpy().astype(np.float64)
    dep = deploy_graph_mx(g, ex, d)
    deployed = ex.forward(x, [name])[0].contiguous().cpu().numpy().astype(np.float64)
    geo = C.geometry([2, 3, 8, 8], 16, 3, 1, 1)
    _, s = C.conv(host(mx_quantize(x, afmt, 1)), host(dep.weights['c1_w']), afmt, wfmt, geo)
    diff = np.abs(deployed - simulated)
    print(f'first Conv, {afmt} x {wfmt}: max |deployed - simulated| / S = {(diff / np.maximum(s, 1e-300)).max():.3e} '
          f'(bound {2 * geo.k * 2.0 ** -23:.3e}); identical bits: {np.array_equal(R.bits(deployed.astype(np.float32)), R.bits(simulated.astype(np.float32)))}')
    assert deployed.shape == simulated.shape == s.shape and (diff <= 2 * C.bound(s, geo)).all()
