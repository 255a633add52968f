"""The fused epilogue of the MXINT8 kernels on the GPU (csrc/mx_int8_tile.hpp fused_tiles): ONE launch ``==`` the
sequence it replaces (the plain int8 kernel, a float32 add, ``relu_positive_zero``, ``mx_quantize`` on the torch arm) and the oracles."""
import numpy as np
import pytest
import torch

import mx_conv_reference as C
import mx_int8_gemm_reference as G
import mx_pack_reference as P
from ppq_amd import MXTensor, deploy_graph_mx, harness, mx_int8_conv2d, mx_int8_conv2d_packed, mx_int8_matmul, mx_quantize, quantize_graph_mx
from ppq_amd.mx import relu_positive_zero

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
M = N = 70              # 2 x 2 workgroups, tile edges both ways; nbo = 3 with 6 live columns in the last block, beside a wave with all 32
TAILS = [(True, True, True), (False, True, False), (True, False, False), (False, False, True)]       # (residual, relu, out_float)
# M = O = 70; stride 2 with dilation 2; a 1 x 3 kernel padded along one axis (nbc = 5)
GEOMETRIES = [C.FIRST, C.geometry([2, 40, 7, 5], 33, 3, 2, 2, 2), C.EDGE_GEOMETRIES[4]]
bits = lambda t: t.contiguous().view(torch.int32)
on_gpu = lambda *arrays: (torch.from_numpy(a).to(DEV) for a in arrays)


def sequence(plain, residual, relu, axis):
    """What the fused launch replaces, from the plain kernel's result: (float32 tensor, its MXINT8 bytes by the torch arm)."""
    v = plain + residual if residual is not None else plain
    if relu: v = relu_positive_zero(v)
    return v, mx_quantize(v, 'MXINT8', axis, use_kernels=False)


def check(got, out_float, v, packed):
    y, p = got if out_float else (None, got)
    assert torch.equal(p.elements, packed.elements) and torch.equal(p.scales, packed.scales) and (p.axis, p.shape) == (packed.axis, packed.shape)
    assert y is None or torch.equal(bits(y), bits(v))
    return p


@pytest.mark.parametrize('k', [40, 160], ids=['k40', 'k160'])                            # one tail chunk; a full chunk plus a tail chunk
@pytest.mark.parametrize('residual,relu,out_float', TAILS)
def test_gemm(k, residual, relu, out_float):
    rng = np.random.default_rng(k)
    a, b = G.raw_operand(rng, M, k, range(118, 131)), G.raw_operand(rng, N, k, range(118, 131))
    bias, res = rng.standard_normal(N).astype(np.float32), (rng.standard_normal((M, N)) * 8).astype(np.float32)
    A, B = (MXTensor('MXINT8', (e.shape[0], k), 1, *on_gpu(e, s)) for e, s in (a, b))
    tb, tr = on_gpu(bias, res)
    if not residual: tr = None
    v, packed = sequence(mx_int8_matmul(A, B, tb), tr, relu, -1)
    p = check(mx_int8_matmul(A, B, tb, residual=tr, relu=relu, out_format='MXINT8', out_float=out_float), out_float, v, packed)
    if k == 160 and residual and relu:                                                   # the NumPy oracles, end to end
        want = G.matmul(a, b, bias)[0] + res
        e, s = P.pack(np.where(want > 0, want, np.float32(0)), 'MXINT8')
        assert np.array_equal(p.elements.cpu().numpy(), e) and np.array_equal(p.scales.cpu().numpy(), s)


def test_values_the_epilogue_can_get_wrong():
    """A NaN row, an all-zero block, a maximum that rounds to 127 (and one that saturates there), negatives under the ReLU."""
    rng = np.random.default_rng(1)
    a, b = G.raw_operand(rng, M, 160, range(120, 131)), G.raw_operand(rng, N, 160, range(120, 131))
    a[1][0, 2] = 0xff                                                                    # row 0 is NaN
    a[0][1:4] = 0                                                                        # rows 1 .. 3: acc is +0, v is the residual
    res = rng.standard_normal((M, N)).astype(np.float32)
    res[1] = np.where(np.arange(N) % 2, np.float32(0), np.float32(-0.0))
    res[2] = np.linspace(-1.9999, 1.99, N)                                               # 127.36 -> 127; block 0 holds -1.9999 -> 127.99 -> -127
    res[3] = -np.abs(res[3]) - 1
    A, B = (MXTensor('MXINT8', (M, 160), 1, *on_gpu(e, s)) for e, s in (a, b))
    tr, = on_gpu(res)
    for relu in (False, True):
        v, packed = sequence(mx_int8_matmul(A, B), tr, relu, -1)
        y, p = mx_int8_matmul(A, B, residual=tr, relu=relu, out_format='MXINT8', out_float=True)
        check((y, p), True, v, packed)
        e, s = p.elements.cpu().numpy(), p.scales.cpu().numpy()
        assert (s[0] == 0xff).all() and not e[0].any() and torch.isnan(y[0]).all()
        assert not e[1].any() and not s[1].any() and not bits(y)[1].any()                # +0 everywhere, never the code of -0
        assert e[2, N - 1] == 127 and s[2, 2] == 127 and e[2, 0] == (0 if relu else 0x81)
        if relu: assert not e[3].any() and not s[3].any() and not bits(y)[3].any() and (e[1:] < 0x80).all()


@pytest.mark.parametrize('g,tail', list(zip(GEOMETRIES, TAILS)), ids=lambda v: str(v))
def test_conv(g, tail):
    residual, relu, out_float = tail
    x, w = on_gpu(*C.random_inputs(g))
    gen = torch.Generator().manual_seed(7)
    bias, res = torch.randn(g.o, generator=gen).to(DEV), torch.randn(g.n, g.o, g.oh, g.ow, generator=gen).to(DEV)
    X, W = mx_quantize(x, 'MXINT8', 1), mx_quantize(w, 'MXINT8', 1)
    args = (g.stride, g.pad, g.dil)
    v, packed = sequence(mx_int8_conv2d_packed(X, W, bias, *args), res if residual else None, relu, 1)
    for r in ((res, res.contiguous(memory_format=torch.channels_last)) if residual else (None,)):     # copied; read in place
        p = check(mx_int8_conv2d_packed(X, W, bias, *args, residual=r, relu=relu, out_format='MXINT8', out_float=out_float), out_float, v, packed)
    W2 = mx_quantize(torch.randn(33, g.o, 1, 1, generator=gen).to(DEV), 'MXINT8', 1)      # the packed result is the x of the next launch
    assert torch.equal(bits(mx_int8_conv2d_packed(p, W2)), bits(mx_int8_conv2d(v, W2)))


def test_deployment():
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    g = harness.small_cnn_graph(seed=3)
    ex = harness.TorchExecutor(g, DEV)
    d = quantize_graph_mx(g, ex, 'MXINT8', 'MXINT8')                                     # Conv -> Relu -> Conv -> Add -> Relu -> GAP -> Gemm
    plain = deploy_graph_mx(g, ex, d, fuse=False)
    want = ex.forward(x)[0]
    plain.remove()
    dep = deploy_graph_mx(g, ex, d, fuse=True, fuse_int8=True)
    assert torch.equal(bits(ex.forward(x)[0]), bits(want))
    c1, c2 = dep.groups['c1'], dep.groups['c2']
    assert (c1.members, c1.relu, c1.residual, c1.out_format.name) == (['c1', 'c1_relu'], True, None, 'MXINT8')      # packed and, for the Add, float
    assert (c2.members, c2.relu, c2.residual, c2.out_format) == (['c2', 'add', 'add_relu'], True, c1.output, None)
    assert dep.groups['fc'].members == ['fc'] and sorted(dep.groups) == ['c1', 'c2', 'fc']
    dep.remove()
