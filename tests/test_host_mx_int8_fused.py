"""The fused epilogue of the MXINT8 kernels without a GPU: the torch arms against the composition they stand
for (the plain torch arm, a float32 add, ``relu_positive_zero``, ``mx_quantize``), the refusals, the deployment.  All on bits."""
import numpy as np
import pytest
import torch

from ppq_amd import (_lib, deploy_graph_mx, harness, mx_int8_conv2d, mx_int8_conv2d_packed, mx_int8_linear, mx_int8_matmul, mx_quantize,
                     quantize_graph_mx)
from ppq_amd.mx import relu_positive_zero

KW = dict(use_kernels=False)
q = lambda t, axis, f='MXINT8': mx_quantize(t, f, axis, use_kernels=False)
bits = lambda t: t.contiguous().view(torch.int32)


same_packed = lambda a, b: a.format is b.format and a.axis == b.axis and torch.equal(a.elements, b.elements) and torch.equal(a.scales, b.scales)


def operands(conv: bool):
    gen = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=gen)
    if conv: return r(2, 40, 6, 5), q(r(70, 40, 3, 3), 1), r(70), r(2, 70, 6, 5)
    return r(3, 70), q(r(37, 70), -1), r(37), r(3, 37)


@pytest.mark.parametrize('conv', [False, True], ids=['matmul', 'conv'])
@pytest.mark.parametrize('residual,relu,out_float', [(True, True, True), (False, True, False), (True, False, None)])
def test_torch_arms_are_the_composition(conv, residual, relu, out_float):
    x, W, bias, res = operands(conv)
    res, axis = (res if residual else None), (1 if conv else -1)
    X = q(x, axis)
    if conv: plain, on_float, args = mx_int8_conv2d_packed(X, W, bias, 1, 1, **KW), mx_int8_conv2d, (1, 1, 1, 1)
    else: plain, on_float, args = mx_int8_matmul(X, W, bias, **KW), mx_int8_linear, ()
    want = plain + res if residual else plain
    if relu: want = relu_positive_zero(want)
    tail = dict(residual=res, relu=relu, out_format='MXINT8', out_float=out_float)
    got = (mx_int8_conv2d_packed(X, W, bias, 1, 1, **KW, **tail) if conv else mx_int8_matmul(X, W, bias, **KW, **tail))
    y, packed = got if out_float else (None, got)                                        # out_float=None with a format: packed only
    assert same_packed(packed, q(want, axis)) and (y is None or torch.equal(bits(y), bits(want)))
    again = on_float(x, W, bias, *args, **KW, **tail)                                    # the two-launch forms pass the keywords on
    assert same_packed(again[1] if out_float else again, packed)
    assert torch.equal(bits(on_float(x, W, bias, *args, **KW, residual=res, relu=relu)), bits(want))         # no format: the float tensor


def test_python_refusals():
    x, W, bias, res = operands(False)
    X = q(x, -1)
    with pytest.raises(RuntimeError, match='mx_int8_matmul: out_format MXFP8_E4M3: the int8 kernels pack MXINT8 only'): mx_int8_matmul(X, W, out_format='MXFP8_E4M3', **KW)
    with pytest.raises(RuntimeError, match='mx_int8_conv2d: out_format MXFP4_E2M1'): mx_int8_conv2d(*operands(True)[:2], out_format='MXFP4_E2M1', **KW)
    with pytest.raises(RuntimeError, match=r'residual of shape \[37, 3\], expected \[3, 37\]'): mx_int8_matmul(X, W, residual=res.t(), **KW)
    with pytest.raises(RuntimeError, match='residual must be a float32 tensor'): mx_int8_matmul(X, W, residual=res.double(), **KW)
    with pytest.raises(RuntimeError, match='residual is on meta'): mx_int8_matmul(X, W, residual=res.to('meta'), **KW)
    with pytest.raises(RuntimeError, match='no output: out_format is None and out_float is False'): mx_int8_linear(x, W, out_float=False, **KW)
    g = harness.small_cnn_graph(seed=3)
    ex = harness.TorchExecutor(g, 'cpu')
    with pytest.raises(RuntimeError, match='fuse_int8=True .* needs fuse=True'): deploy_graph_mx(g, ex, {}, use_kernels=False, fuse_int8=True)


def test_c_entry_points_check_arguments_without_a_device():
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    buf = np.zeros(16384 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    # gemm 2 x 40 x 64 / conv x [1, 64, 4, 4], w [2, 64, 3, 3]: operands below p + 4096, bias there, residual (320 / 32 B) at p + 4608, c / y at
    # p + 5120, the packed pair (128 + 4 B) at p + 6144 and p + 6400
    def gemm(res=p + 4608, c=p + 5120, oe=p + 6144, os_=p + 6400, m=2, n=40, k=64):
        return _lib.lib.ppqhip_mx_int8_gemm_fused(p, p + 512, p + 1024, p + 3840, p + 4096, res, 1, c, oe, os_, m, n, k, None), _lib.last_error()

    def conv(res=p + 4608, c=p + 5120, oe=p + 6144, os_=p + 6400, m=1, n=2, k=64):
        return _lib.lib.ppqhip_mx_int8_conv2d_fused(p, p + 1024, p + 2048, p + 3200, p + 4096, res, 1, c, oe, os_, m, k, 4, 4, n, 3, 3, 1, 1, 0, 0, 1, 1,
                                                    None), _lib.last_error()

    for call, what, y in ((gemm, 'mx_int8_gemm_fused', 'c'), (conv, 'mx_int8_conv2d_fused', 'y')):
        assert call(os_=0) == (-1, f'{what}: out_elements and out_scales must both be set or both be null') == call(oe=0)
        assert call(c=0, oe=0, os_=0) == (-1, f'{what}: no output: {y} and out_elements are both null')
        assert call(oe=p + 6144 + 8) == (-1, f'{what}: out_elements must be 16-byte aligned')
        assert call(c=p + 5120 + 4) == (-1, f'{what}: elements and {y} must be 16-byte aligned')
        assert call(m=-1) == (-1, f'{what}: negative size')
        for out in ({'c': p + 4608}, {'oe': p + 4608}, {'os_': p + 4096}, {'oe': p + 16}): assert call(**out) == (-1, f'{what}: an output overlaps an input')
        assert call(oe=p + 5120) == (-1, f'{what}: two outputs overlap in memory') == call(os_=p + 6144 + 16)
        assert call(m=0)[0] == 0 and call(n=0, c=0)[0] == 0                              # nothing to launch
    assert gemm(m=1 << 30, n=40, k=0) == (-1, 'mx_int8_gemm_fused: more than 2^31 - 1 output blocks')


@pytest.mark.parametrize('int8', [None, ['c1']], ids=['all-int8', 'c1-int8-rest-e4m3'])
def test_deployment_on_the_torch_arms(int8):
    g = harness.small_cnn_graph(seed=3)                                                  # Conv -> Relu -> Conv -> Add -> Relu -> GAP -> Gemm
    ex = harness.TorchExecutor(g, 'cpu')
    d = quantize_graph_mx(g, ex, 'MXINT8', 'MXINT8', operations=int8, use_kernels=False)
    if int8: d.update(quantize_graph_mx(g, ex, 'MXFP8_E4M3', 'MXFP8_E4M3', operations=['c2', 'fc'], use_kernels=False))
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2))
    plain = deploy_graph_mx(g, ex, d, **KW)
    want = ex.forward(x)[0]
    plain.remove()
    without = deploy_graph_mx(g, ex, d, fuse=True, **KW)                                 # opt-in: fuse alone groups no int8 operation
    assert 'c1' not in without.groups and 'c1' not in ex._takes_packed and (int8 or without.groups == {})
    without.remove()
    dep = deploy_graph_mx(g, ex, d, fuse=True, fuse_int8=True, **KW)
    assert torch.equal(bits(ex.forward(x)[0]), bits(want)) and ex._takes_packed == {'c1', 'c2', 'fc'}
    c1, c2, fc = (dep.groups[n] for n in ('c1', 'c2', 'fc'))
    assert (c1.members, c1.relu, c1.residual) == (['c1', 'c1_relu'], True, None) and fc.members == ['fc'] and fc.out_format is None
    assert (c2.members, c2.relu, c2.residual, c2.out_format) == (['c2', 'add', 'add_relu'], True, c1.output, None)
    if int8: assert c1.out_format is None and any('run on different ones' in n for n in c1.notes)      # float32 between the two kinds of launch
    else: assert c1.out_format.name == 'MXINT8'
    dep.remove()
    assert ex._group_overrides == {} and ex._overrides == {}
