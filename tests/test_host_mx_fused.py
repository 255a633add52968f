"""The fused epilogue of the MX GEMM / convolution without a GPU: the torch arm of every new keyword against
the NumPy composition (tests/mx_fused_reference.py), every Python and C refusal, the grouping of deploy_graph_mx(fuse=True) on a CPU
executor, the -0 / NaN rule of the ReLU, and the routing comparison of tests/test_gpu_mx_fused.py refusing two wrong epilogues."""
import numpy as np
import pytest
import torch

import mx_conv_reference as C
import mx_fused_reference as FR
import mx_gemm_reference as G
import mx_pack_reference as P
import mx_reference as R
from ppq_amd import MXFormat, MXTensor, _lib, deploy_graph_mx, ffi, harness, mx_conv2d, mx_conv2d_packed, mx_linear, mx_matmul, mx_quantize
from ppq_amd import mx as mx_module
from ppq_amd.mx import quantize_graph_mx, relu_positive_zero

GEMM = (17, 70, 160)
CASES = ((False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True))


def t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a))


def gemm_operands(fa, fb):
    m, n, k = GEMM
    a, b, _ = G.exact_case(m, n, k, fa, fb)
    rng = np.random.default_rng(11)
    bias = (rng.integers(-64, 64, n) / 8.0).astype(np.float32)                           # multiples of 2^-3: every add is exact
    residual = (rng.integers(-2048, 2048, (m, n)) / 8.0).astype(np.float32)
    A, B = MXTensor(fa, (m, k), 1, t(a[0]), t(a[1])), MXTensor(fb, (n, k), 1, t(b[0]), t(b[1]))
    return a, b, A, B, bias, residual


# ------------------------------------------------------------------------------------------------------------------ the torch arms
@pytest.mark.parametrize('fo', FR.OUT_FORMATS)
def test_torch_arm_of_mx_matmul(fo):
    fa, fb = 'MXFP8_E4M3', 'MXFP4_E2M1'
    a, b, A, B, bias, residual = gemm_operands(fa, fb)
    for use_bias, use_res, relu in CASES:
        bn, rn = (bias if use_bias else None), (residual if use_res else None)
        v, (we, ws) = FR.fused_matmul(a, b, fa, fb, GEMM[2], fo, bn, rn, relu)
        kw = dict(residual=None if rn is None else t(rn), relu=relu)
        y, p = mx_matmul(A, B, None if bn is None else t(bn), False, out_format=fo, out_float=True, **kw)
        assert np.array_equal(R.bits(y.numpy()), R.bits(v)), (fo, use_bias, use_res, relu)
        assert isinstance(p, MXTensor) and p.format.name == fo and p.shape == (GEMM[0], GEMM[1]) and p.axis == 1
        assert np.array_equal(p.elements.numpy(), we) and np.array_equal(p.scales.numpy(), ws)
        only = mx_matmul(A, B, None if bn is None else t(bn), False, out_format=fo, **kw)
        assert isinstance(only, MXTensor) and torch.equal(only.elements, p.elements) and torch.equal(only.scales, p.scales)
        if use_res or relu:
            plain = mx_matmul(A, B, None if bn is None else t(bn), False, **kw)
            assert isinstance(plain, torch.Tensor) and np.array_equal(R.bits(plain.numpy()), R.bits(v))
    assert isinstance(mx_matmul(A, B, None, False), torch.Tensor)                           # the defaults: what it returned before


def test_torch_arm_of_mx_linear_and_lead_shape():
    fa, fb = 'MXFP6_E2M3', 'MXFP6_E3M2'
    _, _, A, B, bias, residual = gemm_operands(fa, fb)
    x = A.dequantize(use_kernels=False)[:16].reshape(2, 8, -1)                               # exactly representable: quantising it again is exact
    r = t(residual[:16]).reshape(2, 8, -1)
    y, p = mx_linear(x, B, fa, t(bias), False, residual=r, relu=True, out_format='MXFP4_E2M1', out_float=True)
    want = relu_positive_zero(mx_linear(x, B, fa, t(bias), False) + r)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32)) and p.shape == (2, 8, GEMM[1]) and p.axis == 2
    q = mx_quantize(want, 'MXFP4_E2M1', -1, use_kernels=False)
    assert torch.equal(p.elements, q.elements) and torch.equal(p.scales, q.scales)


@pytest.mark.parametrize('fo', FR.OUT_FORMATS)
def test_torch_arm_of_mx_conv2d_packed(fo):
    g, fx, fw = C.FIRST, 'MXFP4_E2M1', 'MXFP8_E5M2'
    x, w, _ = C.exact_conv_case(g, fx, fw)
    X = MXTensor(fx, (g.n, g.c, g.h, g.w), 1, t(x[0]), t(x[1]))
    W = MXTensor(fw, (g.o, g.c, g.kh, g.kw), 1, t(w[0]), t(w[1]))
    rng = np.random.default_rng(13)
    bias = (rng.integers(-64, 64, g.o) / 8.0).astype(np.float32)
    residual = (rng.integers(-2048, 2048, (g.n, g.o, g.oh, g.ow)) / 8.0).astype(np.float32)
    for use_bias, use_res, relu in CASES:
        bn, rn = (bias if use_bias else None), (residual if use_res else None)
        v, (we, ws) = FR.fused_conv(x, w, fx, fw, g, fo, bn, rn, relu)
        kw = dict(residual=None if rn is None else t(rn), relu=relu)
        y, p = mx_conv2d_packed(X, W, None if bn is None else t(bn), g.stride, g.pad, g.dil, False, out_format=fo, out_float=True, **kw)
        assert np.array_equal(R.bits(y.contiguous().numpy()), R.bits(v)), (fo, use_bias, use_res, relu)
        assert p.shape == (g.n, g.o, g.oh, g.ow) and p.axis == 1
        assert np.array_equal(p.elements.numpy(), we) and np.array_equal(p.scales.numpy(), ws)
    # mx_conv2d passes the keywords on, and the packed result is the x of the next layer
    xf = X.dequantize(use_kernels=False)
    p2 = mx_conv2d(xf, W, fx, t(bias), g.stride, g.pad, g.dil, use_kernels=False, residual=t(residual), relu=True, out_format=fo)
    assert torch.equal(p2.elements, p.elements) and torch.equal(p2.scales, p.scales)
    W2 = mx_quantize(torch.randn(8, g.o, 1, 1, generator=torch.Generator().manual_seed(0)), 'MXFP4_E2M1', 1, use_kernels=False)
    assert mx_conv2d_packed(p2, W2, use_kernels=False).shape == (g.n, 8, g.oh, g.ow)


def test_relu_rule_on_zero_and_nan():
    """v > 0 ? v : +0: -0 and every negative value become +0 -- F.relu keeps -0 -- and a NaN stays the NaN it is, payload and sign."""
    pattern = np.array([0x80000000, 0x00000000, 0xbf800000, 0x3f800000, 0x7fc00000, 0xffc00001, 0x80000001, 0x00000001, 0xff800000, 0x7f800000], np.uint32)
    want = np.array([0, 0, 0, 0x3f800000, 0x7fc00000, 0xffc00001, 0, 0x00000001, 0, 0x7f800000], np.uint32)
    v = torch.from_numpy(pattern.view(np.float32))
    assert np.array_equal(relu_positive_zero(v).numpy().view(np.uint32), want)
    assert np.array_equal(FR.relu(pattern.view(np.float32)).view(np.uint32), want)
    assert torch.nn.functional.relu(v).numpy().view(np.uint32)[0] in (0, 0x80000000)          # F.relu may keep the -0 ...
    # ... which the packed code would show: the sign bit of the element
    neg = mx_quantize(torch.tensor([[-0.0] + [1.0] * 31]), 'MXFP8_E4M3', -1, use_kernels=False)
    pos = mx_quantize(relu_positive_zero(torch.tensor([[-0.0] + [1.0] * 31])), 'MXFP8_E4M3', -1, use_kernels=False)
    assert int(neg.elements[0, 0]) == 0x80 and int(pos.elements[0, 0]) == 0
    # a NaN through the whole torch arm: the FP8 code, or a dead block
    _, _, A, B, _, residual = gemm_operands('MXFP4_E2M1', 'MXFP4_E2M1')
    r = t(residual); r[3, 40] = float('nan')
    p8 = mx_matmul(A, B, None, False, residual=r, relu=True, out_format='MXFP8_E5M2')
    assert int(p8.elements[3, 40]) & 0x7f == 0x7f and int(p8.scales[3, 1]) != 0xff
    p4 = mx_matmul(A, B, None, False, residual=r, relu=True, out_format='MXFP4_E2M1')
    assert int(p4.scales[3, 1]) == 0xff and (p4.elements[3, 16:32] == 0).all() and int(p4.scales[3, 0]) != 0xff and int(p4.scales[2, 1]) != 0xff


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_python_refusals():
    _, _, A, B, bias, residual = gemm_operands('MXFP8_E4M3', 'MXFP4_E2M1')
    r = t(residual)
    for uk in (False, True):                                                             # refused before any kernel is reached
        with pytest.raises(RuntimeError, match='out_format MXINT8 is not a format the fused epilogue packs'): mx_matmul(A, B, None, uk, out_format='MXINT8')
        with pytest.raises(RuntimeError, match=r'residual of shape \[17, 5\], expected \[17, 70\]'): mx_matmul(A, B, None, uk, residual=r[:, :5])
        with pytest.raises(RuntimeError, match='residual must be a float32 tensor'): mx_matmul(A, B, None, uk, residual=r.double())
        with pytest.raises(RuntimeError, match='residual must be a float32 tensor'): mx_matmul(A, B, None, uk, residual=residual)
        with pytest.raises(RuntimeError, match='no output'): mx_matmul(A, B, None, uk, relu=True, out_float=False)
    with pytest.raises(RuntimeError, match='residual is on'): mx_matmul(A, B, None, False, residual=r.to('meta'))
    with pytest.raises(ValueError, match='unknown MX format'): mx_matmul(A, B, None, False, out_format='MXFP5')
    g = C.FIRST
    x, w, _ = C.exact_conv_case(g, 'MXFP4_E2M1', 'MXFP4_E2M1')
    X = MXTensor('MXFP4_E2M1', (g.n, g.c, g.h, g.w), 1, t(x[0]), t(x[1]))
    W = MXTensor('MXFP4_E2M1', (g.o, g.c, g.kh, g.kw), 1, t(w[0]), t(w[1]))
    with pytest.raises(RuntimeError, match='mx_conv2d: residual of shape'): mx_conv2d_packed(X, W, None, 1, 1, 1, False, residual=torch.zeros(g.n, g.o, g.oh))
    with pytest.raises(RuntimeError, match='mx_conv2d: out_format MXINT8'): mx_conv2d_packed(X, W, None, 1, 1, 1, False, out_format=MXFormat.MXINT8)
    with pytest.raises(RuntimeError, match='not on the GPU'):                             # the binding has no CPU path
        ffi.CUDA.MXMatmulFused(A.elements, A.scales, A.format, B.elements, B.scales, B.format, GEMM[2], out_format='MXFP4_E2M1')


def test_c_entry_points_check_arguments_without_a_device():
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    lib = _lib.lib
    buf = np.zeros(16384 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    E4M3, FP6, FP4, INT8 = (MXFormat[f].value for f in ('MXFP8_E4M3', 'MXFP6_E3M2', 'MXFP4_E2M1', 'MXINT8'))

    # A [4, 64] E4M3: elements 256 B at p, scales 8 B at p + 256; B [40, 64] FP4: elements 1280 B at p + 512, scales 80 B at p + 1792; bias 160 B
    # at p + 2048; residual 640 B at p + 2560; c 640 B at p + 4096; out_elements (2 blocks a row: up to 256 B) at p + 8192, out_scales 8 B at p + 9216
    def gemm(ae=p, as_=p + 256, fa=E4M3, be=p + 512, bs=p + 1792, fb=FP4, bias=p + 2048, res=p + 2560, relu=1, c=p + 4096, oe=p + 8192, os_=p + 9216,
             fo=E4M3, m=4, n=40, k=64):
        return lib.ppqhip_mx_gemm_fused(ae, as_, fa, be, bs, fb, bias, res, relu, c, oe, os_, fo, m, n, k, None), _lib.last_error()
    w = 'mx_gemm_fused: '
    assert gemm(fa=INT8) == (-1, w + 'A: MXINT8 is not an operand type of the scaled MFMA')
    assert gemm(fb=9) == (-1, w + 'B: unknown MX format 9')
    assert gemm(fo=INT8) == (-1, w + 'out_format: MXINT8 is not a format the fused epilogue packs')
    assert gemm(fo=INT8, oe=0, os_=0) == (-1, w + 'out_format: MXINT8 is not a format the fused epilogue packs')       # checked even when nothing is packed
    assert gemm(fo=-1) == (-1, w + 'out_format: unknown MX format -1')
    assert gemm(oe=0) == (-1, w + 'out_elements and out_scales must both be set or both be null')
    assert gemm(os_=0) == (-1, w + 'out_elements and out_scales must both be set or both be null')
    assert gemm(c=0, oe=0, os_=0) == (-1, w + 'no output: c and out_elements are both null')
    assert gemm(oe=p + 8192 + 8) == (-1, w + 'out_elements must be 16-byte aligned')
    for size in ('m', 'n', 'k'):
        assert gemm(**{size: -1}) == (-1, w + 'negative size')
        assert gemm(**{size: 1 << 31}) == (-1, w + 'a size above 2^31 - 1')
    for ptr in ('ae', 'as_', 'be', 'bs'): assert gemm(**{ptr: 0}) == (-1, w + 'null pointer')
    unaligned = w + 'elements and c must be 16-byte aligned'
    assert gemm(ae=p + 8) == (-1, unaligned) and gemm(be=p + 512 + 4) == (-1, unaligned) and gemm(c=p + 4096 + 4) == (-1, unaligned)
    overlap, two = w + 'an output overlaps an input', w + 'two outputs overlap in memory'
    assert gemm(c=p + 2560) == (-1, overlap)                                              # c on the residual
    assert gemm(c=p + 2048) == (-1, overlap)                                              # ... on the bias
    assert gemm(oe=p + 2560 + 512) == (-1, overlap)                                      # out_elements reach into the residual's tail
    assert gemm(os_=p + 256) == (-1, overlap)                                             # out_scales on A's scales
    assert gemm(oe=p + 4096 + 512) == (-1, two)                                           # out_elements inside c
    assert gemm(os_=p + 8192 + 255) == (-1, two)                                          # out_scales on the last byte of out_elements (E4M3: 256 B)
    assert gemm(fo=FP6, os_=p + 8192 + 191) == (-1, two)                                  # FP6: 192 B
    assert gemm(m=(1 << 31) - 1, n=64) == (-1, w + 'more than 2^31 - 1 output blocks')           # 2 blocks a row
    assert gemm(m=0)[0] == 0 and gemm(n=0)[0] == 0 and gemm(m=0, ae=0, c=0, oe=0, os_=0, res=0)[0] == -1          # no output is refused first
    assert gemm(m=0, ae=0, be=0)[0] == 0

    # x [1, 64, 4, 4] E4M3 at p / p + 1024; w [2, 64, 3, 3] FP4 at p + 2048 / p + 2624; bias at p + 2688, as in tests/test_host_mx_conv.py;
    # residual [1, 2, 2, 2] 32 B at p + 3072; y 32 B at p + 4096; out_elements (1 block a pixel: 4 * 32 B) at p + 8192, out_scales 4 B at p + 9216
    def conv(xe=p, xs=p + 1024, fx=E4M3, we=p + 2048, ws=p + 2624, fw=FP4, bias=p + 2688, res=p + 3072, relu=0, y=p + 4096, oe=p + 8192, os_=p + 9216,
             fo=E4M3, n=1, c=64, h=4, w=4, o=2, kh=3, kw=3, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1):
        return lib.ppqhip_mx_conv2d_fused(xe, xs, fx, we, ws, fw, bias, res, relu, y, oe, os_, fo, n, c, h, w, o, kh, kw, sh, sw, ph, pw, dh, dw, None), _lib.last_error()
    w = 'mx_conv2d_fused: '
    assert conv(fx=INT8) == (-1, w + 'x: MXINT8 is not an operand type of the scaled MFMA')
    assert conv(fo=INT8) == (-1, w + 'out_format: MXINT8 is not a format the fused epilogue packs')
    assert conv(fo=6) == (-1, w + 'out_format: unknown MX format 6')
    assert conv(oe=0) == (-1, w + 'out_elements and out_scales must both be set or both be null')
    assert conv(y=0, oe=0, os_=0) == (-1, w + 'no output: y and out_elements are both null')
    assert conv(oe=p + 8192 + 4) == (-1, w + 'out_elements must be 16-byte aligned')
    assert conv(kh=0) == (-1, w + 'kernel size must be at least 1') and conv(sw=0) == (-1, w + 'stride must be at least 1')
    assert conv(kh=5) == (-1, w + 'the kernel window does not fit the padded input: no output')
    assert conv(xs=0) == (-1, w + 'null pointer')
    assert conv(y=p + 4096 + 4) == (-1, w + 'elements and y must be 16-byte aligned')
    assert conv(y=p + 3072) == (-1, w + 'an output overlaps an input')                   # y on the residual
    assert conv(oe=p + 3072 - 112) == (-1, w + 'an output overlaps an input')            # the last 16 of out_elements' 128 B on the residual
    assert conv(os_=p + 4096 + 31) == (-1, w + 'two outputs overlap in memory')
    assert conv(n=1 << 10, c=32, h=1026, w=1026, o=64) == (-1, w + 'more than 2^31 - 1 output blocks')      # M = 2^30 pixels, 2 blocks each
    assert conv(n=0)[0] == 0 and conv(o=0)[0] == 0


# ---------------------------------------------------------------------------------------- the routing comparison refuses wrong epilogues
@pytest.mark.parametrize('fmt', FR.OUT_FORMATS)
def test_routing_comparison_refuses_wrong_epilogues(fmt):
    fa, fb = 'MXFP8_E4M3', 'MXFP4_E2M1'

    def torch_arm(a, b, fa, fb, k, residual, fmt):
        A, B = MXTensor(fa, (a[0].shape[0], k), 1, t(a[0]), t(a[1])), MXTensor(fb, (b[0].shape[0], k), 1, t(b[0]), t(b[1]))
        p = mx_matmul(A, B, None, False, residual=t(residual), out_format=fmt)
        return p.elements.numpy(), p.scales.numpy()
    assert FR.routing_mismatches(torch_arm, fa, fb, fmt) == []
    over16 = FR.routing_mismatches(FR.wrong_max_over_16, fa, fb, fmt)
    assert {n for n, what in over16 if what == 'scales'} == set(FR.ROUTING_NS)             # a maximum over 16 of the 32 columns: every N
    padding = FR.routing_mismatches(FR.wrong_padding_takes_part, fa, fb, fmt)
    assert {n for n, _ in padding} == {33, 70} and all(what == 'elements' for _, what in padding)      # N = 64 has no padding column


# ------------------------------------------------------------------------------------------------------------------------- the graph
PlainHook, crcrc_graph, same = FR.PlainHook, FR.crcrc_graph, FR.same


def deployed(make, fuse, wf='MXFP4_E2M1', af='MXFP8_E4M3'):
    g = make()
    ex = harness.TorchExecutor(g, 'cpu')
    d = quantize_graph_mx(g, ex, wf, af, use_kernels=False)
    return g, ex, deploy_graph_mx(g, ex, d, use_kernels=False, fuse=fuse)


def test_grouping_on_the_small_cnn():
    g, ex, dep = deployed(lambda: harness.small_cnn_graph(seed=3), True)
    _, ex0, dep0 = deployed(lambda: harness.small_cnn_graph(seed=3), False)
    assert dep0.groups == {} and dep.deployed == dep0.deployed == ['c1', 'c2', 'fc']
    c1, c2, fc = dep.groups['c1'], dep.groups['c2'], dep.groups['fc']
    assert c1.members == ['c1', 'c1_relu'] and c1.relu and c1.residual is None
    assert c1.out_format is MXFormat.MXFP8_E4M3                                            # c2 takes it packed; the Add reads the float copy
    assert c2.members == ['c2', 'add', 'add_relu'] and c2.relu and c2.residual == g.operations['c1_relu'].outputs[0].name
    assert c2.out_format is None and c2.notes == ['float output: no deployed consumer']   # GlobalAveragePool reads it
    assert fc.members == ['fc'] and fc.out_format is None and not fc.relu
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    want = ex0.forward(x)
    assert same(ex.forward(x), want)
    # a hook on a member, a requested intermediate, forward_cached and partial_graph_forward: the values of fuse=False
    for name in ('c1', 'c1_relu', 'add'):
        assert same(ex.forward(x, hooks={name: PlainHook()}), ex0.forward(x, hooks={name: PlainHook()}))
    for out in (g.operations['c1'].outputs[0].name, g.operations['c1_relu'].outputs[0].name, g.operations['add'].outputs[0].name):
        got, ref = ex.forward(x, [out, *g.outputs]), ex0.forward(x, [out, *g.outputs])
        assert isinstance(got[0], torch.Tensor) and same(got, ref)
    assert same(ex.forward_cached(x, list(g.outputs), {}), want)
    # a cache filled by an earlier call: a later request for a member's own output gets ITS values, not the group's last tensor
    names = [v.name for op in g.topological_sort() for v in op.outputs]
    want_all = ex0.forward(x, names)
    cache = {}
    assert same(ex.forward_cached(x, list(g.outputs), cache), want)
    assert g.operations['c1'].outputs[0].name not in cache and g.operations['add'].outputs[0].name not in cache
    for k, n in enumerate(names): assert torch.equal(ex.forward_cached(x, [n], cache)[0], want_all[k]), n
    assert float(ex.forward_cached(x, [g.operations['c1'].outputs[0].name], cache)[0].min()) < 0          # the conv's output, before the ReLU
    ops = g.topological_sort()
    assert same(ex.partial_graph_forward(ops, {'input': x}, list(g.outputs)), want)
    dep.remove()
    assert ex._group_overrides == {} and ex._overrides == {} and ex._takes_packed == set()


def test_grouping_on_conv_relu_conv_relu_conv():
    g, ex, dep = deployed(crcrc_graph, True)
    _, ex0, _ = deployed(crcrc_graph, False)
    assert [dep.groups[n].members for n in ('k0', 'k1', 'k2')] == [['k0', 'k0_relu'], ['k1', 'k1_relu'], ['k2']]
    assert [dep.groups[n].out_format for n in ('k0', 'k1', 'k2')] == [MXFormat.MXFP8_E4M3, MXFormat.MXFP8_E4M3, None]
    x = torch.randn(2, 3, 6, 5, generator=torch.Generator().manual_seed(2))
    seen = []
    # what a plain forward needs as float: only the graph's output; k1 and k2 are handed the packed activation
    plan = ex._group_plan(g.topological_sort(), None, list(g.outputs), False)
    assert plan['k0'][2] == set() and plan['k1'][2] == set() and plan['k2'][2] == set(g.outputs)
    orig = mx_module.mx_quantize
    mx_module.mx_quantize = lambda *a, **k: (seen.append(tuple(a[0].shape)), orig(*a, **k))[1]
    try: got = ex.forward(x)
    finally: mx_module.mx_quantize = orig
    assert same(got, ex0.forward(x))
    # the torch arm packs with mx_quantize too: one call for the graph input, one per packed hand-over, none of a consumer's own
    assert seen == [(2, 3, 6, 5), (2, 40, 6, 5), (2, 40, 6, 5)]
    # a packed-only value never reaches code that expects a float tensor: requesting it makes it float, hooking its consumer too
    mid = g.operations['k0_relu'].outputs[0].name
    assert isinstance(ex.forward(x, [mid])[0], torch.Tensor) and same(ex.forward(x, [mid]), ex0.forward(x, [mid]))
    assert same(ex.forward(x, hooks={'k1': PlainHook()}), ex0.forward(x, hooks={'k1': PlainHook()}))


def test_groups_that_do_not_form():
    """The downsample pair: the convolution that runs later takes the earlier one's output as its residual; an Add whose other
    operand is a parameter or the graph's own later tensor is not fused; a Conv feeding a Gemm through pooling hands over float."""
    gen = torch.Generator().manual_seed(0)
    g = harness.BaseGraph('pair')
    x = g.create_variable('input'); g.inputs['input'] = x

    def conv(inp, name, cin=8, cout=8):
        w = g.create_variable(name + '_w', torch.randn([cout, cin, 1, 1], generator=gen) * 0.3, True)
        b = g.create_variable(name + '_b', torch.randn(cout, generator=gen) * 0.1, True)
        return g.create_operation('Conv', name, [inp, w, b], {'strides': 1, 'pads': 0})
    stem = g.create_operation('Relu', 'stem_relu', [conv(x, 'stem', 3)])
    main, down = conv(stem, 'main'), conv(stem, 'down')
    s = g.create_operation('Relu', 'pair_relu', [g.create_operation('Add', 'pair_add', [main, down])])
    shift = g.create_variable('shift', torch.randn(1, 8, 1, 1, generator=gen), True)
    last = g.create_operation('Add', 'shift_add', [conv(s, 'last'), shift])
    g.outputs[last.name] = last

    def build(fuse):
        import copy
        gg = copy.deepcopy(g)
        ex = harness.TorchExecutor(gg, 'cpu')
        d = quantize_graph_mx(gg, ex, 'MXFP6_E2M3', 'MXFP6_E2M3', use_kernels=False)
        return gg, ex, deploy_graph_mx(gg, ex, d, use_kernels=False, fuse=fuse)
    gg, ex, dep = build(True)
    _, ex0, _ = build(False)
    order = [op.name for op in gg.topological_sort()]
    first, second = sorted(('main', 'down'), key=order.index)
    assert dep.groups[first].members == [first] and dep.groups[first].notes[0] == 'Add pair_add not fused: the other operand of the Add is computed later'
    assert dep.groups[second].members == [second, 'pair_add', 'pair_relu'] and dep.groups[second].residual == gg.operations[first].outputs[0].name
    assert dep.groups['stem'].members == ['stem', 'stem_relu'] and dep.groups['stem'].out_format is MXFormat.MXFP6_E2M3    # two deployed consumers, one format
    assert dep.groups[second].out_format is MXFormat.MXFP6_E2M3                         # 'last' takes it packed
    assert dep.groups['last'].members == ['last'] and dep.groups['last'].notes[0] == 'Add shift_add not fused: the other operand of the Add is a parameter'
    x = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(4))
    assert same(ex.forward(x), ex0.forward(x))
    dep.remove()
    sim = ex.forward(x)
    import copy
    g2 = copy.deepcopy(g)
    ex2 = harness.TorchExecutor(g2, 'cpu')
    quantize_graph_mx(g2, ex2, 'MXFP6_E2M3', 'MXFP6_E2M3', use_kernels=False)
    assert same(sim, ex2.forward(x))                                                     # .remove() restores the simulated path bit for bit


def test_a_delegated_config_keeps_its_operation_out_of_the_tail():
    """The per-operation path applies a delegate registered on a config that is not activated; a fused launch would skip it, so
    such an Add or Relu is not fused (the rule of the executor's own epilogue plan)."""
    g = harness.small_cnn_graph(seed=3)
    ex = harness.TorchExecutor(g, 'cpu')
    d = quantize_graph_mx(g, ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=False)
    relu_cfg = g.operations['c1_relu'].config.output_quantization_config[0]
    add_cfg = g.operations['add'].config.input_quantization_config[0]
    ex.register_quantize_delegate(relu_cfg, lambda tensor, config: tensor * 2.0)
    ex.register_quantize_delegate(add_cfg, lambda tensor, config: tensor + 1.0)
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    plain = deploy_graph_mx(g, ex, d, use_kernels=False, fuse=False)
    want = ex.forward(x)
    plain.remove()
    dep = deploy_graph_mx(g, ex, d, use_kernels=False, fuse=True)
    assert dep.groups['c1'].members == ['c1'] and dep.groups['c2'].members == ['c2']
    assert dep.groups['c2'].notes[0] == 'Add add not fused: a config of the Add is activated or delegated'
    assert same(ex.forward(x), want)
