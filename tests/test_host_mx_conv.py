"""The MX convolution without a GPU: the oracle (tests/mx_conv_reference.py) against a direct float64 ``F.conv2d`` on the decoded
operands, the preconditions of its generators for every geometry and pair the GPU tests use, the packed gather against the decoded
one, the ``use_kernels=False`` arm of ``mx_conv2d`` / ``mx_conv2d_packed`` against the oracle, every argument check, the host-side
refusals of the C entry point (they run before any launch), the executor's operation overrides and ``deploy_graph_mx`` on the torch
arms, and two wrong gathers that the routing comparison must refuse."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mx_conv_reference as C
import mx_gemm_reference as G
import mx_reference as R
from ppq_amd import (MXFormat, MXTensor, _lib, deploy_graph_mx, ffi, harness, mx_conv2d, mx_conv2d_packed, mx_fake_quant, mx_linear,
                     mx_quantize, quantize_graph_mx)


def tensors(x, w, fx: str, fw: str, g: C.Geometry):
    X = MXTensor(fx, (g.n, g.c, g.h, g.w), 1, torch.from_numpy(x[0]), torch.from_numpy(x[1]))
    W = MXTensor(fw, (g.o, g.c, g.kh, g.kw), 1, torch.from_numpy(w[0]), torch.from_numpy(w[1]))
    return X, W


def torch_conv64(x, w, fx, fw, g, bias=None) -> np.ndarray:
    xd = torch.from_numpy(C.decode_x(x, fx, g)).permute(0, 3, 1, 2)
    wd = torch.from_numpy(C.decode_w(w, fw, g)).permute(0, 3, 1, 2)
    return F.conv2d(xd, wd, None if bias is None else torch.from_numpy(bias).double(), g.stride, g.pad, g.dil).numpy()


ALL_GEOMETRIES = [C.FIRST] + C.EDGE_GEOMETRIES


# ------------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize('g', ALL_GEOMETRIES, ids=str)
def test_oracle_against_a_direct_float64_conv2d(g):
    fx, fw = 'MXFP6_E3M2', 'MXFP4_E2M1'
    x, w, y = C.exact_conv_case(g, fx, fw)
    bias = np.arange(g.o) * 0.125 - 2.0                                                  # dyadic: the data stay exact
    got, s = C.conv(x, w, fx, fw, g, bias)
    assert got.shape == (g.n, g.o, g.oh, g.ow) == s.shape
    assert np.array_equal(got, torch_conv64(x, w, fx, fw, g, bias)) and np.array_equal(got, y + bias[None, :, None, None])   # exact data: any order
    xd, wd = np.abs(C.decode_x(x, fx, g)), np.abs(C.decode_w(w, fw, g))
    want_s = F.conv2d(torch.from_numpy(xd).permute(0, 3, 1, 2), torch.from_numpy(wd).permute(0, 3, 1, 2), None, g.stride, g.pad, g.dil).numpy()
    assert np.array_equal(s, want_s)
    assert x[0].shape == (g.n, g.h, g.w, g.nbc * 24) and w[0].shape == (g.o, g.kh, g.kw, g.nbc * 16) and x[1].shape == (g.n, g.h, g.w, g.nbc)
    assert not G.decode(C.flat(x), fx, g.nbc * 32)[:, g.c:].any()                        # the short last block holds +0


def test_the_geometries_reach_what_they_are_there_for():
    g = C.FIRST
    assert (g.nbc, g.nb, g.nb % 4, g.m, g.o) == (2, 18, 2, 70, 70) and g.c % 32 and (g.oh, g.ow) == (7, 5)
    by = {str(e): e for e in C.EDGE_GEOMETRIES}
    assert len(by) == len(C.EDGE_GEOMETRIES) == 7 and {e.o for e in ALL_GEOMETRIES} == {33, 70}
    nbcs = [e.nbc for e in C.EDGE_GEOMETRIES]
    assert nbcs == [2, 2, 1, 4, 5, 2, 2]
    assert C.EDGE_GEOMETRIES[1].stride == (2, 2) and C.EDGE_GEOMETRIES[2][5:7] == (7, 7) and C.EDGE_GEOMETRIES[4].pad == (0, 1)
    assert C.EDGE_GEOMETRIES[4].nbc * 24 % 16 == 8                                       # FP6 pixel pitch 8 mod 16
    assert C.EDGE_GEOMETRIES[5][5:7] == (1, 1) and C.EDGE_GEOMETRIES[5].stride == (2, 2) and C.DILATED.dil == (2, 2)
    for e in ALL_GEOMETRIES:                                                             # padding is met wherever there is padding
        assert (C.tap_pixels(e) < 0).any() == (max(e.pad) > 0)


def test_generators_hold_their_preconditions_for_the_gpu_geometries():
    """The generators assert them; this calls each with every geometry and pair the GPU tests use."""
    for fx, fw in G.PAIRS:
        _, _, y = C.exact_conv_case(C.FIRST, fx, fw)
        assert y.shape == (2, 70, 7, 5)
    for fx, fw in G.EDGE_PAIRS:
        for g in C.EDGE_GEOMETRIES: C.exact_conv_case(g, fx, fw)
    for g in C.ROUTING_GEOMETRIES:
        for fx, fw in G.ROUTING_PAIRS:
            seen = set()
            for tap in range(g.kh * g.kw):
                for cb in range(g.nbc):
                    x, w, y = C.routing_conv_case(g, fx, fw, tap, cb)
                    seen.add(y.tobytes())
                    got, _ = C.conv(x, w, fx, fw, g)
                    assert np.array_equal(got, y) and not np.signbit(y[y == 0]).any()     # the oracle agrees with the closed form
                    assert (y != 0).any() and (y == 0).any() == (C.tap_pixels(g)[:, tap] < 0).any()   # +0 exactly where the tap is padding
                    assert len(np.unique(x[1])) == x[1].size                             # no two activation blocks share a code
            assert len(seen) == g.nb
    with pytest.raises(AssertionError, match='would share a scale code'):
        C.routing_conv_case(C.geometry([2, 160, 4, 4], 33, 2), 'MXFP4_E2M1', 'MXFP4_E2M1', 0, 0)
    for fx, fw, side, kind in C.NAN_CASES:
        x, w, y, nan = C.nan_conv_case(C.NAN_GEOMETRY, fx, fw, side, kind)
        assert nan.shape == y.shape
        if side == 'w': assert nan[:, C.NAN_GEOMETRY.o - 2].all() and nan.sum() == nan[:, C.NAN_GEOMETRY.o - 2].size
        else: assert (nan == nan[:, :1]).all() and not nan[0].any() and 0 < nan[1, 0].sum() < nan[1, 0].size
    for g in C.RANDOM_GEOMETRIES:
        x, w = C.random_inputs(g)
        assert x.shape == (g.n, g.c, g.h, g.w) and w.shape == (g.o, g.c, g.kh, g.kw) and x.dtype == np.float32


@pytest.mark.parametrize('g', ALL_GEOMETRIES, ids=str)
def test_gather_im2col_then_matmul_equals_conv(g):
    for fx, fw in G.EDGE_PAIRS:
        x, w, y = C.exact_conv_case(g, fx, fw)
        a = C.gather_im2col(x, fx, g)
        assert a[0].shape == (g.m, g.nb * C.P.BLOCK_BYTES[fx]) and a[1].shape == (g.m, g.nb)
        c, s = G.matmul(a, C.weight_operand(w), fx, fw, g.k)
        want, want_s = C.conv(x, w, fx, fw, g)
        assert np.array_equal(C.rows_to_nchw(c, g), want) and np.array_equal(want, y) and np.array_equal(C.rows_to_nchw(s, g), want_s)
        pad = C.tap_pixels(g) < 0
        assert (a[1].reshape(g.m, g.kh * g.kw, g.nbc)[pad] == 127).all() and not a[0].reshape(g.m, g.kh * g.kw, -1)[pad].any()
    x, w = C.random_inputs(g)                                                            # real exported bytes, NaN and all
    x[-1, -1, 0, 0] = np.nan
    xp, wp = C.pack4(x, 'MXFP8_E4M3'), C.pack4(w, 'MXFP6_E2M3')
    c, _ = G.matmul(C.gather_im2col(xp, 'MXFP8_E4M3', g), C.weight_operand(wp), 'MXFP8_E4M3', 'MXFP6_E2M3', g.k)
    want, _ = C.conv(xp, wp, 'MXFP8_E4M3', 'MXFP6_E2M3', g)
    assert np.array_equal(np.isnan(C.rows_to_nchw(c, g)), np.isnan(want)) and np.isnan(want).any() and not np.isnan(want).all()
    assert np.allclose(C.rows_to_nchw(c, g)[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------------------------------------------- the torch arm
@pytest.mark.parametrize('g', ALL_GEOMETRIES, ids=str)
def test_torch_arm_on_exact_cases_has_the_oracles_bits(g):
    for fx, fw in G.EDGE_PAIRS:
        x, w, y = C.exact_conv_case(g, fx, fw)
        X, W = tensors(x, w, fx, fw, g)
        got = mx_conv2d_packed(X, W, None, g.stride, g.pad, g.dil, use_kernels=False)
        assert got.dtype == torch.float32 and tuple(got.shape) == (g.n, g.o, g.oh, g.ow)
        assert np.array_equal(R.bits(got.contiguous().numpy()), R.bits(y.astype(np.float32)))
        bias = torch.linspace(-3.0, 5.0, g.o)
        got = X.conv2d(W, bias, g.stride, g.pad, g.dil, use_kernels=False).contiguous().numpy()
        assert np.array_equal(R.bits(got), R.bits((y + bias.double().numpy()[None, :, None, None]).astype(np.float32)))


def test_torch_arm_of_mx_conv2d_and_the_simulation():
    g = C.FIRST
    x, w = (torch.from_numpy(t) for t in C.random_inputs(g))
    bias = torch.linspace(-1.0, 1.0, g.o)
    fx, fw = 'MXFP6_E2M3', 'MXFP4_E2M1'
    W = mx_quantize(w, fw, 1, use_kernels=False)
    y = mx_conv2d(x, W, fx, bias, 1, 1, use_kernels=False)
    assert torch.equal(y, mx_conv2d_packed(mx_quantize(x, fx, 1, use_kernels=False), W, bias, (1, 1), (1, 1), (1, 1), use_kernels=False))
    assert torch.equal(y, mx_conv2d(x.contiguous(memory_format=torch.channels_last), W, fx, bias, 1, 1, use_kernels=False))
    sim = F.conv2d(mx_fake_quant(x, fx, 1, use_kernels=False).double(), mx_fake_quant(w, fw, 1, use_kernels=False).double(), bias.double(), 1, 1)
    assert torch.equal(y, sim.float())                                                   # the same float64 sums up to their order
    want, _ = C.conv(C.pack4(x.numpy(), fx), C.pack4(w.numpy(), fw), fx, fw, g, bias.numpy())
    assert np.allclose(y.numpy(), want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    xn, wn, _, nan = C.nan_conv_case(C.NAN_GEOMETRY, 'MXFP8_E4M3', 'MXFP4_E2M1', 'x', 'code')
    X, W = tensors(xn, wn, 'MXFP8_E4M3', 'MXFP4_E2M1', C.NAN_GEOMETRY)
    got = mx_conv2d_packed(X, W, None, 2, 1, use_kernels=False)
    assert np.array_equal(torch.isnan(got).numpy(), nan)


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    x, w = torch.randn(2, 40, 6, 5), torch.randn(7, 40, 3, 3)
    q = lambda t, f, axis=1: mx_quantize(t, f, axis, use_kernels=False)
    X, W = q(x, 'MXFP8_E4M3'), q(w, 'MXFP4_E2M1')
    for use_kernels in (False, True):
        kw = dict(use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match='x is MXINT8'): mx_conv2d_packed(q(x, 'MXINT8'), W, **kw)
        with pytest.raises(RuntimeError, match='w is MXINT8'): mx_conv2d_packed(X, q(w, 'MXINT8'), **kw)
        with pytest.raises(RuntimeError, match='x .* packed along axis 3'): mx_conv2d_packed(q(x, 'MXFP8_E4M3', 3), W, **kw)
        with pytest.raises(RuntimeError, match='w .* packed along axis 0'): mx_conv2d_packed(X, q(w, 'MXFP4_E2M1', 0), **kw)
        with pytest.raises(RuntimeError, match='x must be 4-d'): mx_conv2d_packed(q(x[0], 'MXFP8_E4M3'), W, **kw)
        with pytest.raises(RuntimeError, match='w must be 4-d'): mx_conv2d_packed(X, q(w[:, :, :, 0], 'MXFP4_E2M1'), **kw)
        with pytest.raises(RuntimeError, match='C mismatch: x has 40 channels, w has 32'): mx_conv2d_packed(X, q(w[:, :32].contiguous(), 'MXFP4_E2M1'), **kw)
        with pytest.raises(RuntimeError, match=r'bias of shape \[6\], expected \[7\]'): mx_conv2d_packed(X, W, torch.zeros(6), **kw)
        with pytest.raises(RuntimeError, match='bias must be a float32 tensor'): mx_conv2d_packed(X, W, torch.zeros(7, dtype=torch.float64), **kw)
        with pytest.raises(RuntimeError, match='stride must be at least 1'): mx_conv2d_packed(X, W, stride=0, **kw)
        with pytest.raises(RuntimeError, match='padding must be at least 0'): mx_conv2d_packed(X, W, padding=(0, -1), **kw)
        with pytest.raises(RuntimeError, match='dilation must be at least 1'): mx_conv2d_packed(X, W, dilation=(1, 0), **kw)
        with pytest.raises(RuntimeError, match='stride must be an int or a pair'): mx_conv2d_packed(X, W, stride=(1, 1, 1), **kw)
        with pytest.raises(RuntimeError, match='does not fit'): mx_conv2d_packed(X, W, dilation=3, **kw)
        with pytest.raises(TypeError, match='MXTensor'): mx_conv2d_packed(x, W, **kw)
        with pytest.raises(TypeError, match='MXTensor'): mx_conv2d_packed(X, w, **kw)
        with pytest.raises(RuntimeError, match='groups must be 1'): mx_conv2d(x, W, 'MXFP8_E4M3', groups=2, **kw)
        with pytest.raises(RuntimeError, match='x must be 4-d'): mx_conv2d(x[0], W, 'MXFP8_E4M3', **kw)
        with pytest.raises(RuntimeError, match='Invalid dtype'): mx_conv2d(x.double(), W, 'MXFP8_E4M3', **kw)
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_conv2d_packed(X, W)     # the kernel arm has no CPU path
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_conv2d(x, W, 'MXFP8_E4M3')
    with pytest.raises(RuntimeError, match='Invalid dtype'): ffi.CUDA.MXConv2d(X.elements.float(), X.scales, 'MXFP8_E4M3', W.elements, W.scales, 'MXFP4_E2M1', 40)
    with pytest.raises(ValueError, match='unknown MX format'): ffi.CUDA.MXConv2d(X.elements, X.scales, 'MXFP8', W.elements, W.scales, 'MXFP4_E2M1', 40)
    assert mx_conv2d_packed(X, W, use_kernels=False).shape == (2, 7, 4, 3)


# ---------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_entry_point_checks_arguments_without_a_device():
    """Formats, sizes, geometry, null pointers, alignment and overlap are checked on the host before anything is launched.  Every
    call below is refused or has nothing to launch: the pointers are host memory."""
    lib = _lib.lib
    buf = np.zeros(8192 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15                                                     # 16-B aligned, 8192 bytes behind it
    E4M3, FP6, FP4, INT8 = (MXFormat[f].value for f in ('MXFP8_E4M3', 'MXFP6_E3M2', 'MXFP4_E2M1', 'MXINT8'))

    # x [1, 64, 4, 4] (E4M3): 32 blocks, elements 1024 B at p, scales 32 B at p + 1024; w [2, 64, 3, 3] (FP4): 36 blocks, elements
    # 576 B at p + 2048, scales 36 B at p + 2624; bias 8 B at p + 2688; y [1, 2, 2, 2]: 32 B at p + 4096
    def conv(xe=p, xs=p + 1024, fx=E4M3, we=p + 2048, ws=p + 2624, fw=FP4, bias=p + 2688, y=p + 4096, n=1, c=64, h=4, w=4, o=2, kh=3, kw=3,
             sh=1, sw=1, ph=0, pw=0, dh=1, dw=1):
        return lib.ppqhip_mx_conv2d(xe, xs, fx, we, ws, fw, bias, y, n, c, h, w, o, kh, kw, sh, sw, ph, pw, dh, dw, None), _lib.last_error()

    assert conv(fx=INT8) == (-1, 'mx_conv2d: x: MXINT8 is not an operand type of the scaled MFMA')
    assert conv(fw=INT8) == (-1, 'mx_conv2d: w: MXINT8 is not an operand type of the scaled MFMA')
    assert conv(fx=6) == (-1, 'mx_conv2d: x: unknown MX format 6')
    assert conv(fw=-1) == (-1, 'mx_conv2d: w: unknown MX format -1')
    for size in ('n', 'c', 'h', 'w', 'o', 'kh', 'kw', 'sh', 'sw', 'ph', 'pw', 'dh', 'dw'):
        assert conv(**{size: -1}) == (-1, 'mx_conv2d: negative size')
        assert conv(**{size: 1 << 31}) == (-1, 'mx_conv2d: a size above 2^31 - 1')
    for size in ('kh', 'kw'): assert conv(**{size: 0}) == (-1, 'mx_conv2d: kernel size must be at least 1')
    for size in ('sh', 'sw'): assert conv(**{size: 0}) == (-1, 'mx_conv2d: stride must be at least 1')
    for size in ('dh', 'dw'): assert conv(**{size: 0}) == (-1, 'mx_conv2d: dilation must be at least 1')
    no_output = 'mx_conv2d: the kernel window does not fit the padded input: no output'
    assert conv(kh=5) == (-1, no_output) and conv(dw=2) == (-1, no_output) and conv(h=2) == (-1, no_output) and conv(h=0) == (-1, no_output)
    assert conv(n=1 << 20, h=1 << 10, w=1 << 10) == (-1, 'mx_conv2d: a size above 2^31 - 1')          # M, and the blocks of x
    assert conv(c=1 << 30, kh=9, kw=9, h=9, w=9) == (-1, 'mx_conv2d: a size above 2^31 - 1')          # kh kw nbc
    assert conv(ph=(1 << 30) + 1) == (-1, 'mx_conv2d: a padded size above 2^31 - 1')
    for ptr in ('xe', 'xs', 'we', 'ws', 'y'): assert conv(**{ptr: 0}) == (-1, 'mx_conv2d: null pointer')
    unaligned = 'mx_conv2d: elements and y must be 16-byte aligned'
    assert conv(xe=p + 8) == (-1, unaligned) and conv(we=p + 2048 + 4) == (-1, unaligned) and conv(y=p + 4096 + 4) == (-1, unaligned)
    overlap = 'mx_conv2d: an output overlaps an input'
    assert conv(y=p + 1008) == (-1, overlap)                                             # y's 32 B reach into x's scales
    assert conv(y=p + 1024) == (-1, overlap)                                             # ... start on them
    assert conv(y=p + 2608) == (-1, overlap)                                             # w's elements and scales
    assert conv(y=p + 2672) == (-1, overlap)                                             # the bias
    assert conv(fx=FP6, y=p + 752) == (-1, overlap)                                      # FP6: 32 * 24 B of x's elements
    assert conv(fx=FP4, y=p + 496) == (-1, overlap)                                      # FP4: 32 * 16 B
    assert conv(n=1 << 21, h=3, w=3, o=1 << 30, xe=0, y=0)[0] == -1                      # refused before anything is touched
    assert conv(n=0)[0] == 0 and conv(o=0)[0] == 0                                       # nothing to launch
    assert conv(n=0, xe=0, y=0)[0] == 0


# --------------------------------------------------------------------------------------------------- the executor's operation overrides
def _mx_cnn(use_kernels=False, device='cpu'):
    g = harness.small_cnn_graph(seed=3)
    ex = harness.TorchExecutor(g, device)
    d = quantize_graph_mx(g, ex, 'MXFP4_E2M1', 'MXFP6_E2M3', use_kernels=use_kernels)
    return g, ex, d


def test_operation_override_seam():
    g, ex, _ = _mx_cnn()
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    names = ['c1', 'c1_relu', 'c2', 'fc']
    out_names = [g.operations[n].outputs[0].name for n in names]
    before = ex.forward(x, out_names)
    plan = harness.plan_epilogues(g.topological_sort(), None, set(g.outputs))
    assert any(m.name == 'c1' for grp in plan for m in grp.ops)                          # conv_ok does not look at input configs
    calls = []

    def fn(op, raw):
        calls.append((op.name, [tuple(t.shape) for t in raw]))
        assert raw[1] is op.inputs[1].value                                              # raw inputs: nothing was quantised
        return torch.full((raw[0].shape[0], raw[1].shape[0], raw[0].shape[2], raw[0].shape[3]), 0.5)

    with pytest.raises(KeyError, match='no operation'): ex.register_operation_override('nope', fn)
    with pytest.raises(TypeError, match='callable'): ex.register_operation_override('c1', 3)
    ex.register_operation_override('c1', fn)
    got = ex.forward(x, out_names)
    assert calls == [('c1', [(2, 3, 8, 8), (16, 3, 3, 3), (16,)])]
    assert (got[0] == 0.5).all() and (got[1] == 0.5).all() and not torch.equal(got[3], before[3])     # fn's output is used, downstream too
    with torch.no_grad():
        groups = ex._epilogue_plan(g.topological_sort(), None, [])
        ex.remove_operation_override('c1')
        assert any(m.name == 'c1' for grp in ex._epilogue_plan(g.topological_sort(), None, []).values() for m in grp.ops)
        ex.register_operation_override('c1', fn)
    assert not any(m.name == 'c1' for grp in groups.values() for m in grp.ops)           # an overridden conv is in no epilogue group
    ops = g.topological_sort()[:2]
    part = ex.partial_graph_forward(ops, {'input': x}, [out_names[1]])
    assert (part[0] == 0.5).all() and len(calls) == 2
    assert (ex.forward_cached(x, [out_names[1]], {})[0] == 0.5).all() and len(calls) == 3

    class Spy:
        def __init__(self): self.seen = []

        def pre_forward_hook(self, inputs, quant_inputs, quant_configs):
            self.seen.append([t.clone() for t in quant_inputs])
            return quant_inputs

        def post_forward_hook(self, outputs, quant_outputs, quant_configs): return quant_outputs

    spy = Spy()
    hooked = ex.forward(x, out_names, hooks={'c1': spy})                                  # hooks bypass the override
    assert len(calls) == 3 and len(spy.seen) == 1
    assert torch.equal(spy.seen[0][0], mx_fake_quant(x, 'MXFP6_E2M3', 1, use_kernels=False))
    for a, b in zip(hooked, before): assert torch.equal(a, b)
    ex.remove_operation_override('c1')
    ex.remove_operation_override('c1')                                                   # idempotent
    after = ex.forward(x, out_names)
    for a, b in zip(after, before): assert torch.equal(a, b)                             # removal restores the bits
    assert len(calls) == 3


@torch.no_grad()
def test_override_names_are_part_of_the_epilogue_signature():
    g, ex, _ = _mx_cnn()
    ops = g.topological_sort()
    assert 'c1' in ex._epilogue_plan(ops, None, [])
    ex.register_operation_override('c1', lambda op, raw: raw[0])
    assert 'c1' not in ex._epilogue_plan(ops, None, [])
    ex.remove_operation_override('c1')
    assert 'c1' in ex._epilogue_plan(ops, None, [])
    assert len(ex._epilogue_cache) == 2


# --------------------------------------------------------------------------------------------------------------------- the deployment
def _chain_cnn(g, x, afmt, weights, use_kernels=False):
    v = lambda n: g.variables[n].value
    a = F.relu(mx_conv2d(x, weights['c1_w'], afmt, v('c1_b'), 1, 1, use_kernels=use_kernels))
    b = mx_conv2d(a, weights['c2_w'], afmt, v('c2_b'), 1, 1, use_kernels=use_kernels)
    s = F.relu(b + a)
    f = torch.flatten(F.adaptive_avg_pool2d(s, 1), 1)
    return mx_linear(f, weights['fc_w'], afmt, v('fc_b'), use_kernels=use_kernels)


def test_deploy_graph_mx_on_the_torch_arms_equals_the_hand_chain():
    g, ex, d = _mx_cnn()
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(2))
    simulated = ex.forward(x)[0]
    dep = deploy_graph_mx(g, ex, d, use_kernels=False)
    assert dep.deployed == ['c1', 'c2', 'fc'] and dep.skipped == {} and sorted(dep.weights) == ['c1_w', 'c2_w', 'fc_w']
    got = ex.forward(x)[0]
    assert torch.equal(got, _chain_cnn(g, x, 'MXFP6_E2M3', dep.weights))
    assert torch.allclose(got, simulated, rtol=1e-4, atol=1e-5)
    g.variables['c2_w'].value = g.variables['c2_w'].value * 2.0                          # the weights changed: re-pack
    dep.refresh()
    assert dep.deployed == ['c1', 'c2', 'fc']
    assert torch.equal(ex.forward(x)[0], _chain_cnn(g, x, 'MXFP6_E2M3', dep.weights)) and not torch.equal(ex.forward(x)[0], got)
    g.variables['c2_w'].value = g.variables['c2_w'].value * 0.5
    dep.remove()
    assert dep.deployed == [] and ex._overrides == {}
    assert torch.equal(ex.forward(x)[0], simulated)
    dep2 = deploy_graph_mx(g, ex, None, use_kernels=False)                               # the formats recorded in the configs
    assert dep2.deployed == ['c1', 'c2', 'fc'] and torch.equal(ex.forward(x)[0], got)
    dep2.remove()


def test_deploy_graph_mx_skips_what_the_kernels_do_not_take():
    g = harness.BaseGraph('mixed')
    x = g.create_variable('input'); g.inputs['input'] = x
    gen = torch.Generator().manual_seed(0)
    w1 = g.create_variable('grouped_w', torch.randn(8, 4, 3, 3, generator=gen), True)
    a = g.create_operation('Conv', 'grouped', [x, w1], {'strides': 1, 'pads': 1, 'group': 2})
    w2 = g.create_variable('conv_w', torch.randn(6, 8, 1, 1, generator=gen), True)
    b = g.create_operation('Conv', 'conv', [a, w2], {'strides': (2, 1), 'pads': 0})
    f = g.create_operation('Flatten', 'flatten', [b])
    w3 = g.create_variable('mm_w', torch.randn(6 * 2 * 4, 5, generator=gen), True)
    m = g.create_operation('MatMul', 'mm', [f, w3])
    t = g.create_operation('Transpose', 'tr', [m], {'perm': (1, 0)})
    y = g.create_operation('MatMul', 'act_act', [m, t])
    g.outputs[y.name] = y
    ex = harness.TorchExecutor(g, 'cpu')
    d = quantize_graph_mx(g, ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=False)
    inp = torch.randn(3, 8, 4, 4, generator=gen)
    simulated = ex.forward(inp)[0]
    dep = deploy_graph_mx(g, ex, d, use_kernels=False)
    assert dep.deployed == ['conv', 'mm']
    assert dep.skipped == {'grouped': 'a grouped convolution', 'act_act': 'the operands are not an activation and a parameter'}
    W = dep.weights['mm_w']
    assert W.axis == 0 and W.shape == (48, 5)
    a = F.conv2d(mx_fake_quant(inp, 'MXFP8_E4M3', 1, use_kernels=False), mx_fake_quant(w1.value, 'MXFP4_E2M1', 1, use_kernels=False), None, 1, 1, groups=2)
    b = mx_conv2d(a, dep.weights['conv_w'], 'MXFP8_E4M3', None, (2, 1), 0, use_kernels=False)
    mm = mx_linear(torch.flatten(b, 1), MXTensor(W.format, (5, 48), 1, W.elements, W.scales), 'MXFP8_E4M3', use_kernels=False)
    assert dep._operands['mm'].elements.data_ptr() == W.elements.data_ptr()              # the weight's own bytes, no copy
    want = torch.matmul(mx_fake_quant(mm, 'MXFP8_E4M3', -1, use_kernels=False), mx_fake_quant(mm.t(), 'MXFP8_E4M3', -2, use_kernels=False))
    got = ex.forward(inp)[0]
    assert torch.equal(got, want) and torch.allclose(got, simulated, rtol=1e-3, atol=1e-3 * float(simulated.abs().max()))
    dep.remove()
    assert torch.equal(ex.forward(inp)[0], simulated)
    g3 = harness.small_cnn_graph(seed=3)
    ex3 = harness.TorchExecutor(g3, 'cpu')
    d3 = quantize_graph_mx(g3, ex3, 'MXINT8', 'MXFP8_E4M3', use_kernels=False)
    dep3 = deploy_graph_mx(g3, ex3, d3, use_kernels=False)
    assert dep3.deployed == [] and set(dep3.skipped) == {'c1', 'c2', 'fc'} and all('MXINT8' in r for r in dep3.skipped.values())


# ------------------------------------------------------------------------------------------- the routing comparison refuses wrong gathers
@pytest.mark.parametrize('wrong', [C.tap_pixels_kx_ky, C.tap_pixels_no_batch_padding], ids=['taps_in_kx_ky_order', 'no_padding_at_the_batch_boundary'])
def test_routing_comparison_refuses_a_wrong_gather(wrong):
    """What the GPU routing test does, with a wrong gather in the kernel's place: the packed operand gathered through the wrong
    tap-to-pixel map, multiplied by the GEMM oracle, must differ from the routing expectation for some (tap, channel block) -- and
    the right gather must pass for every one."""
    fx, fw = G.ROUTING_PAIRS[1]
    for g in C.ROUTING_GEOMETRIES:
        refused = 0
        for tap in range(g.kh * g.kw):
            for cb in range(g.nbc):
                x, w, want = C.routing_conv_case(g, fx, fw, tap, cb)
                right, _ = G.matmul(C.gather_im2col(x, fx, g), C.weight_operand(w), fx, fw, g.k)
                assert np.array_equal(C.rows_to_nchw(right, g), want)
                got, _ = G.matmul(C.gather_im2col(x, fx, g, wrong(g)), C.weight_operand(w), fx, fw, g.k)
                refused += not np.array_equal(C.rows_to_nchw(got, g), want)
        assert refused >= g.nbc, (str(g), refused)
