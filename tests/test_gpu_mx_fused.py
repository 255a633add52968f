"""The fused epilogue of mx_matmul / mx_conv2d_packed (residual, ReLU, MX re-quantisation of the result) on
the GPU.  The reference is the unfused chain on the kernels that exist: mx_matmul (+ bias) + residual, the ReLU as torch.where, then
mx_quantize.  The float32 values come from the same instruction sequence and one IEEE add each, so every comparison is == on bytes
/ bits; packed FP8 NaN codes are compared as code & 0x7f."""
import functools

import numpy as np
import pytest
import torch

import mx_conv_reference as C
import mx_fused_reference as FR
import mx_gemm_reference as G
import mx_pack_reference as P
from ppq_amd import CUDA, MXFormat, MXTensor, _lib, deploy_graph_mx, harness, mx_conv2d, mx_conv2d_packed, mx_linear, mx_matmul, mx_quantize
from ppq_amd import mx as mx_module
from ppq_amd.mx import quantize_graph_mx, relu_positive_zero

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 0xA5
FUSED_SHAPE = (37, 70, 200)          # a short last output block of 6, a partly filled wave both ways, a wave that returns early, a K tail
OUT_ONE = 'MXFP6_E2M3'               # the out_format of the 25-pair sweep: 24-byte blocks, the dword stores
FP8 = ('MXFP8_E4M3', 'MXFP8_E5M2')


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def tensor(packed, fmt: str, k: int) -> MXTensor:
    e, s = packed
    return MXTensor(fmt, (e.shape[0], k), 1, dev(e), dev(s))


def same_packed(got: MXTensor, want: MXTensor, what) -> None:
    """Scales and elements byte for byte; FP8 NaN codes as code & 0x7f (the sign of a NaN is not part of the contract)."""
    assert got.format is want.format and got.shape == want.shape and got.axis == want.axis, what
    assert torch.equal(got.scales, want.scales), (what, 'scales')
    ge, we = got.elements, want.elements
    if got.format.name in FP8:
        nan = (we & 0x7f) == 0x7f if got.format.name == 'MXFP8_E4M3' else (we & 0x7f) > 0x7c
        ge, we = torch.where(nan, ge & 0x7f, ge), torch.where(nan, we & 0x7f, we)
    assert torch.equal(ge, we), (what, 'elements', int((ge != we).sum()))


def same_float(got: torch.Tensor, want: torch.Tensor, what) -> None:
    """== on bits; a NaN against a NaN by position (the payload of a NaN that arithmetic made is not part of the contract)."""
    assert got.shape == want.shape, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, 'NaN positions')
    assert torch.equal(bits(torch.where(gn, torch.zeros_like(got), got)), bits(torch.where(wn, torch.zeros_like(want), want))), what


@functools.lru_cache(maxsize=None)
def random_gemm(shape=FUSED_SHAPE):
    """x [m, k], w [n, k] (by default [37, 200] and [70, 200]) with rows spread over 12 octaves, a bias and a residual of the outputs' own
    magnitude."""
    x, w = G.random_inputs(0, shape)
    rng = np.random.default_rng(5)
    m, n, _ = shape
    bias = rng.standard_normal(n).astype(np.float32)
    residual = (rng.standard_normal((m, n)) * np.exp2(rng.uniform(-4, 8, (m, 1)))).astype(np.float32)
    return dev(x), dev(w), dev(bias), dev(residual)


def unfused(A, B, bias, residual, relu):
    v = mx_matmul(A, B, bias)
    if residual is not None: v = v + residual
    return relu_positive_zero(v) if relu else v


def check_gemm(fa, fb, fo, shape=FUSED_SHAPE):
    x, w, bias, residual = random_gemm(shape)
    A, B = mx_quantize(x, fa, -1), mx_quantize(w, fb, -1)
    for use_bias, use_res, relu in ((True, True, True), (False, False, False), (False, True, False), (True, False, True)):
        b, r = (bias if use_bias else None), (residual if use_res else None)
        want = unfused(A, B, b, r, relu)
        y, packed = mx_matmul(A, B, b, residual=r, relu=relu, out_format=fo, out_float=True)
        what = (fa, fb, fo, use_bias, use_res, relu)
        assert torch.equal(bits(y), bits(want)), what
        same_packed(packed, mx_quantize(want, fo, -1), what)
        only = mx_matmul(A, B, b, residual=r, relu=relu, out_format=fo)              # packed only: no float store
        assert isinstance(only, MXTensor) and torch.equal(only.elements, packed.elements) and torch.equal(only.scales, packed.scales), what
        if relu or use_res:                                                          # float only
            assert torch.equal(bits(mx_matmul(A, B, b, residual=r, relu=relu)), bits(want)), what
    # the elements a short last block lacks are +0: 70 = 2 * 32 + 6
    width = P.WIDTH[fo]
    codes = P.unpack_fields(packed.elements.cpu().numpy().reshape(shape[0], -1, P.BLOCK_BYTES[fo]), width)
    assert codes.shape[1] == 3 and (codes[:, 2, 6:] == 0).all() and (codes[:, 2, :6] != 0).any()


@pytest.mark.parametrize('fa,fb', G.PAIRS)
def test_gemm_all_pairs(fa, fb):
    check_gemm(fa, fb, OUT_ONE)


@pytest.mark.parametrize('fo', FR.OUT_FORMATS)
@pytest.mark.parametrize('fa,fb', G.EDGE_PAIRS)
def test_gemm_all_out_formats(fa, fb, fo):
    check_gemm(fa, fb, fo)


@pytest.mark.parametrize('fa,fb', G.EDGE_PAIRS)
def test_gemm_more_than_one_workgroup_along_m(fa, fb):
    """(130, 70, 416): three tile rows, so the fused epilogue's rows and block index are computed for m0 = 64 and 128 too (the
    shape above has one tile row), with nb = 13: three full K-steps and a tail of one block."""
    assert G.EDGE_SHAPES[-1] == (130, 70, 416)
    check_gemm(fa, fb, OUT_ONE, G.EDGE_SHAPES[-1])


def test_relu_gives_positive_zero():
    """Negative values become +0, whose code is 0 -- the kernel never writes the -0 that F.relu may keep (the rule on -0 itself is
    tests/test_host_mx_fused.py: an accumulator that starts at +0 does not produce one)."""
    a, b, c = G.exact_case(17, 33, 160, 'MXFP4_E2M1', 'MXFP4_E2M1')
    A, B = tensor(a, 'MXFP4_E2M1', 160), tensor(b, 'MXFP4_E2M1', 160)
    residual = dev(-c.astype(np.float32))                                               # every output is then exactly 0 ...
    residual[1, :] -= 1.0                                                               # ... and row 1 is -1
    y, packed = mx_matmul(A, B, residual=residual, relu=True, out_format='MXFP8_E4M3', out_float=True)
    assert (bits(y) == 0).all() and (packed.elements == 0).all()
    assert (bits(mx_matmul(A, B, residual=residual))[1] == bits(torch.full((33,), -1.0, device=DEV))).all()


# ------------------------------------------------------------------------------------------------------------ block-maximum routing
def hip_epilogue(a, b, fa, fb, k, residual, fmt):
    p = mx_matmul(tensor(a, fa, k), tensor(b, fb, k), residual=dev(residual), out_format=fmt)
    return p.elements.cpu().numpy(), p.scales.cpu().numpy()


@pytest.mark.parametrize('fmt', FR.OUT_FORMATS)
@pytest.mark.parametrize('fa,fb', G.EDGE_PAIRS)
def test_block_maximum_routing(fa, fb, fmt):
    """Exact operands and one large power of two per row at column (7 row) % N, N = 33, 64, 70, against the NumPy composition:
    a maximum over the wrong lanes, tile or row gives another scale code (tests/test_host_mx_fused.py shows the comparison
    refusing two wrong epilogues)."""
    assert FR.routing_mismatches(hip_epilogue, fa, fb, fmt) == []


# ---------------------------------------------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize('fo', FR.OUT_FORMATS)
def test_nan_flags_and_residual(fo):
    """A flagged row (5) and a flagged column (40): the FP8 NaN code in every affected element, or scale 0xFF and zero bytes for
    the affected blocks in FP6 / FP4; neighbours untouched.  The flag wins over the residual; a NaN of the residual arrives too."""
    m, n, k = 37, 70, 160
    fa, fb = 'MXFP4_E2M1', 'MXFP6_E3M2'
    a, b, _ = G.exact_case(m, n, k, fa, fb)
    a, b = (a[0].copy(), a[1].copy()), (b[0].copy(), b[1].copy())
    a[1][5, 3] = 0xff
    b[1][40, 1] = 0xff
    A, B = tensor(a, fa, k), tensor(b, fb, k)
    residual = torch.ones(m, n, device=DEV)
    residual[9, 3] = float('nan')
    y, packed = mx_matmul(A, B, residual=residual, out_format=fo, out_float=True)
    want = unfused(A, B, None, residual, False)
    nan = torch.zeros(m, n, dtype=torch.bool, device=DEV); nan[5, :] = True; nan[:, 40] = True
    assert (bits(y)[nan] == 0x7fc00000).all()                                            # the flag's own quiet NaN, residual or not
    nan[9, 3] = True
    assert torch.equal(torch.isnan(y), nan)
    same_float(y, want, fo)
    same_packed(packed, mx_quantize(want, fo, -1), fo)
    e = packed.elements.reshape(m, 3, -1)
    if fo in FP8:
        codes = e.reshape(m, -1)[:, :n]
        assert torch.equal((codes & 0x7f) == 0x7f if fo == 'MXFP8_E4M3' else (codes & 0x7f) > 0x7c, nan)
    else:
        dead = torch.zeros(m, 3, dtype=torch.bool, device=DEV); dead[5, :] = True; dead[:, 1] = True; dead[9, 0] = True
        assert torch.equal(packed.scales == 0xff, dead) and (e[dead] == 0).all()
    # rows and blocks next to the flagged ones have the bytes of the clean result plus the residual
    plain = mx_matmul(tensor((a[0], np.where(a[1] == 0xff, 127, a[1]).astype(np.uint8)), fa, k), tensor((b[0], np.where(b[1] == 0xff, 127, b[1]).astype(np.uint8)), fb, k),
                      residual=torch.ones(m, n, device=DEV), out_format=fo)
    keep = torch.ones(m, 3, dtype=torch.bool, device=DEV); keep[5, :] = False; keep[:, 1] = False; keep[9, 0] = False
    assert torch.equal(packed.scales[keep], plain.scales[keep]) and torch.equal(e[keep], plain.elements.reshape(m, 3, -1)[keep])


# -------------------------------------------------------------------------------------------------------- outputs and robustness
def _raw_gemm(A, B, bias, residual, relu, c_ptr, e_ptr, s_ptr, fo, m, n, k, a_off=0):
    st = _lib.lib.ppqhip_mx_gemm_fused(A.elements.data_ptr() + a_off, A.scales.data_ptr(), A.format.value, B.elements.data_ptr(), B.scales.data_ptr(),
                                       B.format.value, bias, residual, relu, c_ptr, e_ptr, s_ptr, MXFormat[fo].value if isinstance(fo, str) else fo,
                                       m, n, k, None)
    return st, _lib.last_error()


@pytest.mark.parametrize('fo', ['MXFP8_E5M2', 'MXFP6_E3M2', 'MXFP4_E2M1'])
def test_outputs_stay_inside_their_tensors(fo):
    """A null c through the C entry point, sentinels around out_elements, out_scales and c, and two launches with the same bytes."""
    m, n, k = FUSED_SHAPE
    x, w, bias, residual = random_gemm()
    A, B = mx_quantize(x, 'MXFP8_E4M3', -1), mx_quantize(w, 'MXFP4_E2M1', -1)
    want_v = unfused(A, B, bias, residual, True)
    want = mx_quantize(want_v, fo, -1)
    ne, ns, pad = want.elements.numel(), want.scales.numel(), 64
    for with_c in (False, True):
        for _ in range(2):
            be = torch.full((ne + 2 * pad,), SENTINEL, dtype=torch.uint8, device=DEV)
            bs = torch.full((ns + 2 * pad,), SENTINEL, dtype=torch.uint8, device=DEV)
            bc = torch.full((4 * (m * n + 2 * pad),), SENTINEL, dtype=torch.uint8, device=DEV)
            st = _raw_gemm(A, B, bias.data_ptr(), residual.data_ptr(), 1, bc.data_ptr() + 4 * pad if with_c else None, be.data_ptr() + pad,
                           bs.data_ptr() + pad, fo, m, n, k)
            assert st[0] == 0, st
            torch.cuda.synchronize()
            assert torch.equal(be[pad:pad + ne], want.elements.reshape(-1)) and torch.equal(bs[pad:pad + ns], want.scales.reshape(-1))
            for buf, size in ((be, ne), (bs, ns)): assert (buf[:pad] == SENTINEL).all() and (buf[pad + size:] == SENTINEL).all()
            inner = bc[4 * pad:4 * (pad + m * n)]
            if with_c: assert torch.equal(inner.view(torch.int32), bits(want_v).reshape(-1))
            else: assert (inner == SENTINEL).all()
            assert (bc[:4 * pad] == SENTINEL).all() and (bc[4 * (pad + m * n):] == SENTINEL).all()


def test_k_zero_and_empty():
    """K == 0: the epilogue runs on bias (or 0) plus the residual.  M == 0 or N == 0: nothing is launched."""
    m, n = 37, 70
    _, _, bias, residual = random_gemm()
    E4M3, FP4 = MXFormat['MXFP8_E4M3'].value, MXFormat['MXFP4_E2M1'].value
    lib = _lib.lib
    for b in (None, bias):
        v = relu_positive_zero((residual + b) if b is not None else residual + 0.0)
        want = mx_quantize(v, 'MXFP4_E2M1', -1)
        c = torch.empty(m, n, device=DEV); e = torch.empty_like(want.elements); s = torch.empty_like(want.scales)
        st = lib.ppqhip_mx_gemm_fused(None, None, E4M3, None, None, FP4, b.data_ptr() if b is not None else None, residual.data_ptr(), 1, c.data_ptr(),
                                      e.data_ptr(), s.data_ptr(), FP4, m, n, 0, None)
        assert st == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert torch.equal(bits(c), bits(v)) and torch.equal(e, want.elements) and torch.equal(s, want.scales)
    buf = torch.full((4 * m * n,), SENTINEL, dtype=torch.uint8, device=DEV)
    for mm, nn in ((0, n), (m, 0), (0, 0)):
        assert lib.ppqhip_mx_gemm_fused(None, None, E4M3, None, None, FP4, None, None, 0, buf.data_ptr(), None, None, FP4, mm, nn, 0, None) == 0
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


def test_refusals():
    m, n, k = 17, 33, 160
    fa, fb = 'MXFP8_E4M3', 'MXFP4_E2M1'
    a, b, _ = G.exact_case(m, n, k, fa, fb)
    A, B = tensor(a, fa, k), tensor(b, fb, k)
    c = torch.empty(m, n, device=DEV); r = torch.zeros(m, n, device=DEV)
    e = torch.empty(m * 2 * 32 + 16, dtype=torch.uint8, device=DEV); s = torch.empty(m * 2, dtype=torch.uint8, device=DEV)
    E, S, Cp, Rp = e.data_ptr(), s.data_ptr(), c.data_ptr(), r.data_ptr()
    w = 'mx_gemm_fused: '
    assert _raw_gemm(A, B, None, None, 0, None, None, None, 'MXFP8_E4M3', m, n, k) == (-1, w + 'no output: c and out_elements are both null')
    assert _raw_gemm(A, B, None, None, 0, Cp, E, S, 'MXINT8', m, n, k) == (-1, w + 'out_format: MXINT8 is not a format the fused epilogue packs')
    assert _raw_gemm(A, B, None, None, 0, Cp, E, S, 77, m, n, k) == (-1, w + 'out_format: unknown MX format 77')
    assert _raw_gemm(A, B, None, None, 0, Cp, E, None, 'MXFP8_E4M3', m, n, k) == (-1, w + 'out_elements and out_scales must both be set or both be null')
    assert _raw_gemm(A, B, None, None, 0, Cp, E + 8, S, 'MXFP8_E4M3', m, n, k) == (-1, w + 'out_elements must be 16-byte aligned')
    assert _raw_gemm(A, B, None, None, 0, Cp + 4, E, S, 'MXFP8_E4M3', m, n, k) == (-1, w + 'elements and c must be 16-byte aligned')
    assert _raw_gemm(A, B, None, None, 0, Cp, E, S, 'MXFP8_E4M3', m, n, k, a_off=4) == (-1, w + 'elements and c must be 16-byte aligned')
    assert _raw_gemm(A, B, None, Cp, 0, Cp, E, S, 'MXFP8_E4M3', m, n, k) == (-1, w + 'an output overlaps an input')                  # the residual
    assert _raw_gemm(A, B, None, Rp, 0, Cp, A.elements.data_ptr(), S, 'MXFP8_E4M3', m, n, k) == (-1, w + 'an output overlaps an input')
    assert _raw_gemm(A, B, None, Rp, 0, Cp, E, E + 16, 'MXFP8_E4M3', m, n, k) == (-1, w + 'two outputs overlap in memory')
    assert _raw_gemm(A, B, None, Rp, 0, Cp, Cp, S, 'MXFP8_E4M3', m, n, k) == (-1, w + 'two outputs overlap in memory')
    i8 = mx_quantize(torch.randn(m, k, device=DEV), 'MXINT8', -1)
    assert _lib.lib.ppqhip_mx_gemm_fused(i8.elements.data_ptr(), i8.scales.data_ptr(), i8.format.value, B.elements.data_ptr(), B.scales.data_ptr(),
                                         B.format.value, None, None, 0, Cp, None, None, 0, m, n, k, None) == -1
    assert _lib.last_error() == w + 'A: MXINT8 is not an operand type of the scaled MFMA'
    assert _raw_gemm(A, B, None, Rp, 1, Cp, E, S, 'MXFP8_E4M3', m, n, k)[0] == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='MXINT8'): mx_matmul(A, B, out_format='MXINT8')
    with pytest.raises(RuntimeError, match='residual of shape'): mx_matmul(A, B, residual=r[:, :5])
    with pytest.raises(RuntimeError, match='float32'): mx_matmul(A, B, residual=r.double())
    with pytest.raises(RuntimeError, match='residual is on'): mx_matmul(A, B, residual=r.cpu())
    with pytest.raises(RuntimeError, match='no output'): mx_matmul(A, B, relu=True, out_float=False)
    with pytest.raises(RuntimeError, match='MXINT8'): CUDA.MXMatmulFused(A.elements, A.scales, fa, B.elements, B.scales, fb, k, out_format='MXINT8')


def test_linear_and_lead_shape():
    x, w, bias, residual = random_gemm()
    W = mx_quantize(w, 'MXFP4_E2M1', -1)
    x3, r3 = x[:36].reshape(4, 9, -1), residual[:36].reshape(4, 9, -1)
    y, p = mx_linear(x3, W, 'MXFP8_E4M3', bias, residual=r3, relu=True, out_format='MXFP8_E4M3', out_float=True)
    want = relu_positive_zero(mx_linear(x3, W, 'MXFP8_E4M3', bias) + r3)
    assert tuple(y.shape) == (4, 9, 70) and p.shape == (4, 9, 70) and p.axis == 2
    assert torch.equal(bits(y), bits(want))
    same_packed(p, mx_quantize(want, 'MXFP8_E4M3', -1), 'lead shape')


# ---------------------------------------------------------------------------------------------------------------------------- conv
@functools.lru_cache(maxsize=None)
def random_conv(g):
    x, w = C.random_inputs(g)
    rng = np.random.default_rng(7)
    bias = rng.standard_normal(g.o).astype(np.float32)
    residual = rng.standard_normal((g.n, g.o, g.oh, g.ow)).astype(np.float32) * 4.0
    return dev(x), dev(w), dev(bias), dev(residual).contiguous(memory_format=torch.channels_last)


def check_conv(g, fx, fw, fo):
    x, w, bias, residual = random_conv(g)
    X, W = mx_quantize(x, fx, 1), mx_quantize(w, fw, 1)
    for use_bias, use_res, relu in ((False, False, False), (False, True, False), (True, True, True)):
        b, r = (bias if use_bias else None), (residual if use_res else None)
        v = mx_conv2d_packed(X, W, b, g.stride, g.pad, g.dil)
        if r is not None: v = v + r
        if relu: v = relu_positive_zero(v)
        y, packed = mx_conv2d_packed(X, W, b, g.stride, g.pad, g.dil, residual=r, relu=relu, out_format=fo, out_float=True)
        what = (str(g), fx, fw, fo, use_bias, use_res, relu)
        assert y.permute(0, 2, 3, 1).is_contiguous() and torch.equal(bits(y), bits(v)), what
        same_packed(packed, mx_quantize(v, fo, 1), what)
        only = mx_conv2d_packed(X, W, b, g.stride, g.pad, g.dil, residual=r, relu=relu, out_format=fo)
        assert torch.equal(only.elements, packed.elements) and torch.equal(only.scales, packed.scales), what
    assert torch.equal(bits(mx_conv2d_packed(X, W, bias, g.stride, g.pad, g.dil, residual=residual.contiguous(), relu=True, out_format=fo, out_float=True)[0]), bits(v))
    return packed, v


@pytest.mark.parametrize('fx,fw', G.PAIRS)
def test_conv_all_pairs(fx, fw):
    check_conv(C.FIRST, fx, fw, OUT_ONE)


@pytest.mark.parametrize('fo', FR.OUT_FORMATS)
@pytest.mark.parametrize('fx,fw', G.EDGE_PAIRS)
@pytest.mark.parametrize('g', [C.FIRST, C.EDGE_GEOMETRIES[1], C.DILATED], ids=str)
def test_conv_geometries_and_out_formats(g, fx, fw, fo):
    check_conv(g, fx, fw, fo)


@functools.lru_cache(maxsize=None)
def gathered_conv(g, fx, fw):
    """x and w of random_conv with one NaN each, packed, and the same bytes as the operands of the GEMM: gather_im2col(x) [M, K'] and
    the weight viewed as [O, K']."""
    x, w = random_conv(g)[:2]
    x, w = x.clone(), w.clone()
    x[g.n - 1, 5, 1, g.w - 1] = float('nan')
    w[3, g.c - 1, 0, g.kw - 1] = float('nan')
    X, W = mx_quantize(x, fx, 1), mx_quantize(w, fw, 1)
    ae, as_ = C.gather_im2col((X.elements.cpu().numpy(), X.scales.cpu().numpy()), fx, g)
    we, ws = C.weight_operand((W.elements.cpu().numpy(), W.scales.cpu().numpy()))
    return X, W, MXTensor(fx, (g.m, g.k), 1, dev(ae), dev(as_)), MXTensor(fw, (g.o, g.k), 1, dev(we), dev(ws))


@pytest.mark.parametrize('fo', FR.OUT_FORMATS)
@pytest.mark.parametrize('g', C.RANDOM_GEOMETRIES, ids=str)
@pytest.mark.parametrize('fx,fw', G.EDGE_PAIRS)
def test_fused_conv_has_the_bits_of_fused_matmul_on_the_gathered_operand(fx, fw, g, fo):
    """Both kernels run one K-step and one fused epilogue on two A sources, so the tie that
    tests/test_gpu_mx_conv.py pins for the plain kernels holds for the fused ones: bias, residual, ReLU, a NaN in x and one in w, the float and the packed output.  M = 70
    and 18, O = 70 and 33: a short last output block, waves that return early, a K tail.  Both sides run on the device: ==."""
    _, _, bias, residual = random_conv(g)
    X, W, A, B = gathered_conv(g, fx, fw)
    y, packed = mx_conv2d_packed(X, W, bias, g.stride, g.pad, g.dil, residual=residual, relu=True, out_format=fo, out_float=True)
    v, p = mx_matmul(A, B, bias, residual=residual.permute(0, 2, 3, 1).reshape(g.m, g.o), relu=True, out_format=fo, out_float=True)
    what = (fx, fw, str(g), fo)
    nan = torch.isnan(y)
    assert nan.any() and not nan.all() and nan[:, 3].all(), what
    same_float(y, v.reshape(g.n, g.oh, g.ow, g.o).permute(0, 3, 1, 2), what)
    lead = (g.n, g.oh, g.ow)
    same_packed(packed, MXTensor(fo, packed.shape, 1, p.elements.reshape(*lead, -1), p.scales.reshape(*lead, -1)), what)


@pytest.mark.parametrize('fo', FR.OUT_FORMATS)
def test_two_layer_chain(fo):
    """The packed result IS the x of the next mx_conv2d_packed: the two-layer chain has the bits of the chain done unfused."""
    g = C.FIRST
    packed, v = check_conv(g, 'MXFP8_E4M3', 'MXFP4_E2M1', fo)
    w2 = torch.randn(33, g.o, 3, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    W2 = mx_quantize(w2, 'MXFP4_E2M1', 1)
    got = mx_conv2d_packed(packed, W2, None, 1, 1)
    want = mx_conv2d(v, W2, fo, None, 1, 1)
    assert torch.equal(bits(got), bits(want))


def test_conv_refusals_and_c_zero():
    g = C.FIRST
    x, w, bias, residual = random_conv(g)
    X, W = mx_quantize(x, 'MXFP4_E2M1', 1), mx_quantize(w, 'MXFP4_E2M1', 1)
    geo = (g.n, g.c, g.h, g.w, g.o, g.kh, g.kw, *g.stride, *g.pad, *g.dil)
    lib, FP4 = _lib.lib, MXFormat['MXFP4_E2M1'].value
    y = torch.empty(g.n, g.oh, g.ow, g.o, device=DEV)
    nbo = 3
    e = torch.empty(g.m * nbo * 16, dtype=torch.uint8, device=DEV); s = torch.empty(g.m * nbo, dtype=torch.uint8, device=DEV)

    def raw(res, yp, ep, sp, fo, geo=geo):
        st = lib.ppqhip_mx_conv2d_fused(X.elements.data_ptr(), X.scales.data_ptr(), FP4, W.elements.data_ptr(), W.scales.data_ptr(), FP4, None, res, 1,
                                        yp, ep, sp, fo, *geo, None)
        return st, _lib.last_error()
    p = 'mx_conv2d_fused: '
    assert raw(None, None, None, None, FP4) == (-1, p + 'no output: y and out_elements are both null')
    assert raw(None, y.data_ptr(), e.data_ptr(), s.data_ptr(), MXFormat['MXINT8'].value) == (-1, p + 'out_format: MXINT8 is not a format the fused epilogue packs')
    assert raw(None, y.data_ptr(), None, s.data_ptr(), FP4) == (-1, p + 'out_elements and out_scales must both be set or both be null')
    assert raw(None, y.data_ptr(), e.data_ptr() + 4, s.data_ptr(), FP4) == (-1, p + 'out_elements must be 16-byte aligned')
    assert raw(y.data_ptr(), y.data_ptr(), e.data_ptr(), s.data_ptr(), FP4) == (-1, p + 'an output overlaps an input')
    assert raw(None, y.data_ptr(), y.data_ptr(), s.data_ptr(), FP4) == (-1, p + 'two outputs overlap in memory')
    assert raw(None, y.data_ptr(), e.data_ptr(), s.data_ptr(), FP4, geo=(g.n, g.c, g.h, g.w, g.o, 0, 3, 1, 1, 1, 1, 1, 1)) == (-1, p + 'kernel size must be at least 1')
    # c == 0: bias (none here) plus the residual, through the ReLU
    rl = residual.permute(0, 2, 3, 1).contiguous()
    zero = (g.n, 0, g.h, g.w, g.o, g.kh, g.kw, *g.stride, *g.pad, *g.dil)
    assert lib.ppqhip_mx_conv2d_fused(None, None, FP4, None, None, FP4, None, rl.data_ptr(), 1, y.data_ptr(), e.data_ptr(), s.data_ptr(), FP4, *zero, None) == 0, _lib.last_error()
    torch.cuda.synchronize()
    v = relu_positive_zero(rl)
    want = mx_quantize(v, 'MXFP4_E2M1', -1)
    assert torch.equal(bits(y), bits(v)) and torch.equal(e, want.elements.reshape(-1)) and torch.equal(s, want.scales.reshape(-1))
    with pytest.raises(RuntimeError, match='residual of shape'): mx_conv2d_packed(X, W, None, 1, 1, residual=residual[:, :3])
    with pytest.raises(RuntimeError, match='MXINT8'): mx_conv2d_packed(X, W, None, 1, 1, out_format='MXINT8')


# ------------------------------------------------------------------------------------------------------------------------- the graph
PlainHook, crcrc_graph, same = FR.PlainHook, FR.crcrc_graph, FR.same
ACTIVATIONS = ('MXFP4_E2M1', 'MXFP8_E4M3')           # both under MXFP4 weights: MXFP4 x MXFP4 hands over 16-byte blocks, E4M3 32-byte ones


def quantized(make, afmt):
    g = make()
    ex = harness.TorchExecutor(g, DEV)
    d = quantize_graph_mx(g, ex, 'MXFP4_E2M1', afmt)
    return g, ex, d


def counted_forward(ex, *args, **kwargs):
    """(results, shapes of the tensors mx_quantize was called on) of one forward."""
    seen, orig = [], mx_module.mx_quantize
    mx_module.mx_quantize = lambda *a, **k: (seen.append(tuple(a[0].shape)), orig(*a, **k))[1]
    try: out = ex.forward(*args, **kwargs)
    finally: mx_module.mx_quantize = orig
    return out, seen


@pytest.mark.parametrize('make,shape,unfused_calls,fused_calls', [
    # small_cnn: the input, c2's and fc's activation; fused: c2's arrives packed, fc's comes through pooling (out of scope)
    (lambda: harness.small_cnn_graph(seed=3), (2, 3, 8, 8), 3, 2),
    # Conv-Relu-Conv-Relu-Conv: one per layer; fused: one per graph input, none between fused layers
    (crcrc_graph, (2, 3, 6, 5), 3, 1)], ids=['small_cnn', 'crcrc'])
@pytest.mark.parametrize('afmt', ACTIVATIONS)
def test_fused_graph_has_the_logits_of_the_unfused_one(afmt, make, shape, unfused_calls, fused_calls):
    """torch.equal on the logits: F.relu on the unfused path may keep a -0 where the kernel writes +0, which torch.equal treats as
    equal -- and which neither the next layer's codes (a -0 activation times a weight adds a zero) nor an Add can tell apart
    beyond the sign of a zero."""
    g, ex, d = quantized(make, afmt)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    simulated = ex.forward(x)
    plain = deploy_graph_mx(g, ex, d, fuse=False)
    want, calls = counted_forward(ex, x)
    assert len(calls) == unfused_calls and calls[0] == shape
    names = [v.name for op in g.topological_sort() for v in op.outputs]
    want_all = ex.forward(x, names)
    hooked_want = {n: ex.forward(x, hooks={n: PlainHook()}) for n in plain.deployed}
    plain.remove()
    dep = deploy_graph_mx(g, ex, d, fuse=True)
    assert dep.deployed and all(n in dep.groups for n in dep.deployed)
    got, calls = counted_forward(ex, x)
    assert same(got, want)
    assert len(calls) == fused_calls and calls[0] == shape, calls
    assert same(ex.forward(x), got)                                                      # and again: the same bits
    # a requested intermediate and a hooked member: the values of the unfused forward, as float tensors
    for k, n in enumerate(names):
        out = ex.forward(x, [n])
        assert isinstance(out[0], torch.Tensor) and torch.equal(out[0], want_all[k]), n
    assert same(ex.forward(x, names), want_all)
    for n, ref in hooked_want.items(): assert same(ex.forward(x, hooks={n: PlainHook()}), ref), n
    for grp in dep.groups.values():
        for member in grp.members[1:]: assert same(ex.forward(x, hooks={member: PlainHook()}), want), member
    # forward_cached: a cache filled by an earlier call answers a later request for a member's own output with ITS values
    cache = {}
    assert same(ex.forward_cached(x, list(g.outputs), cache), want)
    for k, n in enumerate(names): assert torch.equal(ex.forward_cached(x, [n], cache)[0], want_all[k]), n
    dep.remove()
    assert torch.equal(bits(ex.forward(x)[0]), bits(simulated[0]))                       # the simulated bits, as before any deployment


@pytest.mark.parametrize('afmt', ACTIVATIONS)
def test_fused_groups_on_the_gpu(afmt):
    g, ex, d = quantized(crcrc_graph, afmt)
    dep = deploy_graph_mx(g, ex, d, fuse=True)
    assert [dep.groups[n].members for n in ('k0', 'k1', 'k2')] == [['k0', 'k0_relu'], ['k1', 'k1_relu'], ['k2']]
    assert [dep.groups[n].out_format for n in ('k0', 'k1', 'k2')] == [MXFormat[afmt], MXFormat[afmt], None]
    x = torch.rand(2, 3, 6, 5, generator=torch.Generator().manual_seed(2)).to(DEV)
    got = ex.forward(x)[0]
    v = lambda n: g.variables[n].value
    a = mx_conv2d(x, dep.weights['k0_w'], afmt, v('k0_b'), 1, 1, relu=True, out_format=afmt)
    b = mx_conv2d_packed(a, dep.weights['k1_w'], v('k1_b'), 1, 1, relu=True, out_format=afmt)
    assert isinstance(a, MXTensor) and isinstance(b, MXTensor)
    assert torch.equal(bits(got), bits(mx_conv2d_packed(b, dep.weights['k2_w'], v('k2_b'), 1, 1)))
    g2, ex2, d2 = quantized(lambda: harness.transformer_mlp_graph(seed=1), afmt)
    x2 = torch.randn(3, 5, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    plain = deploy_graph_mx(g2, ex2, d2)
    want = ex2.forward(x2)
    plain.remove()
    dep2 = deploy_graph_mx(g2, ex2, d2, fuse=True)
    assert dep2.groups['fc1'].members == ['fc1'] and dep2.groups['fc2'].members == ['fc2', 'residual'] and dep2.groups['fc2'].residual == 'input'
    assert same(ex2.forward(x2), want)                                                   # Gelu stays unfused; the Add rides fc2's launch


def test_fused_launches_are_booked_under_their_own_ids():
    """One fused launch each, booked as mx_gemm_fused / mx_conv_fused and not as the plain kernels."""
    x, w, bias, residual = random_gemm()
    A, B = mx_quantize(x, 'MXFP8_E4M3', -1), mx_quantize(w, 'MXFP4_E2M1', -1)
    g = C.FIRST
    xc, wc, _, rc = random_conv(g)
    X, W = mx_quantize(xc, 'MXFP4_E2M1', 1), mx_quantize(wc, 'MXFP4_E2M1', 1)

    def run():
        mx_matmul(A, B, bias, residual=residual, relu=True, out_format='MXFP4_E2M1')
        mx_conv2d_packed(X, W, None, g.stride, g.pad, g.dil, residual=rc, relu=True, out_format='MXFP8_E4M3', out_float=True)
        mx_matmul(A, B, bias)
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    try: run()
    finally:
        torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 48)()
    n = _lib.lib.ppqhip_prof_collect(arr, 48)
    seen = {arr[i].name.decode(): (arr[i].launches, arr[i].total_bytes) for i in range(n) if arr[i].launches}
    assert {k: v[0] for k, v in seen.items()} == {'mx_gemm_fused': 1, 'mx_conv_fused': 1, 'mx_gemm': 1}
    m, nn, k = FUSED_SHAPE
    nb = (k + 31) // 32
    operands = m * nb * 33 + nn * nb * 17
    assert seen['mx_gemm'][1] == operands + 4 * m * nn
    assert seen['mx_gemm_fused'][1] == operands + 4 * m * nn + m * 3 * 17             # the residual and the packed MXFP4 result; no float output
