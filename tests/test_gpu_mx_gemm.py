"""The MX GEMM on the GPU: the HIP kernel on the block-scaled MFMA (ppq_amd/csrc/mx_gemm.hip) against the oracle
(tests/mx_gemm_reference.py).  The layout tests use data whose every partial sum is exactly representable and compare with ``==`` on
bits: a wrong nibble order, FP6 bit order, lane map or scale byte fails them outright.  The product table, the scale sweep and the
NaN positions give outputs of one non-zero term each and so reach every element code, every scale code and every byte of a fragment
with ``==``.  Random data through the real exporter is held to the derived accumulation bound K 2^-23 sum |a_k| |b_k| (DESIGN.md
section 9.14)."""
import functools

import numpy as np
import pytest
import torch

import mx_gemm_reference as G
import mx_reference as R
from ppq_amd import CUDA, MXFormat, MXTensor, _lib, mx_fake_quant, mx_linear, mx_matmul, mx_quantize

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 0xA5


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def tensor(packed, fmt: str, k: int) -> MXTensor:
    e, s = packed
    return MXTensor(fmt, (e.shape[0], k), 1, dev(e), dev(s))


def hip_matmul(a, b, fmt_a: str, fmt_b: str, k: int, bias=None) -> np.ndarray:
    y = mx_matmul(tensor(a, fmt_a, k), tensor(b, fmt_b, k), None if bias is None else dev(bias))
    assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (a[0].shape[0], b[0].shape[0])
    return y.cpu().numpy()


def assert_bits(got: np.ndarray, want64: np.ndarray, what):
    want = want64.astype(np.float32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
    assert bad.size == 0, f'{what}: {bad.size} of {got.size} outputs differ, first at {bad[:4]}: {got.ravel()[bad[:4]]} != {want.ravel()[bad[:4]]}'


@functools.lru_cache(maxsize=None)
def exact(m, n, k, fa, fb):
    return G.exact_case(m, n, k, fa, fb)


# --------------------------------------------------------------------------------------------------------------- layout: == on bits
@pytest.mark.parametrize('fa,fb', G.PAIRS)
def test_exact_all_pairs(fa, fb):
    m, n, k = G.ALL_PAIRS_SHAPE
    a, b, c = exact(m, n, k, fa, fb)
    assert_bits(hip_matmul(a, b, fa, fb, k), c, f'{fa} x {fb} {m, n, k}')


@pytest.mark.parametrize('fa,fb', G.EDGE_PAIRS)
@pytest.mark.parametrize('shape', G.EDGE_SHAPES)
def test_exact_edges(shape, fa, fb):
    m, n, k = shape
    a, b, c = exact(m, n, k, fa, fb)
    assert_bits(hip_matmul(a, b, fa, fb, k), c, f'{fa} x {fb} {shape}')


@pytest.mark.parametrize('fa,fb', G.ROUTING_PAIRS)
def test_scale_routing(fa, fb):
    m, n, k = G.ROUTING_SHAPE
    for kb in range(G.nblocks(k)):
        a, b, c = G.routing_case(m, n, k, fa, fb, kb)
        assert_bits(hip_matmul(a, b, fa, fb, k), c, f'{fa} x {fb} block {kb}')


@pytest.mark.parametrize('fa,fb', G.PAIRS)
def test_product_table(fa, fb):
    """Every element code of A against every element code of B (subnormals, the largest codes, -0, the FP8 NaN codes), each product
    alone in its output under its own pair of scale codes, at every k of a full K-step and of both kinds of tail."""
    for k in G.TABLE_KS:
        for one_hot in ('a', 'b'):
            a, b, want = G.table_case(fa, fb, k, one_hot)
            nan = np.isnan(want)
            got = hip_matmul(a, b, fa, fb, k)
            what = f'{fa} x {fb}, K = {k}, one-hot {one_hot}'
            assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:4])
            assert_bits(np.where(nan, np.float32(0), got), np.where(nan, 0.0, want), what)


@functools.lru_cache(maxsize=None)
def sweep_on_device(fa, fb, fill):
    a, b, want = G.scale_sweep_case(fa, fb, G.SWEEP_K, fill)
    return hip_matmul(a, b, fa, fb, G.SWEEP_K), want


@pytest.mark.parametrize('fa,fb', G.SWEEP_PAIRS)
def test_scale_sweep(fa, fb):
    """Scale codes 0 .. 254 on both sides, C[i][j] = 2^(i + j - 254).  A normal float32 result is exact, from 2^128 on it is +Inf, and
    the blocks of zeros change nothing whatever their scale code.  Below 2^-126 the contract asks for float32(2^e): the subnormal
    down to 2^-149, +0 below.  What the instruction does there was not known when this was written, so the test first asks that a
    subnormal result be the contract's value or +0, by one rule for all of them, and prints the rule.  Found on the MI355X: all
    2691 subnormal results are kept, in all three pairs; the last assertion pins that."""
    got, want = sweep_on_device(fa, fb, 'neutral')
    same, _ = sweep_on_device(fa, fb, 'same')
    assert np.array_equal(R.bits(got), R.bits(same)), f'{(R.bits(got) != R.bits(same)).sum()} outputs depend on the scale code of a block of zeros'
    e = np.arange(255)[:, None] + np.arange(255)[None, :] - 254
    with np.errstate(over='ignore'): want32 = want.astype(np.float32)
    normal, sub = (e >= -126) & (e <= 127), (e >= -149) & (e < -126)
    bits, wbits = R.bits(got), R.bits(want32)
    bad = np.argwhere(normal & (bits != wbits))
    assert bad.size == 0, f'{len(bad)} in-range outputs differ, first (i, j) {bad[:4].tolist()}: {[got[i, j] for i, j in bad[:4]]}'
    assert (bits[e >= 128] == 0x7f800000).all(), np.unique(bits[e >= 128])[:8]
    assert (bits[e < -149] == 0).all(), np.unique(bits[e < -149])[:8]
    kept, flushed = bits[sub] == wbits[sub], bits[sub] == 0
    print(f'{fa} x {fb}: of {sub.sum()} subnormal results {kept.sum()} are kept, {flushed.sum()} are +0')
    assert (kept | flushed).all(), np.unique(bits[sub][~(kept | flushed)])[:8]
    assert kept.all() or flushed.all(), f'{kept.sum()} subnormal results kept, {flushed.sum()} flushed'
    print(f'{fa} x {fb}: subnormal results are ' + ('kept' if kept.all() else 'flushed to +0'))
    assert kept.all(), 'subnormal results are flushed to +0: the contract (DESIGN.md section 9.14) says they are kept'


@pytest.mark.parametrize('fa,fb,side,kind', G.NAN_POSITION_CASES)
def test_nan_positions(fa, fb, side, kind):
    """A NaN code at every element position of a row (every byte of every fragment of a K-step and of the tail), a scale code 0xFF
    on every block: exactly the poisoned rows (columns) are NaN, their neighbours -- which carry the largest finite codes on an FP8
    side -- keep the bits of the run without the poison."""
    k = G.NAN_POSITION_K
    a, b, clean, c, nan = G.nan_position_case(fa, fb, k, side, kind)
    before = hip_matmul(clean, b, fa, fb, k) if side == 'a' else hip_matmul(a, clean, fa, fb, k)
    assert_bits(before, c, 'the run without the poison')
    got = hip_matmul(a, b, fa, fb, k)
    assert np.array_equal(np.isnan(got), nan), np.argwhere(np.isnan(got) != nan)[:4]
    assert (R.bits(got)[nan] == 0x7fc00000).all()
    assert np.array_equal(R.bits(got)[~nan], R.bits(before)[~nan])


@pytest.mark.parametrize('fa,fb', G.GRID_PAIRS)
@pytest.mark.parametrize('shape', G.GRID_SHAPES)
def test_grid_decomposition(shape, fa, fb):
    """3, 7, 6, 1 and 8 workgroups along N (2, 1, 3, 65, 1 along M): divisors of the block index that are no powers of two."""
    m, n, k = shape
    a, b, c = exact(m, n, k, fa, fb)
    assert_bits(hip_matmul(a, b, fa, fb, k), c, f'{fa} x {fb} {shape}')


@pytest.mark.parametrize('fa,fb', G.EDGE_PAIRS)
def test_long_k(fa, fb):
    m, n, k = G.LONG_K_SHAPE
    a, b, c = exact(m, n, k, fa, fb)
    assert_bits(hip_matmul(a, b, fa, fb, k), c, f'{fa} x {fb} {m, n, k}')


# ------------------------------------------------------------------------------------------------- random data through the exporter
@functools.lru_cache(maxsize=None)
def random_on_device():
    x, w = G.random_inputs()
    return dev(x), dev(w)


@pytest.mark.parametrize('fa,fb', G.LONG_K_RANDOM_PAIRS)
def test_long_k_random_within_the_bound(fa, fb):
    """K = 4136 (130 blocks: 32 K-steps and a two-block tail) through the exporter, against the oracle on the exported bytes."""
    m, n, k = G.LONG_K_RANDOM_SHAPE
    x, w = (dev(v) for v in G.random_inputs(1, G.LONG_K_RANDOM_SHAPE))
    a, b = mx_quantize(x, fa, -1), mx_quantize(w, fb, -1)
    got = mx_matmul(a, b).cpu().numpy().astype(np.float64)
    c, s = G.matmul((a.elements.cpu().numpy(), a.scales.cpu().numpy()), (b.elements.cpu().numpy(), b.scales.cpu().numpy()), fa, fb, k)
    err = np.abs(got - c)
    print(f'{fa} x {fb}, K = {k}: max |err| / S = {(err / np.maximum(s, 1e-300)).max():.3e} (bound {k * 2.0 ** -23:.3e})')
    assert got.shape == (m, n) and np.isfinite(got).all() and (err <= G.bound(s, k)).all(), (fa, fb, float((err / np.maximum(s, 1e-300)).max()))


@pytest.mark.parametrize('fa,fb', G.PAIRS)
def test_random_within_the_bound(fa, fb):
    """|C - C_float64| <= K 2^-23 S for every output, against the oracle on the exported bytes and against the simulation:
    mx_fake_quant of both operands multiplied in float64 -- the simulation predicts the hardware."""
    x, w = random_on_device()
    k = x.shape[1]
    a, b = mx_quantize(x, fa, -1), mx_quantize(w, fb, -1)
    got = mx_matmul(a, b).cpu().numpy().astype(np.float64)
    c, s = G.matmul((a.elements.cpu().numpy(), a.scales.cpu().numpy()), (b.elements.cpu().numpy(), b.scales.cpu().numpy()), fa, fb, k)
    err = np.abs(got - c)
    print(f'{fa} x {fb}: max |err| / S = {(err / np.maximum(s, 1e-300)).max():.3e} (bound {k * 2.0 ** -23:.3e})')
    assert np.isfinite(got).all() and (err <= G.bound(s, k)).all(), (fa, fb, float((err / np.maximum(s, 1e-300)).max()))
    sim = mx_fake_quant(x, fa, -1).cpu().numpy().astype(np.float64) @ mx_fake_quant(w, fb, -1).cpu().numpy().astype(np.float64).T
    assert (np.abs(got - sim) <= G.bound(s, k)).all(), (fa, fb)


# ----------------------------------------------------------------------------------------------------------------------- non-finite
def _nan_case(fa, fb, poison):
    m, n, k = G.ALL_PAIRS_SHAPE
    a, b, c = exact(m, n, k, fa, fb)
    clean = hip_matmul(a, b, fa, fb, k)
    assert_bits(clean, c, 'clean')
    a, b = (a[0].copy(), a[1].copy()), (b[0].copy(), b[1].copy())
    want_nan = np.zeros((m, n), bool)
    poison(a, b, want_nan)
    got = hip_matmul(a, b, fa, fb, k)
    ref, _ = G.matmul(a, b, fa, fb, k)
    assert np.array_equal(np.isnan(ref), want_nan)                                       # the oracle agrees on where
    assert np.array_equal(np.isnan(got), want_nan), np.argwhere(np.isnan(got) != want_nan)[:4]
    assert np.array_equal(R.bits(got)[~want_nan], R.bits(clean)[~want_nan])


def test_nan_scale_in_a():
    def poison(a, b, nan): a[1][5, 3] = 0xff; nan[5, :] = True
    _nan_case('MXFP4_E2M1', 'MXFP6_E3M2', poison)


def test_nan_scale_in_b():
    def poison(a, b, nan): b[1][20, 4] = 0xff; nan[:, 20] = True                         # block 4 of 5: fed by the tail step
    _nan_case('MXFP6_E2M3', 'MXFP4_E2M1', poison)


def test_fp8_nan_codes():
    def poison(a, b, nan):
        a[0][16, 2 * 32 + 7] = 0xff; nan[16, :] = True                                  # E4M3 S.1111.111, sign set
        b[0][0, 4 * 32 + 31] = 0x7e; nan[:, 0] = True                                   # E5M2 S.11111.10
    _nan_case('MXFP8_E4M3', 'MXFP8_E5M2', poison)


def test_nan_row_with_bias():
    """A flagged output is the quiet NaN 0x7fc00000 with a finite bias as well: the bias is not added to it."""
    m, n, k = G.ALL_PAIRS_SHAPE
    fa, fb = 'MXFP8_E4M3', 'MXFP6_E2M3'
    a, b, c = exact(m, n, k, fa, fb)
    a, b = (a[0].copy(), a[1].copy()), (b[0].copy(), b[1].copy())
    a[0][2, 100] = 0xff                                                                  # a NaN code in row 2 of A
    b[1][7, 0] = 0xff                                                                    # a NaN scale in column 7 of B
    nan = np.zeros((m, n), bool); nan[2, :] = True; nan[:, 7] = True
    bias = np.linspace(-3.0, 5.0, n).astype(np.float32)
    got = hip_matmul(a, b, fa, fb, k, bias)
    assert (R.bits(got)[nan] == 0x7fc00000).all()
    assert np.array_equal(R.bits(got)[~nan], R.bits(c.astype(np.float32) + bias[None, :])[~nan])     # one float32 add per output


# ------------------------------------------------------------------------------------------------------------------- the Python API
def test_misaligned_contiguous_view():
    """A row slice of a 6-bit operand with an odd nb that starts at an odd row is contiguous and 8 mod 16: a valid operand, which
    the binding copies (the C entry point refuses such a pointer)."""
    m, n, k = G.ALL_PAIRS_SHAPE                                                          # nb = 5: a row of FP6 elements is 120 bytes
    for fa, fb, side in (('MXFP6_E3M2', 'MXFP4_E2M1', 'a'), ('MXFP8_E4M3', 'MXFP6_E2M3', 'b')):
        a, b, c = exact(m + 1, n + 1, k, fa, fb)
        A, B = tensor(a, fa, k), tensor(b, fb, k)
        ops = {'a': (A.elements, A.scales), 'b': (B.elements, B.scales)}
        ops[side] = tuple(t[1:] for t in ops[side])
        assert ops[side][0].is_contiguous() and ops[side][0].data_ptr() % 16 == 8
        got = CUDA.MXMatmul(*ops['a'], fa, *ops['b'], fb, k)
        want = CUDA.MXMatmul(*(t.clone() for t in ops['a']), fa, *(t.clone() for t in ops['b']), fb, k)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert_bits(got.cpu().numpy(), c[1:] if side == 'a' else c[:, 1:], f'{fa} x {fb}, a slice of {side}')


def test_linear_bias_and_lead_shape():
    x, w = random_on_device()
    bias = torch.linspace(-3.0, 5.0, w.shape[0], device=DEV)
    W = mx_quantize(w, 'MXFP4_E2M1', -1)
    for fmt in ('MXFP8_E4M3', 'MXFP6_E2M3'):
        q = mx_quantize(x, fmt, -1)
        y = mx_linear(x, W, fmt, bias)
        assert torch.equal(y.view(torch.int32), (mx_matmul(q, W) + bias).view(torch.int32))
        assert torch.equal(y.view(torch.int32), CUDA.MXMatmul(q.elements, q.scales, q.format, W.elements, W.scales, W.format, x.shape[1], bias=bias).view(torch.int32))
        assert torch.equal(y.view(torch.int32), q.matmul(W, bias).view(torch.int32))
    x3 = x[:36].reshape(4, 9, x.shape[1])
    y3 = mx_linear(x3, W, 'MXFP8_E4M3', bias)
    assert tuple(y3.shape) == (4, 9, w.shape[0])
    assert torch.equal(y3.reshape(36, -1).view(torch.int32), mx_linear(x[:36], W, 'MXFP8_E4M3', bias).view(torch.int32))
    ref = mx_linear(x3.cpu(), W.to('cpu'), 'MXFP8_E4M3', bias.cpu(), use_kernels=False)  # the torch arm: close, not identical
    assert tuple(ref.shape) == tuple(y3.shape) and torch.allclose(y3.cpu(), ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))


def test_two_calls_give_the_same_bits():
    m, n, k = 130, 70, 416
    a, b, _ = exact(m, n, k, 'MXFP8_E4M3', 'MXFP4_E2M1')
    x, w = random_on_device()
    A, B = mx_quantize(x, 'MXFP6_E3M2', -1), mx_quantize(w, 'MXFP8_E5M2', -1)
    assert torch.equal(mx_matmul(A, B).view(torch.int32), mx_matmul(A, B).view(torch.int32))
    assert np.array_equal(R.bits(hip_matmul(a, b, 'MXFP8_E4M3', 'MXFP4_E2M1', k)), R.bits(hip_matmul(a, b, 'MXFP8_E4M3', 'MXFP4_E2M1', k)))


def _raw(a, b, fa, fb, bias, c_ptr, m, n, k, a_off=0):
    lib = _lib.lib
    st = lib.ppqhip_mx_gemm(a.elements.data_ptr() + a_off, a.scales.data_ptr(), MXFormat[fa].value, b.elements.data_ptr(), b.scales.data_ptr(),
                            MXFormat[fb].value, bias, c_ptr, m, n, k, None)
    return st, _lib.last_error()


def test_output_outside_the_matrix_is_untouched():
    m, n, k = G.ALL_PAIRS_SHAPE
    fa, fb = 'MXFP6_E3M2', 'MXFP8_E4M3'
    a, b, c = exact(m, n, k, fa, fb)
    A, B = tensor(a, fa, k), tensor(b, fb, k)
    pad = 8                                                                              # floats: the view stays 16-B aligned
    buf = torch.full((4 * (2 * pad + m * n),), SENTINEL, dtype=torch.uint8, device=DEV).view(torch.float32)
    out = buf[pad:pad + m * n]
    assert _raw(A, B, fa, fb, None, out.data_ptr(), m, n, k)[0] == 0
    torch.cuda.synchronize()
    assert_bits(out.cpu().numpy().reshape(m, n), c, 'the view')
    raw = buf.view(torch.uint8).cpu().numpy()
    assert (raw[:4 * pad] == SENTINEL).all() and (raw[4 * (pad + m * n):] == SENTINEL).all()


def test_k_zero_and_empty():
    """K = 0: every output is +0, or the bias's bits; M = 0 or N = 0: nothing is written.  Through the C entry point: the Python
    API refuses k = 0."""
    lib = _lib.lib
    m, n = 70, 67
    E4M3, FP4 = MXFormat['MXFP8_E4M3'].value, MXFormat['MXFP4_E2M1'].value
    buf = torch.full((4 * m * n,), SENTINEL, dtype=torch.uint8, device=DEV).view(torch.float32)
    bias = torch.linspace(-2.0, 2.0, n, device=DEV)
    assert lib.ppqhip_mx_gemm(None, None, E4M3, None, None, FP4, None, buf.data_ptr(), m, n, 0, None) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert (buf.view(torch.int32) == 0).all()
    assert lib.ppqhip_mx_gemm(None, None, FP4, None, None, E4M3, bias.data_ptr(), buf.data_ptr(), m, n, 0, None) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32).reshape(m, n), bias.view(torch.int32).expand(m, n))
    a, b, _ = exact(*G.ALL_PAIRS_SHAPE, 'MXFP8_E4M3', 'MXFP4_E2M1')
    A, B = tensor(a, 'MXFP8_E4M3', G.ALL_PAIRS_SHAPE[2]), tensor(b, 'MXFP4_E2M1', G.ALL_PAIRS_SHAPE[2])
    buf = torch.full((4 * m * n,), SENTINEL, dtype=torch.uint8, device=DEV)
    for mm, nn in ((0, n), (m, 0), (0, 0)):
        assert _raw(A, B, 'MXFP8_E4M3', 'MXFP4_E2M1', bias.data_ptr(), buf.data_ptr(), mm, nn, G.ALL_PAIRS_SHAPE[2])[0] == 0
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


def test_refusals():
    m, n, k = G.ALL_PAIRS_SHAPE
    fa, fb = 'MXFP8_E4M3', 'MXFP4_E2M1'
    a, b, _ = exact(m, n, k, fa, fb)
    A, B = tensor(a, fa, k), tensor(b, fb, k)
    out = torch.empty(m, n, device=DEV)
    x, _ = random_on_device()
    with pytest.raises(RuntimeError, match='MXINT8'): mx_matmul(mx_quantize(x, 'MXINT8', -1), mx_quantize(x, 'MXFP4_E2M1', -1))
    i8 = mx_quantize(x, 'MXINT8', -1)
    with pytest.raises(RuntimeError, match='MXINT8 is not an operand type'):
        CUDA.MXMatmul(i8.elements, i8.scales, 'MXINT8', i8.elements, i8.scales, 'MXINT8', x.shape[1])
    assert _raw(A, B, fa, fb, None, out.data_ptr(), m, n, k, a_off=4) == (-1, 'mx_gemm: elements and c must be 16-byte aligned')
    assert _raw(A, B, fa, fb, None, out.data_ptr() + 4, m, n, k) == (-1, 'mx_gemm: elements and c must be 16-byte aligned')
    assert _raw(A, B, fa, fb, None, B.elements.data_ptr(), m, n, k) == (-1, 'mx_gemm: an output overlaps an input')
    assert _raw(A, B, fa, fb, out.data_ptr(), out.data_ptr(), m, n, k) == (-1, 'mx_gemm: an output overlaps an input')     # the bias
    assert _raw(A, B, fa, fb, None, out.data_ptr(), m, n, k)[0] == 0
    with pytest.raises(RuntimeError, match='expected'): CUDA.MXMatmul(A.elements, A.scales, fa, B.elements, B.scales, fb, k + 32)
