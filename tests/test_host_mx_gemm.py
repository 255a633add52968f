"""The MX GEMM without a GPU: the oracle (tests/mx_gemm_reference.py) against an explicit loop, the preconditions of its generators
for the shapes the GPU tests use, the ``use_kernels=False`` arm of ``mx_matmul`` / ``mx_linear`` against the oracle and against the
simulation, every argument check, and the host-side refusals of the C entry point (they run before any launch)."""
import numpy as np
import pytest
import torch

import mx_gemm_reference as G
import mx_pack_reference as P
import mx_reference as R
from ppq_amd import MXFormat, MXTensor, _lib, ffi, mx_fake_quant, mx_linear, mx_matmul, mx_quantize


def tensor(packed, fmt: str, k: int) -> MXTensor:
    e, s = packed
    return MXTensor(fmt, (e.shape[0], k), 1, torch.from_numpy(e), torch.from_numpy(s))


# ------------------------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_against_an_explicit_loop():
    m, n, k = 3, 2, 40
    fa, fb = 'MXFP6_E3M2', 'MXFP4_E2M1'
    a, b, c = G.exact_case(m, n, k, fa, fb)
    va, vb = G.decode(a, fa, k), G.decode(b, fb, k)
    bias = np.array([0.5, -2.0])
    want = np.array([[sum(float(va[i, t]) * float(vb[j, t]) for t in range(k)) + bias[j] for j in range(n)] for i in range(m)])
    got, s = G.matmul(a, b, fa, fb, k, bias)
    assert np.array_equal(got, want) and np.array_equal(c + bias[None], want)
    assert np.array_equal(s, np.array([[sum(abs(va[i, t] * vb[j, t]) for t in range(k)) for j in range(n)] for i in range(m)]))
    assert a[0].shape == (m, 2 * 24) and b[0].shape == (n, 2 * 16) and a[1].shape == (m, 2)
    assert not G.decode(a, fa, 64)[:, k:].any()                                          # the short last block holds +0


def test_small_codes_are_small():
    for fmt in G.FLOAT_FORMATS:
        pool = G.small_codes(fmt)
        v = P.decode_bits(pool[None, None, :].astype(np.uint8), np.full((1, 1), 127, np.uint8), fmt).view(np.float32).astype(np.float64).ravel()
        assert (np.abs(v) <= 4).all() and np.array_equal(np.rint(8 * v), 8 * v) and len(set(pool)) == len(pool)
        assert (np.signbit(v) & (v == 0)).any() and (v == 4).any() and (v == -4).any()   # -0 and both ends are there
        assert G.code_of(1.0, fmt) in pool


def test_generators_hold_their_preconditions_for_the_gpu_shapes():
    """The generators assert them; this calls each with every shape and pair the GPU tests use."""
    for fa, fb in G.PAIRS:
        a, b, c = G.exact_case(*G.ALL_PAIRS_SHAPE, fa, fb)
        assert c.shape == G.ALL_PAIRS_SHAPE[:2] and np.abs(c).max() > 0
    for fa, fb in G.EDGE_PAIRS:
        for shape in G.EDGE_SHAPES: G.exact_case(*shape, fa, fb)
    m, n, k = G.ROUTING_SHAPE
    for fa, fb in G.ROUTING_PAIRS:
        seen = set()
        for kb in range(G.nblocks(k)):
            _, _, c = G.routing_case(m, n, k, fa, fb, kb)
            seen.add(c.tobytes())
            assert len(np.unique(c[:, 0])) == m and len(np.unique(c[0])) == n            # every row and column has its own power of two
        assert len(seen) == G.nblocks(k)
    with pytest.raises(AssertionError, match='more than 24 bits'): G.exact_case(2, 2, 1024, 'MXFP4_E2M1', 'MXFP4_E2M1')
    for fa, fb in G.GRID_PAIRS:
        for shape in G.GRID_SHAPES: G.exact_case(*shape, fa, fb)
    for fa, fb in G.EDGE_PAIRS: G.exact_case(*G.LONG_K_SHAPE, fa, fb)
    assert [((m + 63) // 64, (n + 63) // 64) for m, n, _ in G.GRID_SHAPES] == [(2, 3), (1, 7), (3, 6), (65, 1), (1, 8)]
    assert G.nblocks(G.LONG_K_SHAPE[2]) == 31 and G.nblocks(G.LONG_K_RANDOM_SHAPE[2]) == 130 and G.LONG_K_RANDOM_SHAPE[2] % 32 == 8


def torch_bits(a, b, fa, fb, k) -> np.ndarray:
    """The torch arm on CPU tensors; a -0 (one term, no accumulator behind it) is taken as +0."""
    return R.bits(mx_matmul(tensor(a, fa, k), tensor(b, fb, k), use_kernels=False).numpy() + np.float32(0))


@pytest.mark.parametrize('fa,fb', G.PAIRS)
def test_table_case_and_the_torch_arm_on_it(fa, fb):
    """Every element code of both formats, at both K and in both arrangements: the generator's preconditions hold, and
    ``mx_dequantize``'s torch arm decodes every code as the tables do."""
    for k in G.TABLE_KS:
        for one_hot in ('a', 'b'):
            a, b, want = G.table_case(fa, fb, k, one_hot)
            hot, dense = (a, b) if one_hot == 'a' else (b, a)
            assert hot[0].shape[0] >= k and dense[0].shape[0] == len(G.all_codes(fb if one_hot == 'a' else fa))
            nan = np.isnan(want)
            assert nan.any() == (fa in G.NAN_CODES or fb in G.NAN_CODES)
            for f, line in ((fa, nan.all(axis=1)), (fb, nan.all(axis=0))): assert line.sum() >= len(G.NAN_CODES.get(f, ()))
            got = torch_bits(a, b, fa, fb, k)
            assert np.array_equal(got[~nan], R.bits(want.astype(np.float32))[~nan]) and np.isnan(got.view(np.float32)[nan]).all()


def test_all_codes_and_their_values():
    assert [len(G.all_codes(f)) for f in G.FLOAT_FORMATS] == [256, 254, 64, 64, 16]
    for fmt in G.FLOAT_FORMATS:
        codes = G.all_codes(fmt)
        v = G.code_values(codes, fmt)
        ref = P.decode_bits(codes[None, :], np.full(1, 127, np.uint8), fmt).view(np.float32).astype(np.float64)[0]
        assert np.array_equal(np.isnan(v), np.isnan(ref)) and np.array_equal(v[~np.isnan(v)], ref[~np.isnan(v)])
        assert np.isnan(v).sum() == len(G.NAN_CODES.get(fmt, ())) and set(codes[np.isnan(v)]) == set(G.NAN_CODES.get(fmt, ()))
        assert np.nanmax(v) == R.table(fmt)[-1] and np.nanmin(v) == -R.table(fmt)[-1] and np.signbit(v[v == 0]).any()
    for fmt, pair in G.NAN_NEIGHBOURS.items():
        assert list(G.code_values(np.asarray(pair, np.uint8), fmt)) == [R.table(fmt)[-1], -R.table(fmt)[-1]]


def _wrong_decode(monkeypatch, mutate):
    right = P.decode_bits
    monkeypatch.setattr(P, 'decode_bits', lambda c, scales, fmt: mutate(right, c, scales, fmt))


def test_the_table_catches_a_wrong_decode(monkeypatch):
    """Three decodes that are wrong the way a kernel could be, put in place of the oracle's: the table's closed form refuses each
    (its comparison with the oracle is the comparison the GPU test makes with the kernel).  The same cases pass unmutated above."""
    def e5m2_subnormals_as_zero(right, c, scales, fmt):
        out = right(c, scales, fmt)
        return np.where((c & 0x7c) == 0, out & np.uint32(0x80000000), out) if fmt == 'MXFP8_E5M2' else out

    def fp6_ids_swapped(right, c, scales, fmt):
        return right(c, scales, {'MXFP6_E3M2': 'MXFP6_E2M3', 'MXFP6_E2M3': 'MXFP6_E3M2'}.get(fmt, fmt))

    def fp8_half_under_its_lanes_scale(right, c, scales, fmt):
        """The 16-element chunk q of a 128-element K-step scaled by block q % 4 of the step, not by its own block q // 2."""
        if P.WIDTH[fmt] != 8: return right(c, scales, fmt)
        nb = scales.shape[-1]
        chunk = np.arange(2 * nb)
        block = np.minimum(chunk // 8 * 4 + chunk % 8 % 4, nb - 1)
        return right(c.reshape(c.shape[:-2] + (2 * nb, 16)), scales[..., block], fmt).reshape(c.shape)

    cases = [(e5m2_subnormals_as_zero, ('MXFP8_E5M2', 'MXFP4_E2M1'), ('MXFP6_E2M3', 'MXFP8_E5M2')),
             (fp6_ids_swapped, ('MXFP6_E3M2', 'MXFP4_E2M1'), ('MXFP8_E4M3', 'MXFP6_E2M3')),
             (fp8_half_under_its_lanes_scale, ('MXFP8_E4M3', 'MXFP4_E2M1'), ('MXFP6_E3M2', 'MXFP8_E5M2'))]
    for mutate, *pairs in cases:
        for fa, fb in pairs:
            for k in G.TABLE_KS:
                for one_hot in ('a', 'b'):
                    G.table_case(fa, fb, k, one_hot)
                    with monkeypatch.context() as mp:
                        _wrong_decode(mp, mutate)
                        with pytest.raises(AssertionError): G.table_case(fa, fb, k, one_hot)


@pytest.mark.parametrize('fa,fb', G.SWEEP_PAIRS)
def test_scale_sweep_case_and_the_torch_arm_on_it(fa, fb):
    """Every scale code on both sides: the torch arm gives float32(2^(i + j - 254)) -- +Inf from 2^128 on, the subnormals kept, +0
    below 2^-149 -- whatever sits on the blocks of zeros."""
    e = np.arange(255)[:, None] + np.arange(255)[None, :] - 254
    for fill in ('neutral', 'same'):
        a, b, want = G.scale_sweep_case(fa, fb, G.SWEEP_K, fill)
        assert np.array_equal(want, np.exp2(e.astype(np.float64)))
        assert (a[1] == 127).sum() >= 255 * 4 if fill == 'neutral' else (a[1] == np.arange(255, dtype=np.uint8)[:, None]).all()
        with np.errstate(over='ignore'): want32 = want.astype(np.float32)
        assert np.isposinf(want32[e >= 128]).all() and (want32[e < -149] == 0).all() and (want32[e >= -149] > 0).all()
        assert np.array_equal(torch_bits(a, b, fa, fb, G.SWEEP_K), R.bits(want32))


@pytest.mark.parametrize('fa,fb,side,kind', G.NAN_POSITION_CASES)
def test_nan_position_case_and_the_torch_arm_on_it(fa, fb, side, kind):
    k = G.NAN_POSITION_K
    a, b, clean, c, nan = G.nan_position_case(fa, fb, k, side, kind)
    fmt, poisoned = (fa, a) if side == 'a' else (fb, b)
    codes = P.unpack_fields(poisoned[0].reshape(2 * k, G.nblocks(k), -1), P.WIDTH[fmt]).reshape(2 * k, -1)
    before = P.unpack_fields(clean[0].reshape(2 * k, G.nblocks(k), -1), P.WIDTH[fmt]).reshape(2 * k, -1)
    t = np.arange(k)
    if kind == 'code':
        assert set(codes[2 * t, t]) == set(G.NAN_CODES[fmt]) and np.array_equal(poisoned[1], clean[1])
        assert (codes != before).sum() <= k and set(np.argwhere(codes != before)[:, 1]) <= set(t)
    else:
        assert (poisoned[1][2 * t, t % G.nblocks(k)] == 0xff).all() and (poisoned[1] == 0xff).sum() == k and np.array_equal(codes, before)
    if fmt in G.NAN_NEIGHBOURS: assert set(codes[2 * t + 1, t]) == set(G.NAN_NEIGHBOURS[fmt])
    assert np.array_equal(nan.all(axis=1 if side == 'a' else 0), np.arange(2 * k) % 2 == 0)
    got = torch_bits(a, b, fa, fb, k)
    assert np.array_equal(np.isnan(got.view(np.float32)), nan) and np.array_equal(got[~nan], R.bits(c.astype(np.float32))[~nan])


# -------------------------------------------------------------------------------------------------------- the torch arm on the CPU
@pytest.mark.parametrize('fa,fb', [('MXFP8_E4M3', 'MXFP4_E2M1'), ('MXFP6_E3M2', 'MXFP6_E2M3'), ('MXFP4_E2M1', 'MXFP8_E5M2')])
def test_torch_arm_equals_the_oracle_and_the_simulation(fa, fb):
    xn, wn = G.random_inputs()
    x, w = torch.from_numpy(xn), torch.from_numpy(wn)
    k = x.shape[1]
    bias = torch.linspace(-1.0, 1.0, w.shape[0])
    a, b = mx_quantize(x, fa, -1, use_kernels=False), mx_quantize(w, fb, -1, use_kernels=False)
    for bi in (None, bias):
        got = mx_matmul(a, b, bi, use_kernels=False)
        assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0], w.shape[0])
        c, s = G.matmul((a.elements.numpy(), a.scales.numpy()), (b.elements.numpy(), b.scales.numpy()), fa, fb, k, None if bi is None else bi.numpy())
        assert np.abs(got.numpy().astype(np.float64) - c).max() <= 2.0 ** -24 * np.abs(c).max() * 1.0001 + 1e-12 * s.max()   # one rounding to float32
        assert np.array_equal(got.numpy(), c.astype(np.float32)) or np.abs(got.numpy() - c.astype(np.float32)).max() <= np.spacing(np.abs(c).max().astype(np.float32))
        sim = mx_fake_quant(x, fa, -1, use_kernels=False).double() @ mx_fake_quant(w, fb, -1, use_kernels=False).double().t()
        if bi is not None: sim = sim + bi.double()
        assert torch.equal(got, sim.float())
        assert torch.equal(mx_linear(x, b, fa, bi, use_kernels=False), got) and torch.equal(a.matmul(b, bi, use_kernels=False), got)
    x3 = x[:36].reshape(2, 18, k)
    y3 = mx_linear(x3, b, fa, bias, use_kernels=False)
    assert tuple(y3.shape) == (2, 18, w.shape[0]) and torch.equal(y3.reshape(36, -1), mx_linear(x[:36], b, fa, bias, use_kernels=False))


def test_torch_arm_on_an_exact_case_has_the_oracles_bits():
    m, n, k = G.ALL_PAIRS_SHAPE
    for fa, fb in G.EDGE_PAIRS:
        a, b, c = G.exact_case(m, n, k, fa, fb)
        got = mx_matmul(tensor(a, fa, k), tensor(b, fb, k), use_kernels=False).numpy()
        assert np.array_equal(R.bits(got + np.float32(0)), R.bits(c.astype(np.float32)))


def test_torch_arm_nan():
    m, n, k = G.ALL_PAIRS_SHAPE
    a, b, _ = G.exact_case(m, n, k, 'MXFP8_E4M3', 'MXFP4_E2M1')
    a[0][3, 40] = 0x7f
    b[1][9, 1] = 0xff
    got = mx_matmul(tensor(a, 'MXFP8_E4M3', k), tensor(b, 'MXFP4_E2M1', k), use_kernels=False).numpy()
    want = np.zeros((m, n), bool); want[3, :] = True; want[:, 9] = True
    assert np.array_equal(np.isnan(got), want) and np.array_equal(np.isnan(G.matmul(a, b, 'MXFP8_E4M3', 'MXFP4_E2M1', k)[0]), want)


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks():
    x, w = torch.randn(6, 70), torch.randn(5, 70)
    a, b = mx_quantize(x, 'MXFP8_E4M3', use_kernels=False), mx_quantize(w, 'MXFP4_E2M1', use_kernels=False)
    for use_kernels in (False, True):
        with pytest.raises(RuntimeError, match='MXINT8'): mx_matmul(mx_quantize(x, 'MXINT8', use_kernels=False), b, use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match='MXINT8'): mx_matmul(a, mx_quantize(w, 'MXINT8', use_kernels=False), use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match='packed along axis 0'): mx_matmul(mx_quantize(x, 'MXFP8_E4M3', 0, use_kernels=False), b, use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match='packed along axis 0'): mx_matmul(a, mx_quantize(w, 'MXFP4_E2M1', 0, use_kernels=False), use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match='K mismatch: a has 70, b has 64'): mx_matmul(a, mx_quantize(w[:, :64].contiguous(), 'MXFP4_E2M1', use_kernels=False), use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match='b must be 2-d'): mx_matmul(a, mx_quantize(w.reshape(5, 1, 70), 'MXFP4_E2M1', use_kernels=False), use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match=r'bias of shape \[6\], expected \[5\]'): mx_matmul(a, b, torch.zeros(6), use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match='bias must be a float32 tensor'): mx_matmul(a, b, torch.zeros(5, dtype=torch.float64), use_kernels=use_kernels)
        with pytest.raises(TypeError, match='MXTensor'): mx_matmul(x, b, use_kernels=use_kernels)
        with pytest.raises(TypeError, match='MXTensor'): mx_matmul(a, w, use_kernels=use_kernels)
        with pytest.raises(RuntimeError, match='Invalid dtype'): mx_linear(x.double(), b, 'MXFP8_E4M3', use_kernels=use_kernels)
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_matmul(a, b)            # the kernel arm has no CPU path
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_linear(x, b, 'MXFP8_E4M3')
    with pytest.raises(RuntimeError, match='Invalid dtype'): ffi.CUDA.MXMatmul(a.elements.float(), a.scales, 'MXFP8_E4M3', b.elements, b.scales, 'MXFP4_E2M1', 70)
    with pytest.raises(ValueError, match='unknown MX format'): ffi.CUDA.MXMatmul(a.elements, a.scales, 'MXFP8', b.elements, b.scales, 'MXFP4_E2M1', 70)
    assert mx_matmul(a, b, use_kernels=False).shape == (6, 5)


# ---------------------------------------------------------------------------------------------------------------------- the C ABI
def test_c_entry_point_checks_arguments_without_a_device():
    """Formats, sizes, null pointers, alignment and overlap are checked on the host before anything is launched."""
    lib = _lib.lib
    buf = np.zeros(4096 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15                                                     # 16-B aligned, 4096 bytes behind it
    E4M3, FP6, FP4, INT8 = (MXFormat[f].value for f in ('MXFP8_E4M3', 'MXFP6_E3M2', 'MXFP4_E2M1', 'MXINT8'))

    # m = 4, n = 2, k = 64 (nb = 2).  A (E4M3): elements 256 B at p, scales 8 B at p + 256; B (FP4): elements 64 B at p + 512,
    # scales 4 B at p + 576; bias 8 B at p + 640; c 32 B at p + 1024
    def gemm(ae=p, as_=p + 256, fa=E4M3, be=p + 512, bs=p + 576, fb=FP4, bias=p + 640, c=p + 1024, m=4, n=2, k=64):
        return lib.ppqhip_mx_gemm(ae, as_, fa, be, bs, fb, bias, c, m, n, k, None), _lib.last_error()

    assert gemm(fa=INT8) == (-1, 'mx_gemm: A: MXINT8 is not an operand type of the scaled MFMA')
    assert gemm(fb=INT8) == (-1, 'mx_gemm: B: MXINT8 is not an operand type of the scaled MFMA')
    assert gemm(fa=6) == (-1, 'mx_gemm: A: unknown MX format 6')
    assert gemm(fb=-1) == (-1, 'mx_gemm: B: unknown MX format -1')
    for size in ('m', 'n', 'k'):
        assert gemm(**{size: -1}) == (-1, 'mx_gemm: negative size')
        assert gemm(**{size: 1 << 31}) == (-1, 'mx_gemm: a size above 2^31 - 1')
    for ptr in ('ae', 'as_', 'be', 'bs', 'c'): assert gemm(**{ptr: 0}) == (-1, 'mx_gemm: null pointer')
    assert gemm(ae=p + 8) == (-1, 'mx_gemm: elements and c must be 16-byte aligned')
    assert gemm(be=p + 512 + 4) == (-1, 'mx_gemm: elements and c must be 16-byte aligned')
    assert gemm(c=p + 1024 + 4) == (-1, 'mx_gemm: elements and c must be 16-byte aligned')
    assert gemm(c=p + 240) == (-1, 'mx_gemm: an output overlaps an input')              # c's 32 B reach into A's scales
    assert gemm(c=p + 256) == (-1, 'mx_gemm: an output overlaps an input')              # ... start on them
    assert gemm(c=p + 544) == (-1, 'mx_gemm: an output overlaps an input')              # B's elements and scales
    assert gemm(c=p + 624) == (-1, 'mx_gemm: an output overlaps an input')              # the bias
    assert gemm(fa=FP6, c=p + 176) == (-1, 'mx_gemm: an output overlaps an input')      # FP6: 4 * 48 B of A's elements
    assert gemm(fa=FP4, c=p + 112) == (-1, 'mx_gemm: an output overlaps an input')      # FP4: 4 * 32 B
    assert gemm(m=1 << 30, n=1 << 30) == (-1, 'mx_gemm: too many workgroups in one launch')
    assert gemm(m=0)[0] == 0 and gemm(n=0)[0] == 0                                       # nothing to launch
    assert gemm(m=0, ae=0, c=0)[0] == 0
