"""The oracle of the MX GEMM tests: the contract of DESIGN.md section 9.14 in NumPy, built on ``mx_pack_reference``.

``matmul`` decodes both packed operands through the tables of ``mx_reference`` (``mx_pack_reference.unpack``), multiplies in float64
and returns the result together with S = sum_k |a_k| |b_k|, the quantity the accumulation bound is stated in.  The two generators
build packed operands for which the answer does not depend on the order or the width of the accumulation, so that the GPU tests can
compare with ``==``; each asserts its own precondition in float64.  Not a test module."""
import numpy as np

import mx_pack_reference as P
import mx_reference as R

FLOAT_FORMATS = [f for f in R.FORMATS if f != 'MXINT8']
PAIRS = [(a, b) for a in FLOAT_FORMATS for b in FLOAT_FORMATS]

# the shapes (M, N, K) of the GPU tests: tests/test_host_mx_gemm.py checks the generators' preconditions for them without a GPU
ALL_PAIRS_SHAPE = (17, 33, 160)
EDGE_PAIRS = [('MXFP4_E2M1', 'MXFP4_E2M1'), ('MXFP8_E4M3', 'MXFP4_E2M1'), ('MXFP6_E3M2', 'MXFP6_E2M3')]
# one block; one instruction; nb = 3 is no multiple of 4; a short last block; more than one 64 x 64 workgroup tile in both directions
# (three along M: 130 >= 2 * 64 + 1) with nb = 13
EDGE_SHAPES = [(1, 1, 32), (16, 16, 128), (48, 80, 96), (33, 17, 40), (130, 70, 416)]
ROUTING_SHAPE = (20, 24, 224)
ROUTING_PAIRS = [('MXFP8_E4M3', 'MXFP8_E5M2'), ('MXFP6_E2M3', 'MXFP4_E2M1'), ('MXFP4_E2M1', 'MXFP4_E2M1')]
RANDOM_SHAPE = (37, 29, 200)


def nblocks(k: int) -> int:
    return (k + P.BLOCK - 1) // P.BLOCK


def decode(packed, fmt: str, k: int) -> np.ndarray:
    """float64 [rows, k] of a packed operand (elements [rows, nb * B], scales [rows, nb])."""
    e, s = packed
    return P.unpack(e, s, fmt, (e.shape[0], k)).astype(np.float64)


def matmul(a_packed, b_packed, fmt_a: str, fmt_b: str, k: int, bias=None):
    """(C, S) in float64: C = A . B^T (+ bias), S = |A| . |B|^T.  A zero result is +0, as an accumulator that starts at +0 gives."""
    a, b = decode(a_packed, fmt_a, k), decode(b_packed, fmt_b, k)
    with np.errstate(invalid='ignore', over='ignore'):
        c = a @ b.T + 0.0
        if bias is not None: c = c + np.asarray(bias, np.float64)[None, :]
        s = np.abs(a) @ np.abs(b).T
    return c, s


def from_codes(codes: np.ndarray, scales: np.ndarray, fmt: str):
    """codes uint8 [rows, nb, 32], scales uint8 [rows, nb] -> the packed operand."""
    e = P.pack_fields(codes, P.WIDTH[fmt])
    return np.ascontiguousarray(e.reshape(e.shape[0], -1)), np.ascontiguousarray(scales.astype(np.uint8))


def small_codes(fmt: str) -> np.ndarray:
    """The codes of the format whose value v has |v| <= 4 and 8 v an integer, both signs (and so -0)."""
    t = R.table(fmt)
    index = np.flatnonzero((t <= 4.0) & (np.rint(8.0 * t) == 8.0 * t))
    return np.concatenate([index, index | (1 << (P.WIDTH[fmt] - 1))]).astype(np.uint8)


def code_of(value: float, fmt: str) -> int:
    t = R.table(fmt)
    index = int(np.searchsorted(t, abs(value)))
    assert t[index] == abs(value), (value, fmt)
    return index | (int(value < 0) << (P.WIDTH[fmt] - 1))


def _tail_mask(k: int) -> np.ndarray:
    """[nb, 32] bool: the elements of a row that exist (the export holds +0 behind them)."""
    nb = nblocks(k)
    return (np.arange(nb * P.BLOCK) < k).reshape(nb, P.BLOCK)


def exact_case(m: int, n: int, k: int, fmt_a: str, fmt_b: str, seed: int = 0):
    """(a_packed, b_packed, C float64): random small codes under scale codes 126 .. 128.  Every term a_k b_k is then a multiple of
    2^-8 of magnitude at most 2^6, so every partial sum of a row, in any order, is a multiple of 2^-8 below K 2^6 <= 2^24 2^-8:
    exactly representable in float32 (and in anything wider).  A and B come from different streams (A is never B)."""
    assert k * 64 < 2 ** 24 * 2.0 ** -8, f'K = {k}: a partial sum may need more than 24 bits'
    rng = np.random.default_rng([seed, m, n, k])
    nb, live = nblocks(k), _tail_mask(k)
    out = []
    for rows, fmt in ((m, fmt_a), (n, fmt_b)):
        pool = small_codes(fmt)
        codes = np.where(live[None], pool[rng.integers(0, len(pool), (rows, nb, P.BLOCK))], np.uint8(0))
        scales = rng.integers(126, 129, (rows, nb)).astype(np.uint8)
        out.append(from_codes(codes, scales, fmt))
    a, b = decode(out[0], fmt_a, k), decode(out[1], fmt_b, k)
    for v in (a, b): assert (np.abs(v) <= 8.0).all() and np.array_equal(np.rint(16.0 * v), 16.0 * v)        # |v| <= 4 * 2, a multiple of 2^-4
    c, s = matmul(out[0], out[1], fmt_a, fmt_b, k)
    assert s.max() < 2.0 ** 16 and np.array_equal(c.astype(np.float32).astype(np.float64), c)
    assert m == 1 or n == 1 or not np.array_equal(c[:min(m, n), :min(m, n)], c[:min(m, n), :min(m, n)].T)   # a row <-> column swap shows
    return out[0], out[1], c


def routing_scales(rows: int, nb: int, base: int, span: int) -> np.ndarray:
    return (base + np.arange(rows * nb).reshape(rows, nb) % span).astype(np.uint8)


def routing_case(m: int, n: int, k: int, fmt_a: str, fmt_b: str, kb: int):
    """(a_packed, b_packed, C float64): A is 1.0 everywhere, B is 1.0 in block ``kb`` and +0 elsewhere; the scale codes differ from
    (row, block) to (row, block): A's run over 64 .. 183, B's over 100 .. 149.  C[i][j] = count 2^(sa[i][kb] - 127) 2^(sb[j][kb] - 127)
    with count = the elements of block kb (32 unless it is a short last block): one term, exact, and a normal float32 since
    -90 <= sa + sb - 254 <= 78.  A scale taken from another lane, block or row gives another power of two."""
    nb, live = nblocks(k), _tail_mask(k)
    assert 0 <= kb < nb
    one_a, one_b = code_of(1.0, fmt_a), code_of(1.0, fmt_b)
    ca = np.where(live[None], np.uint8(one_a), np.uint8(0)) * np.ones((m, 1, 1), np.uint8)
    cb = np.zeros((n, nb, P.BLOCK), np.uint8)
    cb[:, kb] = np.where(live[kb], np.uint8(one_b), np.uint8(0))
    sa, sb = routing_scales(m, nb, 64, 120), routing_scales(n, nb, 100, 50)
    count = int(live[kb].sum())
    want = count * np.exp2(sa[:, kb].astype(np.float64) - 127)[:, None] * np.exp2(sb[:, kb].astype(np.float64) - 127)[None, :]
    assert (want >= 2.0 ** -126).all() and (want < 2.0 ** 127).all() and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    a, b = from_codes(ca, sa, fmt_a), from_codes(cb, sb, fmt_b)
    c, _ = matmul(a, b, fmt_a, fmt_b, k)
    assert np.array_equal(c, want)                                                       # the oracle agrees with the closed form
    return a, b, want


def random_inputs(seed: int = 0):
    """x [37, 200] and w [29, 200] in float32: standard normal times a per-row factor 2^U(-6, 6)."""
    m, n, k = RANDOM_SHAPE
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, k)) * np.exp2(rng.uniform(-6, 6, (m, 1)))
    w = rng.standard_normal((n, k)) * np.exp2(rng.uniform(-6, 6, (n, 1)))
    return x.astype(np.float32), w.astype(np.float32)


def bound(s: np.ndarray, k: int) -> np.ndarray:
    """K additions in any order, each off by at most one unit in the last place of a truncating float32 adder."""
    return k * 2.0 ** -23 * s
