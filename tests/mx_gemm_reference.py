"""The oracle of the MX GEMM tests: the contract of DESIGN.md section 9.14 in NumPy, built on ``mx_pack_reference``.

``matmul`` decodes both packed operands through the tables of ``mx_reference`` (``mx_pack_reference.unpack``), multiplies in float64
and returns the result together with S = sum_k |a_k| |b_k|, the quantity the accumulation bound is stated in.  The two generators
build packed operands for which the answer does not depend on the order or the width of the accumulation, so that the GPU tests can
compare with ``==``; each asserts its own precondition in float64.  ``exact_case`` and ``routing_case`` cover the layout with small
codes; ``table_case`` (every element code of both formats), ``scale_sweep_case`` (every scale code) and ``nan_position_case`` (every
position of a NaN code or scale) give outputs of at most one non-zero term.  Not a test module."""
import math

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
# nb = 5: one full K-step plus a one-block tail; nb = 7: a three-block tail whose last block has 8 live elements
TABLE_KS = (160, 200)
SWEEP_PAIRS, SWEEP_K = ROUTING_PAIRS, 160
# (fmt_a, fmt_b, side, kind) of nan_position_case
NAN_POSITION_CASES = [('MXFP8_E4M3', 'MXFP4_E2M1', 'a', 'code'), ('MXFP4_E2M1', 'MXFP8_E5M2', 'b', 'code'),
                      ('MXFP4_E2M1', 'MXFP6_E2M3', 'a', 'scale'), ('MXFP6_E2M3', 'MXFP6_E3M2', 'b', 'scale')]
NAN_POSITION_K = 160
# workgroups along N = 3, 7, 6, 1, 8 and along M = 2, 1, 3, 65, 1
GRID_SHAPES = [(65, 129, 32), (3, 385, 32), (129, 321, 64), (4100, 3, 32), (1, 449, 32)]
GRID_PAIRS = [('MXFP8_E4M3', 'MXFP4_E2M1'), ('MXFP6_E3M2', 'MXFP6_E2M3')]
LONG_K_SHAPE = (20, 18, 992)                          # nb = 31: seven full K-steps plus a three-block tail
LONG_K_RANDOM_SHAPE = (18, 20, 4136)                  # nb = 130: 32 full K-steps, a two-block tail, 8 live elements in the last block
LONG_K_RANDOM_PAIRS = [('MXFP8_E4M3', 'MXFP8_E4M3'), ('MXFP4_E2M1', 'MXFP6_E3M2')]
NAN_CODES = {'MXFP8_E4M3': (0x7f, 0xff), 'MXFP8_E5M2': (0x7d, 0x7e, 0x7f, 0xfd, 0xfe, 0xff)}
# the largest finite codes, one step below the NaN (E4M3) resp. Inf (E5M2) codes, both signs: they must not be flagged
NAN_NEIGHBOURS = {'MXFP8_E4M3': (0x7e, 0xfe), 'MXFP8_E5M2': (0x7b, 0xfb)}


STEP_BLOCKS = 4                                       # MX blocks of one row per instruction


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
    exactly representable in float32 (and in anything wider).  The terms lie within 14 bits of each other, which matters on the
    instruction: with an FP8 operand it sums unequal terms more coarsely than float32 (see ``nan_position_case``).  A and B come from
    different streams (A is never B)."""
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


def all_codes(fmt: str) -> np.ndarray:
    """Every code of the format in code order: both signs, -0 and the FP8 NaN codes; the two E5M2 Inf codes are outside the contract."""
    c = np.arange(1 << P.WIDTH[fmt]).astype(np.uint8)
    return c[(c & 0x7f) != 0x7c] if fmt == 'MXFP8_E5M2' else c


def code_values(codes: np.ndarray, fmt: str) -> np.ndarray:
    """float64 value of each code straight from ``mx_reference.table``; NaN for the codes the table leaves out."""
    t = R.table(fmt)
    w = P.WIDTH[fmt]
    mag = codes.astype(np.int64) & ((1 << (w - 1)) - 1)
    v = np.where(mag < len(t), t[np.minimum(mag, len(t) - 1)], np.nan)
    return np.where((codes.astype(np.int64) >> (w - 1)) == 1, -v, v)


def _is_float32_normal_or_zero(v: np.ndarray) -> bool:
    with np.errstate(over='ignore'):
        same = np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return bool(same and ((v == 0) | (np.abs(v) >= 2.0 ** -126)).all())


def table_case(fmt_a: str, fmt_b: str, k: int, one_hot: str = 'a'):
    """(a_packed, b_packed, C float64 with NaN): the multiplication table of two formats.  ``one_hot='a'``: row i of A holds code
    ``all_codes(fmt_a)[i % ncodes]`` at the one position p(i) and +0 elsewhere, column j of B holds ``all_codes(fmt_b)[j]`` in every
    live element; ``'b'`` is the mirror image.  p runs over 0 .. K - 1 with a stride coprime to K, so every k carries a code.  Scale
    codes differ from (row, block) to (row, block) within 107 .. 147.  The one non-zero term of C[i][j] is
    value_a value_b 2^(sa[i][blk] - 127) 2^(sb[j][blk] - 127) with blk = p // 32: at most 8 significant bits, a normal float32.  A
    NaN code makes its row (column) NaN.  A zero is +0: -0 meets the +0 the accumulator starts from."""
    assert one_hot in ('a', 'b')
    nb, live = nblocks(k), _tail_mask(k)
    hot = 0 if one_hot == 'a' else 1
    fmts = (fmt_a, fmt_b)
    pool_hot, pool_dense = all_codes(fmts[hot]), all_codes(fmts[1 - hot])
    rows = max(len(pool_hot), k)
    stride = next(s for s in range(7, k + 8, 2) if math.gcd(s, k) == 1)
    index = np.arange(rows)
    pos = (stride * index + 3) % k
    code_hot = pool_hot[index % len(pool_hot)]
    assert set(pos) == set(range(k)) and set(code_hot) == set(pool_hot)                  # every k is used and every code appears
    c_hot = np.zeros((rows, nb * P.BLOCK), np.uint8)
    c_hot[index, pos] = code_hot
    c_dense = np.where(live[None], pool_dense[:, None, None], np.uint8(0))
    s_hot = routing_scales(rows, nb, 107, 41)
    s_dense = (107 + (11 * np.arange(len(pool_dense) * nb).reshape(len(pool_dense), nb) + 5) % 41).astype(np.uint8)
    blk = pos // P.BLOCK
    v_hot = code_values(code_hot, fmts[hot]) * np.exp2(s_hot[index, blk].astype(np.float64) - 127)
    v_dense = code_values(pool_dense, fmts[1 - hot])[None, :] * np.exp2(s_dense[:, blk].T.astype(np.float64) - 127)    # [rows, dense]
    want = v_hot[:, None] * v_dense + 0.0
    nan_hot, nan_dense = np.isnan(code_values(code_hot, fmts[hot])), np.isnan(code_values(pool_dense, fmts[1 - hot]))
    want_nan = nan_hot[:, None] | nan_dense[None, :]
    packed = [from_codes(c_hot.reshape(rows, nb, P.BLOCK), s_hot, fmts[hot]), from_codes(c_dense, s_dense, fmts[1 - hot])]
    if hot == 1: packed, want, want_nan = packed[::-1], want.T, want_nan.T
    a, b = decode(packed[0], fmt_a, k), decode(packed[1], fmt_b, k)
    assert ((a != 0).astype(np.int64) @ (b != 0).astype(np.int64).T <= 1).all()          # at most one non-zero term (NaN != 0)
    c, _ = matmul(packed[0], packed[1], fmt_a, fmt_b, k)
    assert np.array_equal(np.isnan(want), want_nan) and np.array_equal(np.isnan(c), want_nan) and not np.isinf(want).any()
    assert np.array_equal(c[~want_nan], want[~want_nan])                                 # the oracle agrees with the closed form
    assert _is_float32_normal_or_zero(want[~want_nan]) and (want < 0).any() and (want > 0).any()
    assert not np.signbit(want[want == 0]).any()
    return packed[0], packed[1], want


def scale_sweep_case(fmt_a: str, fmt_b: str, k: int, fill: str):
    """(a_packed, b_packed, C float64), M = N = 255: row i of A holds one 1.0, in block i % nb, under scale code i; B is 1.0 in every
    live element under scale code j in every block of column j: C[i][j] = 2^(i + j - 254), every scale code 0 .. 254 on both sides
    and results from 2^-254 to 2^254.  The other blocks of A's row (all zeros) carry code 127 (``fill='neutral'``) or code i as well
    (``'same'``): zero elements under extreme scales must stay zero."""
    assert fill in ('neutral', 'same')
    nb, live = nblocks(k), _tail_mask(k)
    assert nb > STEP_BLOCKS and nb % STEP_BLOCKS                                         # all four K-groups of a full step and a tail step
    m = n = 255
    i = np.arange(m)
    blk = i % nb
    pos = P.BLOCK * blk + (3 * i) % live.sum(axis=1)[blk]
    assert set(blk) == set(range(nb)) and live.reshape(-1)[pos].all()
    ca = np.zeros((m, nb * P.BLOCK), np.uint8)
    ca[i, pos] = code_of(1.0, fmt_a)
    sa = np.full((m, nb), 127, np.uint8) if fill == 'neutral' else np.repeat(i[:, None], nb, axis=1).astype(np.uint8)
    sa[i, blk] = i
    cb = np.where(live[None], np.uint8(code_of(1.0, fmt_b)), np.uint8(0)) * np.ones((n, 1, 1), np.uint8)
    sb = np.repeat(np.arange(n)[:, None], nb, axis=1).astype(np.uint8)
    want = np.exp2(i[:, None] + np.arange(n)[None, :] - 254.0)
    a, b = from_codes(ca.reshape(m, nb, P.BLOCK), sa, fmt_a), from_codes(cb, sb, fmt_b)
    c, _ = matmul(a, b, fmt_a, fmt_b, k)
    assert np.array_equal(c, want) and want.min() == 2.0 ** -254 and want.max() == 2.0 ** 254
    return a, b, want


def nan_position_case(fmt_a: str, fmt_b: str, k: int, side: str, kind: str):
    """(a_packed, b_packed, clean_packed, C float64, nan bool [M, N]) with 2 K rows (columns) on ``side`` and 20 on the other.  Even
    row 2 t is poisoned: ``kind='code'`` (FP8 only) puts a NaN code, cycling through all of the format's, at element t -- every byte
    of every fragment once; ``kind='scale'`` puts scale code 0xFF on block t % nb.  ``clean_packed`` is ``side``'s operand before the
    poison, C the exact result of the clean pair.  Odd rows are clean in both.  On an FP8 side odd row 2 t + 1 holds the largest
    finite code (sign alternating), one step from the NaN / Inf codes, at element t and +0 elsewhere: its outputs have one term and
    are exact whatever the adder does.  (Among the small terms of ``exact_case`` such a term is NOT summed exactly although every
    partial sum is a float32: the instruction aligns the products of an FP8 operand more coarsely -- 425.5 came out for 425.53125,
    E4M3 x E2M1 at K = 160.)  Everything else is drawn as in ``exact_case``."""
    assert side in ('a', 'b') and kind in ('code', 'scale')
    fmt = fmt_a if side == 'a' else fmt_b
    assert kind == 'scale' or fmt in NAN_CODES
    rng = np.random.default_rng([k, side == 'b', kind == 'scale'])
    nb, live = nblocks(k), _tail_mask(k)
    rows = {'a': 20, 'b': 20, side: 2 * k}
    out = {}
    for which, f in (('a', fmt_a), ('b', fmt_b)):
        pool = small_codes(f)
        codes = np.where(live[None], pool[rng.integers(0, len(pool), (rows[which], nb, P.BLOCK))], np.uint8(0))
        out[which] = [codes, rng.integers(126, 129, (rows[which], nb)).astype(np.uint8)]
    codes, scales = out[side]
    codes = codes.reshape(2 * k, nb * P.BLOCK)
    t = np.arange(k)
    if fmt in NAN_NEIGHBOURS:
        codes[1::2] = 0
        codes[2 * t + 1, t] = np.asarray(NAN_NEIGHBOURS[fmt], np.uint8)[t % 2]
    clean = from_codes(codes.reshape(2 * k, nb, P.BLOCK), scales, fmt)
    codes, scales = codes.copy(), scales.copy()
    if kind == 'code': codes[2 * t, t] = np.asarray(NAN_CODES[fmt], np.uint8)[t % len(NAN_CODES[fmt])]
    else: scales[2 * t, t % nb] = 0xff
    poisoned = from_codes(codes.reshape(2 * k, nb, P.BLOCK), scales, fmt)
    other = from_codes(*out['b' if side == 'a' else 'a'], fmt_b if side == 'a' else fmt_a)
    pair = lambda x: (x, other) if side == 'a' else (other, x)
    va, vb = decode(pair(clean)[0], fmt_a, k), decode(pair(clean)[1], fmt_b, k)
    for v in (va, vb): assert np.array_equal(np.rint(16.0 * v), 16.0 * v)                # every term is a multiple of 2^-8
    c, s = matmul(*pair(clean), fmt_a, fmt_b, k)
    single = (va != 0).astype(np.int64) @ (vb != 0).astype(np.int64).T <= 1
    assert (single | (s < 2.0 ** 16)).all() and np.array_equal(c.astype(np.float32).astype(np.float64), c)
    line = np.zeros(2 * k, bool); line[0::2] = True
    want_nan = np.broadcast_to(line[:, None] if side == 'a' else line[None, :], c.shape).copy()
    got, _ = matmul(*pair(poisoned), fmt_a, fmt_b, k)
    assert np.array_equal(np.isnan(got), want_nan) and np.array_equal(got[~want_nan], c[~want_nan]) and np.abs(c[~want_nan]).max() > 0
    return (*pair(poisoned), clean, c, want_nan)


def random_inputs(seed: int = 0, shape=RANDOM_SHAPE):
    """x [m, k] and w [n, k] in float32 (by default [37, 200] and [29, 200]): standard normal times a per-row factor 2^U(-6, 6)."""
    m, n, k = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((m, k)) * np.exp2(rng.uniform(-6, 6, (m, 1)))
    w = rng.standard_normal((n, k)) * np.exp2(rng.uniform(-6, 6, (n, 1)))
    return x.astype(np.float32), w.astype(np.float32)


def bound(s: np.ndarray, k: int) -> np.ndarray:
    """K additions in any order, each off by at most one unit in the last place of a truncating float32 adder."""
    return k * 2.0 ** -23 * s
