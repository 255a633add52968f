"""The oracle of the MX tests: the contract of DESIGN.md section 9 in NumPy, by tables of representable values.

It shares nothing with the bit arithmetic of ppq_amd/csrc/mx.hip or of ppq_amd/mx.py: the element values of a format are
enumerated from their OCP encodings, a value is cast to the nearest table entry by float64 distance (a tie goes to the even table
index, which is the even encoding: the tables list the non-negative encodings in order), and the shared exponent comes from
``math.frexp`` of the block maximum.  Not a test module."""
import math

import numpy as np

BLOCK = 32
# name -> (exponent bits, mantissa bits, bias, emax); MXINT8 is not a float format
FLOAT_FORMATS = {
    'MXFP8_E4M3': (4, 3, 7, 8),
    'MXFP8_E5M2': (5, 2, 15, 15),
    'MXFP6_E3M2': (3, 2, 3, 4),
    'MXFP6_E2M3': (2, 3, 1, 2),
    'MXFP4_E2M1': (2, 1, 1, 2),
}
EMAX = {**{k: v[3] for k, v in FLOAT_FORMATS.items()}, 'MXINT8': 0}
FORMATS = list(EMAX)


def table(fmt: str) -> np.ndarray:
    """The non-negative finite element values of the format in encoding order, as float64.  FP8: codes that the OCP encodings give
    to Inf / NaN are left out (E4M3: S.1111.111; E5M2: exponent field 31); FP6 / FP4 have none; MXINT8: k / 64, 0 <= k <= 127."""
    if fmt == 'MXINT8': return np.arange(128, dtype=np.float64) / 64.0
    ebits, mbits, bias, _ = FLOAT_FORMATS[fmt]
    values = []
    for code in range(1 << (ebits + mbits)):
        e, m = code >> mbits, code & ((1 << mbits) - 1)
        if fmt == 'MXFP8_E4M3' and code == 0x7f: continue
        if fmt == 'MXFP8_E5M2' and e == 31: continue
        if e == 0: values.append(math.ldexp(m, 1 - bias - mbits))
        else: values.append(math.ldexp((1 << mbits) + m, e - bias - mbits))
    return np.asarray(values, dtype=np.float64)


_TABLES = {}


def _table(fmt):
    if fmt not in _TABLES: _TABLES[fmt] = table(fmt)
    return _TABLES[fmt]


def cast(u: np.ndarray, fmt: str) -> np.ndarray:
    """Nearest table value to each FINITE u (float64 in, float64 out), ties to the even index, magnitude saturating at the last
    entry; the sign is kept (also on zero)."""
    t = _table(fmt)
    u = np.asarray(u, dtype=np.float64)
    a = np.minimum(np.abs(u), t[-1])
    hi = np.clip(np.searchsorted(t, a, side='left'), 1, len(t) - 1)       # t[hi - 1] <= a <= t[hi] (a == t[0] == 0: hi = 1)
    lo = hi - 1
    dl, dh = a - t[lo], t[hi] - a
    pick = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    return np.copysign(t[pick], u)


def quantize_blocks(blocks: np.ndarray, fmt: str):
    """blocks: float32 [n, <= 32].  Returns (float32 [n, len], uint8 [n] scale codes)."""
    blocks = np.asarray(blocks, dtype=np.float32)
    emax, top = EMAX[fmt], _table(fmt)[-1]
    finite, inf, nan = np.isfinite(blocks), np.isinf(blocks), np.isnan(blocks)
    v = np.where(finite, blocks, np.float32(0)).astype(np.float64)
    amax = np.abs(v).max(axis=1)
    _, e = np.frexp(amax)                                # amax = f * 2^e with 0.5 <= f < 1, so floor(log2(amax)) = e - 1
    se = np.where(amax > 0.0, np.clip(e - 1 - emax, -127, 127), -127).astype(np.int64)
    y = np.ldexp(cast(np.ldexp(v, -se[:, None]), fmt), se[:, None])
    y = np.where(inf, np.copysign(np.ldexp(top, se)[:, None], blocks.astype(np.float64)), y)
    out = y.astype(np.float32)                           # exact: the contract says every result is a float32
    assert np.array_equal(out.astype(np.float64)[~nan], y[~nan])
    out[nan] = blocks[nan]
    return out, (se + 127).astype(np.uint8)


def quantize(x: np.ndarray, fmt: str, axis: int = -1):
    """x: float32 array.  Returns (y like x, uint8 codes with the axis replaced by ceil(len / 32))."""
    x = np.asarray(x, dtype=np.float32)
    axis %= x.ndim
    moved = np.moveaxis(x, axis, -1)
    lead, length = moved.shape[:-1], moved.shape[-1]
    nb = (length + BLOCK - 1) // BLOCK
    flat = np.ascontiguousarray(moved).reshape(-1, length)
    y = np.empty_like(flat)
    codes = np.empty((flat.shape[0], nb), dtype=np.uint8)
    for b in range(nb):
        lo, hi = b * BLOCK, min(length, (b + 1) * BLOCK)
        y[:, lo:hi], codes[:, b] = quantize_blocks(flat[:, lo:hi], fmt)
    y = np.moveaxis(y.reshape(*lead, length), -1, axis)
    codes = np.moveaxis(codes.reshape(*lead, nb), -1, axis)
    return np.ascontiguousarray(y), np.ascontiguousarray(codes)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- the inputs both MX test files use -------------------------------------------------------------------------------------------
# (shape, axis): rows of whole blocks, a short tail, a row shorter than a block, a one-element tail with rows that are not 16-byte
# aligned; then the strided layouts: odd inner with a short tail, inner 9, a 3x3 weight
LAYOUTS = [((3, 32), -1), ((3, 64), -1), ((3, 40), -1), ((5, 7), -1), ((2, 33), -1), ((2, 40, 3, 5), 1), ((70, 9), 0), ((4, 35, 3, 3), 1)]
CHANNELS_LAST_SHAPE = (2, 64, 4, 4)


def layout_input(shape, seed: int = 0) -> np.ndarray:
    """Gaussian values whose magnitude wanders over 16 octaves from element to element, so that blocks differ in scale."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * np.exp2(rng.integers(-8, 8, shape))).astype(np.float32)


def gaussian_blocks() -> np.ndarray:
    """[2048, 64]: two blocks per row, the rows spread over 40 octaves."""
    rng = np.random.default_rng(7)
    return (rng.standard_normal((2048, 64)) * np.exp2(rng.integers(-20, 20, (2048, 1)))).astype(np.float32)


def special_blocks(fmt: str) -> np.ndarray:
    """[n, 32]: the corner cases of the contract, one per row."""
    rng = np.random.default_rng(3)
    normal = rng.standard_normal(BLOCK).astype(np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows = []
    zeros = np.zeros(BLOCK, np.float32); zeros[1::2] = -0.0
    rows.append(zeros)                                                                    # all zeros, mixed signs
    tiny = np.zeros(BLOCK, np.float32); tiny[:6] = [1e-39, -5e-40, 3e-40, 1e-45, -1e-45, 7e-41]
    rows.append(tiny)                                                                     # subnormal amax: se clamps to -127
    huge = normal.copy(); huge[:6] = [3e38, -1e38, 2.5e38, 1e30, -3e38, 1e-10]
    rows.append(huge)                                                                     # amax 3e38
    a = normal.copy(); a[5] = nan
    rows.append(a)                                                                        # a NaN inside a normal block
    b = normal.copy(); b[3], b[17] = inf, -inf
    rows.append(b)                                                                        # +Inf and -Inf inside a normal block
    c = np.full(BLOCK, nan, np.float32); c[::3] = inf; c[1::6] = -inf
    rows.append(c)                                                                        # only NaN and Inf
    ties = np.zeros(BLOCK, np.float32)
    ties[0] = np.float32(2.0 ** EMAX[fmt])                                                # X = 1
    ties[1:9] = [0.75, 1.25, 2.5, 5, -0.75, -1.25, -2.5, -5]
    if fmt == 'MXINT8':                                                                   # the grid is k / 64: (k + 0.5) / 64; 127.5 / 64 saturates
        ties[1:9] = [32.5 / 64, 33.5 / 64, -32.5 / 64, -33.5 / 64, 0.5 / 64, 1.5 / 64, 127.5 / 64, -127.5 / 64]
    rows.append(ties)                                                                     # exact ties
    return np.stack(rows)


def exhaustive_blocks(fmt: str) -> np.ndarray:
    """[n, 32] blocks that hold every float32 pattern with an exponent of at most emax, as high half-word x three low half-words
    (zero and two random ones); element 0 of every block is 2^emax, so X = 1 throughout and the patterns between the largest normal
    and 2^(emax + 1) saturate."""
    emax = EMAX[fmt]
    rng = np.random.default_rng(11)
    mags = np.arange((127 + emax + 1) << 7, dtype=np.uint32)
    high = np.concatenate([mags, mags | np.uint32(0x8000)])
    low = [np.zeros(len(high), np.uint32), rng.integers(0, 1 << 16, len(high)).astype(np.uint32), rng.integers(0, 1 << 16, len(high)).astype(np.uint32)]
    patterns = np.concatenate([(high << np.uint32(16)) | l for l in low])
    pad = (-len(patterns)) % (BLOCK - 1)
    patterns = np.concatenate([patterns, np.zeros(pad, np.uint32)]).reshape(-1, BLOCK - 1)
    lead = np.full((len(patterns), 1), np.float32(2.0 ** emax).view(np.uint32), np.uint32)
    return np.ascontiguousarray(np.concatenate([lead, patterns], axis=1)).view(np.float32)


KNOWN_BLOCK = np.array([0.3, -1.3, 2.6, 5.1, -7, 0.24, 0.26, 0.75] + [0.0] * 24, np.float32)
KNOWN_ANSWERS = {        # format -> (scale code, first eight outputs)
    'MXFP4_E2M1': (127, [0.5, -1.5, 3, 6, -6, 0, 0.5, 1]),
    'MXFP6_E2M3': (127, [0.25, -1.25, 2.5, 5, -7, 0.25, 0.25, 0.75]),
    'MXFP6_E3M2': (125, [0.3125, -1.25, 2.5, 5, -7, 0.25, 0.25, 0.75]),
    'MXFP8_E4M3': (121, [0.3125, -1.25, 2.5, 5, -7, 0.234375, 0.25, 0.75]),
    'MXFP8_E5M2': (114, [0.3125, -1.25, 2.5, 5, -7, 0.25, 0.25, 0.75]),
}
