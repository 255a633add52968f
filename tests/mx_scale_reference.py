"""The oracle of the MX scale rules in NumPy, on ``mx_reference``'s value tables.

It shares nothing with the bit arithmetic of ppq_amd/csrc/mx_common.hpp or ppq_amd/mx.py: a rule is stated on VALUES in float64 --
amax against the largest normal (CEIL), amax plus half an element ULP (EVEN), the two squared errors by table look-up (MSE) -- and
the cast is ``mx_reference.cast``.  Not a test module."""
import numpy as np

import mx_reference as R
from mx_reference import EMAX, _table, cast

RULES = ('FLOOR', 'CEIL', 'EVEN', 'MSE')
NEW_RULES = RULES[1:]
MANTISSA = {'MXFP8_E4M3': 3, 'MXFP8_E5M2': 2, 'MXFP6_E3M2': 2, 'MXFP6_E2M3': 3, 'MXFP4_E2M1': 1, 'MXINT8': 6}
BLOCK = R.BLOCK


def floor_exponent(amax: np.ndarray) -> np.ndarray:
    """floor(log2(amax)) for amax > 0 (float64, exact through frexp); -10**6 for amax == 0."""
    _, e = np.frexp(amax)
    return np.where(amax > 0.0, e - 1, -10 ** 6).astype(np.int64)


def floor_code(amax: np.ndarray, fmt: str) -> np.ndarray:
    """The OCP rule: clamp(floor(log2(amax)) - emax, -127, 127) + 127, 0 for amax == 0."""
    return (np.clip(floor_exponent(amax) - EMAX[fmt], -127, 127) + 127).astype(np.int64)


def values_under(blocks: np.ndarray, code: np.ndarray, fmt: str) -> np.ndarray:
    """cast(v / X) * X with X = 2^(code - 127) per row, float32: NaN keeps its bits, +-Inf saturates."""
    blocks = np.asarray(blocks, dtype=np.float32)
    se = code.astype(np.int64) - 127
    finite, inf, nan = np.isfinite(blocks), np.isinf(blocks), np.isnan(blocks)
    v = np.where(finite, blocks, np.float32(0)).astype(np.float64)
    y = np.ldexp(cast(np.ldexp(v, -se[:, None]), fmt), se[:, None])
    y = np.where(inf, np.copysign(np.ldexp(_table(fmt)[-1], se)[:, None], blocks.astype(np.float64)), y)
    with np.errstate(over='ignore'): out = y.astype(np.float32)
    # exact: every result is a float32 -- but for 2^128, which a raised scale makes of an amax that rounds up out of float32's
    # last binade: the float32 product cast(v / X) * X is then +-Inf
    exact = ~nan & (np.abs(y) < 2.0 ** 128)
    assert np.array_equal(out.astype(np.float64)[exact], y[exact]) and np.all(np.abs(y[~nan & ~exact]) == 2.0 ** 128)
    out[nan] = blocks[nan]
    return out


def squared_error(blocks: np.ndarray, code: np.ndarray, fmt: str) -> np.ndarray:
    """Sum over the FINITE elements of (cast(v / X) * X - v)^2 in float64, per row."""
    blocks = np.asarray(blocks, dtype=np.float32)
    finite = np.isfinite(blocks)
    with np.errstate(invalid='ignore'):
        d = np.where(finite, values_under(blocks, code, fmt).astype(np.float64) - blocks.astype(np.float64), 0.0)
    return (d * d).sum(axis=1)


def scale_codes(blocks: np.ndarray, fmt: str, rule: str):
    """(codes int64 [n], (err(c0), err(c1)) for MSE or None) of float32 blocks [n, <= 32]."""
    assert rule in RULES, rule
    blocks = np.asarray(blocks, dtype=np.float32)
    top, m = _table(fmt)[-1], MANTISSA[fmt]
    amax = np.abs(np.where(np.isfinite(blocks), blocks, np.float32(0)).astype(np.float64)).max(axis=1)
    c0 = floor_code(amax, fmt)
    if rule == 'FLOOR': return c0, None
    if rule == 'CEIL':                                   # the smallest scale >= the floor scale under which amax does not saturate
        return np.minimum(c0 + (np.ldexp(amax, 127 - c0) > top), 254), None
    if rule == 'EVEN':                                   # amax plus half an element ULP of its binade (float32's subnormals: of 2^-126)
        rounded = amax + np.ldexp(1.0, np.maximum(floor_exponent(amax), -126) - m - 1)
        field = np.where(rounded < 2.0 ** -126, 0, floor_exponent(rounded) + 127)      # the float32 exponent field, up to 255
        return np.clip(field - EMAX[fmt], 0, 254).astype(np.int64), None
    c1 = np.minimum(c0 + 1, 254)
    e0, e1 = squared_error(blocks, c0, fmt), squared_error(blocks, c1, fmt)
    return np.where(e1 < e0, c1, c0), (e0, e1)


def quantize_blocks(blocks: np.ndarray, fmt: str, rule: str = 'FLOOR'):
    """blocks: float32 [n, <= 32].  Returns (float32 [n, len], uint8 [n] scale codes, (err(c0), err(c1)) for MSE, else None)."""
    code, errors = scale_codes(blocks, fmt, rule)
    assert code.min() >= 0 and code.max() <= 254
    return values_under(blocks, code, fmt), code.astype(np.uint8), errors


def quantize(x: np.ndarray, fmt: str, axis: int = -1, rule: str = 'FLOOR'):
    """x: float32 array.  Returns (y like x, uint8 codes with the axis replaced by ceil(len / 32), for MSE the two errors stacked
    last on the codes' shape -- float64 [..., 2] -- else None)."""
    x = np.asarray(x, dtype=np.float32)
    axis %= x.ndim
    moved = np.moveaxis(x, axis, -1)
    lead, length = moved.shape[:-1], moved.shape[-1]
    nb = (length + BLOCK - 1) // BLOCK
    flat = np.ascontiguousarray(moved).reshape(-1, length)
    y = np.empty_like(flat)
    codes = np.empty((flat.shape[0], nb), dtype=np.uint8)
    errors = np.zeros((flat.shape[0], nb, 2), dtype=np.float64) if rule == 'MSE' else None
    for b in range(nb):
        lo, hi = b * BLOCK, min(length, (b + 1) * BLOCK)
        y[:, lo:hi], codes[:, b], e = quantize_blocks(flat[:, lo:hi], fmt, rule)
        if e is not None: errors[:, b, 0], errors[:, b, 1] = e
    y = np.moveaxis(y.reshape(*lead, length), -1, axis)
    codes = np.moveaxis(codes.reshape(*lead, nb), -1, axis)
    if errors is not None: errors = np.ascontiguousarray(np.moveaxis(errors.reshape(*lead, nb, 2), -2, axis))
    return np.ascontiguousarray(y), np.ascontiguousarray(codes), errors


def near_ties(errors, relative: float = 2.0 ** -40) -> int:
    """Blocks whose two errors differ, but by no more than ``relative`` of the larger: where a sum taken in another order could
    decide otherwise."""
    e0, e1 = errors[..., 0], errors[..., 1]
    with np.errstate(invalid='ignore'): gap = np.abs(e1 - e0)
    return int(((gap > 0) & np.isfinite(gap) & (gap <= relative * np.maximum(e0, e1))).sum())      # an infinite error is no tie


# ---- crafted blocks ----------------------------------------------------------------------------------------------------------------
def _f32(pattern: int) -> np.float32:
    return np.array([pattern], np.uint32).view(np.float32)[0]


def _pattern(v) -> int:
    return int(np.array([v], np.float32).view(np.uint32)[0])


def _block(amax, fill=0.0) -> np.ndarray:
    b = np.full(BLOCK, fill, np.float32)
    b[0] = amax
    return b


def crafted_blocks(fmt: str):
    """[(name, float32 [32])]: the corners of the rules, one block each (section 9.17's list)."""
    top, emax, m = np.float32(_table(fmt)[-1]), EMAX[fmt], MANTISSA[fmt]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows = []
    for k in (-20, 0, 9):                                # amax exactly top * 2^k: CEIL stays; one ulp above: CEIL bumps
        at = _pattern(np.float32(np.ldexp(float(top), k)))
        rows.append((f'top*2^{k}', _block(_f32(at), 0.0)))
        rows.append((f'top*2^{k}+ulp', _block(-_f32(at + 1), 0.0)))
    # EVEN bumps from the pattern whose mantissa is all ones above bit 22 - m: 2 - 2^-(m + 1) in its binade
    threshold = _pattern(np.float32(np.ldexp(2.0 - 2.0 ** -(m + 1), 3)))
    rows.append(('even threshold', _block(_f32(threshold))))
    rows.append(('even threshold-ulp', _block(_f32(threshold - 1))))
    rows.append(('exponent 254', _block(_f32(0x7f000000 | 0x7fffff), 1e30)))              # the largest float32
    rows.append(('exponent 254 low', _block(_f32(0x7f000001), -1e30)))
    rows.append(('subnormal amax', _block(_f32(0x00400001), 1e-45)))
    rows.append(('e == emax', _block(_f32(((emax << 23) | 0x7fffff)), 0.0)))              # exponent field emax: floor code 0, CEIL 1
    rows.append(('e == emax + 1', _block(_f32((((emax + 1) << 23) | 0x7fffff)), 0.0)))
    rows.append(('all zero', np.zeros(BLOCK, np.float32)))
    rows.append(('all NaN', np.full(BLOCK, nan, np.float32)))
    rows.append(('all Inf', np.where(np.arange(BLOCK) % 2 == 0, inf, -inf).astype(np.float32)))
    mixed = (np.linspace(-1.0, 1.0, BLOCK) * float(top) * 0.99).astype(np.float32)
    a = mixed.copy(); a[7] = nan
    rows.append(('NaN with finite', a))
    b = mixed.copy(); b[3], b[11] = inf, -inf
    rows.append(('Inf with finite', b))
    # both candidates quantise alike: every element is representable under either scale
    rows.append(('candidates alike', _block(np.float32(2.0 ** emax), 0.0)))
    rows.append(('fp4 7.5', _block(np.float32(7.5), 0.0)))                                 # MXFP4: err 2.25 under c0, 0.25 under c1
    return rows


def crafted(fmt: str) -> np.ndarray:
    return np.stack([b for _, b in crafted_blocks(fmt)])


def ceil_bumps_mse_does_not(fmt: str, blocks: np.ndarray):
    """Indices of the blocks where CEIL raises the floor code and MSE keeps it."""
    floor, _ = scale_codes(blocks, fmt, 'FLOOR')
    ceil, _ = scale_codes(blocks, fmt, 'CEIL')
    mse, _ = scale_codes(blocks, fmt, 'MSE')
    return np.flatnonzero((ceil > floor) & (mse == floor))


# ---- the inputs both test files use -------------------------------------------------------------------------------------------------
def layout_cases():
    """[(x, axis)]: ``mx_reference.LAYOUTS`` and the channels-last shape, the seeds both files use."""
    return [(R.layout_input(shape, seed=k), axis) for k, (shape, axis) in enumerate(R.LAYOUTS + [(R.CHANNELS_LAST_SHAPE, 1)])]


def gaussian_blocks() -> np.ndarray:
    """The first 256 rows of ``mx_reference.gaussian_blocks``: 512 blocks over 40 octaves."""
    return R.gaussian_blocks()[:256]


def block_cases(fmt: str):
    """[(name, float32 [n, 32 or 64])]: the random, the special and the crafted blocks."""
    return [('gaussian', gaussian_blocks()), ('special', R.special_blocks(fmt)), ('crafted', crafted(fmt))]
