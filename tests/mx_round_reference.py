"""The oracle of MX round tuning in NumPy, on ``mx_reference``'s value tables.

It shares nothing with the integer trick of ppq_amd/csrc/mx_common.hpp (``mx_floor`` / ``mx_up``) or of ppq_amd/mx_roundtune.py: the
block's code comes from ``mx_scale_reference.scale_codes``; ``u = v * 2^(127 - c)`` is the float32 product the contract names; ``lo``
is the largest table value <= |u| and ``hi`` the next entry (the last entry is its own ``hi``), found by ``searchsorted``; the
rounding is formed in float64 and must be a float32 as it stands; ``floored`` and the forward's ``up * X`` are float32 products.
Not a test module."""
import numpy as np

import mx_reference as R
import mx_scale_reference as S
from mx_reference import _table

BLOCK = R.BLOCK


def _pow2(e: np.ndarray) -> np.ndarray:
    """2^e as float32, -127 <= e <= 127 (2^-127 is a subnormal)."""
    return np.ldexp(1.0, np.asarray(e, dtype=np.int64)).astype(np.float32)


def _index_below(a: np.ndarray, t: np.ndarray) -> np.ndarray:
    """The index of the largest table value <= a (a >= 0, Inf allowed)."""
    return np.searchsorted(t, np.minimum(a, t[-1]), side='right') - 1


def split_blocks(blocks: np.ndarray, fmt: str, rule: str = 'FLOOR'):
    """blocks: float32 [n, <= 32].  Returns (floored float32, rounding float32, uint8 [n] scale codes)."""
    blocks = np.asarray(blocks, dtype=np.float32)
    t = _table(fmt)
    code, _ = S.scale_codes(blocks, fmt, rule)
    se = code.astype(np.int64) - 127
    nan = np.isnan(blocks)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        u = blocks * _pow2(-se)[:, None]                           # the float32 product
        a = np.abs(np.where(nan, np.float32(0), u)).astype(np.float64)
        k = _index_below(a, t)
        lo, hi = t[k], t[np.minimum(k + 1, len(t) - 1)]
        open_ = (hi > lo) & np.isfinite(a)
        r64 = np.where(open_, (np.where(open_, a, 0.0) - lo) / np.where(open_, hi - lo, 1.0), 0.0)
        rounding = r64.astype(np.float32)
        assert np.array_equal(rounding.astype(np.float64), r64) and np.all((r64 >= 0) & (r64 < 1))        # exact, in [0, 1)
        floored = np.copysign(lo, u).astype(np.float32) * _pow2(se)[:, None]
    floored[nan] = blocks[nan]
    rounding[nan] = 0
    return floored, rounding, code.astype(np.uint8)


def forward_blocks(floored: np.ndarray, rounding: np.ndarray, codes: np.ndarray, fmt: str) -> np.ndarray:
    """floored, rounding: float32 [n, <= 32]; codes: [n].  Every finite |floored / X| must be a table value (but under a
    code of 0xFF, whose block passes through)."""
    floored, rounding = np.asarray(floored, dtype=np.float32), np.asarray(rounding, dtype=np.float32)
    t = _table(fmt)
    codes = np.asarray(codes).astype(np.int64)
    se = np.minimum(codes, 254) - 127
    nan = np.isnan(floored)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        u = floored * _pow2(-se)[:, None]
        a = np.abs(np.where(nan, np.float32(0), u)).astype(np.float64)
        k = _index_below(a, t)
        on_grid = (t[k] == a) | np.isinf(a)
        assert np.all(on_grid | nan | (codes == 0xff)[:, None]), 'forward_blocks: floored is not on the grid'
        hi = t[np.minimum(k + 1, len(t) - 1)]
        up = np.copysign(hi, u).astype(np.float32) * _pow2(se)[:, None]
        take = (rounding > np.float32(0.5)) & ~nan & (codes != 0xff)[:, None]
    return np.where(take, up, floored)


def _by_blocks(x: np.ndarray, axis: int):
    moved = np.moveaxis(x, axis, -1)
    lead, length = moved.shape[:-1], moved.shape[-1]
    return np.ascontiguousarray(moved).reshape(-1, length), lead, length, (length + BLOCK - 1) // BLOCK


def split(x: np.ndarray, fmt: str, axis: int = -1, rule: str = 'FLOOR'):
    """x: float32 array.  Returns (floored, rounding like x, uint8 codes with the axis replaced by ceil(len / 32))."""
    x = np.asarray(x, dtype=np.float32)
    axis %= x.ndim
    flat, lead, length, nb = _by_blocks(x, axis)
    floored, rounding = np.empty_like(flat), np.empty_like(flat)
    codes = np.empty((flat.shape[0], nb), dtype=np.uint8)
    for b in range(nb):
        lo, hi = b * BLOCK, min(length, (b + 1) * BLOCK)
        floored[:, lo:hi], rounding[:, lo:hi], codes[:, b] = split_blocks(flat[:, lo:hi], fmt, rule)
    back = lambda a, n: np.ascontiguousarray(np.moveaxis(a.reshape(*lead, n), -1, axis))      # noqa: E731
    return back(floored, length), back(rounding, length), back(codes, nb)


def forward(floored: np.ndarray, rounding: np.ndarray, codes: np.ndarray, fmt: str, axis: int = -1) -> np.ndarray:
    floored = np.asarray(floored, dtype=np.float32)
    axis %= floored.ndim
    flat, lead, length, nb = _by_blocks(floored, axis)
    r, _, _, _ = _by_blocks(np.asarray(rounding, dtype=np.float32), axis)
    c, _, _, _ = _by_blocks(np.asarray(codes), axis)
    out = np.empty_like(flat)
    for b in range(nb):
        lo, hi = b * BLOCK, min(length, (b + 1) * BLOCK)
        out[:, lo:hi] = forward_blocks(flat[:, lo:hi], r[:, lo:hi], c[:, b], fmt)
    return np.ascontiguousarray(np.moveaxis(out.reshape(*lead, length), -1, axis))


def nearest(x: np.ndarray, fmt: str, axis: int = -1, rule: str = 'FLOOR'):
    """(the selection ``rounding > .5`` of the split of x, the mask of its exact ties)."""
    floored, rounding, codes = split(x, fmt, axis, rule)
    return forward(floored, rounding, codes, fmt, axis), rounding == np.float32(0.5)


# ---- the data both test files use ---------------------------------------------------------------------------------------------------
ROUNDINGS = np.array([0.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 1.0, np.nan, -1.0, 2.0], np.float32)


def special_rows(fmt: str) -> np.ndarray:
    """[n, 32]: the corners of section 9.18, one block per row, on top of ``mx_reference.special_blocks`` (zeros of both signs, a
    subnormal amax, NaN, +-Inf, exact ties) and ``mx_scale_reference.crafted`` (a saturating amax at the largest normal and one ulp
    above it, all zero, all NaN, all Inf): every table value of the format under X = 1 (values ON the grid) and the midpoints of
    neighbouring table values (exact ties)."""
    t = _table(fmt)
    lead = np.float32(2.0 ** R.EMAX[fmt])
    rows = []
    for values in (t, (t[:-1] + t[1:]) / 2, np.nextafter(t[1:].astype(np.float32), np.float32(0)).astype(np.float64)):
        values = np.concatenate([values, -values]).astype(np.float32)
        pad = (-len(values)) % (BLOCK - 1)
        body = np.concatenate([values, np.zeros(pad, np.float32)]).reshape(-1, BLOCK - 1)
        rows.append(np.concatenate([np.full((len(body), 1), lead, np.float32), body], axis=1))
    return np.concatenate([R.special_blocks(fmt), S.crafted(fmt)] + rows)


def plant_specials(x: np.ndarray, fmt: str) -> np.ndarray:
    """``x`` (at least 2 x 64 elements along its last two axes' product) with the corners planted at its front in storage order: +-0,
    float32 subnormals, +-Inf, NaN, the format's largest normal times two (saturates) and table values."""
    x = np.array(x, dtype=np.float32)
    flat = x.reshape(-1)
    t = _table(fmt)
    vals = [0.0, -0.0, 1e-39, -1e-45, np.inf, -np.inf, np.nan, 2 * t[-1], -t[-1], t[1], t[len(t) // 2], (t[1] + t[2]) / 2]
    flat[:len(vals)] = np.array(vals, np.float32)
    return x


def scaled_blocks(seed: int, n: int = 256) -> np.ndarray:
    """[n, 64]: two blocks per row, the rows spread over 2^+-100."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 64)) * np.exp2(rng.integers(-100, 100, (n, 1)))).astype(np.float32)


def tiny_graph(seed: int = 0):
    """Conv 8 -> 40 3x3, ReLU, Conv 40 -> 16 1x1, global pool, Gemm 16 -> 10."""
    from ppq_amd import harness
    import torch
    gen = torch.Generator().manual_seed(seed)
    g = harness.BaseGraph('tiny_mx')
    x = g.create_variable('input'); g.inputs['input'] = x
    w1 = g.create_variable('c1_w', torch.randn([40, 8, 3, 3], generator=gen) * 0.2, True)
    b1 = g.create_variable('c1_b', torch.randn(40, generator=gen) * 0.1, True)
    y = g.create_operation('Relu', 'c1_relu', [g.create_operation('Conv', 'c1', [x, w1, b1], {'strides': 1, 'pads': 1})])
    w2 = g.create_variable('c2_w', torch.randn([16, 40, 1, 1], generator=gen) * 0.2, True)
    b2 = g.create_variable('c2_b', torch.randn(16, generator=gen) * 0.1, True)
    y = g.create_operation('Conv', 'c2', [y, w2, b2], {'strides': 1, 'pads': 0})
    y = g.create_operation('Flatten', 'flatten', [g.create_operation('GlobalAveragePool', 'gap', [y])])
    w3 = g.create_variable('fc_w', torch.randn([10, 16], generator=gen) * 0.3, True)
    b3 = g.create_variable('fc_b', torch.zeros(10), True)
    y = g.create_operation('Gemm', 'fc', [y, w3, b3])
    g.outputs[y.name] = y
    return g
