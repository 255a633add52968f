"""The oracle of the packed MX tests: the contract of DESIGN.md section 9.13 in NumPy, built on ``mx_reference``.

It shares nothing with the bit arithmetic of ppq_amd/csrc/mx_pack.hip or of ppq_amd/mx.py: the quantised values come from
``mx_reference.quantize``, each is divided by its block's scale with ``ldexp`` and its magnitude is looked up EXACTLY in
``mx_reference.table(fmt)`` -- the tables list the non-negative encodings in order, so the index is the encoding -- the sign bit goes
on top, and the 4 / 6 / 8-bit fields are laid out with ``np.packbits(..., bitorder='little')``.  ``unpack`` inverts it through the
same tables.  Not a test module."""
import numpy as np

import mx_reference as R

BLOCK = R.BLOCK
WIDTH = {'MXFP8_E4M3': 8, 'MXFP8_E5M2': 8, 'MXFP6_E3M2': 6, 'MXFP6_E2M3': 6, 'MXFP4_E2M1': 4, 'MXINT8': 8}
BLOCK_BYTES = {fmt: BLOCK * w // 8 for fmt, w in WIDTH.items()}
HAS_NAN = ('MXFP8_E4M3', 'MXFP8_E5M2')
QUIET_NAN = np.uint32(0x7fc00000)


def _blocks(a: np.ndarray, axis: int, fill):
    """a with the axis moved last, padded with ``fill`` to whole blocks: [lead..., nb, 32]."""
    moved = np.ascontiguousarray(np.moveaxis(a, axis, -1))
    length = moved.shape[-1]
    nb = (length + BLOCK - 1) // BLOCK
    out = np.full(moved.shape[:-1] + (nb * BLOCK,), fill, dtype=a.dtype)
    out[..., :length] = moved
    return out.reshape(moved.shape[:-1] + (nb, BLOCK))


def codes(x: np.ndarray, fmt: str, axis: int = -1):
    """(element codes uint8 [lead..., nb, 32], scale codes uint8 [lead..., nb]) of float32 x, blocks along ``axis``."""
    x = np.asarray(x, dtype=np.float32)
    axis %= x.ndim
    y, scales = R.quantize(x, fmt, axis)
    xb, yb = _blocks(x, axis, np.float32(0)), _blocks(y, axis, np.float32(0))
    scales = np.ascontiguousarray(np.moveaxis(scales, axis, -1))
    nan = np.isnan(xb)
    se = scales.astype(np.int64) - 127
    v = np.ldexp(np.where(nan, np.float32(0), yb).astype(np.float64), -se[..., None])          # the element values: exact
    t = R.table(fmt)
    index = np.searchsorted(t, np.abs(v))
    assert (index < len(t)).all() and np.array_equal(t[index], np.abs(v)), 'a quantised value is not an element value'
    sign = np.signbit(xb)
    if fmt == 'MXINT8':
        k = np.rint(v * 64.0).astype(np.int64)
        assert np.array_equal(np.abs(k), index) and (np.abs(k) <= 127).all()
        out = k.astype(np.int8).view(np.uint8)                                                   # two's complement; -0 is 0
    else:
        out = (index | (sign.astype(np.int64) << (WIDTH[fmt] - 1))).astype(np.uint8)
    if fmt in HAS_NAN:
        out = np.where(nan, np.uint8(0x7f) | (sign.astype(np.uint8) << np.uint8(7)), out)        # S.1111.111 / S.11111.11
    else:                                              # no NaN encoding: the whole block is NaN -- scale 0xFF, zero bytes
        dead = nan.any(axis=-1)
        out = np.where(dead[..., None], np.uint8(0), out)
        scales = np.where(dead, np.uint8(0xff), scales)
    return out.astype(np.uint8), scales.astype(np.uint8)


def pack_fields(c: np.ndarray, width: int) -> np.ndarray:
    """[..., 32] codes -> [..., 4 * width] bytes: field i at bits [i * width, i * width + width) of the little-endian bit string."""
    b = np.unpackbits(np.ascontiguousarray(c, dtype=np.uint8)[..., None], axis=-1, bitorder='little')[..., :width]
    return np.packbits(b.reshape(c.shape[:-1] + (BLOCK * width,)), axis=-1, bitorder='little')


def unpack_fields(e: np.ndarray, width: int) -> np.ndarray:
    """[..., 4 * width] bytes -> [..., 32] codes."""
    b = np.unpackbits(np.ascontiguousarray(e, dtype=np.uint8), axis=-1, bitorder='little').reshape(e.shape[:-1] + (BLOCK, width))
    b = np.concatenate([b, np.zeros(b.shape[:-1] + (8 - width,), np.uint8)], axis=-1)
    return np.packbits(b, axis=-1, bitorder='little')[..., 0]


def pack(x: np.ndarray, fmt: str, axis: int = -1):
    """(elements uint8 [lead..., nb * B], scales uint8 [lead..., nb]): the packed tensor, block axis last."""
    c, scales = codes(x, fmt, axis)
    e = pack_fields(c, WIDTH[fmt])
    return np.ascontiguousarray(e.reshape(e.shape[:-2] + (-1,))), np.ascontiguousarray(scales)


def decode_bits(c: np.ndarray, scales: np.ndarray, fmt: str) -> np.ndarray:
    """float32 patterns (uint32) of codes [..., nb, 32] under scale codes [..., nb]: value(code) * 2^(scale - 127)."""
    t = R.table(fmt)
    c = c.astype(np.int64)
    se = scales.astype(np.int64)[..., None] - 127
    nan = np.broadcast_to(scales[..., None] == 0xff, c.shape).copy()
    nan_bits = np.full(c.shape, QUIET_NAN, np.uint32)
    if fmt == 'MXINT8':
        v = np.where(c >= 128, c - 256, c) / 64.0
    else:
        w = WIDTH[fmt]
        sign, mag = c >> (w - 1), c & ((1 << (w - 1)) - 1)
        inf = np.zeros(c.shape, bool)
        if fmt == 'MXFP8_E4M3': nan |= mag == 0x7f
        if fmt == 'MXFP8_E5M2': nan |= mag > 0x7c; inf = mag == 0x7c
        v = np.where(inf, np.inf, t[np.minimum(mag, len(t) - 1)])
        v = np.where(sign == 1, -v, v)
        if fmt in HAS_NAN: nan_bits = nan_bits | (sign.astype(np.uint32) << np.uint32(31))
    with np.errstate(over='ignore'):
        y = np.ldexp(v, np.where(nan, 0, se)).astype(np.float32)
    return np.where(nan, nan_bits, y.view(np.uint32))


def unpack(elements: np.ndarray, scales: np.ndarray, fmt: str, shape, axis: int = -1) -> np.ndarray:
    """The float32 array of ``shape`` (as uint32 patterns viewed as float32): tail padding dropped, the axis moved back."""
    axis %= len(shape)
    nb = scales.shape[-1]
    c = unpack_fields(elements.reshape(elements.shape[:-1] + (nb, BLOCK_BYTES[fmt])), WIDTH[fmt])
    bits = decode_bits(c, scales, fmt).reshape(scales.shape[:-1] + (nb * BLOCK,))[..., :shape[axis]]
    return np.ascontiguousarray(np.moveaxis(bits, -1, axis)).view(np.float32)


def foreign_codes(fmt: str):
    """Every code of the format, in whole blocks under scale 127 and again under scale 0xFF: (elements [2, n * B], scales [2, n])."""
    n = max(1, (1 << WIDTH[fmt]) // BLOCK)
    c = (np.arange(n * BLOCK) % (1 << WIDTH[fmt])).astype(np.uint8).reshape(n, BLOCK)
    e = pack_fields(c, WIDTH[fmt]).reshape(-1)
    return np.stack([e, e]), np.stack([np.full(n, 127, np.uint8), np.full(n, 0xff, np.uint8)])


def same_but_nan(got: np.ndarray, want: np.ndarray, nan_mask: np.ndarray, fmt: str) -> bool:
    """The parity statement: got (dequantised) has the bits of want (fake-quantised) outside ``nan_mask`` -- for MXINT8 after -0 ->
    +0 -- and NaN inside it."""
    g, w = R.bits(got).copy(), R.bits(want).copy()
    if fmt == 'MXINT8': w[w == np.uint32(0x80000000)] = 0
    return bool(np.array_equal(g[~nan_mask], w[~nan_mask]) and np.isnan(np.asarray(got)[nan_mask]).all())


def nan_mask(x: np.ndarray, fmt: str, axis: int = -1) -> np.ndarray:
    """Where the round trip gives NaN: the NaN elements (MXFP8), every element of a block that holds one (the other formats)."""
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    if fmt in HAS_NAN: return nan
    axis %= x.ndim
    moved = np.moveaxis(nan, axis, -1)
    out = np.zeros_like(moved)
    for lo in range(0, moved.shape[-1], BLOCK): out[..., lo:lo + BLOCK] = moved[..., lo:lo + BLOCK].any(axis=-1, keepdims=True)
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))
