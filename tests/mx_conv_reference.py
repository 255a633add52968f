"""The oracle of the MX convolution tests: the contract of DESIGN.md section 9.15 in NumPy, built on ``mx_gemm_reference`` and
``mx_pack_reference``.

A packed operand is ``(elements, scales)`` as ``mx_quantize(t, fmt, axis=1)`` leaves a 4-D tensor: the activation x [N, C, H, W] as
elements [N, H, W, nbc * B] / scales [N, H, W, nbc], the weight w [O, C, kh, kw] as elements [O, kh, kw, nbc * B] / scales
[O, kh, kw, nbc].  ``conv`` decodes both, builds the im2col matrix of the DECODED activation (zeros in the padding), multiplies in
float64 and returns Y [N, O, OH, OW] with S, the same sum over absolute values.  ``gather_im2col`` builds the PACKED im2col operand
[M, nb'] the kernel reads by address -- rows (n, oy, ox), blocks (ky, kx, channel block), zero bits under scale code 127 in the
padding --, which ``mx_gemm_reference.matmul`` multiplies with the weight viewed as [O, nb'].  The generators build operands for which
the answer does not depend on the order or the width of the accumulation; each asserts its own precondition.  Not a test module."""
from collections import namedtuple

import numpy as np

import mx_gemm_reference as G
import mx_pack_reference as P


class Geometry(namedtuple('Geometry', 'n c h w o kh kw stride pad dil')):
    """x [n, c, h, w], weight [o, c, kh, kw]; stride, pad (symmetric) and dil are (h, w) pairs."""
    __slots__ = ()

    @ property
    def oh(self) -> int: return (self.h + 2 * self.pad[0] - self.dil[0] * (self.kh - 1) - 1) // self.stride[0] + 1

    @ property
    def ow(self) -> int: return (self.w + 2 * self.pad[1] - self.dil[1] * (self.kw - 1) - 1) // self.stride[1] + 1

    @ property
    def nbc(self) -> int: return G.nblocks(self.c)

    @ property
    def m(self) -> int: return self.n * self.oh * self.ow

    @ property
    def nb(self) -> int: return self.kh * self.kw * self.nbc                    # blocks of one row of the implicit GEMM

    @ property
    def k(self) -> int: return self.nb * P.BLOCK                                # the K of the accumulation bound

    def __str__(self) -> str:
        return (f'x{[self.n, self.c, self.h, self.w]}-o{self.o}-k{self.kh}x{self.kw}-s{self.stride[0]}{self.stride[1]}'
                f'-p{self.pad[0]}{self.pad[1]}-d{self.dil[0]}{self.dil[1]}')


def geometry(x_shape, o, kernel, stride=1, pad=0, dil=1) -> Geometry:
    two = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    n, c, h, w = x_shape
    kh, kw = two(kernel)
    return Geometry(n, c, h, w, o, kh, kw, two(stride), two(pad), two(dil))


# x [2, 40, 7, 5], 3x3, pad 1: nbc = 2 with a short last block; 18 blocks = four K-steps plus a tail of two; taps straddle K-steps;
# M = 70 > 64 and O = 70 > 64: 2 x 2 workgroups
FIRST = geometry([2, 40, 7, 5], 70, 3, 1, 1)
DILATED = geometry([2, 40, 7, 5], 33, 3, 1, 2, 2)
EDGE_GEOMETRIES = [
    geometry([2, 40, 7, 5], 33, 3, 1, 1),            # the first one with one column of workgroups
    geometry([2, 40, 7, 5], 33, 3, 2, 1),            # strided addressing
    geometry([1, 3, 9, 9], 33, 7, 2, 3),             # nbc = 1: 49 blocks, twelve K-steps and a tail of one
    geometry([2, 128, 4, 4], 70, 2),                 # nbc = 4, aligned: a K-step is one tap
    geometry([1, 160, 3, 6], 33, (1, 3), 1, (0, 1)),  # nbc = 5: FP8 half-pairs across taps; FP6 pixel pitch 8 mod 16
    geometry([2, 40, 7, 5], 33, 1, 2),               # strided 1x1
    DILATED,                                         # dilation
]
ROUTING_GEOMETRIES = [FIRST, DILATED]
NAN_GEOMETRY = geometry([2, 40, 7, 5], 33, 3, 2, 1)
RANDOM_GEOMETRIES = [FIRST, geometry([1, 160, 3, 6], 33, (1, 3), 1, (0, 1))]
# (fmt_x, fmt_w, side, kind) of nan_conv_case
NAN_CASES = [('MXFP8_E4M3', 'MXFP4_E2M1', 'x', 'code'), ('MXFP4_E2M1', 'MXFP8_E5M2', 'w', 'code'),
             ('MXFP4_E2M1', 'MXFP6_E2M3', 'x', 'scale'), ('MXFP6_E2M3', 'MXFP6_E3M2', 'w', 'scale'),
             ('MXFP8_E5M2', 'MXFP8_E4M3', 'x', 'scale')]


def flat(packed):
    """A packed 4-D operand as the 2-D one of ``mx_gemm_reference``: the weight [O, kh, kw, nbc] -> [O, nb'] is a view; the
    activation becomes [pixels, nbc]."""
    e, s = packed
    return np.ascontiguousarray(e.reshape(-1, e.shape[-1])), np.ascontiguousarray(s.reshape(-1, s.shape[-1]))


def weight_operand(w_packed):
    """The weight as the B operand [O, nb' * B] / [O, nb']."""
    e, s = w_packed
    return np.ascontiguousarray(e.reshape(e.shape[0], -1)), np.ascontiguousarray(s.reshape(s.shape[0], -1))


def tap_pixels(g: Geometry) -> np.ndarray:
    """int64 [M, kh * kw]: the flat input pixel (n * H + iy) * W + ix behind tap (ky, kx) of output pixel (n, oy, ox), -1 in the
    padding.  Rows in (n, oy, ox) order, taps in (ky, kx) order."""
    n, oy, ox = np.meshgrid(np.arange(g.n), np.arange(g.oh), np.arange(g.ow), indexing='ij')
    ky, kx = np.meshgrid(np.arange(g.kh), np.arange(g.kw), indexing='ij')
    iy = (oy.reshape(-1, 1) * g.stride[0] - g.pad[0]) + ky.reshape(1, -1) * g.dil[0]
    ix = (ox.reshape(-1, 1) * g.stride[1] - g.pad[1]) + kx.reshape(1, -1) * g.dil[1]
    inside = (iy >= 0) & (iy < g.h) & (ix >= 0) & (ix < g.w)
    return np.where(inside, (n.reshape(-1, 1) * g.h + iy) * g.w + ix, -1).astype(np.int64)


def gather_im2col(x_packed, fmt_x: str, g: Geometry, pixels: np.ndarray = None):
    """The packed A operand (elements [M, nb' * B], scales [M, nb']) of the implicit GEMM: block (tap, cb) of row m is channel block
    cb of pixel ``pixels[m, tap]`` (default ``tap_pixels``), zero bits under scale code 127 where that is -1."""
    e, s = flat(x_packed)
    B = P.BLOCK_BYTES[fmt_x]
    pixels = tap_pixels(g) if pixels is None else pixels
    assert pixels.shape == (g.m, g.kh * g.kw) and pixels.max() < e.shape[0]
    inside = pixels >= 0
    safe = np.where(inside, pixels, 0)
    ge = np.where(inside[:, :, None], e[safe], np.uint8(0))                      # [M, taps, nbc * B]
    gs = np.where(inside[:, :, None], s[safe], np.uint8(127))                    # [M, taps, nbc]
    return np.ascontiguousarray(ge.reshape(g.m, g.nb * B)), np.ascontiguousarray(gs.reshape(g.m, g.nb))


def decode_x(x_packed, fmt_x: str, g: Geometry) -> np.ndarray:
    """float64 [N, H, W, C]."""
    return G.decode(flat(x_packed), fmt_x, g.c).reshape(g.n, g.h, g.w, g.c)


def decode_w(w_packed, fmt_w: str, g: Geometry) -> np.ndarray:
    """float64 [O, kh, kw, C]."""
    return G.decode(flat(w_packed), fmt_w, g.c).reshape(g.o, g.kh, g.kw, g.c)


def conv(x_packed, w_packed, fmt_x: str, fmt_w: str, g: Geometry, bias=None):
    """(Y, S) in float64, both [N, O, OH, OW]: Y = conv2d(x, w) (+ bias), S the same sum over |x| |w|: an explicit im2col of the
    decoded operands, zeros in the padding.  A zero result is +0, as an accumulator that starts at +0 gives."""
    x, w = decode_x(x_packed, fmt_x, g), decode_w(w_packed, fmt_w, g)
    (sh, sw), (ph, pw), (dh, dw) = g.stride, g.pad, g.dil
    xp = np.zeros((g.n, g.h + 2 * ph, g.w + 2 * pw, g.c))
    xp[:, ph:ph + g.h, pw:pw + g.w] = x
    cols = np.empty((g.n, g.oh, g.ow, g.kh, g.kw, g.c))
    for ky in range(g.kh):
        for kx in range(g.kw):
            cols[:, :, :, ky, kx] = xp[:, ky * dh: ky * dh + (g.oh - 1) * sh + 1: sh, kx * dw: kx * dw + (g.ow - 1) * sw + 1: sw]
    cols, wm = cols.reshape(g.m, -1), w.reshape(g.o, -1)
    with np.errstate(invalid='ignore', over='ignore'):
        y = cols @ wm.T + 0.0
        if bias is not None: y = y + np.asarray(bias, np.float64)[None, :]
        s = np.abs(cols) @ np.abs(wm).T
    nchw = lambda a: np.ascontiguousarray(a.reshape(g.n, g.oh, g.ow, g.o).transpose(0, 3, 1, 2))
    return nchw(y), nchw(s)


def rows_to_nchw(c: np.ndarray, g: Geometry) -> np.ndarray:
    """[M, O] of the implicit GEMM -> [N, O, OH, OW]."""
    return np.ascontiguousarray(c.reshape(g.n, g.oh, g.ow, g.o).transpose(0, 3, 1, 2))


def _from_codes(codes: np.ndarray, scales: np.ndarray, fmt: str):
    """codes uint8 [a, b, c, nbc, 32], scales uint8 [a, b, c, nbc] -> the packed 4-D operand."""
    e = P.pack_fields(codes, P.WIDTH[fmt])
    return np.ascontiguousarray(e.reshape(e.shape[:3] + (-1,))), np.ascontiguousarray(scales.astype(np.uint8))


def _live(g: Geometry) -> np.ndarray:
    """[nbc, 32] bool: the channels that exist (the export holds +0 behind them)."""
    return (np.arange(g.nbc * P.BLOCK) < g.c).reshape(g.nbc, P.BLOCK)


def _exact_codes(g: Geometry, fmt_x: str, fmt_w: str, rng):
    live, out = _live(g), []
    for lead, fmt in (((g.n, g.h, g.w), fmt_x), ((g.o, g.kh, g.kw), fmt_w)):
        pool = G.small_codes(fmt)
        codes = np.where(live, pool[rng.integers(0, len(pool), lead + (g.nbc, P.BLOCK))], np.uint8(0))
        out.append([codes, rng.integers(126, 129, lead + (g.nbc,)).astype(np.uint8)])
    return out


def exact_conv_case(g: Geometry, fmt_x: str, fmt_w: str, seed: int = 0):
    """(x_packed, w_packed, Y float64 [N, O, OH, OW]): random small codes (``G.small_codes``) under scale codes 126 .. 128, as
    ``mx_gemm_reference.exact_case``: every term is a multiple of 2^-8 of magnitude at most 2^6 and S < 2^16, so every partial sum
    in any order is exactly representable in float32."""
    rng = np.random.default_rng([seed, *g[:7], *g.stride, *g.pad, *g.dil])
    (cx, sx), (cw, sw) = _exact_codes(g, fmt_x, fmt_w, rng)
    x, w = _from_codes(cx, sx, fmt_x), _from_codes(cw, sw, fmt_w)
    for v in (decode_x(x, fmt_x, g), decode_w(w, fmt_w, g)): assert (np.abs(v) <= 8.0).all() and np.array_equal(np.rint(16.0 * v), 16.0 * v)
    y, s = conv(x, w, fmt_x, fmt_w, g)
    assert s.max() < 2.0 ** 16 and np.array_equal(y.astype(np.float32).astype(np.float64), y)
    assert np.abs(y).max() > 0
    return x, w, y


ROUTING_X_BASE, ROUTING_X_SPAN = 50, 140
ROUTING_W_BASE, ROUTING_W_SPAN = 100, 50


def routing_conv_case(g: Geometry, fmt_x: str, fmt_w: str, tap: int, cb: int, pixels: np.ndarray = None):
    """(x_packed, w_packed, Y float64): the activation is 1.0 in every channel, each (pixel, channel block) under its own scale code
    50 .. 189 (no two equal: N H W nbc <= 140); the weight is 1.0 in block (tap, cb) and +0 elsewhere, its codes running over
    100 .. 149 from (o, tap, cb) to (o, tap, cb).  Every output is the one term count 2^(sx - 127) 2^(sw - 127) of the pixel behind
    ``tap`` -- count = the channels of block cb -- or exactly +0 where the tap is padding: a normal float32 since
    -104 <= sx + sw - 254 <= 84.  A wrong tap-to-pixel map, stride, dilation, padding test or batch boundary picks another pixel's
    code, hence another power of two, or a non-zero value.  ``pixels``: the map to state the expectation with (default ``tap_pixels``)."""
    live = _live(g)
    assert 0 <= tap < g.kh * g.kw and 0 <= cb < g.nbc
    blocks = g.n * g.h * g.w * g.nbc
    assert blocks <= ROUTING_X_SPAN, f'{blocks} activation blocks: two would share a scale code'
    cx = np.where(live, np.uint8(G.code_of(1.0, fmt_x)), np.uint8(0)) * np.ones((g.n, g.h, g.w, 1, 1), np.uint8)
    # channel-block major: neighbouring blocks of a pixel are far apart, so that 8 channels under the next code never look like 32
    sx = np.ascontiguousarray((ROUTING_X_BASE + np.arange(blocks)).reshape(g.nbc, g.n, g.h, g.w).transpose(1, 2, 3, 0)).astype(np.uint8)
    cw = np.zeros((g.o, g.kh * g.kw, g.nbc, P.BLOCK), np.uint8)
    cw[:, tap, cb] = np.where(live[cb], np.uint8(G.code_of(1.0, fmt_w)), np.uint8(0))
    sw = G.routing_scales(g.o, g.nb, ROUTING_W_BASE, ROUTING_W_SPAN).reshape(g.o, g.kh, g.kw, g.nbc)
    x, w = _from_codes(cx, sx, fmt_x), _from_codes(cw.reshape(g.o, g.kh, g.kw, g.nbc, P.BLOCK), sw, fmt_w)
    pix = (tap_pixels(g) if pixels is None else pixels)[:, tap]                  # [M]
    count = int(live[cb].sum())
    ex = sx.reshape(-1, g.nbc)[np.where(pix >= 0, pix, 0), cb].astype(np.float64) - 127
    ew = sw.reshape(g.o, g.kh * g.kw, g.nbc)[:, tap, cb].astype(np.float64) - 127
    want = np.where((pix >= 0)[:, None], count * np.exp2(ex)[:, None] * np.exp2(ew)[None, :], 0.0)
    live_out = want[want != 0]
    assert (live_out >= 2.0 ** -126).all() and (live_out < 2.0 ** 127).all() and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return x, w, rows_to_nchw(want, g)


def nan_conv_case(g: Geometry, fmt_x: str, fmt_w: str, side: str, kind: str, seed: int = 0):
    """(x_packed, w_packed, Y float64, nan bool), the last two [N, O, OH, OW]: the operands of ``exact_conv_case`` with one poison --
    ``kind='code'``: an FP8 NaN code, ``'scale'``: scale code 0xFF -- on ``side``: in x at pixel (n, iy, ix) = (N - 1, 1, W - 1) in
    the last channel block -- a pixel next to the right border of the last image, so that padding, the stride and the batch
    boundary all decide which windows cover it --, in w at output channel O - 2, the last tap, channel block 0.  Y is the exact
    result of the clean pair; the expected NaN set is every output channel of the outputs whose window covers the pixel, resp. the
    whole output channel (a padding zero times NaN is NaN)."""
    assert side in ('x', 'w') and kind in ('code', 'scale')
    fmt = fmt_x if side == 'x' else fmt_w
    assert kind == 'scale' or fmt in G.NAN_CODES
    rng = np.random.default_rng([seed, side == 'w', kind == 'scale'])
    (cx, sx), (cw, sw) = _exact_codes(g, fmt_x, fmt_w, rng)
    clean_x, clean_w = _from_codes(cx, sx, fmt_x), _from_codes(cw, sw, fmt_w)
    y, s = conv(clean_x, clean_w, fmt_x, fmt_w, g)
    assert s.max() < 2.0 ** 16 and np.array_equal(y.astype(np.float32).astype(np.float64), y)
    want_nan = np.zeros((g.n, g.o, g.oh, g.ow), bool)
    if side == 'x':
        at = (g.n - 1, 1, g.w - 1, g.nbc - 1)
        covered = (tap_pixels(g) == (at[0] * g.h + at[1]) * g.w + at[2]).any(axis=1)
        want_nan[:] = covered.reshape(g.n, 1, g.oh, g.ow)
        codes, scales = cx, sx
    else:
        at = (g.o - 2, g.kh - 1, g.kw - 1, 0)
        want_nan[:, at[0]] = True
        codes, scales = cw, sw
    if kind == 'code': codes[at + (3,)] = G.NAN_CODES[fmt][-1]
    else: scales[at] = 0xff
    x, w = _from_codes(cx, sx, fmt_x), _from_codes(cw, sw, fmt_w)
    got, _ = conv(x, w, fmt_x, fmt_w, g)
    assert want_nan.any() and not want_nan.all()
    assert np.array_equal(np.isnan(got), want_nan) and np.array_equal(got[~want_nan], y[~want_nan]) and np.abs(y[~want_nan]).max() > 0
    return x, w, y, want_nan


def random_inputs(g: Geometry, seed: int = 0):
    """x [N, C, H, W] and w [O, C, kh, kw] in float32: standard normal times a factor 2^U(-6, 6) per image resp. per output channel.
    Only those: taps of different pixels meet inside one K-step, so a per-pixel spread would be an in-block spread, for which the
    bound of DESIGN.md section 9.14 is open with FP8 operands."""
    rng = np.random.default_rng([seed, *g[:7]])
    x = rng.standard_normal((g.n, g.c, g.h, g.w)) * np.exp2(rng.uniform(-6, 6, (g.n, 1, 1, 1)))
    w = rng.standard_normal((g.o, g.c, g.kh, g.kw)) * np.exp2(rng.uniform(-6, 6, (g.o, 1, 1, 1)))
    return x.astype(np.float32), w.astype(np.float32)


def pack4(t: np.ndarray, fmt: str):
    """float32 [a, C, b, c] -> the packed operand (elements [a, b, c, nbc * B], scales [a, b, c, nbc]): ``mx_pack_reference.pack``
    along axis 1."""
    return P.pack(t, fmt, 1)


def bound(s: np.ndarray, g: Geometry) -> np.ndarray:
    """Section 9.14's bound with K = kh * kw * 32 * nbc."""
    return G.bound(s, g.k)


# ---- two wrong gathers: what the routing comparison must refuse (tests/test_host_mx_conv.py) ----------------------------------------
def tap_pixels_kx_ky(g: Geometry) -> np.ndarray:
    """``tap_pixels`` with the taps enumerated in (kx, ky) order."""
    p = tap_pixels(g).reshape(g.m, g.kh, g.kw)
    return np.ascontiguousarray(p.transpose(0, 2, 1)).reshape(g.m, g.kh * g.kw)


def tap_pixels_no_batch_padding(g: Geometry) -> np.ndarray:
    """``tap_pixels`` that tests the column only: a row above or below the image is taken from the neighbouring image of the batch
    (the flat pixel index runs on), and is padding only where it leaves the tensor."""
    n, oy, ox = np.meshgrid(np.arange(g.n), np.arange(g.oh), np.arange(g.ow), indexing='ij')
    ky, kx = np.meshgrid(np.arange(g.kh), np.arange(g.kw), indexing='ij')
    iy = (oy.reshape(-1, 1) * g.stride[0] - g.pad[0]) + ky.reshape(1, -1) * g.dil[0]
    ix = (ox.reshape(-1, 1) * g.stride[1] - g.pad[1]) + kx.reshape(1, -1) * g.dil[1]
    row = n.reshape(-1, 1) * g.h + iy
    inside = (row >= 0) & (row < g.n * g.h) & (ix >= 0) & (ix < g.w)
    return np.where(inside, row * g.w + ix, -1).astype(np.int64)
