"""The oracle of the MXINT8 convolution tests: the contract of DESIGN.md section 9.20 in NumPy, built from ``mx_conv_reference`` (the
geometry, the tap-to-pixel map, the packed gather: zero bytes under scale code 127 in the padding) and ``mx_int8_gemm_reference`` (the
product of the gathered operand with the weight viewed as [O, nb']).  A packed operand is ``(elements, scales)`` as
``mx_quantize(t, 'MXINT8', 1)`` leaves a 4-D tensor.  Not a test module."""
import numpy as np

import mx_conv_reference as C
import mx_int8_gemm_reference as G


def conv(x_packed, w_packed, g: C.Geometry, bias=None):
    """(y, exact, s), each [N, O, OH, OW]: y float32 with the contract's bits, exact and s = sum_b |t_b| in float64."""
    a = C.gather_im2col(x_packed, 'MXINT8', g)
    return tuple(C.rows_to_nchw(v, g) for v in G.matmul(a, C.weight_operand(w_packed), bias))


def bound(s: np.ndarray, g: C.Geometry, bias=None) -> np.ndarray:
    """The derived bound: nb' + 1 float32 adds, each rounded to nearest, on partial sums of magnitude at most S + |bias|."""
    b = 0.0 if bias is None else np.abs(np.asarray(bias, np.float64))[None, :, None, None]
    return (g.nb + 1) * 2.0 ** -24 * (s + b)


def raw_operands(g: C.Geometry, scale_pool, seed: int = 0):
    """(x_packed, w_packed): random element codes over all 256 byte values, zeros behind C in the last channel block (as the export
    leaves them), scale codes drawn from the pool."""
    rng = np.random.default_rng([seed, *g[:7]])
    live = (np.arange(g.nbc * G.BLOCK) < g.c)
    out = []
    for lead in ((g.n, g.h, g.w), (g.o, g.kh, g.kw)):
        e = np.where(live, rng.integers(0, 256, lead + (g.nbc * G.BLOCK,)), 0).astype(np.uint8)
        out.append((e, rng.choice(np.asarray(scale_pool), lead + (g.nbc,)).astype(np.uint8)))
    return out
