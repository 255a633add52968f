"""NumPy oracle of the grouped linear INT8 contract: the dense block-diagonal weight, then the gather and the
layer of int8_reference as they stand -- and the geometries both test files run."""
import numpy as np

from int8_reference import ceil32, gather, layer as dense_layer


def block_diagonal(w, groups):
    """w [O, kh, kw, C_g] int8 codes -> the dense [O, kh, kw, ceil32(C)] weight that is zero outside a row's own group."""
    o, kh, kw, cg = w.shape
    dense = np.zeros((o, kh, kw, ceil32(cg * groups)), np.int8)
    for row in range(o):
        g = row // (o // groups)
        dense[row, :, :, g * cg:(g + 1) * cg] = w[row]
    return dense


def layer(x, w, groups, zx, mul, stride, pad, dil, bias=None, residual=None, relu=False, out_q=None):
    """x [N, H, W, Cp], w [O, kh, kw, C_g] int8 codes, residual [N, OH, OW, O] -> (I int64 [M, O], v float32 [N, OH, OW, O], codes int8
    [N, OH, OW, ceil32(O)] or None); out_q = (sy, zy, qmin, qmax, rounding, q_nan)."""
    o, kh, kw, _ = w.shape
    a, (oh, ow) = gather(x, kh, kw, stride, pad, dil, zx)
    i, v, q = dense_layer(a, block_diagonal(w, groups).reshape(o, -1), zx, mul, bias, None if residual is None else residual.reshape(-1, o), relu, out_q)
    return i, v.reshape(len(x), oh, ow, o), None if q is None else q.reshape(len(x), oh, ow, -1)


# (G, C_g, O_g, N, H, W, kh, kw, stride, padding, dilation) and what packing must make of it, (cb0, nbs):
# one slice, eight groups inside one channel block, 162 rows (a full row tile and a partial one), 9 blocks: a K tail of 1;
# cb0 differs per slice, nbs = 1;
# groups straddle block and slice borders: slice 2 starts at block 1 of 3, so its last block is clamped and killed by zeros; 8 live columns;
# 25 rows (three idle waves), several blocks per tap, O_g no multiple of 32, a single short chunk; slice 1 holds outputs of both groups: 4 blocks;
# a channel multiplier, C = 8 inside one padded block
GEOMETRIES = [((8, 4, 4, 2, 9, 9, 3, 3, (1, 1), (1, 1), (1, 1)), ([0], 1)),
              ((2, 32, 32, 2, 9, 9, 3, 3, (2, 2), (1, 1), (1, 1)), ([0, 1], 1)),
              ((3, 24, 24, 2, 7, 7, 3, 3, (1, 1), (2, 2), (2, 2)), ([0, 0, 1], 3)),
              ((2, 64, 40, 1, 5, 5, 1, 1, (1, 1), (0, 0), (1, 1)), ([0, 0, 2], 4)),
              ((8, 1, 2, 2, 6, 6, 3, 3, (1, 1), (1, 1), (1, 1)), ([0], 1))]
