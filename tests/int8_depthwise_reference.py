"""NumPy oracle of the depthwise linear INT8 contract: the sum over the taps of one channel in int64 from the
gather of int8_reference, every later step in np.float32 exactly as int8_reference.layer takes it -- and the geometries both test files run."""
import numpy as np

from int8_reference import f32, gather, to_int


def layer(x, w, c, zx, mul, stride, pad, dil, bias=None, residual=None, relu=False, out_q=None):
    """x [N, H, W, Cp], w [kh, kw, Cp] int8 codes of c channels, residual [N, OH, OW, c] -> (I int64 [M, Cp], v float32 [N, OH, OW, c],
    codes int8 [N, OH, OW, Cp] or None); out_q = (sy, zy, qmin, qmax, rounding, q_nan)."""
    kh, kw, cp = w.shape
    a, (oh, ow) = gather(x, kh, kw, stride, pad, dil, zx)
    i = ((a.reshape(len(a), kh * kw, cp).astype(np.int64) - zx) * w.reshape(1, kh * kw, cp).astype(np.int64)).sum(1)
    assert np.abs(i).max(initial=0) < 2 ** 31
    with np.errstate(all='ignore'):
        v = i[:, :c].astype(f32) * mul.astype(f32)[None, :]
        if bias is not None: v = v + bias[None, :]
        if residual is not None: v = v + residual.reshape(-1, c)
        if relu: v = np.where(v > 0, v, np.where(np.isnan(v), v, f32(0)))
    if out_q is None: return i, v.reshape(len(x), oh, ow, c), None
    q = np.full((len(a), cp), out_q[1], np.int8)
    q[:, :c] = to_int(v, *out_q)
    return i, v.reshape(len(x), oh, ow, c), q.reshape(len(x), oh, ow, cp)


# (C, H, W, kh, kw, stride, padding, dilation): one block and 2 x 2 tiles with one live row / column at the edge; two blocks, stride 2;
# C % 4 != 0 (scalar stores), 5 x 5, a stride per axis; dilation on one axis, three blocks; one tap, a block with one live channel; a
# window larger than the image
GEOMETRIES = [(32, 9, 9, 3, 3, (1, 1), (1, 1), (1, 1)), (40, 17, 9, 3, 3, (2, 2), (1, 1), (1, 1)), (3, 9, 10, 5, 5, (1, 2), (2, 2), (1, 1)),
              (70, 7, 12, 3, 3, (1, 1), (2, 1), (2, 1)), (33, 5, 5, 1, 1, (1, 1), (0, 0), (1, 1)), (32, 6, 6, 7, 7, (2, 2), (3, 3), (1, 1))]
