"""NumPy oracle of int8_bmm: per batch the layer of int8_reference on (b - zb) laid out as a weight [N, Kp]."""
import numpy as np

import int8_reference as R


def bmm(a, b, transpose_b, n, za, zb, mul, residual=None, relu=False, out_q=None):
    """a [B, M, Kp]; b [B, N, Kp] (transpose_b) or [B, K, Np] with n live columns -> (I int64, v float32 [B, M, n], codes or None)."""
    out = []
    for g in range(len(a)):
        w = np.zeros((n, a.shape[2]), np.int64)
        if transpose_b: w[:] = b[g].astype(np.int64) - zb
        else: w[:, :b.shape[1]] = b[g, :, :n].T.astype(np.int64) - zb
        out.append(R.layer(a[g], w, za, np.full(n, mul, np.float32), None, residual[g] if residual is not None else None, relu, out_q))
    i, v, q = zip(*out)
    return np.stack(i), np.stack(v), np.stack(q) if out_q is not None else None
