"""The arithmetic contract of ppqhip_conv1x1 (include/ppq_hip.h) restated in NumPy, for the tests of the kernel:

    y[n, o, p] = (((+0 (+) w[o,0] x[n,0,src p]) (+) w[o,1] x[n,1,src p]) ... ) [+ bias[o]]

where every (+) is ONE float32 fused multiply-add (a single rounding of the exact a * b + c), k ascends, and the bias is a separate
float32 add after the chain.  ``fma32`` is that fused operation, vectorised:
  * the product of two float32 is exact in float64 (24 + 24 significant bits);
  * one float64 add follows; TwoSum gives its rounding error exactly;
  * the float64 sum is rounded to float32; only when it lies exactly on a float32 tie can the discarded error change the result,
    and then its sign says which neighbour the exact value is nearer to.  (An exact value on the other side of a tie from the
    float64 sum is impossible: ties are float64 numbers, and the sum is the float64 nearest to the exact value.)
"""
import numpy as np


def fma32(a, b, c):
    """float32 fmaf(a, b, c), elementwise with broadcasting, correctly rounded (NaN / Inf as IEEE 754 gives them)."""
    a64, b64, c64 = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all='ignore'):
        p = a64 * b64                                   # exact
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)                 # TwoSum: p + c == s + e exactly
        r = s.astype(np.float32)
        d = s - r.astype(np.float64)                    # exact; 0 when s is a float32 number
        other = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = (d != 0) & np.isfinite(other) & np.isfinite(r) & ((r.astype(np.float64) + other.astype(np.float64)) * 0.5 == s)
        toward_other = tie & (e != 0) & ((e > 0) == (d > 0))      # exact value beyond the tie, on other's side
        out = np.where(toward_other, other, r)          # (an error on r's side, or none, leaves the tie's own choice / r)
    return out.astype(np.float32)


def gather(x: np.ndarray, stride: int) -> np.ndarray:
    """x[n, c, ::stride, ::stride] flattened to [n, c, ho * wo]: what src(p) reads."""
    g = x[:, :, ::stride, ::stride]
    return np.ascontiguousarray(g).reshape(x.shape[0], x.shape[1], -1), g.shape[2], g.shape[3]


def conv1x1_reference(x: np.ndarray, w: np.ndarray, bias=None, stride: int = 1) -> np.ndarray:
    """The contract: x [n, c, h, w], w [o, c] (or [o, c, 1, 1]) float32 -> y [n, o, ho, wo] float32."""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32).reshape(w.shape[0], -1)
    xs, ho, wo = gather(x, stride)
    n, c, p = xs.shape
    acc = np.zeros((n, w.shape[0], p), dtype=np.float32)
    for k in range(c):
        acc = fma32(w[None, :, k, None], xs[:, None, k, :], acc)
    if bias is not None:
        with np.errstate(all='ignore'):
            acc = (acc + np.asarray(bias, dtype=np.float32)[None, :, None]).astype(np.float32)
    return acc.reshape(n, w.shape[0], ho, wo)


def conv1x1_float64(x: np.ndarray, w: np.ndarray, stride: int = 1):
    """(exact-ish float64 result, sum_k |w| |x|) for the error bound gamma_c * sum |w| |x|, gamma_c = c u / (1 - c u), u = 2^-24."""
    w64 = np.asarray(w, dtype=np.float64).reshape(w.shape[0], -1)
    xs, ho, wo = gather(np.asarray(x, dtype=np.float64), stride)
    y = np.einsum('ok,nkp->nop', w64, xs)
    mag = np.einsum('ok,nkp->nop', np.abs(w64), np.abs(xs))
    return y.reshape(y.shape[0], y.shape[1], ho, wo), mag.reshape(y.shape[0], y.shape[1], ho, wo)


def gamma(c: int) -> float:
    u = 2.0 ** -24
    return c * u / (1.0 - c * u)
