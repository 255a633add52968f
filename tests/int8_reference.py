"""NumPy oracle of the linear INT8 contract: the integer sum in int64, every later step in np.float32, the
rounding table of ppq_tensor_round, the gather of the implicit GEMM -- and the operands the host and the GPU tests both run."""
import numpy as np

f32 = np.float32
half = f32(0.5)
ROUND = {0: np.rint, 1: lambda v: np.floor(v + half), 2: lambda v: np.ceil(v - half), 3: lambda v: np.sign(v) * np.ceil(np.abs(v) - half),
         4: lambda v: np.sign(v) * np.floor(np.abs(v) + half), 6: np.ceil}
ceil32 = lambda k: (k + 31) // 32 * 32


def to_int(v, sy, zy, qmin, qmax, rounding, q_nan=0):
    """LinearQuantize_ToInt: clamp(round(v / sy) + zy, qmin, qmax) in float32, truncated; NaN gives q_nan."""
    with np.errstate(all='ignore'):
        t = ROUND[rounding](v / f32(sy)).astype(f32) + f32(zy)
        t = np.where(t > qmax, f32(qmax), np.where(t < qmin, f32(qmin), t))
    return np.where(np.isnan(t), q_nan, np.nan_to_num(t)).astype(np.int8)


def layer(a, b, zx, mul, bias=None, residual=None, relu=False, out_q=None):
    """a [M, Kp], b [N, Kp] int8 codes -> (I int64, v float32 [M, N], codes int8 [M, ceil32(N)] or None); out_q = (sy, zy, qmin, qmax, rounding, q_nan)."""
    i = (a.astype(np.int64) - zx) @ b.astype(np.int64).T
    assert np.abs(i).max(initial=0) < 2 ** 31
    with np.errstate(all='ignore'):
        v = i.astype(f32) * mul.astype(f32)[None, :]
        if bias is not None: v = v + bias[None, :]
        if residual is not None: v = v + residual
        if relu: v = np.where(v > 0, v, np.where(np.isnan(v), v, f32(0)))
    if out_q is None: return i, v, None
    q = np.full((len(a), ceil32(len(b))), out_q[1], np.int8)
    q[:, :len(b)] = to_int(v, *out_q)
    return i, v, q


def gather(x, kh, kw, stride, pad, dil, zx):
    """x [N, H, W, Cp] int8 -> the A operand [N OH OW, kh kw Cp] of the implicit GEMM, a tap in the padding holding the code zx; (OH, OW)."""
    (sh, sw), (ph, pw), (dh, dw) = stride, pad, dil
    xp = np.pad(x, ((0, 0), (ph, ph), (pw, pw), (0, 0)), constant_values=zx)
    oh, ow = (xp.shape[1] - dh * (kh - 1) - 1) // sh + 1, (xp.shape[2] - dw * (kw - 1) - 1) // sw + 1
    taps = [xp[:, ky * dh: ky * dh + (oh - 1) * sh + 1: sh, kx * dw: kx * dw + (ow - 1) * sw + 1: sw] for ky in range(kh) for kx in range(kw)]
    return np.concatenate(taps, axis=-1).reshape(len(x) * oh * ow, -1), (oh, ow)


def operands(rng, rows, k, zero_point=0):
    """Uniform random codes over the full -128 .. 127 as [rows, ceil32(k)], the padding holding the zero point."""
    codes = np.full((rows, ceil32(k)), zero_point, np.int8)
    codes[:, :k] = rng.integers(-128, 128, (rows, k))
    return codes


# (C, H, W, kh, kw, stride, padding, dilation, O): 1x1; 3x3 pad 1; stride 2; dilation 2; the 7x7 stem on 3 channels; a non-square kernel
# and image with channel padding
GEOMETRIES = [(64, 6, 6, 1, 1, (1, 1), (0, 0), (1, 1), 70), (32, 7, 7, 3, 3, (1, 1), (1, 1), (1, 1), 64), (32, 9, 9, 3, 3, (2, 2), (1, 1), (1, 1), 7),
              (32, 7, 7, 3, 3, (1, 1), (2, 2), (2, 2), 70), (3, 9, 9, 7, 7, (2, 2), (3, 3), (1, 1), 64), (40, 7, 5, 1, 3, (1, 1), (0, 1), (1, 1), 7)]
