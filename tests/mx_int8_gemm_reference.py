"""The oracle of the MXINT8 GEMM tests: the contract of DESIGN.md section 9.19 in NumPy.  An operand is ``(elements [rows, nb * 32],
scales [rows, nb])``, uint8, as ``mx_quantize(t, 'MXINT8', -1)`` leaves it.  Not a test module."""
import numpy as np

BLOCK = 32


def matmul(a, b, bias=None):
    """(c, exact, s): c float32 [m, n] with the contract's bits (ONE rounding of P 2^e per block, a sequential float32 chain from +0, the
    bias, 0x7fc00000 where a scale code is 0xFF); exact = sum_b P_b 2^e (+ bias) and s = sum_b |t_b| in float64."""
    (ae, sa), (be, sb) = a, b
    nb = sa.shape[1]
    ka = ae.view(np.int8).astype(np.int64).reshape(ae.shape[0], nb, BLOCK)               # 0x80 is -128
    kb = be.view(np.int8).astype(np.int64).reshape(be.shape[0], nb, BLOCK)
    p = np.einsum('mbk,nbk->bmn', ka, kb)
    e = sa.astype(np.int64).T[:, :, None] + sb.astype(np.int64).T[:, None, :] - 266     # [nb, m, n]
    t64 = p.astype(np.float64) * 2.0 ** e                                                # exact
    c = np.zeros(p.shape[1:], np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for t in t64.astype(np.float32): c = c + t
        if bias is not None: c = c + bias.astype(np.float32)
    nan = (sa == 0xff).any(axis=1)[:, None] | (sb == 0xff).any(axis=1)[None, :]
    exact = t64.sum(axis=0) + (0 if bias is None else bias.astype(np.float64))
    return np.where(nan, np.uint32(0x7fc00000), c.view(np.uint32)).view(np.float32), exact, np.abs(t64).sum(axis=0)


def raw_operand(rng, rows: int, k: int, scale_pool):
    """Random element codes over all 256 byte values (a short last block holds zeros, as the export does) and scales from the pool."""
    nb = (k + BLOCK - 1) // BLOCK
    e = rng.integers(0, 256, (rows, nb * BLOCK)).astype(np.uint8)
    e[:, k:] = 0
    return e, rng.choice(np.asarray(scale_pool), (rows, nb)).astype(np.uint8)


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:                            # where want is NaN, got is a NaN
    nan = np.isnan(want)
    return bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and np.isnan(got[nan]).all())
