"""int8_bmm without a GPU: the torch arm against the NumPy oracle on bits, the refusals by message, the C entry
point's argument checks on host pointers -- and the operands the GPU tests run too."""
import numpy as np
import pytest
import torch

import int8_bmm_reference as RB
import int8_reference as R
from ppq_amd import Int8Tensor, _lib, int8_bmm
from test_host_int8 import bits, config, stored

SA, SB = 0.02, 0.015
MUL = np.float32(SA) * np.float32(SB)


def tensors(dev, a, b, transpose_b, n, k, za, zb):
    """Int8Tensors of raw codes a [B, M, Kp] and b [B, N, Kp] / [B, K, Np]: two activations with the scales SA, SB."""
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    return (Int8Tensor(t(a), a.shape[:2] + (k,), 2, torch.tensor(SA, device=dev), za, -128, 127, 0),
            Int8Tensor(t(b), (len(b), n, k) if transpose_b else (len(b), k, n), 2, torch.tensor(SB, device=dev), zb, -128, 127, 0))


def case(batch, m, n, k, transpose_b, za, zb, residual=False):
    """Uniform random codes over -128 .. 127, the padding holding the zero points; a residual."""
    rng = np.random.default_rng(1000 * m + k + batch)
    a = R.operands(rng, batch * m, k, za).reshape(batch, m, -1)
    b = R.operands(rng, batch * n, k, zb).reshape(batch, n, -1) if transpose_b else R.operands(rng, batch * k, n, zb).reshape(batch, k, -1)
    return a, b, (rng.standard_normal((batch, m, n)) * 40).astype(np.float32) if residual else None


def run(dev, use_kernels, batch, m, n, k, transpose_b, za=-7, zb=5, residual=False, relu=False, out=None, out_float=None):
    """One case on ``dev`` against the oracle, on bits: the float32 result and the codes with their padding columns."""
    a, b, tr = case(batch, m, n, k, transpose_b, za, zb, residual)
    A, B = tensors(dev, a, b, transpose_b, n, k, za, zb)
    got = int8_bmm(A, B, transpose_b, torch.from_numpy(tr).to(dev) if residual else None, relu, out, out_float, use_kernels=use_kernels)
    _, v, q = RB.bmm(a, b, transpose_b, n, za, zb, MUL, tr, relu, stored(out) if out is not None else None)
    y, p = (got, None) if out is None else (got if out_float else (None, got))
    if y is not None: assert np.array_equal(bits(y), v.view(np.int32))
    if p is not None: assert np.array_equal(p.values.cpu().numpy(), q) and (p.shape, p.axis, p.zero_point) == ((batch, m, n), 2, stored(out)[1])


@pytest.mark.parametrize('transpose_b', [True, False])
def test_torch_arm_is_the_oracle(transpose_b):
    for m, n, k in ((1, 1, 1), (15, 17, 33), (33, 48, 160), (65, 70, 197)): run('cpu', False, 3, m, n, k, transpose_b)
    run('cpu', False, 2, 17, 33, 300, transpose_b, 0, 5, residual=True, relu=True, out=config(0.25, -3, -128, 127, 4), out_float=True)
    run('cpu', False, 1, 17, 33, 33, transpose_b, -7, 0, out=config(0.25, 131, 0, 255), out_float=False)


def test_refusals():
    a, b, _ = case(2, 4, 8, 40, True, 3, -2)
    A, B = tensors('cpu', a, b, True, 8, 40, 3, -2)
    other = lambda t, **kw: Int8Tensor(*[kw.get(s, getattr(t, s)) for s in ('values', 'shape', 'axis', 'scale', 'zero_point', 'qmin', 'qmax', 'rounding')])
    long = Int8Tensor(torch.zeros(1, 1, 32800, dtype=torch.int8), (1, 1, 32800), 2, A.scale, 0, -128, 127, 0)
    for call, msg in ((lambda: int8_bmm(A.values, B, True), 'a: expected an Int8Tensor'), (lambda: int8_bmm(A, other(B, values=B.values.to(torch.uint8)), True), 'b: the codes are torch.uint8'),
                      (lambda: int8_bmm(A, other(B, scale=torch.ones(8)), True), 'b must be quantised per tensor'),
                      (lambda: int8_bmm(A, other(B, axis=1), True), r'b \[2, 8, 40\] must be at least 2-d and packed along its last axis, not along axis 1'),
                      (lambda: int8_bmm(A, B, False), 'K mismatch: a reduces over 40, b over 8'),
                      (lambda: int8_bmm(A, other(B, values=B.values[:1], shape=(1, 8, 40)), True), 'batch mismatch'),
                      (lambda: int8_bmm(A, other(B, values=B.values.to('meta')), True), 'a is on cpu, b on meta'),
                      (lambda: int8_bmm(long, long, True, use_kernels=False), 'a padded reduction length of 32800: more than 32768'),
                      (lambda: int8_bmm(A, B, True, torch.zeros(2, 4, 7), use_kernels=False), r'residual of shape \[2, 4, 7\], expected \[2, 4, 8\]'),
                      (lambda: int8_bmm(A, B, True, torch.zeros(2, 4, 8, dtype=torch.float64), use_kernels=False), 'residual must be a float32 tensor'),
                      (lambda: int8_bmm(A, B, True, torch.zeros(2, 4, 8, device='meta'), use_kernels=False), 'residual is on meta')):
        with pytest.raises((RuntimeError, TypeError), match='int8_bmm: ' + msg): call()


def test_c_entry_point_checks_arguments_without_a_device():
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    buf = np.zeros(16384 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    # 2 batches of 2 x 40 x 64: operands below p + 4096, mul there, residual (640 B) at p + 5120, c at p + 6144, q (2 x 2 x 64 B) at p + 7168
    def call(a=p, b=p + 1024, tb=1, za=3, zb=-2, mul=p + 4096, res=p + 5120, c=p + 6144, q=p + 7168, grid=(1.0, 0, -128, 127, 0, 0), batch=2, m=2, n=40, k=64):
        return _lib.lib.ppqhip_int8_bmm(a, b, tb, za, zb, mul, res, 1, c, q, *grid, batch, m, n, k, None), _lib.last_error()

    assert call(c=0, q=0) == (-1, 'int8_bmm: no output: c and q are both null')
    assert call(za=128) == (-1, 'int8_bmm: za 128 / zb -2 is not an int8 zero point') and call(zb=-129)[0] == -1
    assert call(grid=(1.0, 0, -129, 127, 0, 0))[0] == -1 and call(grid=(1.0, 0, -128, 127, 5, 0)) == (-1, 'int8_bmm: rounding policy 5 has no tensor form (ppq_tensor_round)')
    assert call(batch=-1) == (-1, 'int8_bmm: negative size') == call(m=-1) and call(batch=2 ** 31, m=1)[1] == 'int8_bmm: a size above 2^31 - 1' == call(batch=2 ** 30)[1]
    assert call(k=32769) == (-1, 'int8_bmm: a padded reduction length of 32800: more than 32768 could overflow int32') == call(k=32769, tb=0, m=0)
    assert call(a=0) == (-1, 'int8_bmm: null pointer') == call(b=0) == call(mul=0)
    assert call(a=p + 8) == (-1, 'int8_bmm: operands, c and q must be 16-byte aligned') == call(b=p + 1032) == call(c=p + 6144 + 4) == call(q=p + 7168 + 8)
    for out in ({'c': p + 5120}, {'q': p + 4096}, {'q': p + 16}, {'c': p + 1024 + 40 * 64}): assert call(**out) == (-1, 'int8_bmm: an output overlaps an input')
    assert call(q=p + 6144) == (-1, 'int8_bmm: two outputs overlap in memory')
    assert call(batch=0)[0] == 0 and call(m=0)[0] == 0 and call(n=0)[0] == 0              # nothing to launch
