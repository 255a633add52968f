"""The linear INT8 kernels on the GPU (ppq_amd/csrc/int8_gemm.hip, int8_conv.hip) against the NumPy oracle
(tests/int8_reference.py) with == on bits.  The chunk of the K loop is 128 bytes: K = 96 / 160 lie 32 around it, K = 300 is two chunks
and a tail of two blocks."""
import numpy as np
import pytest
import torch

import int8_reference as R
from ppq_amd import CUDA, Int8Tensor, int8_conv2d_packed, int8_matmul, int8_quantize
from test_host_int8 import MN, SX, accuracy_statement, bits, config, pair, run_conv, run_gemm, stored

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIGNED, UNSIGNED = (0.25, -3, -128, 127), (0.25, 131, 0, 255)
# every variant beside the plain round: (name, keywords of run_gemm, extra (M, N))
VARIANTS = [('no bias', dict(bias=False), []), ('residual', dict(residual=True), []), ('relu', dict(relu=True), []),
            ('int8 only', dict(out=UNSIGNED, out_float=False), [(17, 63)]), ('both outputs', dict(out=SIGNED, out_float=True), [(17, 63)]),
            ('whole tail', dict(residual=True, relu=True, out=UNSIGNED, out_float=True), [(17, 63)]),
            ('sums null', dict(zx=0), [(15, 17)])]


@pytest.mark.parametrize('k', [1, 31, 32, 33, 96, 160, 300])
def test_gemm_on_every_tile_edge(k):
    for m, n in MN: run_gemm(DEV, True, m, n, k)


@pytest.mark.parametrize('name,kw,extra', VARIANTS, ids=[v[0] for v in VARIANTS])
def test_gemm_variants(name, kw, extra):
    kw = dict(kw, out=config(*kw['out'], rounding=4)) if 'out' in kw else kw
    for k in (33, 300):
        for m, n in [(1, 1), (63, 65), (65, 130)] + extra: run_gemm(DEV, True, m, n, k, **kw)


@pytest.mark.parametrize('v', range(4))
def test_routing_of_every_k_byte(v):
    """One non-zero odd code per row of A, at byte (7 i + v) % 32 of block (i + v) % 4; the weights are signed powers of two that move
    with (column, byte) -- an odd code times 2^e names its row and its byte's e -- and every column has its own scale."""
    m = n = 32; k = 128; i = np.arange(m)
    a = np.zeros((m, k), np.int8)
    a[i, 32 * ((i + v) % 4) + (7 * i + v) % 32] = np.where(i % 2, -(2 * i + 1), 2 * i + 1)
    kk = np.arange(k)[None, :]
    b = ((1 << ((kk + 3 * i[:, None] + v) % 7)) * np.where((kk // 7 + i[:, None]) % 2, -1, 1)).astype(np.int8)
    sw = np.exp(np.arange(n) / 7).astype(np.float32)
    A, B = pair(DEV, a, b, (m, k), (n, k), 0, sw)
    _, want, _ = R.layer(a, b, 0, np.float32(SX) * sw)
    assert len(np.unique(want)) == m * n and np.array_equal(bits(int8_matmul(A, B)), want.view(np.int32))


@pytest.mark.parametrize('zx', [0, 5])
def test_the_accumulator_chain_and_the_conversion(zx):
    """K = 4096: |I| = 2^26 and its neighbour, and an odd I above 2^24, which float32(I) rounds."""
    k = 4096
    a, b = np.full((2, k), -128, np.int8), np.full((3, k), -128, np.int8)
    b[1] = 127; b[2, 0] = 1; a[1, 0] = -127
    A, B = pair(DEV, a, b, (2, k), (3, k), zx, np.ones(3, np.float32))
    i, want, _ = R.layer(a, b, zx, np.full(3, SX, np.float32))
    if zx == 0: assert i[0, 0] == 2 ** 26 and i[0, 1] == -127 * 2 ** 19 and i[1, 2] % 2 == 1
    assert (i.astype(np.float32).astype(np.int64) != i).any() and np.abs(i).max() > 2 ** 24
    assert np.array_equal(bits(int8_matmul(A, B)), want.view(np.int32))


@pytest.mark.parametrize('g', R.GEOMETRIES, ids=str)
def test_conv_geometries(g):
    run_conv(DEV, True, g, tail=g[0] == 32)
    if g[0] == 40: run_conv(DEV, True, g, zx=0)                                          # sums null: no correction, zero bytes in the padding


@pytest.mark.parametrize('grid', [SIGNED, UNSIGNED], ids=['signed', 'unsigned'])
@pytest.mark.parametrize('rounding', [0, 1, 2, 3, 4, 6])
def test_requantisation_is_linear_quantize_to_int(rounding, grid):
    """The int8 output == LinearQuantize_ToInt (through int8_quantize) of the same launch's float32 output, padding included; the
    residual carries ties of the grid (sy = 0.25), values far past both ends, infinities and a NaN onto I = 0 in row 0."""
    m, n, k = 17, 40, 64
    rng = np.random.default_rng(rounding)
    a, b = R.operands(rng, m, k, 3), R.operands(rng, n, k)
    a[0] = 3                                                                             # x - zx = 0: row 0 of v is the residual itself
    res = (rng.standard_normal((m, n)) * 30).astype(np.float32)
    res[0] = np.resize(np.array([0.125, -0.125, 0.375, -0.375, 31.875, -32.125, 1e9, -1e9, np.inf, -np.inf, np.nan, -0.0, 1e30, 2.0 ** 22 + 0.125], np.float32), n)
    A, B = pair(DEV, a, b, (m, k), (n, k), 3, np.full(n, 0.01, np.float32))
    out, tr = config(*grid, rounding=rounding), torch.from_numpy(res).to(DEV)
    for residual, relu in ((True, False), (False, True), (True, True)):
        y, p = int8_matmul(A, B, None, tr if residual else None, relu, out, True)
        want = int8_quantize(y, out)
        assert torch.equal(p.values, want.values) and (p.zero_point, p.qmin, p.qmax, p.rounding) == (want.zero_point, want.qmin, want.qmax, want.rounding)
        assert (p.values[:, n:] == p.zero_point).all() and torch.equal(int8_matmul(A, B, None, tr if residual else None, relu, out, False).values, p.values)
        _, v, q = R.layer(a, b, 3, np.float32(SX) * np.full(n, 0.01, np.float32), None, res if residual else None, relu, stored(out))
        assert np.array_equal(bits(y), v.view(np.int32)) and np.array_equal(p.values.cpu().numpy(), q)
        if residual and not relu: assert len(np.unique(q[0, :n])) > 3 and q.min() == stored(out)[2] and q.max() == stored(out)[3]


def test_a_chain_of_two_launches():
    """The int8 output of one launch, fed to the next as its activation, gives the bits of quantising the float32 output."""
    c, h, w, kh, kw, stride, pad, dil, o = R.GEOMETRIES[1]
    rng = np.random.default_rng(4)
    x, w1, w2 = R.operands(rng, 2 * h * w, c, 5).reshape(2, h, w, -1), R.operands(rng, o * kh * kw, c).reshape(o, kh, kw, -1), R.operands(rng, 33, o).reshape(33, 1, 1, -1)
    X, W1 = pair(DEV, x, w1, (2, c, h, w), (o, c, kh, kw), 5, np.full(o, 0.01, np.float32))
    _, W2 = pair(DEV, x, w2, (2, c, h, w), (33, o, 1, 1), 5, np.full(33, 0.02, np.float32))
    mid = config(0.5, 140, 0, 255, rounding=1)
    y, p = int8_conv2d_packed(X, W1, None, stride, pad, dil, relu=True, out_config=mid, out_float=True)
    assert torch.equal(bits_t(int8_conv2d_packed(p, W2)), bits_t(int8_conv2d_packed(int8_quantize(y, mid, 1), W2)))


bits_t = lambda t: t.contiguous().view(torch.int32)


def test_the_bindings_refuse_what_the_kernels_cannot_take():
    a = torch.zeros(4, 64, dtype=torch.int8, device=DEV)
    mul, sums = torch.ones(4, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    for call, msg in ((lambda: CUDA.Int8Matmul(a[:, :40], a, sums, 1, mul), 'must be contiguous'), (lambda: CUDA.Int8Matmul(a, a, None, 1, mul), 'sums is required'),
                      (lambda: CUDA.Int8Matmul(a.cpu(), a, sums, 1, mul), 'not on the GPU'), (lambda: CUDA.Int8Matmul(a, a, sums, 1, mul, out_float=False), 'no output'),
                      (lambda: CUDA.Int8Matmul(a, a[:, :32].contiguous(), sums, 1, mul), 'differ in their last axis'),
                      (lambda: CUDA.Int8Matmul(a, a, sums, 1, mul, out_q=(1.0, 0, -128, 127, 5, 0)), 'rounding policy 5 has no tensor form')):
        with pytest.raises(RuntimeError, match=msg): call()


def test_accuracy_statement():
    accuracy_statement(DEV, True)
