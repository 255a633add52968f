"""int8_bmm on the GPU (ppq_amd/csrc/int8_bmm.hpp) against the NumPy oracle (tests/int8_bmm_reference.py) with ==
on bits.  The tile is 64 x 64 and a chunk of K 128 bytes: (65, 70) and K = 128 / 160 lie on both sides of them; a B packed along N is
staged in 4 x 4 blocks, which K = 1, 33 and 197 cut."""
import numpy as np
import pytest
import torch

import int8_bmm_reference as RB
from ppq_amd import CUDA, Int8Tensor, int8_bmm, int8_matmul
from test_gpu_int8 import SIGNED, UNSIGNED
from test_host_int8 import bits, config, stored
from test_host_int8_bmm import MUL, SA, case, run, tensors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAYOUTS = pytest.mark.parametrize('transpose_b', [True, False], ids=['a.bT', 'a.b'])
TAILS = [dict(residual=True), dict(relu=True), dict(out=UNSIGNED, out_float=False), dict(out=SIGNED, out_float=True),
         dict(residual=True, relu=True, out=UNSIGNED, out_float=True)]


def check(a, b, transpose_b, n, k, za, zb):
    """The float32 result of int8_bmm on raw codes against the oracle; returns the oracle's integer sums and values."""
    A, B = tensors(DEV, a, b, transpose_b, n, k, za, zb)
    i, want, _ = RB.bmm(a, b, transpose_b, n, za, zb, MUL)
    assert np.array_equal(bits(int8_bmm(A, B, transpose_b)), want.view(np.int32))
    return i, want


@LAYOUTS
@pytest.mark.parametrize('za,zb', [(0, 0), (-7, 0), (0, 5), (-7, 5)])
@pytest.mark.parametrize('batch', [1, 3])
def test_every_edge_of_the_tile_and_of_the_k_loop(batch, za, zb, transpose_b):
    for m, n in ((1, 1), (15, 17), (33, 48), (65, 70)):
        for k in (1, 33, 128, 160, 197): run(DEV, True, batch, m, n, k, transpose_b, za, zb)


@LAYOUTS
@pytest.mark.parametrize('v', range(4))
def test_routing_of_every_k_byte(v, transpose_b):
    """One non-zero code per row of a at byte 32 i + 8 v + (3 i + v) % 8, odd and no multiple of 3, its own for every (batch, row); b
    holds +-2^e, -128 and 96 = 3 * 32, sixteen values that move with (batch, column, k): a product names its batch and row by its odd
    part, its column and byte by the rest."""
    batch, m, n, k = 2, 16, 16, 512
    g, i, kk = np.arange(batch)[:, None, None], np.arange(m)[None, :, None], np.arange(k)
    odd = np.array([c for c in range(1, 128, 2) if c % 3])[:batch * m].reshape(batch, m)
    a = np.zeros((batch, m, k), np.int8)
    a[g[:, :, 0], i[:, :, 0], 32 * i[:, :, 0] + 8 * v + (3 * i[:, :, 0] + v) % 8] = np.where((g[:, :, 0] + i[:, :, 0]) % 2, -odd, odd)
    vals = np.array([s << e for e in range(7) for s in (1, -1)] + [-128, 96], np.int8)
    bt = vals[(i + 3 * kk + 5 * g + v) % 16]                                              # [batch, n, k]
    b = bt if transpose_b else np.concatenate([bt.transpose(0, 2, 1), np.zeros((batch, k, 16), np.int8)], 2)
    _, want = check(a, b, transpose_b, n, k, 0, 0)
    assert len(np.unique(want)) == batch * m * n


@LAYOUTS
def test_the_zero_point_algebra_at_the_int32_limit(transpose_b):
    """K = 32768, the longest the host admits, every term of the algebra at its largest: |I| = 32768 * 255 * 255."""
    k = 32768
    a, b = np.full((1, 2, k), -128, np.int8), np.full((1, 3, k) if transpose_b else (1, k, 32), -128, np.int8)
    if not transpose_b: b[..., 3:] = 127
    i, _ = check(a, b, transpose_b, 3, k, 127, 127)
    assert (np.abs(i) == 2130739200).all()


@LAYOUTS
@pytest.mark.parametrize('za,zb', [(0, 0), (5, -3)])
def test_the_accumulator_chain_and_the_conversion(za, zb, transpose_b):
    """The K = 4096 pair of test_gpu_int8: sums above 2^24 that float32(I) rounds."""
    k = 4096
    a, bt = np.full((1, 2, k), -128, np.int8), np.full((1, 3, k), -128, np.int8)
    bt[0, 1] = 127; bt[0, 2, 0] = 1; a[0, 1, 0] = -127
    b = bt if transpose_b else np.concatenate([bt.transpose(0, 2, 1), np.full((1, k, 29), zb, np.int8)], 2)
    i, _ = check(a, b, transpose_b, 3, k, za, zb)
    assert (i.astype(np.float32).astype(np.int64) != i).any() and np.abs(i).max() > 2 ** 24


@LAYOUTS
@pytest.mark.parametrize('kw', TAILS, ids=['residual', 'relu', 'int8 only', 'both outputs', 'whole tail'])
def test_the_tail(kw, transpose_b):
    kw = dict(kw, out=config(*kw['out'], rounding=4)) if 'out' in kw else kw
    for m, n, k in ((17, 33, 300), (65, 70, 33)): run(DEV, True, 3, m, n, k, transpose_b, **kw)


@LAYOUTS
def test_requantisation_of_ties_infinities_and_nan(transpose_b):
    """The residual row of test_gpu_int8's requantisation test onto I = 0 in row 0 of every batch: ties of the grid, both ends,
    infinities, NaN, -0."""
    batch, m, n, k = 2, 17, 40, 64
    a, b, res = case(batch, m, n, k, transpose_b, 3, -2, residual=True)
    a[:, 0] = 3
    res[:, 0] = np.resize(np.array([0.125, -0.125, 0.375, -0.375, 31.875, -32.125, 1e9, -1e9, np.inf, -np.inf, np.nan, -0.0, 1e30, 2.0 ** 22 + 0.125], np.float32), n)
    A, B = tensors(DEV, a, b, transpose_b, n, k, 3, -2)
    out = config(*UNSIGNED, rounding=3)
    for relu in (False, True):
        y, p = int8_bmm(A, B, transpose_b, torch.from_numpy(res).to(DEV), relu, out, True)
        _, v, q = RB.bmm(a, b, transpose_b, n, 3, -2, MUL, res, relu, stored(out))
        assert np.array_equal(bits(y), v.view(np.int32)) and np.array_equal(p.values.cpu().numpy(), q)


def test_the_bits_of_the_family():
    """One batch against a symmetric b is a linear layer: the bits of int8_matmul on b as a weight with sums."""
    m, n, k = 33, 48, 1000
    a, b, res = case(1, m, n, k, True, -7, 0, residual=True)
    A, B = tensors(DEV, a, b, True, n, k, -7, 0)
    W = Int8Tensor(B.values[0], (n, k), 1, B.scale, 0, -128, 127, 0, B.values[0].sum(1, dtype=torch.int32))
    A2 = Int8Tensor(A.values[0], (m, k), 1, A.scale, -7, -128, 127, 0)
    out, tr = config(*UNSIGNED, rounding=4), torch.from_numpy(res).to(DEV)
    (y, p), (y2, p2) = int8_bmm(A, B, True, tr, True, out, True), int8_matmul(A2, W, None, tr[0], True, out, True)
    assert torch.equal(y[0].view(torch.int32), y2.contiguous().view(torch.int32)) and torch.equal(p.values[0], p2.values)


def test_refusals_that_need_the_device():
    long, mul = torch.zeros(1, 1, 32800, dtype=torch.int8, device=DEV), torch.ones(1, device=DEV)
    T = Int8Tensor(long, (1, 1, 32800), 2, torch.tensor(SA, device=DEV), 0, -128, 127, 0)
    with pytest.raises(RuntimeError, match='int8_bmm: a padded reduction length of 32800: more than 32768'): int8_bmm(T, T, True)
    with pytest.raises(RuntimeError, match='a padded reduction length of 32800: more than 32768'): CUDA.Int8Bmm(long, long, True, 0, 0, mul)
    with pytest.raises(RuntimeError, match='A and B differ in their batch: 2 and 3'): CUDA.Int8Bmm(long[:, :, :64].expand(2, 1, 64).contiguous(), long[:, :, :64].expand(3, 1, 64).contiguous(), True, 0, 0, mul)
