"""The skinny linear INT8 GEMM on the GPU (ppq_amd/csrc/int8_skinny.hpp), int8 and packed INT4 weights, against
the NumPy oracle (tests/int8_reference.py) with == on bits; every call here passes skinny=True.  A piece of the K loop is 64 int8 or
128 int4 codes, a round of the four waves 256 / 512, and a step of all four waves (4 kU pieces) 1024 codes for both codecs: the K
values lie on both sides of the half piece, the piece, the round and the step."""
import numpy as np
import pytest
import torch

import int8_reference as R
from ppq_amd import CUDA, int4_pack, int8_matmul
from test_gpu_int8 import SIGNED, UNSIGNED, VARIANTS
from test_host_int8 import SX, bits, config, pair, stored

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CODECS = ['int8', 'int4']
EDGES = [(1, 1), (15, 17), (16, 16), (17, 33), (33, 48), (64, 70)]
KS = [('int8', k) for k in (1, 33, 64, 96, 256, 288, 1000, 1056)] + [('int4', k) for k in (1, 33, 128, 160, 512, 544, 1000, 1056)]
packed = lambda B, codec: int4_pack(B) if codec == 'int4' else B
same = lambda got, want: torch.equal(got[0].contiguous().view(torch.int32), want[0].contiguous().view(torch.int32)) and torch.equal(got[1].values, want[1].values)


def case(codec, m, n, k, zx, residual=False):
    """Random operands of one layer (an int4 weight's codes in -8 .. 7), per-column scales, a bias and a residual."""
    rng = np.random.default_rng(1000 * m + k)
    a, b = R.operands(rng, m, k, zx), R.operands(rng, n, k) >> (4 if codec == 'int4' else 0)
    sw, tb = (rng.random(n) * 0.01 + 0.005).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    return a, b, sw, tb, (rng.standard_normal((m, n)) * 40).astype(np.float32) if residual else None


def run(codec, m, n, k, zx=-7, bias=True, residual=False, relu=False, out=None, out_float=None):
    """One layer on the skinny kernel against the oracle, on bits: the float32 result and the codes with their padding columns."""
    a, b, sw, tb, tr = case(codec, m, n, k, zx, residual)
    A, B = pair(DEV, a, b, (m, k), (n, k), zx, sw)
    if zx == 0: B.sums = None
    dv = lambda v: torch.from_numpy(v).to(DEV) if v is not None else None
    got = int8_matmul(A, packed(B, codec), dv(tb) if bias else None, dv(tr), relu, out, out_float, skinny=True)
    _, v, q = R.layer(a, b, zx, np.float32(SX) * sw, tb if bias else None, tr, relu, stored(out) if out is not None else None)
    y, p = (got, None) if out is None else (got if out_float else (None, got))
    if y is not None: assert np.array_equal(bits(y), v.view(np.int32))
    if p is not None: assert np.array_equal(p.values.cpu().numpy(), q) and (p.shape, p.axis, p.zero_point) == ((m, n), 1, stored(out)[1])


@pytest.mark.parametrize('codec,k', KS)
def test_every_edge_of_the_tile_and_of_the_k_loop(codec, k):
    for m, n in EDGES: run(codec, m, n, k)


@pytest.mark.parametrize('codec', CODECS)
@pytest.mark.parametrize('v', range(4))
def test_routing_of_every_k_byte(v, codec):
    """One odd non-zero code per row of A at byte 32 i + 8 v + (3 i + v) % 8: over the rows and v every piece (so every wave), every
    K-group, both halves of a 16-byte load and, for int4, every dword and nibble place.  The weights are signed powers of two that move
    with (column, byte) and every column has its own scale: an output names its row, its column and its byte."""
    m = n = 16; k = 512; i = np.arange(m)
    a = np.zeros((m, k), np.int8)
    a[i, 32 * i + 8 * v + (3 * i + v) % 8] = np.where(i % 2, -(2 * i + 1), 2 * i + 1)
    kk = np.arange(k)[None, :]
    b = ((1 << ((kk + 3 * i[:, None] + v) % (3 if codec == 'int4' else 7))) * np.where((kk // 7 + i[:, None]) % 2, -1, 1)).astype(np.int8)
    sw = np.exp(np.arange(n) / 7).astype(np.float32)
    A, B = pair(DEV, a, b, (m, k), (n, k), 0, sw)
    _, want, _ = R.layer(a, b, 0, np.float32(SX) * sw)
    assert len(np.unique(want)) == m * n and np.array_equal(bits(int8_matmul(A, packed(B, codec), skinny=True)), want.view(np.int32))


@pytest.mark.parametrize('codec', CODECS)
@pytest.mark.parametrize('name,kw,extra', VARIANTS, ids=[v[0] for v in VARIANTS])
def test_the_tail(name, kw, extra, codec):
    kw = dict(kw, out=config(*kw['out'], rounding=4)) if 'out' in kw else kw
    for m, n, k in ((17, 33, 300), (64, 70, 33)): run(codec, m, n, k, **kw)


@pytest.mark.parametrize('codec', CODECS)
def test_requantisation_of_ties_infinities_and_nan(codec):
    """The residual row of test_gpu_int8's requantisation test onto I = 0 in row 0: ties of the grid, both ends, infinities, NaN, -0."""
    m, n, k = 17, 40, 64
    a, b, _, _, res = case(codec, m, n, k, 3, residual=True)
    a[0] = 3
    res[0] = np.resize(np.array([0.125, -0.125, 0.375, -0.375, 31.875, -32.125, 1e9, -1e9, np.inf, -np.inf, np.nan, -0.0, 1e30, 2.0 ** 22 + 0.125], np.float32), n)
    A, B = pair(DEV, a, b, (m, k), (n, k), 3, np.full(n, 0.01, np.float32))
    out = config(*UNSIGNED, rounding=3)
    for relu in (False, True):
        y, p = int8_matmul(A, packed(B, codec), None, torch.from_numpy(res).to(DEV), relu, out, True, skinny=True)
        _, v, q = R.layer(a, b, 3, np.float32(SX) * np.full(n, 0.01, np.float32), None, res, relu, stored(out))
        assert np.array_equal(bits(y), v.view(np.int32)) and np.array_equal(p.values.cpu().numpy(), q)


@pytest.mark.parametrize('codec', CODECS)
def test_the_reduce_across_waves_at_the_int32_limit(codec):
    """K = 65504, the longest the host admits: |I| = 65504 * 128 * 255 = 2 138 050 560 < 2^31 is the sum of four waves' partials, none of
    which may wrap on its own or in the reduce (int4: 16 I = -2 138 050 560 from codes -8 against 127 - -128)."""
    k = 65504
    a, b, zx = (np.full((2, k), -128, np.int8), np.full((3, k), -128, np.int8), 127) if codec == 'int8' else (np.full((2, k), 127, np.int8), np.full((3, k), -8, np.int8), -128)
    A, B = pair(DEV, a, b, (2, k), (3, k), zx, np.ones(3, np.float32))
    i, want, _ = R.layer(a, b, zx, np.full(3, SX, np.float32))
    assert abs(int(i[0, 0])) << (4 if codec == 'int4' else 0) == 2138050560
    assert np.array_equal(bits(int8_matmul(A, packed(B, codec), skinny=True)), want.view(np.int32))


@pytest.mark.parametrize('zx', [0, 5])
def test_the_accumulator_chain_and_the_conversion(zx):
    """The K = 4096 pair of test_gpu_int8: |I| = 2^26 and its neighbour, and an odd I above 2^24, which float32(I) rounds."""
    k = 4096
    a, b = np.full((2, k), -128, np.int8), np.full((3, k), -128, np.int8)
    b[1] = 127; b[2, 0] = 1; a[1, 0] = -127
    A, B = pair(DEV, a, b, (2, k), (3, k), zx, np.ones(3, np.float32))
    i, want, _ = R.layer(a, b, zx, np.full(3, SX, np.float32))
    assert (i.astype(np.float32).astype(np.int64) != i).any() and np.abs(i).max() > 2 ** 24
    assert np.array_equal(bits(int8_matmul(A, B, skinny=True)), want.view(np.int32))


@pytest.mark.parametrize('codec', CODECS)
def test_the_bits_of_the_tile_kernel(codec):
    m, n, k = 33, 48, 1000
    a, b, sw, tb, tr = case(codec, m, n, k, -7, residual=True)
    A, B = pair(DEV, a, b, (m, k), (n, k), -7, sw)
    args = (A, packed(B, codec), torch.from_numpy(tb).to(DEV), torch.from_numpy(tr).to(DEV), True, config(*UNSIGNED, rounding=4), True)
    assert same(int8_matmul(*args, skinny=True), int8_matmul(*args, skinny=False))


def test_more_than_64_rows_are_refused():
    a, b = np.zeros((65, 32), np.int8), np.zeros((4, 32), np.int8)
    A, B = pair(DEV, a, b, (65, 32), (4, 32), 0, np.ones(4, np.float32))
    with pytest.raises(RuntimeError, match=r'skinny=True takes M = 1 \.\. 64 rows, got M = 65'): int8_matmul(A, B, skinny=True)
    with pytest.raises(RuntimeError, match='M = 65: the skinny kernel takes at most 64 rows'):
        CUDA.Int8MatmulSkinny(A.values, B.values, None, 0, torch.ones(4, device=DEV))
