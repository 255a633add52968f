"""The linear INT8 kernels with a packed INT4 weight on the GPU (ppq_amd/csrc/int4_gemm.hip, int4_conv.hip)
against the NumPy oracle (tests/int8_reference.py) on the unpacked codes with == on bits.  The chunk of the K loop is 128 codes, a
nibble group 8: K = 7 / 8 / 9 lie around a group, 96 / 160 lie 32 around a chunk, K = 300 is two chunks and a tail of two blocks."""
import numpy as np
import pytest
import torch

import int8_reference as R
from ppq_amd import Int4Weight, Int8Tensor, int4_pack, int8_conv2d_packed, int8_matmul
from test_host_int4 import conv_case, run_conv, run_gemm, weights
from test_host_int8 import MN, SX, bits, config, pair

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIGNED, UNSIGNED = (0.25, -3, -128, 127), (0.25, 131, 0, 255)
VARIANTS = [('no bias, sums null', dict(zx=0, bias=False)), ('residual, relu, int8 only', dict(residual=True, relu=True, out=UNSIGNED, out_float=False)),
            ('residual, relu, both outputs', dict(residual=True, relu=True, out=SIGNED, out_float=True))]


@pytest.mark.parametrize('k', [1, 7, 8, 9, 31, 32, 33, 96, 128, 160, 300])
def test_gemm_on_every_tile_and_nibble_edge(k):
    for m, n in MN: run_gemm(DEV, True, m, n, k)


@pytest.mark.parametrize('k', [128, 160])
def test_routing_of_every_nibble(k):
    """A is the identity, so C[k, n] = w[n, k] * mul[n]: every nibble position of a full and of a tail chunk, all 16 codes, a scale
    of its own per column."""
    n = 33
    b = weights(np.random.default_rng(k), n, k)
    sw = np.exp(np.arange(n) / 7).astype(np.float32)
    A, B = pair(DEV, np.eye(k, dtype=np.int8), b, (k, k), (n, k), 0, sw)
    want = b.T.astype(np.float32) * (np.float32(SX) * sw)[None, :]
    assert len(np.unique(b)) == 16 and b.min() == -8 and np.array_equal(want, R.layer(np.eye(k, dtype=np.int8), b, 0, np.float32(SX) * sw)[1])
    assert np.array_equal(bits(int8_matmul(A, int4_pack(B))), want.view(np.int32))


def test_the_accumulator_at_its_bound_and_the_shift():
    """K = 65504, the longest the host admits: 16 I reaches -2 138 050 560, and an odd I has to survive the shift."""
    k = 65504
    a, b = np.full((1, k), 127, np.int8), np.full((3, k), -8, np.int8)
    b[1] = 7; b[2, 12345] = 1
    A, B = pair(DEV, a, b, (1, k), (3, k), -128, np.ones(3, np.float32))
    i, want, _ = R.layer(a, b, -128, np.full(3, SX, np.float32))
    assert 16 * i[0, 0] == -2138050560 and np.abs(i).min() > 2 ** 24 and i[0, 2] % 2 == 1
    assert np.array_equal(bits(int8_matmul(A, int4_pack(B))), want.view(np.int32))
    big = Int4Weight(torch.zeros(1, 32768, dtype=torch.uint8, device=DEV), (1, 65505), 1, B.scale[:1], -8, 7, 0, B.sums[:1])
    with pytest.raises(RuntimeError, match='int8_matmul: a padded reduction length of 65536'):
        int8_matmul(Int8Tensor(torch.zeros(1, 65536, dtype=torch.int8, device=DEV), (1, 65505), 1, A.scale, -128, -128, 127, 0), big)


@pytest.mark.parametrize('name,kw', VARIANTS, ids=[v[0] for v in VARIANTS])
def test_the_tail_on_this_kernel(name, kw):
    kw = dict(kw, out=config(*kw['out'], rounding=4)) if 'out' in kw else kw
    for k in (33, 300):
        for m, n in [(17, 63), (65, 130)]: run_gemm(DEV, True, m, n, k, **kw)


@pytest.mark.parametrize('g', R.GEOMETRIES, ids=str)
def test_conv_geometries(g):
    run_conv(DEV, True, g)
    if g[0] == 40: run_conv(DEV, True, g, zx=0)                                          # sums null: no correction, zero bytes in the padding


def test_the_bytes_of_the_int8_kernel_on_the_same_codes():
    rng = np.random.default_rng(6)
    a, b = R.operands(rng, 65, 300, 9), weights(rng, 130, 300)
    A, B = pair(DEV, a, b, (65, 300), (130, 300), 9, np.full(130, 0.01, np.float32))
    out, res = config(*UNSIGNED, rounding=1), torch.randn(65, 130, device=DEV)
    same = lambda got, want: torch.equal(got[0].contiguous().view(torch.int32), want[0].contiguous().view(torch.int32)) and torch.equal(got[1].values, want[1].values)
    assert same(int8_matmul(A, int4_pack(B), None, res, True, out, True), int8_matmul(A, B, None, res, True, out, True))
    X, W, bias, _, out, _ = conv_case(DEV, R.GEOMETRIES[3], 5)
    assert same(int8_conv2d_packed(X, int4_pack(W), bias, 1, 2, 2, out_config=out, out_float=True), int8_conv2d_packed(X, W, bias, 1, 2, 2, out_config=out, out_float=True))
