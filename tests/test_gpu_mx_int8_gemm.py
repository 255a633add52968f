"""The MXINT8 GEMM on the GPU (ppq_amd/csrc/mx_int8_gemm.hip): the kernel against the oracle
(tests/mx_int8_gemm_reference.py) with == on the float32 bits, NaN-ness only where the oracle is NaN."""
import numpy as np
import pytest
import torch

import mx_int8_gemm_reference as G
from ppq_amd import CUDA, MXTensor, mx_int8_linear, mx_int8_matmul, mx_quantize

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MN = [(1, 1), (15, 17), (17, 63), (63, 65), (65, 15), (65, 130)]          # the 16 / 32 / 64 tile edges; several workgroups
KS = [1, 31, 32, 33, 96, 128, 160, 288]                                   # a short last block; nb = 3 / 4 / 5 around the chunk; nb = 9


def hip(a, b, k: int, bias=None, lead=None) -> np.ndarray:
    ta, tb = (MXTensor('MXINT8', (len(e), k), 1, torch.from_numpy(e).to(DEV), torch.from_numpy(s).to(DEV)) for e, s in (a, b))
    if lead is not None: ta = MXTensor('MXINT8', (*lead, k), len(lead), ta.elements.reshape(*lead, -1), ta.scales.reshape(*lead, -1))
    y = mx_int8_matmul(ta, tb, None if bias is None else torch.from_numpy(bias).to(DEV))
    assert y.dtype == torch.float32 and y.is_contiguous()
    return y.cpu().numpy()


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('m,n', MN)
def test_raw_codes_on_every_tile_edge(m, n, k):
    rng = np.random.default_rng(1000 * m + k)
    a, b = G.raw_operand(rng, m, k, range(110, 141)), G.raw_operand(rng, n, k, range(110, 141))
    assert G.same_bits(hip(a, b, k), G.matmul(a, b)[0])


@pytest.mark.parametrize('v', range(4))
def test_routing_of_every_k_byte_and_every_scale(v):
    """One non-zero code per row of A, at byte (7 i + v) % 32 of block (i + v) % 4; all-ones B with scale codes distinct per (column, block)."""
    m = n = 32; k = 128; i = np.arange(m)
    ae = np.zeros((m, k), np.uint8)
    ae[i, 32 * ((i + v) % 4) + (7 * i + v) % 32] = np.where(i % 2, 256 - (2 * i + 1), 2 * i + 1).astype(np.uint8)     # odd, distinct, both signs
    a = ae, (60 + 4 * i[:, None] + np.arange(4)[None, :]).astype(np.uint8)
    b = np.ones((n, k), np.uint8), (70 + 4 * ((i[:, None] * 5) % 32) + (np.arange(4)[None, :] + v) % 4).astype(np.uint8)
    want = G.matmul(a, b)[0]
    assert len(np.unique(want)) == m * n and np.array_equal(hip(a, b, k), want)


@pytest.mark.parametrize('pool', [[0, 1, 126, 127, 253, 254], [0, 1, 100, 105, 110, 116]], ids=['every class', 'subnormal rounding'])
def test_extreme_scales(pool):
    """Every pairing: subnormal terms, underflow, overflow, Inf - Inf; the second pool has 2^e in [2^-166, 2^-149]: a subnormal term's rounding."""
    codes, rng = np.array([1, 127, 0x80, 0xff], np.uint8), np.random.default_rng(5)
    scales = np.repeat(np.array(pool, np.uint8)[np.arange(16) % 6][:, None], 2, axis=1)
    a, b = (codes[rng.integers(0, 4, (16, 64))], scales), (codes[rng.integers(0, 4, (16, 64))], scales)
    want, exact, _ = G.matmul(a, b)
    tiny = (np.abs(want) < 2.0 ** -126) & (want != 0)
    if 254 in pool: assert tiny.any() and (want == 0).any() and np.isposinf(want).any() and np.isneginf(want).any() and np.isnan(want).any()
    else: assert (want[tiny].astype(np.float64) != exact[tiny]).any()
    assert G.same_bits(hip(a, b, 64), want)


def test_nan_scale_bias_leading_dimensions_and_determinism():
    m, n, k = 6, 70, 160
    rng = np.random.default_rng(9)
    a, b, bias = G.raw_operand(rng, m, k, range(110, 141)), G.raw_operand(rng, n, k, range(110, 141)), rng.standard_normal(n).astype(np.float32)
    a[1][4, 3] = b[1][66, 0] = 0xff
    want = G.matmul(a, b, bias)[0]
    got = hip(a, b, k, bias, lead=[2, 3])
    assert got.shape == (2, 3, n) and np.array_equal(got.reshape(m, n).view(np.uint32), want.view(np.uint32))     # 0x7fc00000 included
    nan = np.zeros((m, n), bool); nan[4, :] = True; nan[:, 66] = True
    assert np.array_equal(np.isnan(want), nan) and np.array_equal(hip(a, b, k, bias, lead=[2, 3]).view(np.uint32), got.view(np.uint32))


def test_quantised_operands_and_the_linear_layer():
    m, n, k = 65, 130, 288
    g = torch.Generator().manual_seed(3)
    x, w, bias = torch.randn(m, k, generator=g).to(DEV), (torch.randn(n, k, generator=g) * 0.1).to(DEV), torch.randn(n, generator=g).to(DEV)
    qx, qw = mx_quantize(x, 'MXINT8', -1), mx_quantize(w, 'MXINT8', -1)
    got = mx_int8_matmul(qx, qw, bias)
    want, exact, s = G.matmul(*((t.elements.cpu().numpy(), t.scales.cpu().numpy()) for t in (qx, qw)), bias.cpu().numpy())
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    bound = (k // 32 + 1) * 2.0 ** -24 * (s + np.abs(bias.cpu().numpy().astype(np.float64)))       # nb + 1 round-to-nearest adds
    assert (np.abs(got.cpu().numpy().astype(np.float64) - exact) <= bound).all()
    y = mx_int8_linear(x, qw, bias)
    assert torch.equal(y.view(torch.int32), got.view(torch.int32))
    assert torch.equal(y.view(torch.int32), mx_int8_linear(x, qw, bias, use_kernels=False).view(torch.int32))


@pytest.mark.parametrize('what,match', [('strided', 'must be contiguous'), ('dtype', 'Invalid dtype'), ('scales', 'expected')])
def test_binding_refuses(what, match):
    q = mx_quantize(torch.randn(8, 64, device=DEV), 'MXINT8', -1)
    e, s = q.elements, q.scales
    bad = {'strided': (torch.cat([e, e], dim=1)[:, :64], s), 'dtype': (e.float(), s), 'scales': (e, torch.cat([s, s], dim=1))}[what]
    with pytest.raises(RuntimeError, match=match): CUDA.MXInt8Matmul(*bad, e, s, 64)
