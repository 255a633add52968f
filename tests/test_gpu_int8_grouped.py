"""The grouped linear INT8 kernel on the GPU (ppq_amd/csrc/int8_gconv.hip) against the NumPy oracle
(tests/int8_grouped_reference.py) with == on bits: y as int32, q as bytes with its padding columns, on every geometry of the oracle's
list, the variants of the tail and the largest |I| -- and against the dense kernel on the block-diagonal weight."""
import numpy as np
import pytest
import torch

import int8_grouped_reference as G
from ppq_amd import Int8Tensor, int8_conv2d_packed, int8_grouped_conv2d_packed
from test_host_int8 import bits, config
from test_host_int8_grouped import CASES, STRADDLE, operands, run

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('g,kw', CASES, ids=str)
def test_kernel_is_the_oracle(g, kw):
    run(DEV, True, g, **kw)


def test_kernel_has_the_bits_of_the_dense_kernel_on_the_block_diagonal_weight():
    groups, cg, og = STRADDLE[:3]
    stride, pad, dil = STRADDLE[8:]
    rng, x, wt, sw, X, W = operands(DEV, STRADDLE, 5, use_kernels=True)
    dense = G.block_diagonal(wt, groups)
    B = Int8Tensor(torch.from_numpy(dense).to(DEV), (groups * og, groups * cg, *wt.shape[1:3]), 1, W.scale, 0, -128, 127, 0, W.sums)
    bias, out = torch.from_numpy(rng.standard_normal(groups * og).astype(np.float32)).to(DEV), config(0.25, 131, 0, 255)
    (y, p), (yd, pd) = (f(X, w, bias, stride, pad, dil, None, True, out, True) for f, w in ((int8_grouped_conv2d_packed, W), (int8_conv2d_packed, B)))
    assert np.array_equal(bits(y), bits(yd)) and torch.equal(p.values, pd.values)
