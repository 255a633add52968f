"""The depthwise linear INT8 kernel on the GPU (ppq_amd/csrc/int8_dwconv.hip) against the NumPy oracle
(tests/int8_depthwise_reference.py) with == on bits: y as int32, q as bytes with its padding channels, on every geometry of the oracle's
list -- tile edges, channel blocks with 8, 1 and 6 live channels, both store paths, both pixel pitches, the unrolled 3 x 3 instance and
the runtime loop -- and the variants of the tail."""
import numpy as np
import pytest
import torch

import int8_depthwise_reference as D
from ppq_amd import int8_conv2d_packed, int8_depthwise_conv2d_packed
from test_host_int8 import bits, config
from test_host_int8_depthwise import C40, EXTREME, VARIANTS, operands, run

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('g,kw', [(g, {}) for g in D.GEOMETRIES] + [(C40, kw) for kw in VARIANTS] + [EXTREME], ids=str)
def test_kernel_is_the_oracle(g, kw):
    run(DEV, True, g, **kw)


def test_kernel_has_the_bits_of_the_dense_kernel_on_the_block_diagonal_weight():
    from ppq_amd import Int8Tensor
    c, _, _, kh, kw, stride, pad, dil = C40
    rng, x, wt, sw, X, W = operands(DEV, C40, 5)
    dense = np.zeros((c, kh, kw, wt.shape[-1]), np.int8)
    dense[np.arange(c), :, :, np.arange(c)] = wt[..., :c].transpose(2, 0, 1)
    B = Int8Tensor(torch.from_numpy(dense).to(DEV), (c, c, kh, kw), 1, W.scale, 0, -128, 127, 0, W.sums)
    bias, out = torch.from_numpy(rng.standard_normal(c).astype(np.float32)).to(DEV), config(0.25, 131, 0, 255)
    (y, p), (yd, pd) = (f(X, w, bias, stride, pad, dil, None, True, out, True) for f, w in ((int8_depthwise_conv2d_packed, W), (int8_conv2d_packed, B)))
    assert np.array_equal(bits(y), bits(yd)) and torch.equal(p.values, pd.values)
