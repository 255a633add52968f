"""The skinny linear INT8 GEMM without a GPU: the C entry points' argument checks on host pointers, and the
skinny flag of int8_matmul under the torch arm, which already has the bits."""
import numpy as np
import pytest
import torch

from ppq_amd import _lib, int4_pack, int8_matmul, int8_quantize
from test_host_int8 import config


@pytest.mark.parametrize('what', ['int8_gemm_skinny', 'int4_gemm_skinny'])
def test_c_entry_points_check_arguments_without_a_device(what):
    """Every call below is refused on the host or has nothing to launch: the pointers are host memory."""
    buf = np.zeros(16384 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15
    # 2 x 40 x 64: operands below p + 4096, sums, mul and bias there, residual at p + 5120, c at p + 6144, q (2 x 64 B) at p + 7168
    def call(a=p, b=p + 1024, sums=p + 4096, zx=3, mul=p + 4352, res=p + 5120, c=p + 6144, q=p + 7168, grid=(1.0, 0, -128, 127, 0, 0), m=2, n=40, k=64):
        return getattr(_lib.lib, 'ppqhip_' + what)(a, b, sums, zx, mul, p + 4608, res, 1, c, q, *grid, m, n, k, None), _lib.last_error()

    assert call(c=0, q=0) == (-1, f'{what}: no output: c and q are both null')
    assert call(zx=128) == (-1, f'{what}: zx 128 is not an int8 zero point')
    assert call(grid=(1.0, 0, -129, 127, 0, 0))[0] == -1 and call(grid=(1.0, 0, 5, 4, 0, 0))[0] == -1 and call(grid=(1.0, 0, 0, 127, 0, 128))[0] == -1
    assert call(grid=(1.0, 0, -128, 127, 5, 0)) == (-1, f'{what}: rounding policy 5 has no tensor form (ppq_tensor_round)')
    assert call(m=-1) == (-1, f'{what}: negative size')
    assert call(m=65) == (-1, f'{what}: m = 65: the skinny kernel takes at most 64 rows') and call(m=65, n=0)[0] == -1
    assert call(a=0) == (-1, f'{what}: null pointer') == call(b=0) == call(mul=0)
    assert call(sums=0) == (-1, f'{what}: sums is required with a zero point other than 0') and call(sums=0, zx=0, m=0)[0] == 0
    assert call(a=p + 8) == (-1, f'{what}: operands, c and q must be 16-byte aligned') == call(b=p + 1032) == call(c=p + 6144 + 4) == call(q=p + 7168 + 8)
    for out in ({'c': p + 5120}, {'q': p + 4352}, {'q': p + 16}): assert call(**out) == (-1, f'{what}: an output overlaps an input')
    assert call(q=p + 6144) == (-1, f'{what}: two outputs overlap in memory')
    assert call(k=65505)[1].startswith(f'{what}: a padded reduction length of 65536')
    assert call(m=0)[0] == 0 and call(n=0)[0] == 0                                       # nothing to launch


def test_the_flag_changes_nothing_under_the_torch_arm_but_the_bound_on_m():
    gen = torch.Generator().manual_seed(5)
    x, w = torch.randn(3, 5, 40, generator=gen), torch.randn(37, 40, generator=gen)
    X = int8_quantize(x, config(0.03, 120, 0, 255, 1), use_kernels=False)
    W = int8_quantize(w, config(0.3, 0, -8, 7), 1, weight=True, use_kernels=False)
    out = config(0.25, -3, -128, 127, 4)
    for B in (W, int4_pack(W)):
        (y, p), (y0, p0) = (int8_matmul(X, B, out_config=out, out_float=True, use_kernels=False, skinny=s) for s in (True, False))
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32)) and torch.equal(p.values, p0.values)
    big = int8_quantize(torch.randn(5, 13, 40, generator=gen), config(0.03, 120, 0, 255, 1), use_kernels=False)
    with pytest.raises(RuntimeError, match=r'int8_matmul: skinny=True takes M = 1 \.\. 64 rows, got M = 65'): int8_matmul(big, W, use_kernels=False, skinny=True)
    assert int8_matmul(big, W, use_kernels=False).shape == (5, 13, 37)
