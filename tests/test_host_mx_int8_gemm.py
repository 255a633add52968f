"""The MXINT8 GEMM without a GPU: the ``use_kernels=False`` arm of ``mx_int8_matmul`` / ``mx_int8_linear`` against the oracle
(tests/mx_int8_gemm_reference.py) bit for bit, every argument check, and the host-side refusals of the C entry point."""
import numpy as np
import pytest
import torch

import mx_int8_gemm_reference as G
from ppq_amd import MXTensor, _lib, mx_int8_linear, mx_int8_matmul, mx_quantize

def tensor(op, k: int) -> MXTensor: return MXTensor('MXINT8', (op[0].shape[0], k), 1, torch.from_numpy(op[0]), torch.from_numpy(op[1]))


@pytest.mark.parametrize('m,n,k', [(1, 1, 1), (3, 5, 33), (17, 9, 160)])
def test_torch_arm_has_the_oracles_bits(m, n, k):
    rng, pool = np.random.default_rng(m * 1000 + k), [0, 1, *range(100, 151), 253, 254]
    a, b = G.raw_operand(rng, m, k, pool), G.raw_operand(rng, n, k, pool)
    assert G.same_bits(mx_int8_matmul(tensor(a, k), tensor(b, k), use_kernels=False).numpy(), G.matmul(a, b)[0])
    x, w, bias = torch.randn(2, m, k, generator=torch.Generator().manual_seed(k)), torch.randn(n, k) * 0.1, torch.linspace(-1.0, 1.0, n)
    qx, qw = mx_quantize(x, 'MXINT8', -1, use_kernels=False), mx_quantize(w, 'MXINT8', -1, use_kernels=False)
    got = mx_int8_matmul(qx, qw, bias, use_kernels=False)
    want = G.matmul((qx.elements.reshape(2 * m, -1).numpy(), qx.scales.reshape(2 * m, -1).numpy()), (qw.elements.numpy(), qw.scales.numpy()), bias.numpy())[0]
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, m, n) and G.same_bits(got.numpy().reshape(2 * m, n), want)
    assert torch.equal(mx_int8_linear(x, qw, bias, use_kernels=False), got)


def _refusals():
    x, w = torch.randn(6, 70), torch.randn(5, 70)
    a, b = mx_quantize(x, 'MXINT8', use_kernels=False), mx_quantize(w, 'MXINT8', use_kernels=False)
    return [('an MXTensor', TypeError, lambda: (x, b, None)),
            ('mx_matmul', RuntimeError, lambda: (mx_quantize(x, 'MXFP8_E4M3', use_kernels=False), b, None)),
            ('packed along axis 0', RuntimeError, lambda: (a, mx_quantize(w, 'MXINT8', 0, use_kernels=False), None)),
            ('K mismatch: a has 70, b has 64', RuntimeError, lambda: (a, mx_quantize(w[:, :64].contiguous(), 'MXINT8', use_kernels=False), None)),
            ('a is on cpu, b on meta', RuntimeError, lambda: (a, b.to('meta'), None)),
            ('bias must be a float32 tensor', RuntimeError, lambda: (a, b, torch.zeros(5, dtype=torch.float64))),
            (r'bias of shape \[6\], expected \[5\]', RuntimeError, lambda: (a, b, torch.zeros(6)))]


@pytest.mark.parametrize('match,error,args', _refusals(), ids=[r[0][:12] for r in _refusals()])
def test_argument_checks(match, error, args):
    with pytest.raises(error, match=match): mx_int8_matmul(*args(), use_kernels=False)


def test_c_entry_point_checks_arguments_without_a_device():
    """Sizes, null pointers, alignment and overlap are checked on the host before anything is launched.  m = 4, n = 2, k = 64: A's
    elements 256 B at p, its scales 8 B at p + 256; B's 128 B at p + 512 and 4 B at p + 640; bias 8 B at p + 704; c 32 B at p + 1024."""
    buf = np.zeros(4096 + 16, np.uint8)
    p = (buf.ctypes.data + 15) & ~15                                                     # 16-B aligned, 4096 bytes behind it

    def gemm(ae=p, as_=p + 256, be=p + 512, bs=p + 640, bias=p + 704, c=p + 1024, m=4, n=2, k=64):
        return _lib.lib.ppqhip_mx_int8_gemm(ae, as_, be, bs, bias, c, m, n, k, None), _lib.last_error()

    for size in ('m', 'n', 'k'):
        assert gemm(**{size: -1}) == (-1, 'mx_int8_gemm: negative size')
        assert gemm(**{size: 1 << 31}) == (-1, 'mx_int8_gemm: a size above 2^31 - 1')
    for ptr in ('ae', 'as_', 'be', 'bs', 'c'): assert gemm(**{ptr: 0}) == (-1, 'mx_int8_gemm: null pointer')
    for ptr, at in (('ae', p + 8), ('be', p + 516), ('c', p + 1028)): assert gemm(**{ptr: at}) == (-1, 'mx_int8_gemm: elements and c must be 16-byte aligned')
    for at in (p + 240, p + 624, p + 688): assert gemm(c=at) == (-1, 'mx_int8_gemm: an output overlaps an input')     # A's scales, B's, the bias
    assert gemm(m=1 << 30, n=1 << 30) == (-1, 'mx_int8_gemm: too many workgroups in one launch')
    assert gemm(m=0)[0] == 0 and gemm(n=0)[0] == 0 and gemm(m=0, ae=0, c=0)[0] == 0     # nothing to launch
