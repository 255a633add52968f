"""The fused epilogue of the MX GEMM / convolution in NumPy: a composition of ``mx_gemm_reference`` /
``mx_conv_reference`` (the product) and ``mx_pack_reference`` (the packing), plus the routing case and the graph helpers both test
files share.

Per output, in this order: v = c (+ bias) (+ residual) in float32, one add each; ReLU: v > 0 ? v : +0 with a NaN staying the NaN it
is; then v packed along the columns (output channels) in blocks of 32 exactly as ``mx_pack_reference.pack`` packs a float32 tensor."""
import numpy as np

import mx_conv_reference as C
import mx_gemm_reference as G
import mx_pack_reference as P

OUT_FORMATS = G.FLOAT_FORMATS
ROUTING_M = 37                                        # three row tiles of 16, two waves, a partly filled one
ROUTING_NS = (33, 64, 70)                             # one live element in block 1; two whole blocks; a short last block of 6
ROUTING_K = 160


def relu(v: np.ndarray) -> np.ndarray:
    """v > 0 ? v : +0, NaN kept: never -0."""
    v = np.asarray(v, np.float32)
    return np.where(v > 0, v, np.where(np.isnan(v), v, np.float32(0.0))).astype(np.float32)


def epilogue(c, bias=None, residual=None, use_relu=False) -> np.ndarray:
    """float32 v of the product c (float64 or float32, exactly representable or already rounded): the adds are float32 adds."""
    v = np.asarray(c).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        if bias is not None: v = (v + np.asarray(bias, np.float32)).astype(np.float32)
        if residual is not None: v = (v + np.asarray(residual, np.float32)).astype(np.float32)
    return relu(v) if use_relu else v


def fused_matmul(a, b, fa, fb, k, fmt, bias=None, residual=None, use_relu=False):
    """(v float32 [M, N], (elements, scales)) of the packed operands a and b."""
    c, _ = G.matmul(a, b, fa, fb, k)
    v = epilogue(c, bias, residual, use_relu)
    return v, P.pack(v, fmt, -1)


def fused_conv(x, w, fx, fw, g, fmt, bias=None, residual=None, use_relu=False):
    """(v float32 [N, O, OH, OW], (elements [N, OH, OW, nbo * B], scales [N, OH, OW, nbo])); bias [O], residual [N, O, OH, OW]."""
    y, _ = C.conv(x, w, fx, fw, g)
    v = epilogue(y, None if bias is None else np.asarray(bias, np.float32)[None, :, None, None], residual, use_relu)
    return v, P.pack(v, fmt, 1)


def routing_residual(m: int, n: int) -> np.ndarray:
    """One large value per row, 1.5 * 2^(20 + row) at column (7 * row) % n: with |c| < 2^16 it alone decides the scale code of its
    block, 20 + row + 127 - emax, and no two rows share it.  A block maximum taken over the wrong lanes, the wrong tile or the wrong
    row gives another scale code; every other block keeps the small scale of c alone."""
    r = np.zeros((m, n), np.float32)
    rows = np.arange(m)
    r[rows, (7 * rows) % n] = (1.5 * np.exp2(20.0 + rows)).astype(np.float32)
    return r


def routing_case(n: int, fa: str, fb: str):
    """(a, b, residual, k) with exact operands (``G.exact_case``)."""
    a, b, c = G.exact_case(ROUTING_M, n, ROUTING_K, fa, fb)
    assert np.abs(c).max() < 2.0 ** 16
    return a, b, routing_residual(ROUTING_M, n), ROUTING_K


def routing_mismatches(epilogue_under_test, fa: str, fb: str, fmt: str):
    """Run ``epilogue_under_test(a, b, fa, fb, k, residual, fmt) -> (elements [M, nbo * B], scales [M, nbo])`` on the routing case of
    every N and return the list of (n, what) where it departs from the reference: [] for a correct epilogue."""
    bad = []
    for n in ROUTING_NS:
        a, b, residual, k = routing_case(n, fa, fb)
        _, (we, ws) = fused_matmul(a, b, fa, fb, k, fmt, residual=residual)
        rows = np.arange(ROUTING_M)
        emax = {'MXFP8_E4M3': 8, 'MXFP8_E5M2': 15, 'MXFP6_E3M2': 4, 'MXFP6_E2M3': 2, 'MXFP4_E2M1': 2}[fmt]
        assert np.array_equal(ws[rows, ((7 * rows) % n) // P.BLOCK], 20 + rows + 127 - emax)       # the case does what it says
        ge, gs = epilogue_under_test(a, b, fa, fb, k, residual, fmt)
        if not np.array_equal(np.asarray(gs), ws): bad.append((n, 'scales'))
        if not np.array_equal(np.asarray(ge), we): bad.append((n, 'elements'))
    return bad


def wrong_max_over_16(a, b, fa, fb, k, residual, fmt):
    """A wrong epilogue: the block maximum is taken over the first 16 columns of a block only (the fold over the wave's two column
    tiles is missing), so the scale code is that of half a block."""
    v, (elements, _) = fused_matmul(a, b, fa, fb, k, fmt, residual=residual)
    m, n = v.shape
    nbo = G.nblocks(n)
    padded = np.zeros((m, nbo * P.BLOCK), np.float32)
    padded[:, :n] = v
    halves = padded.reshape(m, nbo, P.BLOCK)[:, :, :16]
    _, scales = P.codes(halves, fmt, -1)                                                         # [m, nbo, 1]: 16 values and 16 zeros
    return elements, scales[:, :, 0]


def wrong_padding_takes_part(a, b, fa, fb, k, residual, fmt):
    """A wrong epilogue: the columns past N are not masked; they hold copies of the last column (the kernel's loads are clamped)
    and are packed like any other."""
    v, _ = fused_matmul(a, b, fa, fb, k, fmt, residual=residual)
    m, n = v.shape
    nbo = G.nblocks(n)
    padded = np.concatenate([v, np.repeat(v[:, -1:], nbo * P.BLOCK - n, axis=1)], axis=1)
    return P.pack(padded, fmt, -1)


# ---- what the graph tests of both files share ----------------------------------------------------------------------------------------
class PlainHook:
    """A hook that changes nothing: a hooked operation runs the simulated path."""
    def pre_forward_hook(self, inputs, quant_inputs, quant_configs): return quant_inputs

    def post_forward_hook(self, outputs, quant_outputs, quant_configs): return quant_outputs


def crcrc_graph(seed: int = 0, width: int = 40):
    """Conv-Relu-Conv-Relu-Conv: every hand-over between two layers is packed only."""
    import torch
    from ppq_amd import harness
    gen = torch.Generator().manual_seed(seed)
    g = harness.BaseGraph('crcrc')
    x = g.create_variable('input'); g.inputs['input'] = x
    h, cin = x, 3
    for k, relu in enumerate((True, True, False)):
        w = g.create_variable(f'k{k}_w', torch.randn([width, cin, 3, 3], generator=gen) * (2.0 / (9 * cin)) ** 0.5, True)
        b = g.create_variable(f'k{k}_b', torch.randn(width, generator=gen) * 0.1, True)
        h = g.create_operation('Conv', f'k{k}', [h, w, b], {'strides': 1, 'pads': 1})
        if relu: h = g.create_operation('Relu', f'k{k}_relu', [h])
        cin = width
    g.outputs[h.name] = h
    return g


def same(a, b) -> bool:
    """Two lists of tensors are torch.equal one by one."""
    import torch
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
