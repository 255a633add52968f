"""The MX scale rules on the GPU: the RULED instantiations of the fake-quant and pack kernels
(ppq_amd/csrc/mx.hip, mx_pack.hip) against the oracle (tests/mx_scale_reference.py), ``==`` on values, codes and bytes.  The MSE
search compares two float64 sums whose order is the kernel's own: tests/test_host_mx_scale.py shows that the inputs used here hold
no block whose two errors are closer than the rounding of those sums, so nothing is excluded and nothing has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import mx_fused_reference as FR
import mx_pack_reference as P
import mx_reference as R
import mx_scale_reference as S
from ppq_amd import (CUDA, MXFormat, MXScaleRule, _lib, deploy_graph_mx, ffi, harness, mx_conv2d, mx_conv2d_packed, mx_dequantize, mx_fake_quant,
                     mx_linear, mx_matmul, mx_quantize, quantize_graph_mx)
from ppq_amd import mx as mx_module

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORMATS = R.FORMATS
NEW_RULES = S.NEW_RULES


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def cases(fmt: str):
    """[(name, x, axis)]: the layouts, the random, special and crafted blocks as rows, and the crafted ones down a strided axis."""
    out = [(f'layout {k}', x, axis) for k, (x, axis) in enumerate(S.layout_cases())]
    out += [(name, b, -1) for name, b in S.block_cases(fmt)]
    out.append(('crafted, strided', np.ascontiguousarray(S.crafted(fmt).T), 0))
    out.append(('special, scalar rows', np.ascontiguousarray(R.special_blocks(fmt)[:, :31]), -1))
    return out


@functools.lru_cache(maxsize=None)
def wanted(fmt: str, rule: str):
    """The oracle's (values, codes) of every case, and the torch arm's packed bytes of it (equal to the oracle: the host tests)."""
    out = []
    for _, x, axis in cases(fmt):
        y, c, _ = S.quantize(x, fmt, axis, rule)
        packed = mx_quantize(torch.from_numpy(x), fmt, axis, use_kernels=False, scale_rule=rule)
        out.append((y, c, packed))
    return out


def check(t: torch.Tensor, x: np.ndarray, fmt: str, axis: int, rule: str, want, what: str):
    y, c, packed = want
    shape = list(x.shape)
    shape[axis % x.ndim] = (shape[axis % x.ndim] + 31) // 32
    codes = torch.full(shape, 255, dtype=torch.uint8, device=DEV)
    got = mx_fake_quant(t, fmt, axis, scale_codes=codes, scale_rule=rule)
    assert np.array_equal(codes.cpu().numpy(), c), f'{what}: scale codes differ'
    bad = np.flatnonzero(R.bits(got.cpu().contiguous().numpy()).ravel() != R.bits(y).ravel())
    assert bad.size == 0, f'{what}: {bad.size} elements differ, first at {bad[:4]}'
    q = mx_quantize(t, fmt, axis, scale_rule=rule)
    assert torch.equal(q.scales.cpu(), packed.scales), f'{what}: packed scales differ'
    assert torch.equal(q.elements.cpu(), packed.elements), f'{what}: packed elements differ'
    assert P.same_but_nan(mx_dequantize(q).cpu().numpy(), y, P.nan_mask(x, fmt, axis), fmt), f'{what}: the round trip is not the fake quant'


@pytest.mark.parametrize('rule', NEW_RULES)
@pytest.mark.parametrize('fmt', FORMATS)
def test_kernels_equal_the_oracle(fmt, rule):
    """rows4 (layouts 0-2, the blocks), rows1 (layouts 3-4, the 31-wide rows), strided (layouts 5-7, the transposed blocks) and
    the channels-last view of layout 8, which is rows4 in storage order."""
    for (name, x, axis), want in zip(cases(fmt), wanted(fmt, rule)):
        t = torch.from_numpy(x).to(DEV)
        check(t, x, fmt, axis, rule, want, f'{fmt} {rule} {name}')
        if x.shape == R.CHANNELS_LAST_SHAPE:
            nhwc = t.contiguous(memory_format=torch.channels_last)
            assert ffi._mx_dense(nhwc, 1) is nhwc
            check(nhwc, x, fmt, axis, rule, want, f'{fmt} {rule} channels-last')


def test_one_launch_mixes_rules_and_formats():
    picks = [(0, 'MXFP8_E4M3', 'MSE'), (2, 'MXFP4_E2M1', 'CEIL'), (4, 'MXINT8', 'EVEN'), (5, 'MXFP6_E2M3', 'MSE'), (7, 'MXFP8_E5M2', 'FLOOR'),
             (8, 'MXFP6_E3M2', 'EVEN'), (3, 'MXFP4_E2M1', 'MSE')]
    items = []
    for k, fmt, rule in picks:
        _, x, axis = cases(fmt)[k]
        t = torch.from_numpy(x).to(DEV)
        if k == 8: t = t.contiguous(memory_format=torch.channels_last)
        items.append((t, MXFormat[fmt], axis, MXScaleRule[rule]))
    # all seven: the launch takes the instantiation with the search; without the MSE items: the one of the amax rules
    for keep in (lambda rule: True, lambda rule: rule != 'MSE'):
        chosen = [(p, i) for p, i in zip(picks, items) if keep(p[2])]
        plan = ffi.MXQuantizePlan([i for _, i in chosen], with_codes=True)
        outs = plan.run()
        packs = ffi.MXPackPlan([i for _, i in chosen]).run()
        for ((k, fmt, rule), _), out, codes, (e, s) in zip(chosen, outs, plan.codes, packs):
            y, c, packed = wanted(fmt, rule)[k]
            assert np.array_equal(R.bits(out.cpu().contiguous().numpy()), R.bits(y)), (k, fmt, rule)
            assert np.array_equal(codes.cpu().contiguous().numpy(), c), (k, fmt, rule)
            assert torch.equal(e.cpu(), packed.elements) and torch.equal(s.cpu(), packed.scales), (k, fmt, rule)
    with pytest.raises(ValueError, match='unknown MX scale rule'): ffi.MXQuantizePlan([(items[0][0], 'MXINT8', -1, 'NEAREST')])
    with pytest.raises(ValueError, match='entries'): ffi.MXPackPlan([(items[0][0], 'MXINT8')])


@pytest.mark.parametrize('fmt', FORMATS)
def test_in_place_under_mse(fmt):
    """y == x: a block is read whole -- and its two errors summed -- before any of it is written."""
    for k in (2, 4, 5):                                                                  # rows4 with a short tail; rows1; strided
        (_, x, axis), (y, c, _) = cases(fmt)[k], wanted(fmt, 'MSE')[k]
        t = torch.from_numpy(x).to(DEV)
        outer, length, inner, codes_shape = ffi._mx_geometry(t, axis % t.dim())
        codes = torch.zeros(codes_shape, dtype=torch.uint8, device=DEV)
        arg = ffi.mx_format_arg(fmt, 'MSE')
        assert _lib.lib.ppqhip_mx_fq(t.data_ptr(), t.data_ptr(), codes.data_ptr(), outer, length, inner, arg, None) == 0
        assert np.array_equal(R.bits(t.cpu().numpy()), R.bits(y)) and np.array_equal(codes.cpu().numpy(), c), (fmt, k)


def test_pack_into_unaligned_elements():
    """The byte-store body of the strided pack (elements not 16-byte aligned), under MSE."""
    fmt = 'MXFP6_E2M3'
    (_, x, axis), (_, _, packed) = cases(fmt)[5], wanted(fmt, 'MSE')[5]
    t = torch.from_numpy(x).to(DEV)
    outer, length, inner, _ = ffi._mx_geometry(t, axis % t.dim())
    arena = torch.zeros(packed.elements.numel() + 16, dtype=torch.uint8, device=DEV)
    scales = torch.zeros(packed.scales.numel(), dtype=torch.uint8, device=DEV)
    offset = 4 + (-arena.data_ptr()) % 16                                                # 4 past a 16-byte boundary
    e = arena[offset: offset + packed.elements.numel()]
    assert e.data_ptr() % 16 == 4
    assert _lib.lib.ppqhip_mx_pack(t.data_ptr(), e.data_ptr(), scales.data_ptr(), outer, length, inner, ffi.mx_format_arg(fmt, 'MSE'), None) == 0
    assert torch.equal(e.cpu(), packed.elements.reshape(-1)) and torch.equal(scales.cpu(), packed.scales.reshape(-1))
    assert not arena[:offset].any() and not arena[offset + packed.elements.numel():].any()


def test_c_entry_points_refuse_bad_rules():
    """Before any launch: an unknown rule where scales are made, any rule byte where they are not."""
    lib = _lib.lib
    x = torch.zeros(64, device=DEV)
    y = torch.zeros(64, device=DEV)
    e = torch.zeros(64, dtype=torch.uint8, device=DEV)
    s = torch.zeros(16, dtype=torch.uint8, device=DEV)
    bad, mse = 4 | 4 << 8, 4 | 3 << 8
    assert lib.ppqhip_mx_fq(x.data_ptr(), y.data_ptr(), None, 1, 64, 1, bad, None) == -1 and 'unknown MX scale rule' in _lib.last_error()
    assert lib.ppqhip_mx_pack(x.data_ptr(), e.data_ptr(), s.data_ptr(), 1, 64, 1, bad, None) == -1 and 'unknown MX scale rule' in _lib.last_error()
    jobs = np.zeros(1, dtype=ffi._MX_JOB)
    jobs[0] = (x.data_ptr(), y.data_ptr(), 0, 1, 64, 1, bad, 0)
    assert lib.ppqhip_mx_fq_multi(jobs.ctypes.data, 1, None) == -1 and 'unknown MX scale rule' in _lib.last_error()
    pjobs = np.zeros(1, dtype=ffi._MX_PACK_JOB)
    pjobs[0] = (x.data_ptr(), e.data_ptr(), s.data_ptr(), 1, 64, 1, bad, 0)
    assert lib.ppqhip_mx_pack_multi(pjobs.ctypes.data, 1, None) == -1 and 'unknown MX scale rule' in _lib.last_error()
    assert lib.ppqhip_mx_unpack(e.data_ptr(), s.data_ptr(), y.data_ptr(), 1, 64, 1, mse, None) == -1 and 'unknown MX format' in _lib.last_error()
    assert lib.ppqhip_mx_gemm(e.data_ptr(), s.data_ptr(), mse, e.data_ptr(), s.data_ptr(), 4, None, y.data_ptr(), 1, 1, 32, None) == -1
    assert 'unknown MX format' in _lib.last_error()
    assert lib.ppqhip_mx_conv2d(e.data_ptr(), s.data_ptr(), 4, e.data_ptr(), s.data_ptr(), mse, None, y.data_ptr(), 1, 32, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, None) == -1
    assert 'unknown MX format' in _lib.last_error()
    assert lib.ppqhip_mx_gemm_fused(e.data_ptr(), s.data_ptr(), 4, e.data_ptr(), s.data_ptr(), 4, None, None, 0, y.data_ptr(), None, None, mse, 1, 1, 32, None) == -1
    assert 'out_format: unknown MX format' in _lib.last_error()
    assert not y.any() and not e.any() and not s.any()                                   # nothing ran
    with pytest.raises(ValueError, match='unknown MX scale rule'): CUDA.MXQuantize(x.reshape(2, 32), 'MXINT8', -1, scale_rule=4)
    with pytest.raises(ValueError, match='unknown MX scale rule'): CUDA.MXPack(x.reshape(2, 32), 'MXINT8', -1, scale_rule='UP')


@pytest.mark.parametrize('fmt', FORMATS)
def test_floor_through_the_keyword_is_the_plain_call(fmt):
    for _, x, axis in cases(fmt):
        t = torch.from_numpy(x).to(DEV)
        assert torch.equal(bits(mx_fake_quant(t, fmt, axis, scale_rule=MXScaleRule.FLOOR)), bits(mx_fake_quant(t, fmt, axis)))
        assert torch.equal(bits(CUDA.MXQuantize(t, fmt, axis, scale_rule='FLOOR')), bits(CUDA.MXQuantize(t, fmt, axis)))
        a, b = mx_quantize(t, fmt, axis, scale_rule=0), mx_quantize(t, fmt, axis)
        assert torch.equal(a.elements, b.elements) and torch.equal(a.scales, b.scales)


@pytest.mark.parametrize('rows', [65537, 786433], ids=['two float4 per lane', 'streaming loads'])
def test_large_tensors_reach_the_other_instantiations(rows):
    """Above 4 Mi elements a rows4 lane owns two float4, from 48 Mi on the loads are streaming ones: against the torch arm on the
    device, after showing on the device that no block is a near tie."""
    fmt = MXFormat.MXFP4_E2M1
    g = torch.Generator(device=DEV).manual_seed(rows)
    x = torch.randn(rows, 64, device=DEV, generator=g) * torch.exp2(torch.randint(-6, 6, (rows, 1), device=DEV, generator=g).float())
    blocks = x.reshape(rows, 2, 32)
    c0 = mx_module._mx_scale_code(blocks, fmt, MXScaleRule.FLOOR)
    err = []
    for c in (c0, c0 + 1):
        d = (mx_module._mx_values(blocks, c, fmt) - blocks).double()
        err.append((d * d).sum(dim=-1))
    gap = (err[1] - err[0]).abs()
    assert int(((gap > 0) & (gap <= 2.0 ** -40 * torch.maximum(err[0], err[1]))).sum()) == 0
    del blocks, d, gap, err
    for rule in NEW_RULES:
        c1, c2 = (torch.zeros(rows, 2, dtype=torch.uint8, device=DEV) for _ in range(2))
        got = mx_fake_quant(x, fmt, scale_codes=c1, scale_rule=rule)
        want = mx_fake_quant(x, fmt, scale_codes=c2, scale_rule=rule, use_kernels=False)
        assert torch.equal(c1, c2) and torch.equal(bits(got), bits(want)), rule
        assert int((c1 != c0.reshape(rows, 2)).sum()) > 0, rule
        q, qw = mx_quantize(x, fmt, scale_rule=rule), mx_quantize(x, fmt, scale_rule=rule, use_kernels=False)
        assert torch.equal(q.scales, qw.scales) and torch.equal(q.elements, qw.elements), rule


@pytest.mark.parametrize('fmt', FORMATS)
def test_fake_quant_pack_and_round_split_agree_on_every_block_code(fmt):
    """The three kernels take a block's code from one walk (csrc/mx_walk.hpp): on one input, under every rule and on every addressing
    (the shapes of tests/test_gpu_mx_roundtune.py: rows4, rows1 with a short last block, rows1 by misalignment, strided with inner 9
    and with inner 32), the scale codes of mx_fake_quant, the scales of mx_quantize and the codes of mx_round_split are equal byte
    for byte.  One exception, by contract: a format without a NaN encoding packs a block that holds a NaN with scale 0xFF; there the
    other two still agree with each other."""
    from ppq_amd import mx_round_split
    from test_gpu_mx_roundtune import SHAPES, _crafted, _offset
    for k, (shape, axis, offset) in enumerate(SHAPES):
        x = _crafted(shape, axis, fmt, seed=k)
        t = torch.from_numpy(x).to(DEV)
        if offset: t = _offset(t)
        axis %= x.ndim
        dead = torch.from_numpy(P._blocks(np.isnan(x), axis, False).any(axis=-1)).to(DEV)      # [lead..., nb], as the packed scales
        if fmt in P.HAS_NAN: dead = torch.zeros_like(dead)
        else: assert dead.any() and not dead.all(), (fmt, shape)
        for rule in S.RULES:
            what = (fmt, rule, shape, axis, offset)
            fq = torch.full(shape[:axis] + ((shape[axis] + 31) // 32,) + shape[axis + 1:], 0xAA, dtype=torch.uint8, device=DEV)
            mx_fake_quant(t, fmt, axis, scale_codes=fq, scale_rule=rule)
            split = mx_round_split(t, fmt, axis, rule)[2]
            packed = mx_quantize(t, fmt, axis, scale_rule=rule).scales.movedim(-1, axis)
            assert fq.shape == split.shape == packed.shape, what
            assert torch.equal(fq, split), what
            assert torch.equal(packed, torch.where(dead.movedim(-1, axis), torch.full_like(fq, 0xFF), fq)), what


# ------------------------------------------------------------------------------------------------------- the loop on the hardware
def test_linear_and_conv_quantise_their_activation_by_the_rule():
    gen = torch.Generator().manual_seed(9)
    x, w, b = torch.randn(5, 96, generator=gen).to(DEV), torch.randn(40, 96, generator=gen).to(DEV), torch.randn(40, generator=gen).to(DEV)
    W = mx_quantize(w, 'MXFP4_E2M1', -1, scale_rule='MSE')
    got = mx_linear(x, W, 'MXFP4_E2M1', b, scale_rule='MSE')
    X = mx_quantize(x, 'MXFP4_E2M1', -1, scale_rule='MSE')
    assert torch.equal(bits(got), bits(mx_matmul(X, W, b)))
    assert not torch.equal(X.scales, mx_quantize(x, 'MXFP4_E2M1', -1).scales)             # the rule did move a scale
    assert not torch.equal(bits(got), bits(mx_linear(x, W, 'MXFP4_E2M1', b)))
    xc, wc = torch.randn(2, 40, 6, 6, generator=gen).to(DEV), torch.randn(8, 40, 3, 3, generator=gen).to(DEV)
    bc = torch.randn(8, generator=gen).to(DEV)
    Wc = mx_quantize(wc, 'MXFP4_E2M1', 1, scale_rule='MSE')
    got = mx_conv2d(xc, Wc, 'MXFP4_E2M1', bc, 1, 1, scale_rule='MSE')
    Xc = mx_quantize(xc, 'MXFP4_E2M1', 1, scale_rule='MSE')
    assert torch.equal(bits(got), bits(mx_conv2d_packed(Xc, Wc, bc, 1, 1)))
    assert not torch.equal(Xc.scales, mx_quantize(xc, 'MXFP4_E2M1', 1).scales)


def residual_graph(seed: int = 0, width: int = 40):
    """Conv -> Add (with the graph's input) -> Relu -> Conv."""
    gen = torch.Generator().manual_seed(seed)
    g = harness.BaseGraph('conv_add_relu_conv')
    x = g.create_variable('input'); g.inputs['input'] = x
    w0 = g.create_variable('c0_w', torch.randn([width, width, 3, 3], generator=gen) * (2.0 / (9 * width)) ** 0.5, True)
    b0 = g.create_variable('c0_b', torch.randn(width, generator=gen) * 0.1, True)
    h = g.create_operation('Conv', 'c0', [x, w0, b0], {'strides': 1, 'pads': 1})
    h = g.create_operation('Add', 'add', [h, x])
    h = g.create_operation('Relu', 'relu', [h])
    w1 = g.create_variable('c1_w', torch.randn([8, width, 3, 3], generator=gen) * (2.0 / (9 * width)) ** 0.5, True)
    b1 = g.create_variable('c1_b', torch.randn(8, generator=gen) * 0.1, True)
    h = g.create_operation('Conv', 'c1', [h, w1, b1], {'strides': 1, 'pads': 1})
    g.outputs[h.name] = h
    return g


def test_fused_deployment_under_even():
    """The fused epilogue packs by FLOOR: a consumer that reads its activation under EVEN gets the float tensor, with a note, and
    quantises it itself -- the logits of the unfused deployment, and the simulation's within the tolerance of the FLOOR tests."""
    x = torch.randn(2, 40, 6, 6, generator=torch.Generator().manual_seed(2)).to(DEV)
    g = residual_graph()
    ex = harness.TorchExecutor(g, DEV)
    d = quantize_graph_mx(g, ex, 'MXFP4_E2M1', 'MXFP4_E2M1', weight_scale_rule='MSE', activation_scale_rule='EVEN')
    simulated = ex.forward(x)
    plain = deploy_graph_mx(g, ex, d, fuse=False)
    want = ex.forward(x)
    plain.remove()
    dep = deploy_graph_mx(g, ex, d, fuse=True)
    assert dep.deployed == ['c0', 'c1']
    grp = dep.groups['c0']
    assert grp.members == ['c0', 'add', 'relu'] and grp.residual == 'input' and grp.relu and grp.out_format is None
    assert grp.notes == ['float output: a deployed consumer makes its scales by EVEN, the fused epilogue packs by FLOOR']
    seen, orig = [], mx_module.mx_quantize
    mx_module.mx_quantize = lambda *a, **k: (seen.append((tuple(a[0].shape), MXScaleRule.of(k.get('scale_rule')))), orig(*a, **k))[1]
    try: got = ex.forward(x)
    finally: mx_module.mx_quantize = orig
    assert seen == [((2, 40, 6, 6), MXScaleRule.EVEN)] * 2                               # both layers quantise their own input, by EVEN
    assert FR.same(got, want)
    assert torch.allclose(got[0], simulated[0], rtol=1e-3, atol=1e-3 * float(simulated[0].abs().max()))
    # by hand: the packed weights are MSE's, the activations EVEN's
    W0 = mx_quantize(g.variables['c0_w'].value, 'MXFP4_E2M1', 1, scale_rule='MSE')
    assert torch.equal(dep.weights['c0_w'].scales, W0.scales) and torch.equal(dep.weights['c0_w'].elements, W0.elements)
    v = lambda n: g.variables[n].value
    h = mx_conv2d(x, dep.weights['c0_w'], 'MXFP4_E2M1', v('c0_b'), 1, 1, residual=x, relu=True, scale_rule='EVEN')
    assert torch.equal(bits(got[0]), bits(mx_conv2d(h, dep.weights['c1_w'], 'MXFP4_E2M1', v('c1_b'), 1, 1, scale_rule='EVEN')))
    dep.remove()
    assert torch.equal(bits(ex.forward(x)[0]), bits(simulated[0]))
    # with FLOOR activations the same graph does hand over packed
    g2 = residual_graph()
    ex2 = harness.TorchExecutor(g2, DEV)
    d2 = quantize_graph_mx(g2, ex2, 'MXFP4_E2M1', 'MXFP4_E2M1', weight_scale_rule='MSE')
    dep2 = deploy_graph_mx(g2, ex2, d2, fuse=True)
    assert dep2.groups['c0'].out_format is MXFormat.MXFP4_E2M1 and dep2.groups['c0'].notes == []
