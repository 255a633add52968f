"""MX fake quant on the GPU: the HIP kernels (ppq_amd/csrc/mx.hip) against the oracle (tests/mx_reference.py).  The contract is
exact, so every comparison is ``==`` on the uint32 view of the values plus equal scale codes."""
import functools

import numpy as np
import pytest
import torch

import mx_reference as R
from ppq_amd import CUDA, MXFormat, _lib, ffi, harness, mx_fake_quant, quantize_graph_mx
from ppq_amd.analyse import graphwise_error_analyse

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORMATS = R.FORMATS


def hip(x, fmt: str, axis: int = -1):
    """CUDA.MXQuantize of a NumPy array or a CUDA tensor -> (values, codes) as NumPy arrays in logical order."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if isinstance(x, np.ndarray) else x
    shape = list(t.shape)
    shape[axis % t.dim()] = (shape[axis % t.dim()] + 31) // 32
    codes = torch.full(shape, 255, dtype=torch.uint8, device=DEV)
    y = CUDA.MXQuantize(t, MXFormat[fmt], axis, scale_codes=codes)
    return y.cpu().contiguous().numpy(), codes.cpu().numpy()


def assert_same(got, want, what):
    (y, c), (ry, rc) = got, want
    assert y.shape == ry.shape and c.shape == rc.shape, what
    bad = np.flatnonzero(R.bits(y).ravel() != R.bits(ry).ravel())
    assert bad.size == 0, f'{what}: {bad.size} elements differ, first at {bad[:4]}: {y.ravel()[bad[:4]]} != {ry.ravel()[bad[:4]]}'
    assert np.array_equal(c, rc), f'{what}: scale codes differ'


@functools.lru_cache(maxsize=None)
def layout_case(k: int, fmt: str):
    shape, axis = (R.LAYOUTS + [(R.CHANNELS_LAST_SHAPE, 1)])[k]
    x = R.layout_input(shape, seed=k)
    return x, axis, R.quantize(x, fmt, axis)


@pytest.mark.parametrize('fmt', FORMATS)
def test_layouts(fmt):
    for k, (shape, axis) in enumerate(R.LAYOUTS):
        x, axis, want = layout_case(k, fmt)
        assert_same(hip(x, fmt, axis), want, f'{fmt} {shape} axis {axis}')
        if axis == -1: assert_same(hip(x, fmt, len(shape) - 1), want, f'{fmt} {shape} positive axis')
    sliced = torch.from_numpy(layout_case(1, fmt)[0]).to(DEV)[:, 4:36]                 # rows that start 16-B aligned, 256-B pitch: copied
    assert_same(hip(sliced, fmt), R.quantize(sliced.cpu().numpy(), fmt), f'{fmt} non-contiguous slice')


@pytest.mark.parametrize('fmt', FORMATS)
def test_channels_last_takes_the_contiguous_path(fmt):
    x, axis, want = layout_case(len(R.LAYOUTS), fmt)
    nchw = torch.from_numpy(x).to(DEV)
    nhwc = nchw.contiguous(memory_format=torch.channels_last)
    assert ffi._mx_dense(nhwc, 1) is nhwc and ffi._mx_geometry(nhwc, 1)[:3] == (32, 64, 1)       # no copy; blocks are rows
    assert ffi._mx_geometry(nchw, 1)[:3] == (2, 64, 16)
    assert_same(hip(nchw, fmt, 1), want, fmt + ' NCHW')
    assert_same(hip(nhwc, fmt, 1), want, fmt + ' channels-last')
    assert CUDA.MXQuantize(nhwc, fmt, 1).is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize('fmt', FORMATS)
def test_in_place(fmt):
    for k in (2, 5):                                                                   # rows with a short tail; strided
        x, axis, want = layout_case(k, fmt)
        t = torch.from_numpy(x).to(DEV)
        outer, length, inner, codes_shape = ffi._mx_geometry(t, axis % t.dim())
        codes = torch.zeros(codes_shape, dtype=torch.uint8, device=DEV)
        assert _lib.lib.ppqhip_mx_fq(t.data_ptr(), t.data_ptr(), codes.data_ptr(), outer, length, inner, MXFormat[fmt].value, None) == 0
        assert_same((t.cpu().numpy(), codes.cpu().numpy()), want, f'{fmt} in place, layout {k}')


@pytest.mark.parametrize('fmt', FORMATS)
def test_exhaustive_cast(fmt):
    """Every float32 pattern whose exponent is at most emax (high half-word x three low half-words), in blocks with X = 1."""
    x = R.exhaustive_blocks(fmt)
    want = R.quantize(x, fmt)
    assert (want[1] == 127).all() and x.size > 90000
    assert_same(hip(x, fmt), want, fmt)


@pytest.mark.parametrize('fmt', FORMATS)
def test_special_blocks(fmt):
    x = R.special_blocks(fmt)
    want = R.quantize(x, fmt)
    assert_same(hip(x, fmt), want, fmt + ' rows')
    assert_same(hip(np.ascontiguousarray(x.T), fmt, 0), (want[0].T, want[1].T), fmt + ' strided')
    odd = np.ascontiguousarray(x[:, :31])                                              # the one-element-per-lane rows
    assert_same(hip(odd, fmt), R.quantize(odd, fmt), fmt + ' scalar rows')


@pytest.mark.parametrize('fmt', FORMATS)
def test_idempotent_and_equal_to_the_torch_arm(fmt):
    x = torch.from_numpy(R.gaussian_blocks()[:256]).to(DEV)
    c1, c2, c3 = (torch.zeros(256, 2, dtype=torch.uint8, device=DEV) for _ in range(3))
    y = mx_fake_quant(x, fmt, scale_codes=c1)
    again = mx_fake_quant(y, fmt, scale_codes=c2)
    arm = mx_fake_quant(x, fmt, scale_codes=c3, use_kernels=False)
    assert torch.equal(y.view(torch.int32), again.view(torch.int32)) and torch.equal(c1, c2)
    assert torch.equal(y.view(torch.int32), arm.view(torch.int32)) and torch.equal(c1, c3)


@pytest.mark.parametrize('shape, axis', [(((1 << 24) + 1, 64), -1), ((1, 64, (1 << 24) + 1), 1)])
def test_offsets_past_4_gib(shape, axis):
    """2^30 + 64 elements: the byte offsets of the last blocks do not fit 32 bits.  Only the ends are compared (rows4, strided)."""
    x = torch.zeros(shape, device=DEV)
    head, tail = R.layout_input((3, 64), 1), R.layout_input((3, 64), 2)
    if axis == -1: x[:3], x[-3:] = torch.from_numpy(head).to(DEV), torch.from_numpy(tail).to(DEV)
    else: x[0, :, :3], x[0, :, -3:] = torch.from_numpy(head.T.copy()).to(DEV), torch.from_numpy(tail.T.copy()).to(DEV)
    y = CUDA.MXQuantize(x, 'MXFP6_E2M3', axis)
    del x
    got = (y[:3], y[-3:]) if axis == -1 else (y[0, :, :3].T, y[0, :, -3:].T)
    for part, want in zip(got, (head, tail)):
        assert np.array_equal(R.bits(part.cpu().contiguous().numpy()), R.bits(R.quantize(want, 'MXFP6_E2M3')[0]))
    assert not y[3:-3].any() if axis == -1 else not y[0, :, 3:-3].any()


def test_multi_tensor_plan():
    """Six tensors of mixed layouts and formats in one launch equal the six single calls."""
    picks = [(0, 'MXFP8_E4M3'), (2, 'MXFP4_E2M1'), (4, 'MXINT8'), (5, 'MXFP6_E2M3'), (7, 'MXFP8_E5M2'), (8, 'MXFP6_E3M2')]
    items = []
    for k, fmt in picks:
        x, axis, _ = layout_case(k, fmt)
        t = torch.from_numpy(x).to(DEV)
        if k == 8: t = t.contiguous(memory_format=torch.channels_last)
        items.append((t, MXFormat[fmt], axis))
    plan = ffi.MXQuantizePlan(items, with_codes=True)
    outs = plan.run()
    for (k, fmt), (t, _, axis), out, codes in zip(picks, items, outs, plan.codes):
        assert out.shape == t.shape and out.stride() == t.stride()
        assert_same((out.cpu().contiguous().numpy(), codes.cpu().contiguous().numpy()), layout_case(k, fmt)[2], f'plan item {k} {fmt}')
        assert torch.equal(out.view(torch.int32), CUDA.MXQuantize(t, fmt, axis).view(torch.int32))
    with torch.no_grad(): items[1][0].mul_(3.0)                                          # the table holds pointers: in-place updates are seen
    assert torch.equal(plan.run()[1].view(torch.int32), CUDA.MXQuantize(items[1][0], 'MXFP4_E2M1', -1).view(torch.int32))
    with pytest.raises(RuntimeError, match='dense'): ffi.MXQuantizePlan([(items[0][0][:, ::2], 'MXINT8', -1)])
    with pytest.raises(RuntimeError, match='out of range'): CUDA.MXQuantize(items[0][0], 'MXINT8', 2)


def _graph(kind: str, use_kernels: bool):
    graph = harness.transformer_mlp_graph(seed=0) if kind == 'mlp' else harness.small_cnn_graph(seed=0)
    ex = harness.TorchExecutor(graph, DEV)
    delegators = quantize_graph_mx(graph, ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=use_kernels)
    return graph, ex, delegators


def _batches(kind: str, count: int = 3):
    g = torch.Generator().manual_seed(3)
    shape = (4, 16, 64) if kind == 'mlp' else (4, 3, 32, 32)
    return [torch.randn(*shape, generator=g).to(DEV) for _ in range(count)]


@pytest.mark.parametrize('kind', ['mlp', 'cnn'])
def test_graph_both_arms_and_error_analysis(kind):
    batches = _batches(kind)
    graph, ex, delegators = _graph(kind, True)
    _, ex_torch, _ = _graph(kind, False)
    group = next(d.group for d in delegators.values() if d.group is not None)
    for x in batches:
        a, b = ex.forward(x)[0], ex_torch.forward(x)[0]
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert group.launches == 1 and len(group.members) == (2 if kind == 'mlp' else 3)    # all weights, one launch, unchanged since
    fp32 = harness.TorchExecutor(harness.transformer_mlp_graph(seed=0) if kind == 'mlp' else harness.small_cnn_graph(seed=0), DEV)
    assert not torch.equal(fp32.forward(batches[0])[0], ex.forward(batches[0])[0])       # MX does change the output
    report = graphwise_error_analyse(graph, DEV, batches, steps=2, verbose=False, executor=ex)
    assert len(report) == (2 if kind == 'mlp' else 3)
    for name, value in report.items(): assert np.isfinite(value) and value > 0, (name, value)
    assert group.launches == 1                                                           # dequantised and restored: still the same weights
    w = group.members[0][0].value
    with torch.no_grad(): w.mul_(1.5)                                                    # written in place: one refill serves every member
    ex.forward(batches[0])
    assert group.launches == 2
    assert torch.equal(group.outputs[0].view(torch.int32), CUDA.MXQuantize(w, group.members[0][1], group.members[0][2]).view(torch.int32))


def test_neighbours_untouched():
    """An INT8 graph gives the outputs it gave before a sibling graph in the same process was quantised with MX."""
    g = torch.Generator().manual_seed(1)
    calib = [torch.rand(4, 3, 32, 32, generator=g).to(DEV) for _ in range(4)]
    from ppq_amd.calibration import RuntimeCalibrationPass
    graph = harness.small_cnn_graph(seed=0)
    harness.quantize_graph(graph, 'minmax')
    ex = harness.TorchExecutor(graph, DEV)
    harness.ParameterQuantizePass().optimize(graph)
    RuntimeCalibrationPass(check_steps=False).optimize(graph, dataloader=calib, executor=ex, calib_steps=4)
    before = [ex.forward(x)[0].clone() for x in calib]
    _, mx_ex, _ = _graph('cnn', True)
    for x in calib: mx_ex.forward(x)
    assert not ex._delegates
    for x, want in zip(calib, before): assert torch.equal(ex.forward(x)[0], want)
