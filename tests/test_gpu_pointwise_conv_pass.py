"""The executor's native pointwise convolution (TorchExecutor.native_pointwise_conv, harness.pointwise_eligible) on a small graph
with `pointwise_min_work = 0`: Conv1x1 -> Relu, a bottleneck (1x1 -> Relu, 3x3 stride 2 -> Relu, 1x1; a stride-2 1x1 `down`;
Add; Relu), GAP, Flatten, Gemm.  Fused and unfused executors agree bit for bit; the flag and channels-last switch it off; on
against off stays within the float64 bound of one convolution."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ppq_amd import ffi, harness
from pointwise_conv_reference import conv1x1_float64, gamma

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
POINTWISE = ('c1', 'c2', 'c4', 'down')


@pytest.fixture
def deterministic_convs():
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _graph(seed=0):
    gen = torch.Generator().manual_seed(seed)
    g = harness.BaseGraph('pointwise')
    x = g.create_variable('input'); g.inputs['input'] = x

    def conv(inp, cin, cout, name, k=1, stride=1):
        w = g.create_variable(name + '_w', harness._he([cout, cin, k, k], gen), True)
        b = g.create_variable(name + '_b', torch.randn(cout, generator=gen) * 0.1, True)
        return g.create_operation('Conv', name, [inp, w, b], {'strides': stride, 'pads': k // 2})

    stem = g.create_operation('Relu', 'relu1', [conv(x, 8, 16, 'c1')])
    y = g.create_operation('Relu', 'relu2', [conv(stem, 16, 8, 'c2')])
    y = g.create_operation('Relu', 'relu3', [conv(y, 8, 8, 'c3', k=3, stride=2)])
    y = conv(y, 8, 40, 'c4')
    d = conv(stem, 16, 40, 'down', stride=2)
    y = g.create_operation('Relu', 'add_relu', [g.create_operation('Add', 'add', [y, d])])
    y = g.create_operation('Flatten', 'flatten', [g.create_operation('GlobalAveragePool', 'gap', [y])])
    w = g.create_variable('fc_w', torch.randn([10, 40], generator=gen) * 0.3, True)
    y = g.create_operation('Gemm', 'fc', [y, w, g.create_variable('fc_b', torch.zeros(10), True)])
    g.outputs[y.name] = y
    return g


def _batches(n=4):
    gen = torch.Generator().manual_seed(3)
    return [(torch.randn(3, 8, 18, 18, generator=gen) * 2).to(DEV) for _ in range(n)]


def _calibrate(fuse, hip_graph, native=True, channels_last=False):
    """Run the KL pass; returns per phase every observer's range and histogram, the rendered configs, the outputs of a
    forward with the calibrated configs, and how often ffi.conv1x1 was called."""
    from ppq_amd.calibration import RuntimeCalibrationPass
    g = _graph()
    harness.quantize_graph(g, 'kl', hist_bins=2048)
    ex = harness.TorchExecutor(g, DEV)
    if channels_last: ex.use_channels_last()
    ex.fuse_epilogues, ex.native_pointwise_conv, ex.pointwise_min_work = fuse, native, 0
    harness.ParameterQuantizePass().optimize(g)
    batches = _batches()
    p = RuntimeCalibrationPass(method='kl', check_steps=False, use_hip_graph=hip_graph)
    r = {'phases': [], 'calls': 0}
    orig_render, orig_conv = p._render, ffi.conv1x1

    def render():
        orig_render()
        snap = []
        for name, op_ob in p._observers.items():
            for ob in op_ob.observers():
                rng = getattr(ob, '_range', None)
                hist = ob.histogram() if hasattr(ob, 'histogram') else None
                snap.append((name, None if rng is None else rng.clone(), None if hist is None else hist.clone()))
        r['phases'].append(snap)

    def spy(*a, **k):
        r['calls'] += 1
        return orig_conv(*a, **k)
    p._render, ffi.conv1x1 = render, spy
    try:
        p.optimize(g, dataloader=batches, executor=ex, calib_steps=len(batches))
        r['outputs'] = [t.clone() for t in ex.forward(batches[0])]
        torch.cuda.synchronize()
    finally:
        ffi.conv1x1 = orig_conv
    r['rendered'] = [(op.name, c.scale, c.offset) for op in g.operations.values() for c, v in op.config_with_variable if not v.is_parameter]
    r['replays'] = p.graph_replays
    return r


def _same(u, v):
    if u is None or v is None: return u is None and v is None
    u, v = torch.as_tensor(u), torch.as_tensor(v)
    return u.shape == v.shape and (torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32)) if u.dtype == torch.float32 else torch.equal(u, v))


@pytest.mark.parametrize('hip_graph', [False, True])
def test_fused_and_unfused_agree_bit_for_bit_on_the_native_path(hip_graph, deterministic_convs):
    r0, r1 = _calibrate(False, hip_graph), _calibrate(True, hip_graph)
    assert r0['calls'] > 0 and r1['calls'] > 0
    if hip_graph: assert r1['replays'] > 0
    assert len(r0['phases']) == len(r1['phases']) == 2
    for s0, s1 in zip(r0['phases'], r1['phases']):
        assert len(s0) == len(s1) > 0
        for (n0, rng0, h0), (n1, rng1, h1) in zip(s0, s1):
            assert n0 == n1 and _same(rng0, rng1) and _same(h0, h1), n0
    assert len(r0['rendered']) == len(r1['rendered']) > 0
    for (n0, sc0, of0), (n1, sc1, of1) in zip(r0['rendered'], r1['rendered']):
        assert n0 == n1 and _same(sc0, sc1) and _same(of0, of1), n0
    for u, v in zip(r0['outputs'], r1['outputs']): assert _same(u, v)


def test_flag_off_and_channels_last_never_call_the_kernel(deterministic_convs):
    assert _calibrate(True, False, native=False)['calls'] == 0
    assert _calibrate(False, False, native=False)['calls'] == 0
    assert _calibrate(True, False, channels_last=True)['calls'] == 0
    assert _calibrate(False, False, channels_last=True)['calls'] == 0


def test_native_against_vendor_within_the_float64_bound_of_one_convolution():
    """Each pointwise convolution on the SAME input: |native - float64| <= gamma_{c+1} (sum |w||x| + |b|), the recursive-sum bound
    with the bias as one more term; F.conv2d, whatever its order of summation, obeys the same bound, so the two differ by at
    most twice that.  No bound over depth is needed."""
    g = _graph()
    ex = harness.TorchExecutor(g, DEV)
    ex.pointwise_min_work, ex.fuse_epilogues = 0, False      # op by op: every convolution output is stored as the convolution left it
    batch = _batches(1)[0]
    names = sorted({v.name for n in POINTWISE for v in (g.operations[n].inputs[0], g.operations[n].outputs[0])} - {'input'})
    calls = []
    orig = ffi.conv1x1
    ffi.conv1x1 = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try: vals = dict(zip(names, ex.forward(batch, output_names=names)), input=batch)
    finally: ffi.conv1x1 = orig
    assert len(calls) == len(POINTWISE)
    for n in POINTWISE:
        op = g.operations[n]
        x, y = vals[op.inputs[0].name], vals[op.outputs[0].name]
        w, b = op.inputs[1].value, op.inputs[2].value
        stride = op.attributes['strides']
        vendor = F.conv2d(x, w, b, stride=stride)
        y64, mag = conv1x1_float64(x.cpu().numpy(), w.cpu().numpy().reshape(w.shape[0], -1), stride)
        b64 = b.cpu().double().numpy()[None, :, None, None]
        bound = gamma(w.shape[1] + 1) * (mag + np.abs(b64))
        err = np.abs(y.cpu().double().numpy() - (y64 + b64))
        print(f'{n}: native err / bound max {float((err / bound).max()):.3f}; native vs vendor / (2 bound) max '
              f'{float((np.abs((y - vendor).cpu().double().numpy()) / (2 * bound)).max()):.3f}')
        assert np.all(err <= bound), n
        assert np.all(np.abs((y - vendor).cpu().double().numpy()) <= 2 * bound), n
