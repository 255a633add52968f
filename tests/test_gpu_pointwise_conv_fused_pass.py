"""TorchExecutor.fuse_pointwise_epilogue on the small graph of test_gpu_pointwise_conv_pass.py with `pointwise_min_work = 0`: in a
calibration forward the groups whose last-executed convolution is pointwise -- c1 -> relu1, c2 -> relu2 (P1) and c4, down -> add ->
add_relu (P2b, owned by `down`) -- run as ONE ffi.conv1x1_epilogue launch each.  A KL pass and an asymmetric MSE pass, eager and
replayed from a HIP graph: ranges, histograms, rendered scales and offsets and the outputs of a forward afterwards are bit for bit
those of the flag off and of `fuse_epilogues = False`.  The kernel is called in both phases; never with the flag off or in
channels-last; a requested c4 output and a recording `reuse_activations` pass fall back."""
import pytest
import torch

from ppq_amd import ffi, harness
from test_gpu_pointwise_conv_pass import DEV, _batches, _graph, _same

pytestmark = pytest.mark.gpu


@pytest.fixture
def deterministic_convs():
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _calibrate(method, hip_graph, fuse_pointwise=True, fuse=True, channels_last=False, reuse=False, request=None):
    """Run the pass; per phase every observer's range and histogram, the rendered configs, a forward's outputs afterwards, and the
    number of ffi.conv1x1_epilogue calls that launched, per phase."""
    from ppq_amd.calibration import RuntimeCalibrationPass
    g = _graph()
    if method == 'kl': harness.quantize_graph(g, 'kl', hist_bins=2048)
    else: harness.quantize_graph(g, 'mse', symmetrical=False, hist_bins=2048)
    ex = harness.TorchExecutor(g, DEV)
    if channels_last: ex.use_channels_last()
    ex.fuse_epilogues, ex.fuse_pointwise_epilogue, ex.pointwise_min_work = fuse, fuse_pointwise, 0
    harness.ParameterQuantizePass().optimize(g)
    batches = _batches()
    p = RuntimeCalibrationPass(method=method, check_steps=False, use_hip_graph=hip_graph, reuse_activations=reuse)
    r = {'phases': [], 'calls': [0]}
    orig_render, orig = p._render, ffi.conv1x1_epilogue

    def render():
        orig_render()
        snap = []
        for name, op_ob in p._observers.items():
            for ob in op_ob.observers():
                rng = getattr(ob, '_range', None)
                hist = ob.histogram() if hasattr(ob, 'histogram') else None
                snap.append((name, None if rng is None else rng.clone(), None if hist is None else hist.clone()))
        r['phases'].append(snap)
        r['calls'].append(0)

    def spy(*a, **k):
        out = orig(*a, **k)
        if out is not None: r['calls'][-1] += 1
        return out
    p._render, ffi.conv1x1_epilogue = render, spy
    if request is not None:                                       # every calibration forward also asks for this operation's output
        forward, names = p._forward, [g.operations[request].outputs[0].name]
        p._forward = lambda executor, data, hooks, output_names: forward(executor, data, hooks, names)
    try:
        p.optimize(g, dataloader=batches, executor=ex, calib_steps=len(batches))
        r['outputs'] = [t.clone() for t in ex.forward(batches[0])]
        torch.cuda.synchronize()
    finally:
        ffi.conv1x1_epilogue = orig
    r['rendered'] = [(op.name, c.scale, c.offset) for op in g.operations.values() for c, v in op.config_with_variable if not v.is_parameter]
    r['replays'] = p.graph_replays
    return r


def _assert_same_run(r0, r1):
    assert len(r0['phases']) == len(r1['phases']) == 2
    for s0, s1 in zip(r0['phases'], r1['phases']):
        assert len(s0) == len(s1) > 0
        for (n0, rng0, h0), (n1, rng1, h1) in zip(s0, s1):
            assert n0 == n1 and _same(rng0, rng1) and _same(h0, h1), n0
    assert len(r0['rendered']) == len(r1['rendered']) > 0
    for (n0, sc0, of0), (n1, sc1, of1) in zip(r0['rendered'], r1['rendered']):
        assert n0 == n1 and _same(sc0, sc1) and _same(of0, of1), n0
    for u, v in zip(r0['outputs'], r1['outputs']): assert _same(u, v)


@pytest.mark.parametrize('hip_graph', [False, True], ids=['eager', 'hipgraph'])
@pytest.mark.parametrize('method', ['kl', 'mse'])
def test_flag_on_equals_flag_off_and_unfused(method, hip_graph, deterministic_convs):
    on = _calibrate(method, hip_graph)
    off = _calibrate(method, hip_graph, fuse_pointwise=False)
    unfused = _calibrate(method, hip_graph, fuse=False)
    assert on['calls'][0] > 0 and on['calls'][1] > 0                     # both phases (a HIP graph: at least while capturing)
    assert sum(off['calls']) == 0 and sum(unfused['calls']) == 0
    if hip_graph: assert on['replays'] > 0
    _assert_same_run(on, off)
    _assert_same_run(on, unfused)


def test_channels_last_never_calls_the_kernel(deterministic_convs):
    assert sum(_calibrate('kl', False, channels_last=True)['calls']) == 0


def test_recording_pass_falls_back_while_recording(deterministic_convs):
    """`reuse_activations` records the tensors of phase 1: nothing may be elided there, so phase 1 takes today's path."""
    rec = _calibrate('kl', False, reuse=True)
    assert rec['calls'][0] == 0
    _assert_same_run(rec, _calibrate('kl', False, fuse_pointwise=False, reuse=True))


def test_requested_conv_output_falls_back(deterministic_convs):
    """Calibration forwards that ask for c4's output keep that tensor: its group (c4, down, add, add_relu) takes today's path, the
    two P1 groups are still fused, and everything comes out bit-equal to the flag off."""
    whole, kept = _calibrate('kl', False), _calibrate('kl', False, request='c4')
    assert 0 < kept['calls'][0] < whole['calls'][0] and 0 < kept['calls'][1] < whole['calls'][1]
    _assert_same_run(kept, _calibrate('kl', False, fuse_pointwise=False, request='c4'))
