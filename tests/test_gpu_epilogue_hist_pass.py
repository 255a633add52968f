"""RuntimeCalibrationPass with the histogram sinks and the store elision of the convolution epilogues: with fuse_epilogues on,
the running ranges (phase 1) AND the histograms (phase 2) of every tensor an epilogue launch writes are taken inside that
launch, the biased convolution outputs of the residual groups are not stored -- and ranges, histograms, scales and offsets
are, bit for bit, those of the unfused executor (deterministic convolutions).  A tensor somebody asks for is stored."""
import pytest
import torch

from ppq_amd import ffi, harness
from ppq_amd.observer import ObservationQueue

DEV = 'cuda:0'
gpu = pytest.mark.gpu

# 4 x 16 x 132 x 132 = 1 115 136 elements: just above the 2^20 below which the histogram sinks leave a tensor to the
# observers' end-of-forward launch
WIDTH, HW, BATCH = 16, 132, 4
WRITTEN = (BATCH, WIDTH, HW, HW)
EPILOGUE_WRITES = 6               # relu1; c2, down, relu2; c3, relu3


@pytest.fixture
def deterministic_convs():
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _graph(seed=0):
    """Conv-Relu (one bias_act group), Conv + Conv-Add-Relu (bias_add_act, three stored tensors), Conv + identity-Add-Relu
    (two stored tensors), then GAP-Flatten-Gemm: tensors no epilogue writes."""
    gen = torch.Generator().manual_seed(seed)
    g = harness.BaseGraph('epilogue_hist')
    x = g.create_variable('input'); g.inputs['input'] = x

    def conv(inp, cin, cout, name, k=3):
        w = g.create_variable(name + '_w', harness._he([cout, cin, k, k], gen), True)
        b = g.create_variable(name + '_b', torch.randn(cout, generator=gen) * 0.1, True)
        return g.create_operation('Conv', name, [inp, w, b], {'strides': 1, 'pads': k // 2})

    y = g.create_operation('Relu', 'relu1', [conv(x, 3, WIDTH, 'c1')])
    z, d = conv(y, WIDTH, WIDTH, 'c2'), conv(y, WIDTH, WIDTH, 'down', 1)
    y = g.create_operation('Relu', 'relu2', [g.create_operation('Add', 'add2', [z, d])])
    z = conv(y, WIDTH, WIDTH, 'c3')
    y = g.create_operation('Relu', 'relu3', [g.create_operation('Add', 'add3', [z, y])])
    y = g.create_operation('Flatten', 'flatten', [g.create_operation('GlobalAveragePool', 'gap', [y])])
    w = g.create_variable('fc_w', torch.randn([10, WIDTH], generator=gen) * 0.3, True)
    y = g.create_operation('Gemm', 'fc', [y, w, g.create_variable('fc_b', torch.zeros(10), True)])
    g.outputs[y.name] = y
    return g


def _calibrate(method, cfg3, fuse, hip_graph, request=None, reuse=False):
    """Run the pass.  `request`: the name of an operation whose output every calibration forward also asks for through
    output_names.  Returns a dict: per phase every observer's folded range and histogram, the rendered configs, per forward
    the shapes that reached the queue's min/max and histogram launches, the requested tensors, the elide masks used."""
    from ppq_amd.calibration import RuntimeCalibrationPass
    g = _graph()
    if cfg3: harness.quantize_graph(g, method, symmetrical=False, weight_symmetrical=False, hist_bins=2048)
    else: harness.quantize_graph(g, method, hist_bins=2048)
    ex = harness.TorchExecutor(g, DEV)
    ex.fuse_epilogues = fuse
    harness.ParameterQuantizePass().optimize(g)
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(BATCH, 3, HW, HW, generator=gen) * 2).to(DEV) for _ in range(5)]
    p = RuntimeCalibrationPass(method=method, check_steps=False, use_hip_graph=hip_graph, reuse_activations=reuse)
    r = {'phases': [], 'minmax': [], 'hist': [], 'requested': [], 'masks': []}
    orig_render, orig_flush, orig_forward = p._render, ObservationQueue.flush, ex.forward
    orig_stats, orig_hist = ffi.bias_add_act_stats, ffi.bias_add_act_hist

    def render():
        orig_render()
        snap = []
        for name, op_ob in p._observers.items():
            for ob in op_ob.observers():
                rng = getattr(ob, '_range', None)
                hist = ob.histogram() if hasattr(ob, 'histogram') else None
                snap.append((name, type(ob).__name__, None if rng is None else rng.clone(), None if hist is None else hist.clone()))
        r['phases'].append(snap)

    def flush(self):
        r['minmax'].append([tuple(v.shape) for v, _ in self._minmax])
        r['hist'].append([tuple(i[0].shape) for items in self._hist.values() for i in items])
        orig_flush(self)

    def forward(inputs, output_names=None, hooks=None):
        if request is None: return orig_forward(inputs, output_names=output_names, hooks=hooks)
        name = g.operations[request].outputs[0].name
        outs = orig_forward(inputs, output_names=[name] + list(g.outputs), hooks=hooks)
        if not torch.cuda.is_current_stream_capturing(): r['requested'].append(outs[0].clone())
        return outs[1:]

    def spy(real):
        def launch(*args):
            r['masks'].append(args[8] if len(args) > 8 else 0)
            return real(*args)
        return launch
    p._render, ObservationQueue.flush, ex.forward = render, flush, forward
    ffi.bias_add_act_stats, ffi.bias_add_act_hist = spy(orig_stats), spy(orig_hist)
    try:
        p.optimize(g, dataloader=batches, executor=ex, calib_steps=len(batches))
        torch.cuda.synchronize()
    finally:
        ObservationQueue.flush = orig_flush
        ffi.bias_add_act_stats, ffi.bias_add_act_hist = orig_stats, orig_hist
    r['rendered'] = [(op.name, int(getattr(c.state, 'value', c.state)), c.scale, c.offset)
                     for op in g.operations.values() for c, v in op.config_with_variable if not v.is_parameter]
    r['replays'], r['replayed_batches'] = p.graph_replays, p.replayed_batches
    return r


def _same_statistics(r0, r1, two_phase):
    assert len(r0['phases']) == len(r1['phases']) == (2 if two_phase else 1)
    for s0, s1 in zip(r0['phases'], r1['phases']):
        assert len(s0) == len(s1) and len(s0) > 0
        for (n0, t0, rng0, h0), (n1, t1, rng1, h1) in zip(s0, s1):
            assert (n0, t0) == (n1, t1) and (rng0 is None) == (rng1 is None) and (h0 is None) == (h1 is None)
            if rng0 is not None: assert torch.equal(rng0.view(torch.int32), rng1.view(torch.int32)), (n0, rng0, rng1)
            if h0 is not None: assert torch.equal(h0, h1), n0
    assert len(r0['rendered']) == len(r1['rendered'])
    for (n0, st0, sc0, of0), (n1, st1, sc1, of1) in zip(r0['rendered'], r1['rendered']):
        assert (n0, st0) == (n1, st1)
        for u, v in ((sc0, sc1), (of0, of1)):
            assert (u is None) == (v is None)
            if u is not None: assert torch.equal(u, v), n0


@gpu
@pytest.mark.parametrize('method,cfg3,hip_graph', [('kl', False, False), ('kl', False, True), ('mse', True, False), ('mse', True, True),
                                                   ('minmax', False, False), ('minmax', False, True)])
def test_statistics_and_scales_equal_fused_and_unfused(method, cfg3, hip_graph, deterministic_convs):
    r0 = _calibrate(method, cfg3, False, hip_graph)
    r1 = _calibrate(method, cfg3, True, hip_graph)
    if hip_graph: assert r1['replays'] > 0
    two_phase = method != 'minmax'
    _same_statistics(r0, r1, two_phase)
    # the launches of the residual groups left `a` (and the downsample `b`) unwritten: add2 elides both, add3 its one conv
    assert not r0['masks'] and {1, 3} <= set(r1['masks'])
    # with fusion on, only the tensors no epilogue wrote reach the queue's launches -- the min/max launch in phase-1
    # forwards, the histogram launch in phase-2 forwards (eager ones: a graph replay queues nothing)
    for kind in ('minmax', 'hist') if two_phase else ('minmax',):
        q0, q1 = r0[kind], r1[kind]
        assert len(q0) == len(q1) and any(q0)
        for f0, f1 in zip(q0, q1):
            if not f0: continue
            assert f0.count(WRITTEN) >= EPILOGUE_WRITES
            assert WRITTEN not in f1 and len(f1) == len(f0) - f0.count(WRITTEN), (kind, f0, f1)


@gpu
@pytest.mark.parametrize('reuse', [False, True])
def test_a_requested_convolution_output_is_stored(reuse, deterministic_convs):
    """c3's output is `a` of the last residual group.  Asked for through output_names it comes back bit-equal to the unfused
    executor's in every forward of both phases; with reuse_activations the tensors of phase 1 are recorded for phase 2, and
    nothing is elided while they are."""
    r0 = _calibrate('kl', False, False, False, request='c3', reuse=reuse)
    r1 = _calibrate('kl', False, True, False, request='c3', reuse=reuse)
    _same_statistics(r0, r1, True)
    assert len(r0['requested']) == len(r1['requested']) > 0
    for t0, t1 in zip(r0['requested'], r1['requested']):
        assert torch.equal(t0.view(torch.int32), t1.view(torch.int32))
    if reuse:
        assert r1['replayed_batches'] > 0 and r1['masks'] and not any(r1['masks'])     # phase 1 recorded: every store kept
    else:
        assert 3 in r1['masks']                        # add2's group still elides; c3's group (requested) is not formed
