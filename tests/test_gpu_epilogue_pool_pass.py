"""RuntimeCalibrationPass over a graph whose stem is Conv -> Relu -> MaxPool: with fuse_epilogues on the stem runs as ONE pooled
epilogue launch with the Relu observer's sink in it, in both phases, and the Relu tensor is not stored -- and ranges,
histograms, scales and offsets are, bit for bit, those of the unfused executor (deterministic convolutions)."""
import pytest
import torch

from ppq_amd import ffi, harness

DEV = 'cuda:0'
gpu = pytest.mark.gpu
WINDOW = (3, 2, 1)


@pytest.fixture
def deterministic_convs():
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _graph(seed=0):
    """Conv(3 -> 8, 3x3) -> Relu -> MaxPool(3, 2, 1) -> Conv -> Relu -> GAP -> Flatten -> Gemm."""
    gen = torch.Generator().manual_seed(seed)
    g = harness.BaseGraph('epilogue_pool')
    x = g.create_variable('input'); g.inputs['input'] = x

    def conv(inp, cin, cout, name):
        w = g.create_variable(name + '_w', harness._he([cout, cin, 3, 3], gen), True)
        b = g.create_variable(name + '_b', torch.randn(cout, generator=gen) * 0.1, True)
        return g.create_operation('Conv', name, [inp, w, b], {'strides': 1, 'pads': 1})

    y = g.create_operation('Relu', 'relu1', [conv(x, 3, 8, 'c1')])
    y = g.create_operation('MaxPool', 'pool', [y], {'kernel_shape': WINDOW[0], 'strides': WINDOW[1], 'pads': WINDOW[2]})
    y = g.create_operation('Relu', 'relu2', [conv(y, 8, 8, 'c2')])
    y = g.create_operation('Flatten', 'flatten', [g.create_operation('GlobalAveragePool', 'gap', [y])])
    w = g.create_variable('fc_w', torch.randn([10, 8], generator=gen) * 0.3, True)
    y = g.create_operation('Gemm', 'fc', [y, w, g.create_variable('fc_b', torch.zeros(10), True)])
    g.outputs[y.name] = y
    return g


def _calibrate(method, fuse, hip_graph):
    """Run the pass.  Returns per phase every observer's folded range and histogram, the rendered configs, the groups the
    executor ran and, per sink launch, (kind, pool window, store)."""
    from ppq_amd.calibration import RuntimeCalibrationPass
    g = _graph()
    harness.quantize_graph(g, method, hist_bins=2048)
    ex = harness.TorchExecutor(g, DEV)
    ex.fuse_epilogues = fuse
    harness.ParameterQuantizePass().optimize(g)
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(4, 3, 32, 32, generator=gen) * 2).to(DEV) for _ in range(5)]
    p = RuntimeCalibrationPass(method=method, check_steps=False, use_hip_graph=hip_graph)
    r = {'phases': [], 'groups': [], 'launches': []}
    orig_render, orig_run = p._render, ex._run_epilogue
    orig_stats, orig_hist = ffi.bias_act_stats_, ffi.bias_act_hist_

    def render():
        orig_render()
        snap = []
        for name, op_ob in p._observers.items():
            for ob in op_ob.observers():
                rng = getattr(ob, '_range', None)
                hist = ob.histogram() if hasattr(ob, 'histogram') else None
                snap.append((name, type(ob).__name__, None if rng is None else rng.clone(), None if hist is None else hist.clone()))
        r['phases'].append(snap)

    def run_epilogue(grp, raw_of, hooks):
        r['groups'].append((tuple(m.name for m in grp.ops), bool(hooks)))
        return orig_run(grp, raw_of, hooks)

    def spy(kind, real):
        def launch(y, bias, relu, job, pool=None, store=True):
            out = real(y, bias, relu, job, pool=pool, store=store)
            if pool is not None: r['launches'].append((kind, tuple(pool), store, out is not None))
            return out
        return launch
    p._render, ex._run_epilogue = render, run_epilogue
    ffi.bias_act_stats_, ffi.bias_act_hist_ = spy('minmax', orig_stats), spy('hist', orig_hist)
    try:
        p.optimize(g, dataloader=batches, executor=ex, calib_steps=len(batches))
        torch.cuda.synchronize()
    finally:
        ffi.bias_act_stats_, ffi.bias_act_hist_ = orig_stats, orig_hist
    r['rendered'] = [(op.name, int(getattr(c.state, 'value', c.state)), c.scale, c.offset)
                     for op in g.operations.values() for c, v in op.config_with_variable if not v.is_parameter]
    r['replays'] = p.graph_replays
    return r


@gpu
@pytest.mark.parametrize('method,hip_graph', [('kl', False), ('kl', True), ('minmax', False), ('minmax', True)])
def test_statistics_and_scales_equal_fused_and_unfused(method, hip_graph, deterministic_convs):
    r0 = _calibrate(method, False, hip_graph)
    r1 = _calibrate(method, True, hip_graph)
    if hip_graph: assert r1['replays'] > 0
    phases = 2 if method == 'kl' else 1
    assert len(r0['phases']) == len(r1['phases']) == phases
    for s0, s1 in zip(r0['phases'], r1['phases']):
        assert len(s0) == len(s1) and len(s0) > 0
        for (n0, t0, rng0, h0), (n1, t1, rng1, h1) in zip(s0, s1):
            assert (n0, t0) == (n1, t1) and (rng0 is None) == (rng1 is None) and (h0 is None) == (h1 is None)
            if rng0 is not None: assert torch.equal(rng0.view(torch.int32), rng1.view(torch.int32)), (n0, rng0, rng1)
            if h0 is not None: assert torch.equal(h0, h1), n0
    assert len(r0['rendered']) == len(r1['rendered']) > 0
    for (n0, st0, sc0, of0), (n1, st1, sc1, of1) in zip(r0['rendered'], r1['rendered']):
        assert (n0, st0) == (n1, st1)
        for u, v in ((sc0, sc1), (of0, of1)):
            assert (u is None) == (v is None)
            if u is not None: assert torch.equal(u.view(torch.int32), v.view(torch.int32)), n0
    # the pooled group was planned and ran in the hooked forwards; unfused, no group ran at all
    assert not r0['groups'] and not r0['launches']
    assert (('c1', 'relu1', 'pool'), True) in r1['groups'] and (('c2', 'relu2'), True) in r1['groups']
    # every sink launch of the stem took place, pooled, and left the Relu tensor unwritten -- in both phases
    kinds = {'minmax', 'hist'} if method == 'kl' else {'minmax'}
    assert {k for k, *_ in r1['launches']} == kinds
    assert all(launch[1:] == (WINDOW, False, True) for launch in r1['launches']), r1['launches']
