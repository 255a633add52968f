"""The statistics variant of the convolution epilogues (ppqhip_bias_act_stats / ppqhip_bias_add_act_stats): what it stores and
the running range it folds must equal, bit for bit, the plain epilogue launch followed by the observers' own min/max launch on
the tensors it wrote -- at the kernel level (every branch of the kernel) and through RuntimeCalibrationPass (fuse_epilogues
True against False, where the histograms of phase 2 must agree too).  Everything is exact: min/max bit patterns, integer
counts, identical tensors."""
import pytest
import torch

from ppq_amd import CUDA, ffi, harness
from ppq_amd.observer import ObservationQueue, _range_seed

DEV = 'cuda:0'
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- host: the queue's bookkeeping
def test_queue_prepay_drops_the_matching_pair_once():
    q = ObservationQueue()
    v, w = torch.zeros(8), torch.zeros(8)
    slots, other = torch.zeros(4), torch.zeros(4)
    q.prepay(v, slots)
    q.add_minmax(v, other)                    # same tensor, a different buffer: queued
    q.add_minmax(w, slots)                    # same buffer, a different tensor: queued
    assert len(q) == 2
    q.add_minmax(v, slots)                    # the prepaid pair: dropped ...
    assert len(q) == 2
    q.add_minmax(v, slots)                    # ... once
    assert len(q) == 3
    # a size-triggered launch in the middle of a forward keeps what is prepaid, flush() forgets it
    q.prepay(w, other)
    q._minmax, q._hist, q._bytes = [], {}, 0
    q._launch()
    assert q._prepaid
    q.flush()
    assert not q._prepaid and len(q) == 0


# ---------------------------------------------------------------------------------------------- kernels
def _bits_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _inputs(shape, gen, special):
    """(conv output, bias): with `special`, channel 0 has bias 0 and its first elements are -0.0, +0.0, NaN and +-inf."""
    y = torch.randn(shape, generator=gen)
    bias = torch.randn(shape[1], generator=gen) * 0.3
    if special:
        bias[0] = 0.0
        flat = y.view(-1)
        vals = [-0.0, 0.0, float('nan'), float('inf'), float('-inf')]
        n = min(len(vals), shape[2] * shape[3], flat.numel())
        flat[:n] = torch.tensor(vals[:n])
    return y.to(DEV), bias.to(DEV)


class _Stat:
    """One observer-shaped running range and the reference / fused ways of feeding it."""
    def __init__(self):
        self.buf = _range_seed(torch.device(DEV))[1].clone()

    def job(self): return ('minmax', self.buf)

    def observe(self, t): CUDA.MinMax_T_Slots(t, self.buf)          # the observers' own launch

    def folded(self): return CUDA.MinMax_Slots_Finish(self.buf, _range_seed(torch.device(DEV))[0].clone())


def _same(s0: _Stat, s1: _Stat):
    a, b = s0.folded(), s1.folded()
    assert _bits_equal(a, b), (a, b)


def _check(shape, mode, special, gen, launches=1, relu=True, channels_last=False):
    """mode: 'p1' bias_act; 'p2' bias_add_act without bias_b (two sinks); 'p2b' with bias_b (three sinks)."""
    def inputs():
        t, bias = _inputs(shape, gen, special)
        return (t.contiguous(memory_format=torch.channels_last) if channels_last else t), bias
    n_t = {'p1': 1, 'p2': 2, 'p2b': 3}[mode]
    ref = [_Stat() for _ in range(n_t)]
    got = [_Stat() for _ in range(n_t)]
    for _ in range(launches):                  # several launches: the running statistic
        y, bias = inputs()
        if mode == 'p1':
            y1 = y.clone()
            assert ffi.bias_act_(y, bias, relu=relu)
            ref[0].observe(y)
            assert ffi.bias_act_stats_(y1, bias, relu, got[0].job())
            assert _bits_equal(y, y1)
            continue
        b, bias_b = inputs()
        if mode == 'p2': bias_b = None
        y1, b1 = y.clone(), b.clone()
        out = ffi.bias_add_act(y, bias, b, bias_b, relu=relu)
        for s, t in zip(ref, [y, b, out] if mode == 'p2b' else [y, out]): s.observe(t)
        jobs = [g.job() for g in got]
        out1 = ffi.bias_add_act_stats(y1, bias, b1, bias_b, relu, jobs[0], jobs[1] if mode == 'p2b' else None, jobs[-1])
        assert out1 is not None
        assert _bits_equal(y, y1) and _bits_equal(b, b1) and _bits_equal(out, out1)
    for s0, s1 in zip(ref, got): _same(s0, s1)


# [1,8,4,4]: fewer tiles than workgroups; [1,3,5,7]: n % 4 != 0, scalar tail, per-element channels; [2,16,7,7]: 7x7 planes;
# [2,64,96,96]: 1.18 M elements, the two-float4 tile, a ragged last tile; [4,64,96,96]: 2.36 M elements are 576 tiles of
# 512 lanes x 2 float4, more than the 512-workgroup grid cap: a workgroup walks several tiles with the ping-pong prefetch
SHAPES = [(1, 8, 4, 4), (1, 3, 5, 7), (2, 16, 7, 7), (2, 64, 96, 96), (4, 64, 96, 96)]


@gpu
@pytest.mark.parametrize('mode', ['p1', 'p2', 'p2b'])
def test_stats_kernels_equal_epilogue_then_observer_launch(mode):
    gen = torch.Generator().manual_seed(7)
    for shape in SHAPES:
        for special in (False, True):
            _check(shape, mode, special, gen)


# The launch is picked by (tile, relu, per-float4 or per-element channels) for each of the three operand forms: the shapes above
# reach every tile and channel geometry with ReLU only, and the per-element geometry only below 2^20 elements.  Here: no ReLU
# on either tile with either geometry -- channels-last makes [2,64,96,96] a large tensor with per-element channels -- and
# that last shape with ReLU too.  The oracle is the same: the plain launch with that `relu`, then the observers' own launch.
@gpu
@pytest.mark.parametrize('mode', ['p1', 'p2', 'p2b'])
def test_stats_kernels_without_relu_and_large_per_element_channels(mode):
    gen = torch.Generator().manual_seed(11)
    for shape, channels_last, relu in (((1, 8, 4, 4), False, False), ((1, 3, 5, 7), False, False), ((2, 64, 96, 96), False, False),
                                       ((2, 64, 96, 96), True, False), ((2, 64, 96, 96), True, True)):
        _check(shape, mode, True, gen, relu=relu, channels_last=channels_last)


@gpu
def test_stats_accumulate_over_consecutive_launches():
    gen = torch.Generator().manual_seed(8)
    for mode in ('p1', 'p2b'):
        _check((2, 16, 7, 7), mode, True, gen, launches=2)
        _check((2, 64, 96, 96), mode, False, gen, launches=2)


@gpu
def test_signed_zero_minimum_has_the_same_bits():
    """A tensor whose smallest values are -0.0 AND +0.0, in different lanes, waves and workgroups: the fold orders -0.0 below
    +0.0, so the range does not depend on who met which zero first -- in either path."""
    gen = torch.Generator().manual_seed(12)
    shape = (1, 1, 96, 96)                                # 2304 float4: five tiles of the one-float4 kernel
    y = torch.rand(shape, generator=gen) + 0.5
    y.view(-1)[::7] = 0.0
    y.view(-1)[5::1001] = -0.0
    y, b = y.to(DEV), (torch.rand(shape, generator=gen) + 0.5).to(DEV)
    bias = torch.tensor([-0.0], device=DEV)               # -0.0 + -0.0 = -0.0, +0.0 + -0.0 = +0.0
    y1, b1, ref, got = y.clone(), b.clone(), [_Stat(), _Stat()], [_Stat(), _Stat()]
    out = ffi.bias_add_act(y, bias, b, None, relu=True)
    ref[0].observe(y); ref[1].observe(out)
    out1 = ffi.bias_add_act_stats(y1, bias, b1, None, True, got[0].job(), None, got[1].job())
    assert out1 is not None and _bits_equal(y, y1) and _bits_equal(out, out1)
    assert int(ref[0].folded()[0:1].view(torch.int32)) == -2 ** 31          # the minimum of `a` is -0.0
    for s0, s1 in zip(ref, got): _same(s0, s1)


@gpu
def test_channels_last_layout():
    gen = torch.Generator().manual_seed(9)
    y, bias = _inputs((2, 24, 9, 9), gen, True)
    y = y.contiguous(memory_format=torch.channels_last)
    y1, ref, got = y.clone(memory_format=torch.preserve_format), _Stat(), _Stat()
    assert ffi.bias_act_(y, bias, relu=True)
    ref.observe(y)
    assert ffi.bias_act_stats_(y1, bias, True, got.job())
    assert _bits_equal(y, y1)
    _same(ref, got)


@gpu
def test_not_fused_leaves_everything_to_the_fallback():
    """An unaligned view launches NOTHING: tensor and slots stay untouched, and the plain epilogue plus the observers' launch
    give the range of an aligned copy.  A job the kernels have no sink for is not fused either."""
    gen = torch.Generator().manual_seed(10)
    y, bias = _inputs((2, 3, 5, 5), gen, True)
    base = torch.empty(1 + y.numel(), device=DEV)
    view = base[1:].view(y.shape)                # a one-float offset: not 16-B aligned
    view.copy_(y)
    got, ref = _Stat(), _Stat()
    before = got.buf.clone()
    assert not ffi.bias_act_stats_(view, bias, True, got.job())
    assert _bits_equal(view, y) and _bits_equal(got.buf, before)
    assert ffi.bias_act_(view, bias, relu=True) and ffi.bias_act_(y, bias, relu=True)
    got.observe(view); ref.observe(y)
    assert _bits_equal(view, y)
    _same(ref, got)
    y0 = y.clone()
    rows = torch.zeros(CUDA.hist_rows(), 2048, dtype=torch.int32, device=DEV)
    assert not ffi.bias_act_stats_(y, bias, True, ('hist', rows, False, 0.01, 0.0))
    assert not ffi.bias_act_stats_(y, bias, True, None)
    assert _bits_equal(y, y0) and int(rows.sum()) == 0


# ---------------------------------------------------------------------------------------------- the calibration pass
@pytest.fixture
def deterministic_convs():
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


WIDTH, HW, BATCH = 16, 20, 4


def _graph(seed=0):
    """Conv-Relu (one bias_act group), Conv + Conv-Add-Relu (bias_add_act, three stored tensors), Conv + identity-Add-Relu
    (two stored tensors), then GAP-Flatten-Gemm: tensors no epilogue writes."""
    gen = torch.Generator().manual_seed(seed)
    g = harness.BaseGraph('epilogue_stats')
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


EPILOGUE_WRITES = 6               # relu1; c2, down, relu2; c3, relu3


def _calibrate(method, cfg3, fuse, hip_graph):
    """Run the pass; returns (per phase: every observer's folded range and histogram, rendered configs, per forward: shapes
    of the tensors that reached the queue's min/max launch)."""
    from ppq_amd.calibration import RuntimeCalibrationPass
    g = _graph()
    if cfg3: harness.quantize_graph(g, method, symmetrical=False, weight_symmetrical=False, hist_bins=2048)
    else: harness.quantize_graph(g, method, hist_bins=2048)
    ex = harness.TorchExecutor(g, DEV)
    ex.fuse_epilogues = fuse
    harness.ParameterQuantizePass().optimize(g)
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(BATCH, 3, HW, HW, generator=gen) * 2).to(DEV) for _ in range(5)]
    p = RuntimeCalibrationPass(method=method, check_steps=False, use_hip_graph=hip_graph)
    phases, queued = [], []
    orig_render, orig_flush = p._render, ObservationQueue.flush

    def render():
        orig_render()
        snap = []
        for name, op_ob in p._observers.items():
            for ob in op_ob.observers():
                rng = getattr(ob, '_range', None)
                hist = ob.histogram() if hasattr(ob, 'histogram') else None
                snap.append((name, type(ob).__name__, None if rng is None else rng.clone(), None if hist is None else hist.clone()))
        phases.append(snap)

    def flush(self):
        queued.append([tuple(v.shape) for v, _ in self._minmax])
        orig_flush(self)
    p._render, ObservationQueue.flush = render, flush
    try:
        p.optimize(g, dataloader=batches, executor=ex, calib_steps=len(batches))
        torch.cuda.synchronize()
    finally:
        ObservationQueue.flush = orig_flush
    rendered = [(op.name, int(getattr(c.state, 'value', c.state)), c.scale, c.offset)
                for op in g.operations.values() for c, v in op.config_with_variable if not v.is_parameter]
    return phases, rendered, queued, p.graph_replays


@gpu
@pytest.mark.parametrize('method,cfg3,hip_graph', [('kl', False, False), ('kl', False, True), ('mse', False, False), ('mse', True, False),
                                                   ('mse', True, True), ('minmax', False, False), ('minmax', True, False),
                                                   ('percentile', False, False)])
def test_calibration_pass_statistics_and_scales_equal_fused_and_unfused(method, cfg3, hip_graph, deterministic_convs):
    ph0, r0, q0, _ = _calibrate(method, cfg3, False, hip_graph)
    ph1, r1, q1, replays = _calibrate(method, cfg3, True, hip_graph)
    if hip_graph: assert replays > 0
    assert len(ph0) == len(ph1) and len(ph0) == (1 if method in ('minmax', 'percentile') else 2)
    for s0, s1 in zip(ph0, ph1):
        assert len(s0) == len(s1) and len(s0) > 0
        for (n0, t0, rng0, h0), (n1, t1, rng1, h1) in zip(s0, s1):
            assert (n0, t0) == (n1, t1) and (rng0 is None) == (rng1 is None) and (h0 is None) == (h1 is None)
            if rng0 is not None: assert _bits_equal(rng0, rng1), (n0, rng0, rng1)
            if h0 is not None: assert torch.equal(h0, h1), n0
    assert len(r0) == len(r1)
    for (n0, st0, sc0, of0), (n1, st1, sc1, of1) in zip(r0, r1):
        assert (n0, st0) == (n1, st1)
        for u, v in ((sc0, sc1), (of0, of1)):
            assert (u is None) == (v is None)
            if u is not None: assert torch.equal(u, v), n0
    if method == 'percentile': return                      # no sink exists: it simply still agrees
    # with fusion on, only the tensors no epilogue wrote reach the queue's min/max launch (the forwards of the min/max phase;
    # eager ones: a graph replay queues nothing)
    written = (BATCH, WIDTH, HW, HW)
    assert len(q0) == len(q1) and any(q0)
    for f0, f1 in zip(q0, q1):
        if not f0: continue
        assert f0.count(written) >= EPILOGUE_WRITES
        assert written not in f1 and len(f1) == len(f0) - f0.count(written), (f0, f1)
