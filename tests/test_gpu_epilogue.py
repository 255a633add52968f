"""Convolution epilogues on MI355X: ppqhip_bias_act / ppqhip_bias_add_act against the PyTorch sequence they replace, bit for
bit, and the executor's fused forward against its op-by-op loop (graph outputs, every observed tensor, rendered scales)."""
import pytest
import torch
import torch.nn.functional as F

from ppq_amd import ffi, harness
from ppq_amd.observer import CalibrationHook

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits_equal(x: torch.Tensor, y: torch.Tensor) -> bool:
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _resnet_shapes(batch):
    """(conv name, conv input shape, weight shape, attributes, output shape, consumer type) of every ResNet-50 conv,
    from a meta-tensor walk of harness.resnet50_graph."""
    g = harness.resnet50_graph(seed=0)
    vals = {'input': torch.empty(batch, 3, 224, 224, device='meta')}
    rows = []
    for op in g.topological_sort():
        xs = [v.value.to('meta') if v.is_parameter else vals[v.name] for v in op.inputs]
        y = harness._forward(op, xs)
        if op.type == 'Conv':
            rows.append((op.name, tuple(xs[0].shape), tuple(xs[1].shape), op.attributes, tuple(y.shape),
                         op.outputs[0].dest_ops[0].type))
        vals[op.outputs[0].name] = y
    assert len(rows) == 53
    return rows


def _layout(t, cl):
    return t.contiguous(memory_format=torch.channels_last) if cl else t.contiguous()


def _specials(t: torch.Tensor, gen, nans=True) -> torch.Tensor:
    """Sprinkle -0.0, +-inf, NaNs with distinct payloads (when `nans`) and denormals over t (in place, storage order).
    NaNs go into ONE operand of every add: with two NaN operands the payload that survives is whichever the compiler
    puts in the instruction's first source -- unspecified in PyTorch's kernels as in this one."""
    flat = t.view(-1) if t.is_contiguous() else t.permute(0, 2, 3, 1).view(-1)     # storage order, a view
    n = flat.numel()
    vals = torch.tensor([-0.0, 0.0, float('inf'), float('-inf'), 1e-40, -1e-40, 1.5e-45], device=t.device)
    nan_vals = torch.tensor([0x7fc00001, 0x7fc12345, -0x00400001, 0x7f800001], dtype=torch.int32, device=t.device).view(torch.float32)
    k = max(1, n // 97)
    idx = torch.randint(0, n, (k,), generator=gen, device='cpu').to(t.device)
    pool = torch.cat([vals, nan_vals]) if nans else vals
    src = pool[torch.arange(k, device=t.device) % pool.numel()]
    flat[idx] = src
    return t


def _check_p1(shape, cl, gen, special=False):
    y = _layout(torch.randn(shape, generator=gen).to(DEV), cl)
    b = (torch.randn(shape[1], generator=gen) * 0.05).to(DEV)
    if special:
        _specials(y, gen)
        b[::7] = -0.0
    want = F.relu(y + b.view(1, -1, 1, 1))
    got = y.clone(memory_format=torch.preserve_format)
    assert ffi.bias_act_(got, b, relu=True)
    assert _bits_equal(got, want), (shape, cl)
    got = y.clone(memory_format=torch.preserve_format)
    assert ffi.bias_act_(got, b, relu=False)
    assert _bits_equal(got, y + b.view(1, -1, 1, 1))


def _check_p2(shape, cl, gen, with_b_bias, special=False):
    a = _layout(torch.randn(shape, generator=gen).to(DEV), cl)
    b = _layout(torch.randn(shape, generator=gen).to(DEV), cl)
    ba = (torch.randn(shape[1], generator=gen) * 0.05).to(DEV)
    bb = (torch.randn(shape[1], generator=gen) * 0.05).to(DEV) if with_b_bias else None
    if special:
        _specials(a, gen); _specials(b, gen, nans=False)
        ba[::5] = -0.0
    ra = a + ba.view(1, -1, 1, 1)
    rb = b + bb.view(1, -1, 1, 1) if with_b_bias else b
    want = F.relu(ra + rb)
    ga, gb = a.clone(memory_format=torch.preserve_format), b.clone(memory_format=torch.preserve_format)
    out = ffi.bias_add_act(ga, ba, gb, bb, relu=True)
    assert out is not None
    assert _bits_equal(ga, ra) and _bits_equal(gb, rb) and _bits_equal(out, want), (shape, cl, with_b_bias)
    assert out.stride() == a.stride()


@pytest.mark.parametrize('batch', [1, 32])
@pytest.mark.parametrize('cl', [False, True])
def test_kernels_bitwise_on_every_resnet50_shape(batch, cl):
    gen = torch.Generator().manual_seed(batch + 7 * cl)
    seen = set()
    for _, _, _, _, y, consumer in _resnet_shapes(batch):
        if (y, consumer) in seen: continue
        seen.add((y, consumer))
        if consumer == 'Relu': _check_p1(y, cl, gen)
        else:
            _check_p2(y, cl, gen, True)
            _check_p2(y, cl, gen, False)


@pytest.mark.parametrize('cl', [False, True])
def test_kernels_bitwise_odd_shapes_and_special_values(cl):
    gen = torch.Generator().manual_seed(3)
    for shape in [(1, 3, 5, 7), (3, 3, 7, 7), (2, 512, 7, 7), (1, 5, 3, 3), (1, 1, 1, 1), (2, 3, 1, 3), (1, 7, 11, 13),
                  (4, 64, 56, 56), (32, 2048, 7, 7)]:
        for special in (False, True):
            _check_p1(shape, cl, gen, special)
            _check_p2(shape, cl, gen, True, special)
            _check_p2(shape, cl, gen, False, special)


def test_unaligned_views_are_exact():
    gen = torch.Generator().manual_seed(5)
    base = torch.randn(1 + 2 * 3 * 5 * 5, generator=gen).to(DEV)
    y = base[1:].view(2, 3, 5, 5)                   # 4-B offset: the element-wise kernel
    b = torch.randn(3, generator=gen).to(DEV)
    want = F.relu(y + b.view(1, -1, 1, 1))
    assert ffi.bias_act_(y, b, relu=True)
    assert _bits_equal(y, want)


def test_binding_refuses_what_it_cannot_fuse():
    a = torch.randn(2, 4, 6, 6, device=DEV)
    b = torch.randn(4, device=DEV)
    assert not ffi.bias_act_(a[:, :, :, :3], b, relu=True)                 # not dense
    assert not ffi.bias_act_(a, b[:3], relu=True)                          # bias length
    assert not ffi.bias_act_(a.double(), b.double(), relu=True)            # dtype
    assert ffi.bias_add_act(a, b, a.contiguous(memory_format=torch.channels_last), None, relu=True) is None   # layouts differ
    assert ffi.bias_add_act(a, b, a, None, relu=True) is None              # aliased operands


@pytest.mark.parametrize('benchmark', [False, True])
def test_conv_bias_is_conv_then_add_on_every_resnet50_shape(benchmark):
    """What the fused path relies on: F.conv2d(x, w, b) == F.conv2d(x, w, None) + b, bit for bit."""
    gen = torch.Generator().manual_seed(11)
    prev = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = benchmark
    failed, checked = [], 0
    try:
        for cl in (False, True):
            for name, xs, ws, a, _, _ in _resnet_shapes(32):
                x = _layout(torch.randn(xs, generator=gen).to(DEV), cl)
                w = _layout((torch.randn(ws, generator=gen) * (2.0 / (ws[1] * ws[2] * ws[3])) ** 0.5).to(DEV), cl)
                b = (torch.randn(ws[0], generator=gen) * 0.05).to(DEV)
                kw = dict(stride=a.get('strides', 1), padding=a.get('pads', 0))
                y0 = F.conv2d(x, w, None, **kw)
                if not _bits_equal(y0, F.conv2d(x, w, None, **kw)):
                    continue        # the convolution itself does not repeat bit for bit: nothing to compare against
                checked += 1
                if not _bits_equal(F.conv2d(x, w, b, **kw), y0 + b.view(1, -1, 1, 1)): failed.append((name, cl))
    finally:
        torch.backends.cudnn.benchmark = prev
    assert not failed, failed
    assert checked >= 53, checked           # of 106 (shape, layout) pairs; measured with benchmark off: 85 repeat


@pytest.fixture
def deterministic_convs():
    """Some MIOpen convolutions of ResNet-50 (stride-2 3x3 at batch 32, most channels-last 14x14 / 28x28 ones) do not
    repeat bit for bit from call to call; fused and unfused forwards are compared with deterministic algorithms."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _calibrated_graph(method='kl', cfg3=False):
    g = harness.resnet50_graph(seed=0)
    if cfg3: harness.quantize_graph(g, method, symmetrical=False, weight_symmetrical=False, hist_bins=2048)
    else: harness.quantize_graph(g, method, hist_bins=2048)
    return g


def _recorded_forward(ex, g, x, fuse):
    from ppq_amd.observer import OperationObserver
    ex.fuse_epilogues = fuse
    hooks = {n: OperationObserver(op, monitor_parameter=False).hook for n, op in g.operations.items()}
    seen = {}
    orig = CalibrationHook._observe_all

    def spy(self, values, quant_configs):
        for v, c in zip(values, quant_configs):
            if c in self._observer_table: seen.setdefault(id(c), []).append(v.clone(memory_format=torch.preserve_format))
    CalibrationHook._observe_all = spy
    try:
        out = ex.forward(x, hooks=hooks)[0].clone()
    finally:
        CalibrationHook._observe_all = orig
    return out, seen


@pytest.mark.parametrize('cl', [False, True])
def test_whole_forward_and_observed_tensors_equal_fused_and_unfused(cl, deterministic_convs):
    g = _calibrated_graph()
    ex = harness.TorchExecutor(g, DEV)
    if cl: ex.use_channels_last()
    harness.ParameterQuantizePass().optimize(g)
    x = torch.rand(8, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV)
    out0, seen0 = _recorded_forward(ex, g, x, False)
    launches = []
    orig_p1, orig_p2 = ffi.bias_act_, ffi.bias_add_act
    ffi.bias_act_ = lambda *a, **k: launches.append(1) or orig_p1(*a, **k)
    ffi.bias_add_act = lambda *a, **k: launches.append(2) or orig_p2(*a, **k)
    try:
        out1, seen1 = _recorded_forward(ex, g, x, True)
    finally:
        ffi.bias_act_, ffi.bias_add_act = orig_p1, orig_p2
    assert launches.count(1) == 33 and launches.count(2) == 16
    assert _bits_equal(out0, out1)
    assert seen0.keys() == seen1.keys() and len(seen0) > 50
    for k in seen0:
        assert len(seen0[k]) == len(seen1[k])
        for u, v in zip(seen0[k], seen1[k]): assert _bits_equal(u, v)
    # no hooks, requested intermediate outputs (a requested tensor is never fused away) and forward_cached
    names = ['conv2_out', 'add6_out', 'relu6_out', next(iter(g.outputs))]
    ex.fuse_epilogues = False
    ref = [t.clone() for t in ex.forward(x, output_names=names)]
    ex.fuse_epilogues = True
    got = ex.forward(x, output_names=names)
    assert all(_bits_equal(u, v) for u, v in zip(ref, got))
    cache = {}
    got = ex.forward_cached(x, ['relu6_out'], cache)[0]
    assert _bits_equal(got, ref[2]) and 'add6_out' not in cache
    assert _bits_equal(ex.forward_cached(x, ['add6_out'], cache)[0], ref[1])


def _rendered(g):
    out = []
    for op in g.operations.values():
        for c, v in op.config_with_variable:
            if v.is_parameter: continue
            s, o = c.scale, c.offset
            out.append((op.name, int(getattr(c.state, 'value', c.state)),
                        None if s is None else s.detach().reshape(-1).cpu(), None if o is None else o.detach().reshape(-1).cpu()))
    return out


def _pass(method, cfg3, fuse, hip_graph, cl=False):
    from ppq_amd.calibration import RuntimeCalibrationPass
    g = _calibrated_graph(method, cfg3)
    ex = harness.TorchExecutor(g, DEV)
    ex.fuse_epilogues = fuse
    if cl: ex.use_channels_last()
    harness.ParameterQuantizePass().optimize(g)
    gen = torch.Generator().manual_seed(2)
    batches = [torch.rand(32, 3, 224, 224, generator=gen).to(DEV) for _ in range(8)]
    p = RuntimeCalibrationPass(method=method, check_steps=False, use_hip_graph=hip_graph)
    p.optimize(g, dataloader=batches, executor=ex, calib_steps=8)
    torch.cuda.synchronize()
    return _rendered(g), p.graph_replays


@pytest.mark.parametrize('method,cfg3', [('kl', False), ('mse', True), ('percentile', False)])
@pytest.mark.parametrize('hip_graph', [False, True])
def test_calibration_pass_renders_the_same_scales(method, cfg3, hip_graph, deterministic_convs):
    ref, _ = _pass(method, cfg3, False, hip_graph)
    got, replays = _pass(method, cfg3, True, hip_graph)
    if hip_graph and method != 'percentile': assert replays > 0
    assert len(ref) == len(got)
    for (n0, s0, a0, b0), (n1, s1, a1, b1) in zip(ref, got):
        assert n0 == n1 and s0 == s1
        for u, v in ((a0, a1), (b0, b1)):
            assert (u is None) == (v is None)
            if u is not None: assert torch.equal(u.view(torch.int32), v.view(torch.int32)), n0


def test_calibration_pass_channels_last_same_scales(deterministic_convs):
    ref, _ = _pass('kl', False, False, False, cl=True)
    got, _ = _pass('kl', False, True, False, cl=True)
    for (n0, s0, a0, b0), (n1, s1, a1, b1) in zip(ref, got):
        assert n0 == n1 and s0 == s1
        if a0 is not None: assert torch.equal(a0.view(torch.int32), a1.view(torch.int32)), n0
