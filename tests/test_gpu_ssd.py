"""GPU tests of SSD equalization: the three HIP entry points (csrc/ssd.hip) against the reference's recorded scales and
candidate parameters (tests/golden/ssd.npz, written on the CPU by tests/golden/make_ssd.py) and against
fake-quant-then-measure, and the pass that drives them (ppq_amd/ssd.py) against the recorded decisions, against its torch arm
on the device, and against the forward counts it promises."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import ssd_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXECUTABLE = [k for k, c in enumerate(SC.CASES) if c['executable']]
IDS = [SC.CASES[k]['name'] for k in EXECUTABLE]


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'ssd.npz')))


@pytest.fixture(autouse=True)
def deterministic_convolutions():
    """The arm comparisons need a forward that repeats its bits: ask the convolution library for its deterministic algorithms."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def _same(a, b) -> bool:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float32)
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _to_device(g):
    for v in g.variables.values():
        if v.is_parameter: v.value = v.value.to(DEV)
    return g


def _recorded(golden, k):
    out = []
    for it in range(1, SC.CASES[k]['iterations'] + 1):
        p = 0
        while f'c{k}_it{it}_p{p}_losses' in golden:
            out.append((it, p, f'c{k}_it{it}_p{p}_')); p += 1
    return out


def _states(golden, k):
    """[(iteration, pair index, key, {parameter name: value before this (iteration, pair)})] of case k."""
    state = {n[len(f'c{k}_init_'):]: v for n, v in golden.items() if n.startswith(f'c{k}_init_')}
    out = []
    for it, q, key in _recorded(golden, k):
        out.append((it, q, key, dict(state)))
        best = int(golden[key + 'best'])
        if best >= 0:
            pre = f'{key}cand{best}_'
            state.update({n[len(pre):]: v for n, v in golden.items() if n.startswith(pre)})
    return out


def _pass(k, **kw):
    from ppq_amd.ssd import SSDEqualizationPass
    return SSDEqualizationPass(iteration=SC._case(k)['iterations'], channel_ratio=SC.CHANNEL_RATIO, loss_threshold=SC.LOSS_THRESHOLD, **kw)


def _batches(k): return [b.to(DEV) for b in SC.case_batches(k)]


# ---- kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(SC.CASES)), ids=[c['name'] for c in SC.CASES])
def test_scales_kernel_gives_the_recorded_scales_bit_for_bit(golden, k):
    from ppq_amd import ffi
    from ppq_amd import ssd as SSD
    seen = 0
    for it, q, key, state in _states(golden, k):
        g = _to_device(SC.harness_graph(k, {n: torch.from_numpy(v.copy()) for n, v in state.items()}, quantize=False))
        pair = SSD.SSDEqualizationPass().collect_all_pairs(g)[q]
        C, seg1, seg2, _ = SSD.pair_geometry(pair)
        scales = torch.full((4, C), float('nan'), device=DEV)
        ranges = torch.full((2, C), float('nan'), device=DEV)
        ffi.ssd_scales_multi([(seg1, seg2, torch.from_numpy(golden[key + 'act']).to(DEV), SC.CHANNEL_RATIO, scales, ranges)])
        assert _same(ranges[0], golden[key + 'first']) and _same(ranges[1], golden[key + 'last']), (it, q)
        for algo in range(4): assert _same(scales[algo], golden[key + 'scales'][algo]), (SC.CASES[k]['name'], it, q, algo)
        seen += 1
    assert seen >= SC.CASES[k]['iterations']


def test_scales_kernel_takes_many_pairs_in_one_call_and_checks_extents(golden):
    from ppq_amd import ffi
    from ppq_amd import ssd as SSD
    k = SC.case_index('depthwise')
    g = _to_device(SC.harness_graph(k, quantize=False))
    pairs = SSD.SSDEqualizationPass().collect_all_pairs(g)
    items, outs = [], []
    for q, pair in enumerate(pairs):
        C, seg1, seg2, _ = SSD.pair_geometry(pair)
        outs.append((torch.empty((4, C), device=DEV), torch.empty((2, C), device=DEV)))
        items.append((seg1, seg2, torch.from_numpy(golden[f'c{k}_it1_p{q}_act']).to(DEV), SC.CHANNEL_RATIO) + outs[-1])
    ffi.ssd_scales_multi(items)
    for q in range(len(pairs)):
        if q == 0: assert _same(outs[q][0], golden[f'c{k}_it1_p{q}_scales'])      # (later pairs saw equalized parameters in the recording)
        assert torch.isfinite(outs[q][0]).all()
    C, seg1, seg2, _ = SSD.pair_geometry(pairs[0])
    short = (seg1[0].flatten()[:-1].contiguous(),) + seg1[1:]
    with pytest.raises(RuntimeError, match='reads element'):
        ffi.ssd_scales_multi([(short, seg2, torch.ones(C, device=DEV), 0.5, outs[0][0], outs[0][1])])


@pytest.mark.parametrize('k', range(len(SC.CASES)), ids=[c['name'] for c in SC.CASES])
def test_apply_kernel_gives_the_recorded_candidates_and_leaves_the_originals(golden, k):
    from ppq_amd import ffi
    from ppq_amd import ssd as SSD
    vec = scalar = 0
    for it, q, key, state in _states(golden, k):
        g = _to_device(SC.harness_graph(k, {n: torch.from_numpy(v.copy()) for n, v in state.items()}, quantize=False))
        pair = SSD.SSDEqualizationPass().collect_all_pairs(g)[q]
        C, _, _, applies = SSD.pair_geometry(pair)
        scales = torch.from_numpy(golden[key + 'scales']).to(DEV).contiguous()
        outs = {var.name: torch.full((4,) + tuple(var.value.shape), float('nan'), device=DEV) for var, *_ in applies}
        ffi.ssd_apply_multi([(var.value, outs[var.name], scales, run, inner, og, divide) for var, run, inner, og, divide in applies])
        for var, run, *_ in applies:
            assert _same(var.value, state[var.name]), var.name                                   # never written
            for algo in range(4): assert _same(outs[var.name][algo], golden[f'{key}cand{algo}_{var.name}']), (it, q, algo, var.name)
            if run % 4 == 0: vec += 1
            else: scalar += 1
    assert scalar > 0 and (vec > 0 or SC.CASES[k]['name'] in ('gemm', 'pool'))           # 16-B and 4-B paths
    big = torch.ones(160, device=DEV)
    x, out = big[:32].view(8, 4), big[16:144].view(4, 8, 4)                                # the output lies over the input
    with pytest.raises(RuntimeError, match='overlaps'):
        ffi.ssd_apply_multi([(x, out, torch.ones(4, 8, device=DEV), 4, 8, 0, False)])
    with pytest.raises(RuntimeError, match='reads scale'):
        ffi.ssd_apply_multi([(x, torch.empty(4, 8, 4, device=DEV), torch.ones(4, 7, device=DEV), 4, 8, 0, False)])


def _fq_then_measure(y, r, scale, offset, axis, qmin, qmax, rounding):
    from ppq_amd import ffi
    from ppq_amd.ffi import CUDA
    if axis is None: q = CUDA.LinearQuantize_T(y, scale, offset, qmin, qmax, rounding)
    else: q = CUDA.LinearQuantize_C(y, scale, offset, axis, qmin, qmax, rounding)
    return ffi.measure_rows_multi([(q, r, None)])[0]


@pytest.mark.parametrize('rounding', range(8))
def test_fq_measure_rows_is_bit_identical_to_fake_quant_then_measure(rounding):
    """Per-tensor and per-channel configs, every rounding policy, row lengths that are and are not multiples of 4, one row and
    many rows, and every size-dependent path of the row sums (a wave per row, a workgroup per row, split rows + fold)."""
    from ppq_amd import ffi
    gen = torch.Generator().manual_seed(100 + rounding)
    shapes = [(1, 3, 5, 7), (6, 4, 9, 9), (1, 8, 16, 16), (5, 6, 33, 35), (3, 16, 32, 32), (2, 12, 41, 43), (1, 1, 1, 1003), (7, 10)]
    checked = 0
    for shape in shapes:
        y = (torch.randn(shape, generator=gen) * 3).to(DEV)
        r = (torch.randn(shape, generator=gen) * 3).to(DEV)
        y.view(-1)[::17] = torch.round(y.view(-1)[::17] * 8) / 16                              # rounding ties for scale 1 / 16 * k
        C = shape[1]
        for axis, qmin, qmax in ((None, -128, 127), (None, 0, 255), (1, -128, 127), (1, 0, 15)):
            n = 1 if axis is None else C
            scale = (torch.rand(n, generator=gen) * 0.05 + 0.0625 / 4).to(DEV)
            if axis is None: scale = torch.full((1,), 0.0625, device=DEV)
            offset = (torch.randint(0, 200, (n,), generator=gen).float() if qmin == 0 else torch.zeros(n)).to(DEV)
            if qmin == 0 and qmax == 15: offset = offset + 300.0                                 # fake_quant(0) != 0: the padded slots
            want = _fq_then_measure(y, r, scale, offset, axis, qmin, qmax, rounding)
            got = ffi.fq_measure_rows_multi([(y, r, scale, offset, axis, qmin, qmax, rounding)])[0]
            assert got.shape == (shape[0], 4) and torch.equal(got.view(torch.int64), want.view(torch.int64)), (shape, axis, qmin, rounding)
            checked += 1
    # many jobs in one launch, results in caller-owned sums; an unaligned view (row start not 16-B aligned)
    y = torch.randn(4, 3, 11, 13, generator=gen).to(DEV); r = torch.randn(4, 3, 11, 13, generator=gen).to(DEV)
    base = torch.randn(2 * 3 * 11 * 13 + 1, generator=gen).to(DEV)
    y2, r2 = base[1:].view(2, 3, 11, 13), torch.randn(2, 3, 11, 13, generator=gen).to(DEV)
    s, o = torch.full((1,), 0.03, device=DEV), torch.zeros(1, device=DEV)
    sc, oc = torch.tensor([0.02, 0.05, 0.01], device=DEV), torch.tensor([3.0, 0.0, -2.0], device=DEV)
    sums = [torch.empty(4, 4, dtype=torch.float64, device=DEV), torch.empty(2, 4, dtype=torch.float64, device=DEV)]
    ffi.fq_measure_rows_multi([(y, r, s, o, None, -128, 127, rounding), (y2, r2, sc, oc, 1, -128, 127, rounding)], sums)
    assert torch.equal(sums[0], _fq_then_measure(y, r, s, o, None, -128, 127, rounding))
    assert torch.equal(sums[1], _fq_then_measure(y2.contiguous(), r2, sc, oc, 1, -128, 127, rounding))
    assert checked == 4 * len(shapes)
    with pytest.raises(RuntimeError):
        ffi.fq_measure_rows_multi([(y, r, sc, oc, None, -128, 127, rounding)])                  # 3 scales for a per-tensor config


# ---- the pass -------------------------------------------------------------------------------------------------------
def _run(k, use_kernels, executor_cls=None, **kw):
    from ppq_amd import harness
    g = _to_device(SC.harness_graph(k))
    ex = (executor_cls or harness.TorchExecutor)(g, DEV)
    p = _pass(k, use_kernels=use_kernels, **kw)
    p.optimize(g, dataloader=_batches(k), executor=ex, collate_fn=None, calib_steps=SC.CALIB_STEPS)
    return g, ex, p


@pytest.mark.parametrize('k', EXECUTABLE, ids=IDS)
def test_decisions_equal_the_recorded_ones(golden, k):
    """best_idx of every (iteration, pair) is the reference's.  The recorded decisions have a margin of 5 % (make_ssd.py), far
    beyond what a GPU convolution's rounding moves a loss by; the largest relative difference between the losses here and the
    recorded CPU losses is printed for profiles/r12_ssd.txt and not asserted."""
    g, ex, p = _run(k, True)
    worst = 0.0
    for it, q, key in _recorded(golden, k):
        h = p.history[(it - 1, q)]
        want = golden[key + 'losses']
        for a, b in zip([h['basic']] + h['losses'], want): worst = max(worst, abs(a - b) / abs(b))
        assert h['best_idx'] == int(golden[key + 'best']), (SC.CASES[k]['name'], it, q, h, want)
    print(f'ssd {SC.CASES[k]["name"]}: largest relative difference between the GPU losses and the recorded CPU losses: {worst:.3e}')
    for pair in p.pairs:
        for op in pair:
            for v in op.parameters: assert torch.equal(v.stored_value, v.value)
            for cfg in op.config.input_quantization_config + op.config.output_quantization_config:
                assert cfg.state.name in ('INITIAL', 'PASSIVE_INIT', 'OVERLAPPED', 'FP32'), (op.name, cfg.state)


@pytest.mark.parametrize('k', EXECUTABLE, ids=IDS)
def test_kernel_arm_equals_torch_arm_bit_for_bit(k):
    from ppq_amd import harness
    g = _to_device(SC.harness_graph(k))
    ex = harness.TorchExecutor(g, DEV)
    x = _batches(k)[0]
    first, second = ex.forward(x), ex.forward(x)
    assert all(torch.equal(a, b) for a, b in zip(first, second)), \
        'precondition: the forward of the case graph does not repeat its bits on this device, the arms cannot be compared bit for bit'
    ga, _, pa = _run(k, True)
    gb, _, pb = _run(k, False)
    assert pa.history.keys() == pb.history.keys() and len(pa.history) == len(pa.pairs) * SC.CASES[k]['iterations']
    for key in pa.history:
        a, b = pa.history[key], pb.history[key]
        assert a['best_idx'] == b['best_idx'], key
        assert a['basic'] == b['basic'] and a['losses'] == b['losses'], (key, a, b)
    for name, v in ga.variables.items():
        if v.is_parameter: assert _same(v.value, gb.variables[name].value), name
    assert pa.stats['accepted'] == pb.stats['accepted']


def test_kernel_arm_equals_torch_arm_on_a_pair_wider_than_a_workgroup():
    """Conv(3 -> 264) -> Relu -> Conv(264 -> 40), per-tensor weights (ssd_cases.WIDE, not a recorded case): 264 channels are two
    trips of the scales kernel over the channels, 360 elements per channel of the last weight two trips of the ranges kernel, and
    the 95 040 elements of the last weight 372 workgroups of the apply kernel.  Bit for bit as on the case graphs -- and at least
    one candidate is accepted, so that a write-back at this size takes place and the second iteration starts from it."""
    from ppq_amd import harness
    case = SC.WIDE
    assert case not in SC.CASES and case['per_channel'] is False
    g = _to_device(SC.harness_graph(case))
    ex = harness.TorchExecutor(g, DEV)
    x = _batches(case)[0]
    first, second = ex.forward(x), ex.forward(x)
    assert all(torch.equal(a, b) for a, b in zip(first, second)), \
        'precondition: the forward of the wide graph does not repeat its bits on this device, the arms cannot be compared bit for bit'
    ga, _, pa = _run(case, True)
    gb, _, pb = _run(case, False)
    assert [[op.name for op in pair] for pair in pa.pairs] == [['c1', 'r1', 'c2']]
    assert pa.history.keys() == pb.history.keys() and len(pa.history) == len(pa.pairs) * case['iterations']
    for key in pa.history:
        a, b = pa.history[key], pb.history[key]
        assert a['best_idx'] == b['best_idx'], key
        assert a['basic'] == b['basic'] and a['losses'] == b['losses'], (key, a, b)
    for name, v in ga.variables.items():
        if v.is_parameter: assert _same(v.value, gb.variables[name].value), name
    assert pa.stats['accepted'] == pb.stats['accepted']
    print('ssd wide: accepted', pa.stats['accepted'], 'history', pa.history)
    assert any(h['best_idx'] >= 0 for h in pa.history.values()), pa.history
    assert not _same(ga.variables['c2_w'].value, SC.case_parameters(case)['c2_w'])                 # the write-back happened
    assert pa.stats['launches'] > 0


def _counting():
    from ppq_amd import harness

    class Counting(harness.TorchExecutor):
        calls = 0

        def forward(self, *a, **kw):
            self.calls += 1
            return super().forward(*a, **kw)
    return Counting


@pytest.mark.parametrize('k', [SC.case_index('chain'), SC.case_index('pool')], ids=['chain', 'pool'])
def test_forward_counts(k):
    """The torch arm makes the reference's number of executor calls -- per (iteration, pair) calib_steps for the range and, for
    each of the five evaluations, two calibrations of calib_steps and the loss batches; the kernel arm at most one per distinct
    batch per (iteration, pair)."""
    from math import ceil
    instances = None
    for use_kernels in (False, True):
        g, ex, p = _run(k, use_kernels, _counting())
        instances = len(p.pairs) * SC.CASES[k]['iterations']
        steps = p.stats['calib_steps']
        assert steps == SC.CALIB_STEPS
        loss_batches = ceil(steps / SC.BATCHES) * SC.BATCHES
        assert p.stats['prefix_forwards'] == ex.calls
        if use_kernels:
            assert 0 < ex.calls <= SC.BATCHES * instances
            assert p.stats['launches'] > 0
        else: assert ex.calls == instances * (steps + 5 * (2 * steps + loss_batches))
        assert p.stats['pair_forwards'] > 0
    assert instances > 0


def test_ssd_lowers_the_graph_error_on_per_tensor_weights():
    """`chain` with per-tensor weights: SSD, then ParameterQuantizePass + RuntimeCalibrationPass; the SNR error at the graph's
    output is strictly lower than for the same pipeline without SSD."""
    from ppq_amd import harness
    from ppq_amd import lib as PFL
    from ppq_amd.analyse import graphwise_error_analyse
    from ppq_amd.calibration import RuntimeCalibrationPass
    from ppq_amd.ssd import SSDEqualizationPass
    k = SC.case_index('chain')
    assert SC.CASES[k]['per_channel'] is False
    errors = {}
    for with_ssd in (False, True):
        g = _to_device(SC.harness_graph(k))
        ex = harness.TorchExecutor(g, DEV)
        passes = [harness.ParameterQuantizePass(), RuntimeCalibrationPass()]
        if with_ssd: passes.insert(0, SSDEqualizationPass(iteration=SC.CASES[k]['iterations']))
        PFL.Pipeline(passes).optimize(graph=g, dataloader=_batches(k), executor=ex, collate_fn=None, calib_steps=SC.CALIB_STEPS,
                                      verbose=False)
        report = graphwise_error_analyse(g, DEV, _batches(k), method='snr', steps=SC.BATCHES, verbose=False, executor=ex)
        errors[with_ssd] = report['c3']
        if with_ssd: assert passes[0].stats['accepted'].get(-1, 0) < len(passes[0].history)
    print('ssd chain: snr error at the graph output without / with SSD:', errors[False], errors[True])
    assert errors[True] < errors[False], errors


def test_pass_runs_in_a_pipeline_and_prints_only_when_verbose(capsys):
    from ppq_amd import harness
    from ppq_amd import lib as PFL
    from ppq_amd.ssd import SSDEqualizationPass
    k = SC.case_index('pool')
    g = _to_device(SC.harness_graph(k))
    p = SSDEqualizationPass(iteration=1)
    PFL.Pipeline([p]).optimize(graph=g, dataloader=_batches(k), executor=harness.TorchExecutor(g, DEV), collate_fn=None,
                               calib_steps=SC.CALIB_STEPS, verbose=False)
    assert capsys.readouterr().out == ''
    assert p.stats['pairs'] == 1 and sum(p.stats['accepted'].values()) == 1 and len(p.history) == 1
    g = _to_device(SC.harness_graph(k))
    SSDEqualizationPass(iteration=1, verbose=True).optimize(g, dataloader=_batches(k), executor=harness.TorchExecutor(g, DEV),
                                                            collate_fn=None, calib_steps=SC.CALIB_STEPS)
    out = capsys.readouterr().out
    assert 'Now Processing Pair 1/1: c1--r1--p1--c2' in out and 'Loss Before Equalization' in out


def test_mixed_devices_are_refused():
    from ppq_amd import harness
    from ppq_amd.ssd import SSDEqualizationPass
    k = SC.case_index('chain')
    g = SC.harness_graph(k)
    g.variables['c2_w'].value = g.variables['c2_w'].value.to(DEV)
    with pytest.raises(TypeError, match='partly on the GPU and partly not'):
        SSDEqualizationPass().optimize(g, dataloader=SC.case_batches(k), executor=None, collate_fn=None, calib_steps=SC.CALIB_STEPS)
