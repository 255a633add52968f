"""Host-side tests of layerwise equalization (ppq_amd/equalization.py): pair discovery against the reference's recorded pair
lists, the torch arm against the reference's recorded scales and parameters bit for bit (tests/golden/equalization.npz and
equalization_pairs.json, written by tests/golden/make_equalization.py), the level schedule, function preservation, the
constructor's surface and the refusals.  No GPU needed."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import equalization_cases as EC  # noqa: E402

from ppq_amd import harness  # noqa: E402
from ppq_amd import equalization as EQ  # noqa: E402
from ppq_amd.measure import torch_snr_error  # noqa: E402

SNR_BOUND = 1e-7                     # the bound of the reference's own tests/test_layerwise_equalization.py


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'equalization.npz')))


@pytest.fixture(scope='module')
def book():
    with open(os.path.join(HERE, 'golden', 'equalization_pairs.json')) as f: return json.load(f)


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same(a, b) -> bool:
    """Bit equality; NaN equals NaN whatever its payload (the nan_key case)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)): return False
    keep = ~np.isnan(a)
    return np.array_equal(_bits(a[keep]), _bits(b[keep]))


def _names(pairs):
    return [[[op.name for op in p.upstream_layers], [op.name for op in p.downstream_layers]] for p in pairs]


def _pass(k, **kw):
    case = EC.CASES[k]
    return EQ.LayerwiseEqualizationPass(iterations=case['iterations'], value_threshold=EC.VALUE_THRESHOLD,
                                        including_bias=case['including_bias'], including_act=case['including_act'], **kw)


def _activations(golden, k, graph):
    pre = f'c{k}_act_'
    return {n[len(pre):]: torch.from_numpy(v) for n, v in golden.items() if n.startswith(pre)} or None


def _run_case(golden, k, **kw):
    g = EC.harness_graph(k)
    p = _pass(k, **kw)
    p.keep_scales = True
    p.optimize(g, dataloader=EC.case_batches(k), executor=None, activations=_activations(golden, k, g))
    return g, p


def test_case_inputs_are_the_recorded_ones(golden):
    for k in range(len(EC.CASES)):
        for name, t in EC.case_parameters(k).items(): assert _same(t, golden[f'c{k}_init_{name}']), (k, name)


def test_recorded_cases_meet_the_conditions_the_comparisons_rely_on(golden):
    """Every case has first-iteration channels at s == 1 (the threshold) and at s != 1; the clip acts at 0.1 and at 10 somewhere;
    the NaN and the all-zero channel are there; the grouped downstream's key order is not the natural one."""
    low = high = 0
    for k, case in enumerate(EC.CASES):
        s = np.concatenate([v for n, v in golden.items() if n.startswith(f'c{k}_scale_it1_')])
        assert (s == 1).sum() > 0 and (s != 1).sum() > 0, case['name']
        low += int((s == np.float32(0.1)).sum()); high += int((s == 10).sum())
    assert low > 0 and high > 0
    names = [c['name'] for c in EC.CASES]
    assert np.isnan(golden[f'c{names.index("nan_key")}_scale_it1_p0']).sum() == 1
    k = names.index('zero_act')
    assert not golden[f'c{k}_init_c1_w'][3].any() and golden[f'c{k}_scale_it1_p0'][3] == 10
    k = names.index('grouped')
    w = torch.from_numpy(golden[f'c{k}_init_g2_w'])
    reference_order = EQ.key_value_from_downstream(EC.harness_graph(k).operations['g2']).abs().amax(dim=1)
    assert not torch.equal(reference_order, EC.natural_order_keys(w, 2))
    r = torch.arange(8)
    assert torch.equal(reference_order, EC.natural_order_keys(w, 2)[(r % 2) * 4 + r // 2])     # row r reads channel (r % G) * in/G + r // G
    assert {len(v) for v in golden.values() if v.ndim == 1} and all(v.dtype == np.float32 for v in golden.values())


@pytest.mark.parametrize('build', [harness.small_cnn_graph, harness.resnet50_graph, harness.yolov6s_graph])
def test_pair_discovery_equals_the_reference(book, build):
    g = build()
    interested = [op for op in g.operations.values() if op.type in EQ.EQUALIZATION_OPERATION_TYPE]
    for level in (1, 2):
        assert _names(EQ.find_equalization_pair(g, interested, level)) == book['graphs'][g.name][str(level)]['pairs'], level
    every = [p for lv in book['graphs'].values() for x in lv.values() for p in x['pairs']]
    assert any(len(up) > 1 and len(down) > 1 for up, down in every)
    assert any(x['dropped'] for lv in book['graphs'].values() for x in lv.values())


def test_pair_discovery_on_quantised_graphs_and_case_graphs(book):
    g = harness.resnet50_graph()
    harness.quantize_graph(g)
    p = EQ.LayerwiseEqualizationPass(iterations=1)
    assert _names(p.find_equalization_pair(g, p.interested_operations(g))) == book['graphs']['resnet50']['2']['pairs']
    for k, case in enumerate(EC.CASES):
        g = EC.harness_graph(k)
        assert _names(p.find_equalization_pair(g, p.interested_operations(g))) == book['cases'][case['name']], case['name']
    p = EQ.LayerwiseEqualizationPass(iterations=1, interested_layers=['c2', 'nope'])
    g = EC.harness_graph(0)
    assert _names(p.find_equalization_pair(g, p.interested_operations(g))) == [[['c2'], ['c3']]]
    assert EQ.LayerwiseEqualizationPass(iterations=1, interested_layers=[]).interested_operations(g) == []


@pytest.mark.parametrize('k', range(len(EC.CASES)))
def test_torch_arm_equals_the_reference_bit_for_bit(golden, k):
    case = EC.CASES[k]
    g, p = _run_case(golden, k, use_kernels=False)
    pairs = len(p.pairs)
    assert len(p.scales) == pairs * case['iterations']
    for (it, q), s in p.scales.items(): assert _same(s, golden[f'c{k}_scale_it{it + 1}_p{q}']), (case['name'], it, q)
    for v in g.variables.values():
        if v.is_parameter: assert _same(v.value, golden[f'c{k}_it{case["iterations"]}_{v.name}']), (case['name'], v.name)
    # every iteration, not only the last: the pass stopped early equals the recorded intermediate parameters
    for it in range(1, case['iterations']):
        g2 = EC.harness_graph(k)
        EQ.LayerwiseEqualizationPass(iterations=it, including_bias=case['including_bias'], including_act=case['including_act'],
                                     use_kernels=False).optimize(g2, activations=_activations(golden, k, g2))
        for v in g2.variables.values():
            if v.is_parameter: assert _same(v.value, golden[f'c{k}_it{it}_{v.name}']), (case['name'], it, v.name)
    last = np.concatenate([golden[f'c{k}_scale_it{case["iterations"]}_p{q}'] for q in range(pairs)])
    clipped = ((last == np.float32(0.1)) | (last == 10)) & (last != 1)
    assert p.stats['pairs'] == pairs and p.stats['channels'] == last.size
    assert p.stats['scaled_channels'] == int((last != 1).sum()) and p.stats['clipped_channels'] == int(clipped.sum())


def test_collected_activations_equal_the_reference(golden):
    """The torch arm's own collection on the CPU (the harness executor) against the maxima the reference's executor recorded:
    same convolutions on the same CPU, so the same bits; and the pass run from its own collection equals the goldens."""
    k = [c['name'] for c in EC.CASES].index('zero_act')
    g = EC.harness_graph(k)
    p = _pass(k, use_kernels=False)
    p.optimize(g, dataloader=EC.case_batches(k), executor=harness.TorchExecutor(g, 'cpu'))
    assert set(p.activations) == {'c1_out', 'c2_out', 'c3_out'}
    for name, a in p.activations.items(): assert _same(a, golden[f'c{k}_act_{name}']), name
    for v in g.variables.values():
        if v.is_parameter: assert _same(v.value, golden[f'c{k}_it1_{v.name}']), v.name
    assert all(v.value is None for v in g.variables.values() if not v.is_parameter)      # nothing written into the graph


def test_collection_visits_at_most_eighteen_batches():
    k = [c['name'] for c in EC.CASES].index('zero_act')
    g = EC.harness_graph(k)
    seen = []

    class Counting(harness.TorchExecutor):
        def forward(self, inputs, output_names=None, hooks=None):
            seen.append(1)
            return super().forward(inputs, output_names, hooks)
    batch = EC.case_batches(k)[0]
    _pass(k, use_kernels=False).optimize(g, dataloader=[batch] * 40, executor=Counting(g, 'cpu'))
    assert len(seen) == 18                                                              # `if idx > steps: break`, steps = 16


def test_schedule_covers_every_instance_once_and_keeps_dependent_order():
    for build, iterations in ((harness.resnet50_graph, 3), (harness.yolov6s_graph, 2), (lambda: EC.harness_graph(1), 10)):
        g = build()
        p = EQ.LayerwiseEqualizationPass(iterations=iterations)
        pairs = p.find_equalization_pair(g, p.interested_operations(g))
        levels = EQ.build_schedule(pairs, iterations)
        flat = [inst for level in levels for inst in level]
        assert sorted(flat) == [(it, q) for it in range(iterations) for q in range(len(pairs))] and len(set(flat)) == len(flat)
        level_of = {inst: n for n, level in enumerate(levels) for inst in level}
        ops = [{op.name for op in pair.operations} for pair in pairs]
        for a in flat:
            for b in flat:
                if a < b and ops[a[1]] & ops[b[1]]: assert level_of[a] < level_of[b], (a, b)      # (iteration, pair) order is the reference's
        for level in levels:                                                             # a level's pairs are disjoint
            names = [n for _, q in level for n in ops[q]]
            assert len(names) == len(set(names))
        assert len(levels) <= len(flat)
        if g.name != 'add_pair': assert len(levels) < len(flat) / 2          # a chain of two pairs has nothing to gather
        assert EQ.build_schedule(pairs, iterations, 'sequential') == [[inst] for inst in sorted(flat)]
    with pytest.raises(ValueError): EQ.build_schedule([], 1, 'random')


def test_levelled_torch_arm_equals_sequential_bit_for_bit():
    for build, iterations in ((lambda: harness.resnet50_graph(num_classes=10), 2), (lambda: EC.harness_graph(1), 10),
                              (lambda: EC.harness_graph(2), 2)):
        a, b = build(), build()
        pa = EQ.LayerwiseEqualizationPass(iterations=iterations, including_bias=True, use_kernels=False, schedule='levelled')
        pb = EQ.LayerwiseEqualizationPass(iterations=iterations, including_bias=True, use_kernels=False, schedule='sequential')
        pa.optimize(a); pb.optimize(b)
        assert pa.stats['levels'] <= pb.stats['levels'] == iterations * pa.stats['pairs']
        if a.name == 'resnet50': assert pa.stats['levels'] < pb.stats['levels'] / 2
        for name, v in a.variables.items():
            if v.is_parameter: assert _same(v.value, b.variables[name].value), name
        assert {k: v for k, v in pa.stats.items() if k != 'levels'} == {k: v for k, v in pb.stats.items() if k != 'levels'}


@pytest.mark.parametrize('which', ['chain', 'add_pair', 'grouped', 'zero_act', 'resnet50'])
def test_function_is_preserved(golden, which):
    torch.manual_seed(0)
    if which == 'resnet50':
        g, x, kw = harness.resnet50_graph(num_classes=10), torch.rand(2, 3, 64, 64), dict(iterations=3, including_bias=True)
    else:
        k = [c['name'] for c in EC.CASES].index(which)
        case = EC.CASES[k]
        g, x = EC.harness_graph(k), EC.case_batches(k)[0]
        kw = dict(iterations=case['iterations'], including_bias=case['including_bias'], including_act=case['including_act'])
    ex = harness.TorchExecutor(g, 'cpu')
    before = [y.clone() for y in ex.forward(x)]
    p = EQ.LayerwiseEqualizationPass(use_kernels=False, **kw)
    p.optimize(g, dataloader=[x], executor=ex)
    assert p.stats['scaled_channels'] > 0
    for y0, y1 in zip(before, ex.forward(x)):
        err = float(torch_snr_error(y1, y0))
        print(which, 'snr error', err)
        assert err < SNR_BOUND, (which, err)


def test_constructor_matches_the_reference(book):
    sig = inspect.signature(EQ.LayerwiseEqualizationPass.__init__)
    ours = [(n, q.default) for n, q in sig.parameters.items() if n != 'self']
    want = book['constructor']
    assert len(want) == 11
    for (name, default), (ref_name, ref_default, required) in zip(ours, want):
        assert name == ref_name
        if required: assert default is inspect.Parameter.empty
        else: assert default == ref_default and type(default) is type(ref_default)
    assert [n for n, _ in ours[11:]] == ['use_kernels', 'schedule'] and ours[11][1] is True
    p = EQ.LayerwiseEqualizationPass(iterations=4)
    assert p.name == 'PPQ Layerwise Equalization Pass' and p.iterations == 4
    assert EQ.OPTIMIZATION_LAYERTYPE_CONFIG[2] - EQ.OPTIMIZATION_LAYERTYPE_CONFIG[1] == {'Add', 'Sub'}
    assert EQ.EQUALIZATION_OPERATION_TYPE == {'Conv', 'Gemm', 'ConvTranspose'}
    eq = inspect.signature(EQ.EqualizationPair.equalize)
    assert list(eq.parameters)[1:8] == ['value_threshold', 'including_weight', 'weight_multiplier', 'including_act', 'act_multiplier',
                                         'including_bias', 'bias_multiplier']


def test_weight_arguments_are_stored_and_unused(golden):
    """The reference's equalize() does not forward including_weight / weight_multiplier: they act as True and 1.0."""
    a, b = EC.harness_graph(0), EC.harness_graph(0)
    EQ.LayerwiseEqualizationPass(iterations=2, use_kernels=False).optimize(a)
    p = EQ.LayerwiseEqualizationPass(iterations=2, including_weight=False, weight_multiplier=7.0, use_kernels=False)
    p.optimize(b)
    assert p.including_weight is False and p.weight_multiplier == 7.0
    for name, v in a.variables.items():
        if v.is_parameter: assert _same(v.value, b.variables[name].value), name


def test_store_parameter_value_ran_and_pass_runs_in_a_pipeline(capsys):
    from ppq_amd import lib as PFL
    g = EC.harness_graph(0)
    harness.quantize_graph(g)
    before = {op.name: op.inputs[1].stored_value.clone() for op in g.operations.values() if op.type == 'Conv'}
    PFL.Pipeline([EQ.LayerwiseEqualizationPass(iterations=2, use_kernels=False)]).optimize(
        graph=g, dataloader=[], executor=harness.TorchExecutor(g, 'cpu'), collate_fn=None, verbose=False)
    assert capsys.readouterr().out == ''                                                 # nothing printed unless verbose
    changed = 0
    for op in g.operations.values():
        if op.type != 'Conv': continue
        assert torch.equal(op.inputs[1].stored_value, op.inputs[1].value)
        changed += int(not torch.equal(before[op.name], op.inputs[1].value))
    assert changed == 3
    EQ.LayerwiseEqualizationPass(iterations=1, use_kernels=False, verbose=True).optimize(EC.harness_graph(0))
    assert 'equalization pair(s) was found' in capsys.readouterr().out


def test_convtranspose_raises():
    g = harness.BaseGraph('t')
    x = g.create_variable('input'); g.inputs['input'] = x
    w1 = g.create_variable('c1_w', torch.randn(4, 3, 3, 3), True)
    y = g.create_operation('Conv', 'c1', [x, w1])
    w2 = g.create_variable('ct_w', torch.randn(4, 2, 3, 3), True)
    y = g.create_operation('ConvTranspose', 'ct', [y, w2])
    g.outputs[y.name] = y
    for use_kernels in (False, True):
        with pytest.raises(TypeError, match=r'Unsupported Op type ct\(ConvTranspose\) for Equalization Optimization\..*not executable by this harness'):
            EQ.LayerwiseEqualizationPass(iterations=1, use_kernels=use_kernels).optimize(g)
    assert torch.equal(g.variables['c1_w'].value, w1.value)
    with pytest.raises(ValueError): EQ.LayerwiseEqualizationPass(iterations=1, schedule='random')
