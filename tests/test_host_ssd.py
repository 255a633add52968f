"""Host-side tests of SSD equalization (ppq_amd/ssd.py): pair discovery against the reference's recorded pair lists, the torch
arm's scales and candidate parameters against the reference's recorded ones bit for bit, a replay of every recorded decision
(tests/golden/ssd.npz and ssd_pairs.json, written by tests/golden/make_ssd.py), the calib_steps clamp, the activation-range
lift, function preservation, the constructor's surface and the refusals.  No GPU needed."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import ssd_cases as SC  # noqa: E402

from ppq_amd import harness  # noqa: E402
from ppq_amd import ssd as SSD  # noqa: E402
from ppq_amd.core import QuantizationStates  # noqa: E402
from ppq_amd.measure import torch_snr_error  # noqa: E402

SNR_BOUND = 1e-7                     # the bound test_host_equalization.py uses for function preservation


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'ssd.npz')))


@pytest.fixture(scope='module')
def book():
    with open(os.path.join(HERE, 'golden', 'ssd_pairs.json')) as f: return json.load(f)


def _same(a, b) -> bool:
    a, b = np.ascontiguousarray(np.asarray(a, dtype=np.float32)), np.ascontiguousarray(np.asarray(b, dtype=np.float32))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _names(pairs): return [[op.name for op in pair] for pair in pairs]


def _pass(k, cls=SSD.SSDEqualizationPass, **kw):
    return cls(iteration=SC.CASES[k]['iterations'], channel_ratio=SC.CHANNEL_RATIO, loss_threshold=SC.LOSS_THRESHOLD, **kw)


def _set_parameters(graph, golden, prefix):
    for name, v in graph.variables.items():
        if v.is_parameter: v.value = torch.from_numpy(golden[prefix + name].copy())


def test_case_inputs_are_the_recorded_ones(golden):
    for k in range(len(SC.CASES)):
        for name, t in SC.case_parameters(k).items(): assert _same(t, golden[f'c{k}_init_{name}']), (k, name)


def test_recorded_cases_meet_the_conditions_the_comparisons_rely_on(golden):
    """An accepted DFQ candidate, an accepted activation-aware one and an (iteration, pair) with nothing accepted; each of the
    clips 0.1 / 10 / 1 / 2 and the 0.01 activation floor acts somewhere; every recorded comparison has a margin of 5 % (two
    candidates with the same scale bits are one candidate)."""
    best, low, high, one, two, floor = [], 0, 0, 0, 0, 0
    for k, case in enumerate(SC.CASES):
        for it in range(1, case['iterations'] + 1):
            p = 0
            while f'c{k}_it{it}_p{p}_losses' in golden:
                key = f'c{k}_it{it}_p{p}_'
                losses, scales = golden[key + 'losses'], golden[key + 'scales']
                best.append(int(golden[key + 'best']))
                limit = SC.LOSS_THRESHOLD * losses[0]
                assert all(abs(v - limit) >= 0.05 * limit for v in losses[1:]), (case['name'], it, p, losses)
                passing = [a for a in range(4) if losses[a + 1] < limit]
                for i, a in enumerate(passing):
                    for b in passing[i + 1:]:
                        if np.array_equal(scales[a], scales[b]): continue
                        lo, hi = sorted((losses[a + 1], losses[b + 1]))
                        assert hi - lo >= 0.05 * hi, (case['name'], it, p, a, b)
                low += int((scales[0] == np.float32(0.1)).sum()); high += int((scales[0] == 10).sum())
                one += int((scales[2:] == 1).sum()); two += int((scales[2:] == 2).sum())
                floor += int((golden[key + 'act'] < np.float32(0.01)).sum())
                p += 1
            assert p > 0
    assert 0 in best and -1 in best and any(b >= 1 for b in best), best
    assert min(low, high, one, two, floor) > 0, (low, high, one, two, floor)


@pytest.mark.parametrize('build', [harness.small_cnn_graph, harness.resnet50_graph, harness.yolov6s_graph])
def test_pair_discovery_equals_the_reference(book, build):
    g = build()
    want = book['graphs'][g.name]
    assert _names(SSD.SSDEqualizationPass().collect_all_pairs(g)) == want
    harness.quantize_graph(g, per_channel_weight=False)
    assert _names(SSD.SSDEqualizationPass().collect_all_pairs(g)) == want                 # quantising changes nothing


def test_pair_discovery_on_the_case_graphs(book):
    for k, case in enumerate(SC.CASES):
        assert _names(SSD.SSDEqualizationPass().collect_all_pairs(SC.harness_graph(k))) == book['cases'][case['name']], case['name']
    assert book['cases']['branch'] == [['c2', 'r2', 'c4']]                               # nothing starts at the Conv that feeds two
    assert len(book['cases']['chain']) == 2 and book['cases']['chain'][0][-1] == book['cases']['chain'][1][0]
    assert len(book['graphs']['resnet50']) > 20 and len(book['graphs']['yolov6s']) > 20


def test_constructor_matches_the_reference(book):
    sig = inspect.signature(SSD.SSDEqualizationPass.__init__)
    ours = [(n, q.default) for n, q in sig.parameters.items() if n != 'self']
    want = book['constructor']
    assert [n for n, _, _ in want] == ['optimize_level', 'channel_ratio', 'loss_threshold', 'layer_norm', 'quant_func', 'iteration']
    for (name, default), (ref_name, ref_default, required) in zip(ours, want):
        assert name == ref_name and not required
        if name == 'quant_func': assert default.__name__ == ref_default
        else: assert default == ref_default and type(default) is type(ref_default)
    assert ours[6] == ('use_kernels', True)
    p = SSD.SSDEqualizationPass()
    assert p.name == book['name'] == 'SSD Equalization Pass' and p.iteration == 3
    for method in ('collect_all_pairs', 'collect_activation_range', 'layer_weight_norm', 'prepare_weight_for_equalization',
                   'one_step_equalization', 'write_back', 'test_ssd_loss', 'initiate_pair_state', 'calibration_passive_param'):
        assert callable(getattr(p, method))
    assert list(inspect.signature(p.optimize).parameters)[:5] == ['graph', 'dataloader', 'executor', 'collate_fn', 'calib_steps']
    assert SSD.EQUALIZATION_OPERATION_TYPE == {'Conv', 'Gemm', 'ConvTranspose'}
    assert SSD.OPTIMIZATION_LAYERTYPE_CONFIG[1] == {'Relu', 'MaxPool', 'GlobalMaxPool', 'PRelu', 'AveragePool', 'GlobalAveragePool'}


def test_calib_steps_clamp():
    """min(calib_steps, ceil(200 / batchsize)), the batch size read from a tensor, a list / tuple, a dict."""
    x = torch.zeros(32, 3, 4, 4)
    assert SSD.clamp_calib_steps(32, [x]) == 7                                          # ceil(200 / 32)
    assert SSD.clamp_calib_steps(3, [x]) == 3
    assert SSD.clamp_calib_steps(32, [[None, 'label', torch.zeros(50, 2), x]]) == 4     # the first TENSOR of the list
    assert SSD.clamp_calib_steps(32, [(torch.zeros(8, 2),)]) == 25
    assert SSD.clamp_calib_steps(32, [{'name': 'x', 'input': torch.zeros(100, 2), 'other': x}]) == 2
    assert SSD.clamp_calib_steps(500, [{'a': 1}]) == 200                                # no tensor: batch size 1
    assert SSD.clamp_calib_steps(32, [{'image': x}], collate_fn=lambda d: d['image'][:4]) == 32   # read AFTER collate_fn
    assert SSD.clamp_calib_steps(9, []) == 9


def test_activation_range_lift():
    r = torch.tensor([0.1, 4.0, 1.9, 2.0, 0.0, 3.0])
    assert torch.equal(SSD.lift_activation_range(r, 0.5), torch.tensor([2.0, 4.0, 2.0, 2.0, 2.0, 3.0]))
    assert torch.equal(SSD.lift_activation_range(r, 0.0), r)

    class Executor:                                                  # the mean over calib_steps batches of max(relu(y)), then the lift
        def __init__(self, ys): self.ys, self.calls = ys, 0
        def forward(self, data, output_names=None):
            assert output_names == ['c1_out']
            self.calls += 1
            return [self.ys[data]]
    g = SC.harness_graph(SC.case_index('chain'))
    p = SSD.SSDEqualizationPass(use_kernels=False)
    pair = p.collect_all_pairs(g)[0]
    ys = [torch.full((2, 12, 3, 3), -1.0), torch.full((2, 12, 3, 3), -1.0), torch.full((2, 12, 3, 3), 5.0)]
    ys[0][1, 2, 0, 1] = 6.0; ys[1][0, 2, 2, 2] = 3.0; ys[0][0, 5, 1, 1] = 1.5; ys[2][0, 7, 0, 0] = 9.0
    ex = Executor(ys)
    got = p.collect_activation_range(pair, ex, [0, 1, 2], None, 2)[pair[0]]
    want = torch.full((12,), 2.25); want[2] = 4.5                    # channel 2: (6 + 3) / 2; channel 5: 0.75, below half of 4.5
    assert ex.calls == 2 and torch.equal(got, want)


def _recorded(golden, k):
    """[(iteration, pair index, key)] of case k in the pass's order."""
    out = []
    for it in range(1, SC.CASES[k]['iterations'] + 1):
        p = 0
        while f'c{k}_it{it}_p{p}_losses' in golden:
            out.append((it, p, f'c{k}_it{it}_p{p}_')); p += 1
    return out


@pytest.mark.parametrize('k', range(len(SC.CASES)), ids=[c['name'] for c in SC.CASES])
def test_torch_arm_scales_and_candidates_equal_the_reference_bit_for_bit(golden, k):
    """one_step_equalization on the recorded parameters with the recorded activation range: the two weight ranges, the four
    scales and the four candidate parameter sets of every (iteration, pair)."""
    g = SC.harness_graph(k)
    p = _pass(k, use_kernels=False)
    pairs = p.collect_all_pairs(g)
    state = {name: golden[f'c{k}_init_{name}'] for name, v in g.variables.items() if v.is_parameter}
    seen = 0
    for it, q, key in _recorded(golden, k):
        pair = pairs[q]
        act = {pair[0]: torch.from_numpy(golden[key + 'act'])}
        names = [v.name for op in (pair[0], pair[-1]) for v in op.parameters]
        for algo in range(4):
            for name in names: g.variables[name].value = torch.from_numpy(state[name].copy())
            first, last = p.prepare_weight_for_equalization(pair)
            assert _same(first, golden[key + 'first']) and _same(last, golden[key + 'last']), (it, q)
            scale = p.one_step_equalization(pair, act, algo)
            assert _same(scale, golden[key + 'scales'][algo]), (it, q, algo)
            for name in names:
                assert _same(g.variables[name].value, golden[f'{key}cand{algo}_{name}']), (it, q, algo, name)
                seen += 1
        best = int(golden[key + 'best'])
        if best >= 0: state.update({name: golden[f'{key}cand{best}_{name}'] for name in names})
        if q == len(pairs) - 1:
            for name in state: assert _same(state[name], golden[f'c{k}_after{it}_{name}']), (it, name)
    assert seen >= 4 * 3 * len(pairs) * SC.CASES[k]['iterations'] - 4 * len(pairs) * SC.CASES[k]['iterations']


class Replay(SSD.SSDEqualizationPass):
    """The pass with the two device-bound methods answered from the recording."""
    def __init__(self, golden, k, **kw):
        super().__init__(**kw)
        self.recorded = _recorded(golden, k)
        self.golden, self.ranges, self.losses = golden, 0, 0

    def collect_activation_range(self, pair, executor, data_loader, collate_fn, calib_steps):
        key = self.recorded[self.ranges][2]
        self.ranges += 1
        return {pair[0]: torch.from_numpy(self.golden[key + 'act'])}

    def test_ssd_loss(self, pair, executor, data_loader, collate_fn, calib_steps):
        key = self.recorded[self.losses // 5][2]
        value = float(self.golden[key + 'losses'][self.losses % 5])
        self.losses += 1
        for op in pair:                                           # what a real evaluation leaves behind: activated configs
            for cfg in op.config.input_quantization_config + op.config.output_quantization_config:
                if cfg.state == QuantizationStates.INITIAL: cfg.state = QuantizationStates.ACTIVATED
                elif cfg.state == QuantizationStates.PASSIVE_INIT: cfg.state = QuantizationStates.PASSIVE
        return value


@pytest.mark.parametrize('k', range(len(SC.CASES)), ids=[c['name'] for c in SC.CASES])
def test_decision_replay(golden, k):
    """optimize() on CPU parameters with the recorded ranges and losses: the recorded best_idx everywhere, the recorded
    parameters after the last iteration (and, run iteration by iteration, after every one) bit for bit, stored_value == value
    and INITIAL / PASSIVE_INIT configs on every pair."""
    case = SC.CASES[k]
    for upto in range(1, case['iterations'] + 1):
        g = SC.harness_graph(k)
        p = Replay(golden, k, iteration=upto, channel_ratio=SC.CHANNEL_RATIO, loss_threshold=SC.LOSS_THRESHOLD)
        p.optimize(g, dataloader=SC.case_batches(k), executor=None, collate_fn=None, calib_steps=SC.CALIB_STEPS)
        P = len(p.pairs)
        assert p.stats['pairs'] == P and p.stats['calib_steps'] == SC.CALIB_STEPS and p.losses == 5 * P * upto and p.ranges == P * upto
        for it, q, key in p.recorded[:P * upto]:
            h = p.history[(it - 1, q)]
            assert h['best_idx'] == int(golden[key + 'best']), (it, q)
            assert h['basic'] == golden[key + 'losses'][0] and h['losses'] == list(golden[key + 'losses'][1:])
        assert sum(p.stats['accepted'].values()) == P * upto
        for name, v in g.variables.items():
            if v.is_parameter: assert _same(v.value, golden[f'c{k}_after{upto}_{name}']), (upto, name)
        states = set()
        for pair in p.pairs:
            for op in pair:
                for v in op.parameters: assert torch.equal(v.stored_value, v.value), v.name
                for cfg in op.config.input_quantization_config + op.config.output_quantization_config:
                    assert cfg.state in (QuantizationStates.INITIAL, QuantizationStates.PASSIVE_INIT, QuantizationStates.OVERLAPPED,
                                         QuantizationStates.FP32), (op.name, cfg.state)
                    states.add(cfg.state)
        assert QuantizationStates.INITIAL in states
        assert (QuantizationStates.PASSIVE_INIT in states) == case['passive_bias']


def test_passive_bias_takes_weight_scale_times_input_scale():
    k = SC.case_index('passive_bias')
    g = SC.harness_graph(k)
    p = SSD.SSDEqualizationPass(use_kernels=False)
    pair = p.collect_all_pairs(g)[1]
    op = pair[0]
    i_cfg, w_cfg, b_cfg = op.config.input_quantization_config
    assert b_cfg.state == QuantizationStates.PASSIVE_INIT and b_cfg.num_of_bits == 32
    w_cfg.scale, w_cfg.offset, w_cfg.state = torch.tensor(0.25), torch.tensor(0.0), QuantizationStates.ACTIVATED
    i_cfg.dominated_by.scale, i_cfg.dominated_by.offset = torch.tensor(0.5), torch.tensor(0.0)
    p.calibration_passive_param([op])
    assert b_cfg.state == QuantizationStates.PASSIVE and float(b_cfg.scale) == 0.125 and float(b_cfg.offset) == 0.0
    p.initiate_pair_state([op])
    assert b_cfg.state == QuantizationStates.PASSIVE_INIT and w_cfg.state == QuantizationStates.INITIAL


@pytest.mark.parametrize('k', [k for k, c in enumerate(SC.CASES) if c['executable']],
                         ids=[c['name'] for c in SC.CASES if c['executable']])
def test_function_is_preserved(golden, k):
    """Every algo's candidate of every first-iteration pair keeps the FP32 output of the graph."""
    x = SC.case_batches(k)[0]
    checked = 0
    for it, q, key in _recorded(golden, k):
        if it != 1: continue
        for algo in range(4):
            g = SC.harness_graph(k, quantize=False)
            ex = harness.TorchExecutor(g, 'cpu')
            before = [y.clone() for y in ex.forward(x)]
            p = _pass(k, use_kernels=False)
            pair = p.collect_all_pairs(g)[q]
            scale = p.one_step_equalization(pair, {pair[0]: torch.from_numpy(golden[key + 'act'])}, algo)
            assert bool((scale != 1).any())
            for y0, y1 in zip(before, ex.forward(x)):
                err = float(torch_snr_error(y1, y0))
                assert err < SNR_BOUND, (SC.CASES[k]['name'], q, algo, err)
            checked += 1
    assert checked >= 4


def test_gemm_behind_a_flattened_conv_takes_the_reshape_branches():
    """optim/ssd.py:190-204 / :245-259: C channels of H x W feed a Gemm of C * H * W inputs."""
    torch.manual_seed(1)
    g = harness.BaseGraph('flat')
    x = g.create_variable('input'); g.inputs['input'] = x
    y = g.create_operation('Conv', 'c1', [x, g.create_variable('c1_w', torch.randn(4, 3, 3, 3), True),
                                         g.create_variable('c1_b', torch.randn(4), True)], {'strides': 1, 'pads': 1, 'group': 1})
    y = g.create_operation('Relu', 'r1', [y])
    y = g.create_operation('GlobalAveragePool', 'gap', [y])
    y = g.create_operation('Gemm', 'fc', [y, g.create_variable('fc_w', torch.randn(5, 4), True)])
    g.outputs[y.name] = y
    p = SSD.SSDEqualizationPass(use_kernels=False)
    (pair,) = p.collect_all_pairs(g)
    assert [op.name for op in pair] == ['c1', 'r1', 'gap', 'fc'] and SSD.pair_geometry(pair) is not None
    wide = torch.randn(5, 4 * 6)                                   # the same Gemm behind a flattened [4, 2, 3] tensor
    g.variables['fc_w'].value = wide.clone()
    assert SSD.pair_geometry(pair) is None                         # the kernel arm hands this pair to the torch arm
    first, last = p.prepare_weight_for_equalization(pair)
    assert torch.equal(last, wide.reshape(5, 4, 6).abs().amax(dim=(0, 2)))
    scale = p.one_step_equalization(pair, {}, 0)
    assert torch.equal(g.variables['fc_w'].value, (wide.reshape(5, 4, 6) / scale.reshape(1, 4, 1)).reshape(5, 24))


def test_convtranspose_raises():
    g = harness.BaseGraph('t')
    x = g.create_variable('input'); g.inputs['input'] = x
    w1 = g.create_variable('c1_w', torch.randn(4, 3, 3, 3), True)
    y = g.create_operation('Conv', 'c1', [x, w1])
    y = g.create_operation('Relu', 'r1', [y])
    w2 = g.create_variable('ct_w', torch.randn(4, 2, 3, 3), True)
    y = g.create_operation('ConvTranspose', 'ct', [y, w2])
    g.outputs[y.name] = y
    for use_kernels in (False, True):
        with pytest.raises(TypeError, match=r'Unsupported Op type ct\(ConvTranspose\) for Equalization Optimization\..*not executable by this harness'):
            SSD.SSDEqualizationPass(use_kernels=use_kernels).optimize(g, dataloader=[torch.zeros(1, 3, 8, 8)], executor=None,
                                                                      collate_fn=None, calib_steps=1)
    assert torch.equal(g.variables['c1_w'].value, w1.value)


# ---- the NumPy oracle of the kernels (tests/ssd_reference.py) --------------------------------------------------------
import ssd_reference as REF  # noqa: E402


def _pair_forms(case: dict, names: list):
    """(first attributes, last attributes, first channel axis, last channel axis, groups of the last Conv) of a recorded pair."""
    attrs = {name: a for _, name, _, a in case['ops']}
    first, last = attrs[names[0]], attrs[names[-1]]
    first_axis = 0 if 'k' in first or first['transB'] else 1
    last_axis = 1 if 'k' in last or last['transB'] else 0
    return first, last, first_axis, last_axis, last.get('group', 1)


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


@pytest.mark.parametrize('k', range(len(SC.CASES)), ids=[c['name'] for c in SC.CASES])
def test_oracle_equals_every_recorded_range_scale_and_candidate(golden, book, k):
    """ssd_reference.ranges / scales / apply against every (case, iteration, pair) of ssd.npz, on bits."""
    case = SC.CASES[k]
    pairs = book['cases'][case['name']]
    seen = cands = 0
    for it, q, key, state in _states(golden, k):
        first, last, first_axis, last_axis, group = _pair_forms(case, pairs[q])
        n1, n2 = pairs[q][0], pairs[q][-1]
        r = REF.ranges(state[n1 + '_w'], state[n2 + '_w'], group, first_axis, last_axis)
        assert _same(r[0], golden[key + 'first']) and _same(r[1], golden[key + 'last']), (it, q)
        s = REF.scales(r[0], r[1], golden[key + 'act'], SC.CHANNEL_RATIO)
        assert _same(s, golden[key + 'scales']), (it, q)
        # the tensors one by one (the form the kernel tests use) and the pair at once (the form make_ssd.py uses)
        items = [(n1 + '_w', first_axis, False, 1), (n2 + '_w', last_axis, True, group)]
        if first['bias']: items.append((n1 + '_b', 0, False, 1))
        for name, axis, divide, g in items:
            got = REF.apply(state[name], s, axis, divide, g)
            for algo in range(4): assert _same(got[algo], golden[f'{key}cand{algo}_{name}']), (it, q, algo, name)
            cands += 4
        for algo in range(4):
            for name, t in REF.apply_pair(first, last, n1, n2, state, s[algo]).items():
                assert _same(t, golden[f'{key}cand{algo}_{name}']), (it, q, algo, name)
        seen += 1
    assert seen == len(pairs) * case['iterations'] and cands >= 8 * seen


def test_oracle_scales_equal_calculate_scale(golden):
    """The torch arm's scale of the four algorithms on every recorded input.  (The recordings were admitted only where torch's
    CPU square root rounds correctly: make_ssd.py.)"""
    seen = 0
    for k in range(len(SC.CASES)):
        for it, q, key in _recorded(golden, k):
            first, last, act = (golden[key + n] for n in ('first', 'last', 'act'))
            want = REF.scales(first, last, act, SC.CHANNEL_RATIO)
            for algo in range(4):
                got = SSD.calculate_scale(torch.from_numpy(first), torch.from_numpy(last), torch.from_numpy(act), algo, SC.CHANNEL_RATIO)
                assert _same(got.numpy(), want[algo]), (k, it, q, algo)
            seen += 1
    assert seen >= 20


def test_oracle_channel_forms_equal_the_torch_arm_at_width():
    """ranges of the three segment forms (row, column, grouped slices) on weights wider than one workgroup: the oracle against
    prepare_weight_for_equalization, which the recordings pin at C <= 16 only."""
    rng = np.random.default_rng(7)

    def torch_ranges(kind1, w1, a1, kind2, w2, a2):
        g = harness.BaseGraph('wide')
        x = g.create_variable('input'); g.inputs['input'] = x
        y = g.create_operation(kind1, 'a', [x, g.create_variable('a_w', torch.from_numpy(w1), True)], a1)
        y = g.create_operation('Relu', 'r', [y])
        y = g.create_operation(kind2, 'b', [y, g.create_variable('b_w', torch.from_numpy(w2), True)], a2)
        g.outputs[y.name] = y
        p = SSD.SSDEqualizationPass(use_kernels=False)
        (pair,) = p.collect_all_pairs(g)
        return [t.numpy() for t in p.prepare_weight_for_equalization(pair)]

    conv = {'strides': 1, 'pads': 1, 'group': 1}
    w1, w2 = rng.standard_normal((300, 5, 3, 3)).astype(np.float32), rng.standard_normal((7, 300, 3, 3)).astype(np.float32)
    want = torch_ranges('Conv', w1, conv, 'Conv', w2, conv)
    assert _same(REF.ranges(w1, w2), np.stack(want))
    wg = rng.standard_normal((24, 150, 3, 3)).astype(np.float32)
    want = torch_ranges('Conv', w1, conv, 'Conv', wg, dict(conv, group=2))
    assert _same(REF.ranges(w1, wg, 2), np.stack(want))
    g1, g2 = rng.standard_normal((9, 300)).astype(np.float32), rng.standard_normal((11, 300)).astype(np.float32)
    want = torch_ranges('Gemm', g1, {'transB': 0}, 'Gemm', g2, {'transB': 1})                  # [in, C] column, [out, C] column
    assert _same(REF.ranges(g1, g2, 1, 1, 1), np.stack(want))
    want = torch_ranges('Gemm', np.ascontiguousarray(g1.T), {'transB': 1}, 'Gemm', np.ascontiguousarray(g2.T), {'transB': 0})
    assert _same(REF.ranges(g1.T, g2.T, 1, 0, 0), np.stack(want))                             # [C, in] row, [C, out] row


def test_oracle_nan_behaviour():
    """The NaN semantics the kernels document (ssd_reference's module docstring), on the oracle itself."""
    rng = np.random.default_rng(3)
    C = 20
    w1 = rng.standard_normal((C, 4, 3, 3)).astype(np.float32)
    w2 = rng.standard_normal((6, C, 3, 3)).astype(np.float32)
    act = (rng.random(C).astype(np.float32) + np.float32(0.1))
    clean = REF.scales(*REF.ranges(w1, w2), act, 0.5)
    assert not np.isnan(clean).any()
    a = w1.copy(); a[5, 2, 1, 1] = np.nan                                # first weight
    r = REF.ranges(a, w2)
    assert np.array_equal(np.isnan(r[0]), np.arange(C) == 5) and not np.isnan(r[1]).any()
    s = REF.scales(r[0], r[1], act, 0.5)
    assert np.array_equal(np.isnan(s[0]), np.arange(C) == 5) and np.isnan(s[1:]).all()
    assert _same(s[0][np.arange(C) != 5], clean[0][np.arange(C) != 5])
    b = w2.copy(); b[3, 7, 0, 2] = np.nan                                # last weight: algorithm 1 does not read it
    r = REF.ranges(w1, b)
    assert np.array_equal(np.isnan(r[1]), np.arange(C) == 7) and not np.isnan(r[0]).any()
    s = REF.scales(r[0], r[1], act, 0.5)
    assert np.array_equal(np.isnan(s[0]), np.arange(C) == 7) and _same(s[1], clean[1]) and np.isnan(s[2:]).all()
    c = act.copy(); c[11] = np.nan                                       # activation range: algorithm 0 does not read it
    s = REF.scales(*REF.ranges(w1, w2), c, 0.5)
    assert _same(s[0], clean[0]) and np.isnan(s[1:]).all()
    for algo in range(4):                                                # ... and the torch arm says the same
        got = SSD.calculate_scale(torch.from_numpy(r[0]), torch.from_numpy(r[1]), torch.from_numpy(act), algo, 0.5).numpy()
        want = REF.scales(r[0], r[1], act, 0.5)[algo]
        assert np.array_equal(np.isnan(got), np.isnan(want)), algo
    x = np.array([[1.0, np.nan], [-0.0, 3.0]], dtype=np.float32)         # apply: a NaN stays where it is, -0 keeps its sign
    got = REF.apply(x, np.full((4, 2), 2.0, np.float32), 0)
    assert np.array_equal(np.isnan(got[0]), np.isnan(x)) and np.signbit(got[0][1, 0]) and got[0][1, 1] == 6.0
