"""Record what the REFERENCE's SSDEqualizationPass (ppq/quantization/optim/ssd.py:30-573) does on the CPU to the case graphs of
ssd_cases.py, and the pairs it finds on this package's topologies.

Run where the reference is importable (oracle/reference_import.find_reference); no test imports the reference:

    python tests/golden/make_ssd.py

Writes tests/golden/ssd.npz -- per case k the initial parameters (``c{k}_init_<var>``); per iteration n (from 1) and pair p the
lifted activation range (``c{k}_it{n}_p{p}_act``), the two weight ranges (``_first`` / ``_last``), the four scales (``_scales``
[4, C]), the five losses (``_losses``: the unchanged pair, then algo 0..3), ``_best`` and every candidate parameter set
(``_cand{a}_<var>``); and every parameter after every iteration (``c{k}_after{n}_<var>``) -- and tests/golden/ssd_pairs.json:
the pair lists (operation names along the path, in the reference's order) of the cases and of small_cnn_graph /
resnet50_graph / yolov6s_graph, the pass constructor's parameters [name, default, required] and, for `chain`, the reference's
own SNR error at the graph output without and with its SSD pass in front (``effect``).

The pass runs ``iterations`` times with ``iteration = 1`` (an iteration depends on the graph alone), so that the parameters
can be read between iterations.  The conditions the tests lean on (check_conditions) are asserted before anything is written.
Import shims as in make_equalization.py."""
import contextlib
import importlib.machinery
import inspect
import io
import json
import os
import sys
from unittest.mock import MagicMock

os.environ['PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION'] = 'python'
sys.dont_write_bytecode = True
for _name in ['onnx', 'onnx.helper', 'onnx.numpy_helper', 'onnx.mapping', 'onnx.onnx_pb', 'onnx.checker',
              'onnx.external_data_helper', 'onnx.shape_inference', 'onnx.version_converter']:
    _m = MagicMock(); _m.__spec__ = importlib.machinery.ModuleSpec(_name, None); _m.__path__ = []
    sys.modules[_name] = _m
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.reference_import import find_reference, load, quantize_reference_graph, to_reference_graph  # noqa: E402

assert find_reference() is not None, 'the reference is not importable here'
load()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppq import BaseGraph  # noqa: E402
from ppq.core import PPQ_CONFIG, NetworkFramework, QuantizationPolicy, QuantizationProperty, QuantizationStates  # noqa: E402
import ppq.lib as PFL  # noqa: E402
from ppq.quantization.analyse import graphwise_error_analyse  # noqa: E402
from ppq.quantization.optim import ParameterQuantizePass, QuantizeSimplifyPass, RuntimeCalibrationPass  # noqa: E402
from ppq.quantization.optim.ssd import SSDEqualizationPass  # noqa: E402

assert PPQ_CONFIG.USING_CUDA_KERNEL is False
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ssd_cases import CALIB_STEPS, CASES, CHANNEL_RATIO, HIST_BINS, LOSS_THRESHOLD, case_batches, case_parameters  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
# the IEEE restatement of the scales and of write_back lives with the tests' other oracles (it imports nothing but NumPy)
from ssd_reference import apply_pair as ieee_apply  # noqa: E402
from ssd_reference import scales as ieee_scales  # noqa: E402

MARGIN = 0.05
VERBOSE = '--verbose' in sys.argv
F = np.float32


def reference_graph(k: int, parameters: dict):
    """Case k built with the reference's own graph API."""
    case = CASES[k]
    g = BaseGraph(name=case['name'], built_from=NetworkFramework.ONNX)
    made = {'input': g.create_variable(name='input')}
    for kind, name, inputs, a in case['ops']:
        ins = [made[n] for n in inputs]
        attrs = {}
        if kind == 'Conv':
            pad = a['k'] // 2
            attrs = {'kernel_shape': [a['k'], a['k']], 'strides': [1, 1], 'pads': [pad] * 4, 'dilations': [1, 1], 'group': a['group']}
        elif kind == 'Gemm': attrs = {'alpha': 1.0, 'beta': 1.0, 'transA': 0, 'transB': a['transB']}
        elif kind == 'MaxPool': attrs = {'kernel_shape': [a['k'], a['k']], 'strides': [a['k'], a['k']], 'pads': [0] * 4}
        if kind in ('Conv', 'Gemm'):
            ins.append(g.create_variable(name=name + '_w', value=parameters[name + '_w'].clone(), is_parameter=True))
            if a['bias']: ins.append(g.create_variable(name=name + '_b', value=parameters[name + '_b'].clone(), is_parameter=True))
        made[name + '_out'] = g.create_variable(name=name + '_out')
        g.create_operation(op_type=kind, name=name, attributes=attrs, inputs=ins, outputs=[made[name + '_out']])
    g.mark_variable_as_graph_input(made['input'])
    for n in case['outputs']: g.mark_variable_as_graph_output(made[n])
    return g


def mutate_for(case: dict):
    """The case's quantisation policy on top of the TensorRT quantizer's configs (the `mutate` hook of
    quantize_reference_graph): per-tensor weights, and the integer platforms' passive 32-bit bias."""
    def set_tensorwise(cfg):
        if cfg.policy.has_property(QuantizationProperty.PER_CHANNEL): cfg.channel_axis = None      # (the setter wants the old policy)
        cfg.policy = QuantizationPolicy(QuantizationProperty.SYMMETRICAL + QuantizationProperty.LINEAR + QuantizationProperty.PER_TENSOR)

    def mutate(cfg, v):
        if not v.is_parameter: return
        if v.name.endswith('_w') and not case['per_channel']:
            set_tensorwise(cfg)
        if v.name.endswith('_b') and case['passive_bias']:
            if not case['per_channel']:
                set_tensorwise(cfg)
            cfg.num_of_bits = 32
            cfg.quant_min, cfg.quant_max = -(2 ** 31 - 1), 2 ** 31 - 1
            cfg.state = QuantizationStates.PASSIVE_INIT
    return mutate


class Recorder(SSDEqualizationPass):
    """The reference pass, unchanged, with its intermediate values written down."""
    def __init__(self, **kw):
        super().__init__(**kw)
        self.events = []
        self._ranges = None

    def collect_activation_range(self, pair, *a, **kw):
        r = super().collect_activation_range(pair, *a, **kw)
        self.events.append(('act', r[pair[0]].detach().clone()))
        return r

    def prepare_weight_for_equalization(self, pair):
        first, last = super().prepare_weight_for_equalization(pair)
        self._ranges = (first.detach().clone(), last.detach().clone())
        return first, last

    def write_back(self, pair, scale):
        self.events.append(('scale', scale.detach().clone(), self._ranges))
        super().write_back(pair, scale)

    def one_step_equalization(self, pair, op_act_channel_range={}, algo_type=2, **kw):
        super().one_step_equalization(pair, op_act_channel_range, algo_type, **kw)
        self.events.append(('cand', algo_type, {v.name: v.value.detach().clone() for op in (pair[0], pair[-1]) for v in op.parameters}))

    def test_ssd_loss(self, *a, **kw):
        v = super().test_ssd_loss(*a, **kw)
        self.events.append(('loss', v))
        return v


def run_case(k: int, out: dict) -> dict:
    case = CASES[k]
    params = case_parameters(k)
    batches = case_batches(k)
    g, ex = quantize_reference_graph(reference_graph(k, params), 'cpu', batches[0], bins=HIST_BINS, method='kl',
                                     mutate=mutate_for(case), parameter_pass=QuantizeSimplifyPass())
    pre = f'c{k}_'
    for name, t in params.items(): out[pre + 'init_' + name] = t.numpy()
    pairs = None
    current = {name: t.numpy().copy() for name, t in params.items()}
    stats = dict(accepted=[], margins=[], low=0, high=0, one=0, two=0, floor=0, passive=0)
    for it in range(1, case['iterations'] + 1):
        p = Recorder(iteration=1, channel_ratio=CHANNEL_RATIO, loss_threshold=LOSS_THRESHOLD)
        names = [[op.name for op in pair] for pair in p.collect_all_pairs(g)]
        assert pairs is None or pairs == names
        pairs = names
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            p.optimize(graph=g, dataloader=batches, executor=ex, collate_fn=None, calib_steps=CALIB_STEPS)
        ev = list(p.events)
        for q in range(len(pairs)):
            key = f'{pre}it{it}_p{q}_'
            kind, act = ev.pop(0); assert kind == 'act'
            kind, basic = ev.pop(0); assert kind == 'loss'
            losses, scales = [basic], []
            for algo in range(4):
                kind, scale, (first, last) = ev.pop(0); assert kind == 'scale'
                kind, a, cand = ev.pop(0); assert kind == 'cand' and a == algo
                kind, loss = ev.pop(0); assert kind == 'loss'
                losses.append(loss); scales.append(scale.numpy())
                if algo == 0: out[key + 'first'], out[key + 'last'] = first.numpy(), last.numpy()
                else: assert np.array_equal(out[key + 'first'], first.numpy()) and np.array_equal(out[key + 'last'], last.numpy())
                for name, t in cand.items(): out[f'{key}cand{algo}_{name}'] = t.numpy()
            best, best_loss = -1, basic
            for algo in range(4):
                if losses[algo + 1] < basic * LOSS_THRESHOLD and losses[algo + 1] < best_loss: best, best_loss = algo, losses[algo + 1]
            if best >= 0:
                kind, scale, _ = ev.pop(0); assert kind == 'scale' and np.array_equal(scale.numpy(), scales[best])
                kind, a, cand = ev.pop(0); assert kind == 'cand' and a == best
            scales = np.stack(scales)
            out[key + 'act'], out[key + 'scales'] = act.numpy(), scales
            out[key + 'losses'], out[key + 'best'] = np.array(losses, dtype=np.float64), np.array(best)
            # -- the conditions on this (iteration, pair)
            exact = ieee_scales(out[key + 'first'], out[key + 'last'], out[key + 'act'], CHANNEL_RATIO)
            assert np.array_equal(exact, scales), (f'{case["name"]} it {it} pair {q}: {int((exact != scales).sum())} recorded scale(s) '
                                                   'carry a mis-rounded CPU square root or quotient: give the case another seed')
            attrs = {name: a for _, name, _, a in case['ops']}
            for algo in range(4):                                # every candidate is the IEEE product / quotient of the scale
                want = ieee_apply(attrs[pairs[q][0]], attrs[pairs[q][-1]], pairs[q][0], pairs[q][-1], current, scales[algo])
                for name, t in want.items():
                    assert np.array_equal(t, out[f'{key}cand{algo}_{name}']), (case['name'], it, q, algo, name)
            if best >= 0: current.update({name: out[f'{key}cand{best}_{name}'] for name in want})
            for algo in range(4):
                limit = LOSS_THRESHOLD * basic
                stats['margins'].append(abs(losses[algo + 1] - limit) / limit)
            # two candidates below the limit compete for `best`: 5 % apart -- unless their scales are the same bits (two algos
            # clipped to one vector): then so are their parameters and, on any device, their losses, and the first one wins
            passing = [a for a in range(4) if losses[a + 1] < LOSS_THRESHOLD * basic]
            for i, a in enumerate(passing):
                for b in passing[i + 1:]:
                    if np.array_equal(scales[a], scales[b]):
                        assert losses[a + 1] == losses[b + 1]
                        continue
                    lo, hi = sorted((losses[a + 1], losses[b + 1]))
                    stats['margins'].append((hi - lo) / hi)
            stats['accepted'].append(best)
            if VERBOSE: print(f'  {case["name"]} it {it} pair {q}: best {best} losses', ' '.join(f'{v:.4e}' for v in losses))
            stats['low'] += int((scales[0] == F(0.1)).sum()); stats['high'] += int((scales[0] == F(10)).sum())
            stats['one'] += int((scales[2:] == F(1)).sum()); stats['two'] += int((scales[2:] == F(2)).sum())
            stats['floor'] += int((out[key + 'act'] < F(0.01)).sum())
        assert not ev, ev
        for v in g.variables.values():
            if not v.is_parameter: continue
            out[f'{pre}after{it}_{v.name}'] = v.value.detach().clone().numpy()
            assert np.array_equal(out[f'{pre}after{it}_{v.name}'], current[v.name]), (case['name'], it, v.name)
    for op in g.operations.values():                             # the states the pass leaves: INITIAL / PASSIVE_INIT on every pair
        if not hasattr(op, 'config') or not any(op.name in pair for pair in pairs): continue
        for cfg, v in op.config_with_variable:
            assert cfg.state not in (QuantizationStates.ACTIVATED, QuantizationStates.PASSIVE), (op.name, v.name, cfg.state)
            stats['passive'] += int(cfg.state == QuantizationStates.PASSIVE_INIT)
    return dict(pairs=pairs, stats=stats)


def end_to_end_effect(k: int) -> dict:
    """The reference's own answer to "does SSD help this case": its graphwise SNR error at the last operation after
    ParameterQuantizePass + RuntimeCalibrationPass, without and with its SSDEqualizationPass in front.  (The pass minimises the
    MSE of a PAIR; whether the graph's output gains depends on what follows the pair, so this is a condition on the case.)"""
    case, out = CASES[k], {}
    last = case['ops'][-1][1]
    for with_ssd in (False, True):
        batches = case_batches(k)
        g, ex = quantize_reference_graph(reference_graph(k, case_parameters(k)), 'cpu', batches[0], bins=HIST_BINS, method='kl',
                                         mutate=mutate_for(case), parameter_pass=QuantizeSimplifyPass())
        passes = [ParameterQuantizePass(), RuntimeCalibrationPass()]
        if with_ssd: passes.insert(0, SSDEqualizationPass(iteration=case['iterations'], channel_ratio=CHANNEL_RATIO, loss_threshold=LOSS_THRESHOLD))
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            PFL.Pipeline(passes).optimize(graph=g, dataloader=batches, executor=ex, collate_fn=None, calib_steps=CALIB_STEPS, verbose=False)
            report = graphwise_error_analyse(g, 'cpu', batches, method='snr', steps=len(batches), verbose=False)
        out['with' if with_ssd else 'without'] = float(report[last])
    return out


def check_conditions(results: dict) -> None:
    """The conditions without which the tests would pass vacuously or flip on a last bit of a GPU convolution."""
    accepted = [b for r in results.values() for b in r['stats']['accepted']]
    assert 0 in accepted and any(b >= 1 for b in accepted) and -1 in accepted, accepted
    for what in ('low', 'high', 'one', 'two', 'floor'):
        assert sum(r['stats'][what] for r in results.values()) > 0, f'no scale or range meets the `{what}` clip anywhere'
    assert results['passive_bias']['stats']['passive'] > 0
    assert results['branch']['pairs'] == [['c2', 'r2', 'c4']], results['branch']['pairs']
    effect = results['chain']['effect']
    assert effect['with'] < effect['without'] * (1 - MARGIN), (f'chain: the reference\'s SSD does not lower the error at the graph output '
                                                               f'by {MARGIN:.0%} ({effect}): give the case another seed')
    for name, r in results.items():
        assert min(r['stats']['margins']) >= MARGIN, (f'{name}: a recorded decision has a margin of {min(r["stats"]["margins"]):.3f} '
                                                      f'(< {MARGIN}): give the case another seed')


def main():
    from ppq_amd import harness
    out, book, results = {}, {'cases': {}, 'graphs': {}}, {}
    for k, case in enumerate(CASES):
        results[case['name']] = run_case(k, out)
        if case['name'] == 'chain': results['chain']['effect'] = book['effect'] = end_to_end_effect(k)
        book['cases'][case['name']] = results[case['name']]['pairs']
        s = results[case['name']]['stats']
        print(case['name'], 'pairs', len(results[case['name']]['pairs']), 'accepted', s['accepted'], 'min margin %.3f' % min(s['margins']),
              {w: s[w] for w in ('low', 'high', 'one', 'two', 'floor', 'passive')})
    check_conditions(results)
    for build in (harness.small_cnn_graph, harness.resnet50_graph, harness.yolov6s_graph):
        h = build()
        g = to_reference_graph(h)
        book['graphs'][h.name] = [[op.name for op in pair] for pair in SSDEqualizationPass().collect_all_pairs(g)]
        print(h.name, len(book['graphs'][h.name]), 'pairs')
    sig = inspect.signature(SSDEqualizationPass.__init__)
    book['constructor'] = [[n, None if q.default is inspect.Parameter.empty else getattr(q.default, '__name__', q.default),
                            q.default is inspect.Parameter.empty] for n, q in sig.parameters.items() if n != 'self']
    book['name'] = SSDEqualizationPass().name
    np.savez_compressed(os.path.join(HERE, 'ssd.npz'), **out)
    with open(os.path.join(HERE, 'ssd_pairs.json'), 'w') as f: json.dump(book, f, indent=1, sort_keys=True)
    print('ssd.npz', len(CASES), 'cases', os.path.getsize(os.path.join(HERE, 'ssd.npz')), 'bytes')


if __name__ == '__main__':
    main()
