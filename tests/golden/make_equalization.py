"""Record what the REFERENCE's LayerwiseEqualizationPass (ppq/quantization/optim/equalization.py:214-575) does on the CPU to
the case graphs of equalization_cases.py, and the equalization pairs it finds on this package's topologies.

Run where the reference is importable (oracle/reference_import.find_reference); no test imports the reference:

    python tests/golden/make_equalization.py

Writes tests/golden/equalization.npz -- per case k the initial parameters (``c{k}_init_<var>``), every pair's scale in every
iteration (``c{k}_scale_it{n}_p{p}``, n from 1), every parameter after every iteration (``c{k}_it{n}_<var>``) and, for the
cases with ``including_act``, the per-channel activation maxima the reference collected (``c{k}_act_<var>``) -- and
tests/golden/equalization_pairs.json: the pair lists of the cases and of small_cnn_graph / resnet50_graph / yolov6s_graph at
both optimize levels (layers in graph order; the reference lists sets), the start operations whose pair it drops as invalid,
and the pass constructor's parameters [name, default, required].  The conditions the tests rely on (check_conditions)
are asserted before anything is written.  Import shims as in make_roundtune.py."""
import contextlib
import importlib.machinery
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
from oracle.reference_import import find_reference, to_reference_graph  # noqa: E402

assert find_reference() is not None, 'the reference is not importable here'
sys.path.insert(0, find_reference())

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppq import BaseGraph, TorchExecutor  # noqa: E402
from ppq.core import PPQ_CONFIG, NetworkFramework  # noqa: E402
from ppq.IR import SearchableGraph, TraversalCommand  # noqa: E402
from ppq.quantization.algorithm.equalization import EqualizationHelper, EqualizationPair  # noqa: E402
from ppq.quantization.optim.equalization import (EQUALIZATION_OPERATION_TYPE, OPTIMIZATION_LAYERTYPE_CONFIG,  # noqa: E402
                                                 LayerwiseEqualizationPass)

assert PPQ_CONFIG.USING_CUDA_KERNEL is False
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from equalization_cases import CASES, VALUE_THRESHOLD, case_batches, case_parameters, natural_order_keys  # noqa: E402


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
        if kind in ('Conv', 'Gemm'):
            ins.append(g.create_variable(name=name + '_w', value=parameters[name + '_w'].clone(), is_parameter=True))
            if a['bias']: ins.append(g.create_variable(name=name + '_b', value=parameters[name + '_b'].clone(), is_parameter=True))
        made[name + '_out'] = g.create_variable(name=name + '_out')
        g.create_operation(op_type=kind, name=name, attributes=attrs, inputs=ins, outputs=[made[name + '_out']])
    g.mark_variable_as_graph_input(made['input'])
    for n in case['outputs']: g.mark_variable_as_graph_output(made[n])
    return g


def pair_names(graph, pairs) -> list:
    order = {name: i for i, name in enumerate(graph.operations)}
    return [[sorted((op.name for op in p.upstream_layers), key=order.get),
             sorted((op.name for op in p.downstream_layers), key=order.get)] for p in pairs]


def dropped_starts(graph, level: int) -> list:
    """The start operations whose pair the reference drops as invalid: the loop of optim/equalization.py:430-486 driven with the
    reference's own search engine, keeping what it throws away."""
    relay = OPTIMIZATION_LAYERTYPE_CONFIG[level]
    engine = SearchableGraph(graph)
    visited, dropped = set(), []
    for operation in [op for op in graph.operations.values() if op.type in EQUALIZATION_OPERATION_TYPE]:
        if operation in visited: continue
        down = {m[-1] for m in engine(TraversalCommand(sp_expr=lambda x: x == operation, rp_expr=lambda x, y: y.type in relay,
                                                       ep_expr=lambda x: x.type not in relay, direction='down'))}
        up = {m[-1] for m in engine(TraversalCommand(sp_expr=lambda x: x in down, rp_expr=lambda x, y: y.type in relay,
                                                     ep_expr=lambda x: x.type not in relay, direction='up'))}
        visited.update(up)
        if any(op.type not in EQUALIZATION_OPERATION_TYPE for op in up | down): dropped.append(operation.name)
    return dropped


def ieee_scale(up: np.ndarray, down: np.ndarray, value_threshold: float) -> np.ndarray:
    """calculate_scale (algorithm/equalization.py:419-426) with every step the correctly rounded fp32 operation (numpy's division
    and square root are).  torch's CPU square root is NOT always: the build this maker was written against returns the
    neighbouring float for 0.65 % of random inputs, at every vector width -- and after such a scale everything the reference
    computes differs from what correctly rounded arithmetic gives.  A HIP kernel cannot (and should not) reproduce that, so a
    case whose recording contains such a scale is refused here and re-seeded: what is recorded is the reference where its
    arithmetic is IEEE's."""
    with np.errstate(all='ignore'):
        s = (np.float32(1) / np.sqrt((up / down).astype(np.float32))).astype(np.float32)
        s = np.where(np.isnan(s), s, np.minimum(np.maximum(s, np.float32(0.1)), np.float32(10)))
        s[(up + down) < np.float32(value_threshold)] = 1
    return s.astype(np.float32)


def run_case(k: int, out: dict) -> list:
    case = CASES[k]
    params = case_parameters(k)
    g = reference_graph(k, params)
    p = LayerwiseEqualizationPass(iterations=case['iterations'], value_threshold=VALUE_THRESHOLD,
                                  including_bias=case['including_bias'], including_act=case['including_act'])
    interested = [op for op in g.operations.values() if op.type in EQUALIZATION_OPERATION_TYPE]
    pairs = pair_names(g, p.find_equalization_pair(g, interested))
    scales, snaps, down_keys, misrounded = [], [], [], []
    inner_scale, inner_equalize, inner_down = EqualizationPair.calculate_scale, EqualizationPair.equalize, EqualizationHelper.key_value_from_downstream

    def calculate_scale(self, upstream_key_values, downstream_key_values, value_threshold, *a, **kw):
        s = inner_scale(self, upstream_key_values, downstream_key_values, value_threshold, *a, **kw)
        scales.append(s.detach().clone())
        exact = ieee_scale(upstream_key_values.numpy(), downstream_key_values.numpy(), value_threshold)
        misrounded.append(int((~((exact == s.numpy()) | (np.isnan(exact) & np.isnan(s.numpy())))).sum()))
        return s

    def equalize(self, *a, **kw):
        inner_equalize(self, *a, **kw)
        snaps.append({v.name: v.value.detach().clone() for v in g.variables.values() if v.is_parameter})

    def key_value_from_downstream(op, *a, **kw):
        w = inner_down(op, *a, **kw)
        down_keys.append((op.name, w.abs().amax(dim=1).detach().clone(), op.inputs[1].value.detach().clone(), op.attributes.get('group', 1)))
        return w
    EqualizationPair.calculate_scale, EqualizationPair.equalize = calculate_scale, equalize
    EqualizationHelper.key_value_from_downstream = staticmethod(key_value_from_downstream)
    try:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            p.optimize(graph=g, dataloader=case_batches(k), executor=TorchExecutor(g, device='cpu'), collate_fn=None)
    finally:
        EqualizationPair.calculate_scale, EqualizationPair.equalize = inner_scale, inner_equalize
        EqualizationHelper.key_value_from_downstream = staticmethod(inner_down)
    P = len(pairs)
    assert len(scales) == len(snaps) == P * case['iterations'], (case['name'], len(scales), P)
    pre = f'c{k}_'
    for name, t in params.items(): out[pre + 'init_' + name] = t.numpy()
    for it in range(case['iterations']):
        for q in range(P): out[f'{pre}scale_it{it + 1}_p{q}'] = scales[it * P + q].numpy()
        for name, t in snaps[(it + 1) * P - 1].items(): out[f'{pre}it{it + 1}_{name}'] = t.numpy()
    if case['including_act']:
        for op in interested:
            a = op.outputs[0].value                             # [channels, batches], written back by the reference
            assert a is not None and a.ndim == 2, op.name
            out[pre + 'act_' + op.outputs[0].name] = a.amax(dim=-1).numpy()
    assert sum(misrounded) == 0, (f'{case["name"]}: {sum(misrounded)} recorded scale(s) carry a misrounded CPU square root '
                                  '(see ieee_scale): give the case another seed')
    reordered = any(groups > 1 and w.shape[1] > 1 and not torch.equal(keys, natural_order_keys(w, groups))
                    for _, keys, w, groups in down_keys)
    return pairs, reordered


def check_conditions(out: dict) -> dict:
    """The conditions without which the tests would pass vacuously; returns the counts per case.  Every case: first-iteration
    channels with s == 1 (the threshold) and with s != 1.  At least one case each: a scale clipped at 0.1, one at 10."""
    counts = {}
    for k, case in enumerate(CASES):
        s = np.concatenate([v for n, v in out.items() if n.startswith(f'c{k}_scale_it1_')])
        c = dict(one=int((s == 1).sum()), other=int((s != 1).sum()), low=int((s == np.float32(0.1)).sum()),
                 high=int((s == 10).sum()), nan=int(np.isnan(s).sum()))
        assert c['one'] > 0 and c['other'] > 0, (case['name'], c)
        counts[case['name']] = c
    assert any(c['low'] > 0 for c in counts.values()) and any(c['high'] > 0 for c in counts.values()), counts
    assert counts['nan_key']['nan'] > 0 and counts['zero_act']['high'] > 0, counts
    return counts


def main():
    from ppq_amd import harness
    out, book = {}, {'cases': {}, 'graphs': {}}
    reordered = False
    for k, case in enumerate(CASES):
        pairs, r = run_case(k, out)
        book['cases'][case['name']] = pairs
        reordered = reordered or r
    assert reordered, 'no case has a grouped downstream key order that differs from the natural order'
    for name, c in check_conditions(out).items(): print(name, c)
    for build in (harness.small_cnn_graph, harness.resnet50_graph, harness.yolov6s_graph):
        h = build()
        g = to_reference_graph(h)
        interested = [op for op in g.operations.values() if op.type in EQUALIZATION_OPERATION_TYPE]
        book['graphs'][h.name] = {}
        for level in (1, 2):
            p = LayerwiseEqualizationPass(iterations=1, optimize_level=level)
            book['graphs'][h.name][str(level)] = {'pairs': pair_names(g, p.find_equalization_pair(g, interested)),
                                                  'dropped': dropped_starts(g, level)}
            print(h.name, level, len(book['graphs'][h.name][str(level)]['pairs']), 'pairs,',
                  len(book['graphs'][h.name][str(level)]['dropped']), 'dropped')
    every = [p for g in book['graphs'].values() for lv in g.values() for p in lv['pairs']]
    assert any(len(up) > 1 and len(down) > 1 for up, down in every), 'no pair with several upstream and several downstream layers'
    assert any(lv['dropped'] for g in book['graphs'].values() for lv in g.values()), 'no dropped invalid pair'
    import inspect
    sig = inspect.signature(LayerwiseEqualizationPass.__init__)
    book['constructor'] = [[n, None if q.default is inspect.Parameter.empty else q.default, q.default is inspect.Parameter.empty]
                           for n, q in sig.parameters.items() if n != 'self']         # [name, default, required]
    np.savez_compressed(os.path.join(HERE, 'equalization.npz'), **out)
    with open(os.path.join(HERE, 'equalization_pairs.json'), 'w') as f: json.dump(book, f, indent=1, sort_keys=True)
    print('equalization.npz', len(CASES), 'cases', os.path.getsize(os.path.join(HERE, 'equalization.npz')), 'bytes')


if __name__ == '__main__':
    main()
