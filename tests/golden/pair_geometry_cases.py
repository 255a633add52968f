"""The pairs whose kernel geometry tests/golden/pair_geometry.json records (written by make_pair_geometry.py, read by
tests/test_host_pair_geometry.py): every pair of the case graphs of equalization_cases.py, ssd_cases.py and
channel_split_cases.py and of ``harness.small_cnn_graph``, plus hand-built pairs of at most 8 channels for the layouts those
graphs do not hold -- a MatMul downstream, a ``transB = 0`` Gemm upstream of a ``transB = 1`` one, and SSD's Gemm behind a
flattened Conv.

``record()`` runs the three functions that answer "which axis of a weight is the pair's channel, and how do the kernels address
it" -- ``equalization.pair_jobs``, ``ssd.pair_geometry`` and ``channel_split.split_tensors`` -- and returns their result tuples
with every tensor and variable replaced by {var: name, shape: [...]}."""
import torch

import channel_split_cases as CC
import equalization_cases as EC
import ssd_cases as SC

BIAS_MULTIPLIER, ACT_MULTIPLIER = 0.25, 0.75           # not the defaults: a segment that drops its multiplier shows


def _linear_graph(name: str, ops: list):
    """A chain of Gemm / MatMul given as (type, name, weight shape, transB or None, bias)."""
    from ppq_amd import harness
    g = harness.BaseGraph(name)
    y = g.create_variable('input'); g.inputs['input'] = y
    for kind, op, shape, trans_b, bias in ops:
        ins = [y, g.create_variable(op + '_w', torch.zeros(shape), True)]
        if bias: ins.append(g.create_variable(op + '_b', torch.zeros(shape[0] if trans_b else shape[1]), True))
        y = g.create_operation(kind, op, ins, {} if trans_b is None else {'transB': trans_b})
    g.outputs[y.name] = y
    return g


def flat_graph(wide: bool):
    """tests/test_host_ssd.py's Gemm behind a GlobalAveragePool (``wide``: behind a flattened [4, 2, 3] tensor instead)."""
    from ppq_amd import harness
    g = harness.BaseGraph('flat_wide' if wide else 'flat')
    x = g.create_variable('input'); g.inputs['input'] = x
    y = g.create_operation('Conv', 'c1', [x, g.create_variable('c1_w', torch.zeros(4, 3, 3, 3), True),
                                         g.create_variable('c1_b', torch.zeros(4), True)], {'strides': 1, 'pads': 1, 'group': 1})
    y = g.create_operation('Relu', 'r1', [y])
    y = g.create_operation('GlobalAveragePool', 'gap', [y])
    y = g.create_operation('Gemm', 'fc', [y, g.create_variable('fc_w', torch.zeros(5, 24 if wide else 4), True)])
    g.outputs[y.name] = y
    return g


def _names(graph) -> dict:
    return {id(v.value): n for n, v in graph.variables.items() if isinstance(v.value, torch.Tensor)}


def _plain(x, names: dict):
    if isinstance(x, (tuple, list)): return [_plain(v, names) for v in x]
    if isinstance(x, torch.Tensor): return {'var': names[id(x)], 'shape': list(x.shape)}
    if hasattr(x, 'value') and hasattr(x, 'name'): return {'var': x.name, 'shape': list(x.value.shape)}
    if isinstance(x, (bool, int, float)) or x is None: return x
    raise TypeError(f'unexpected {type(x).__name__} in a geometry tuple')


def _equalization(graph, pairs, including_bias: bool, including_act: bool) -> list:
    """pair_jobs (and, for an ungrouped pair, split_tensors) of every pair."""
    from ppq_amd import channel_split as CS
    from ppq_amd import equalization as EQ
    names, out = _names(graph), []
    for pair in pairs:
        C = pair.num_channel()
        scale = torch.empty(C)
        acts = {op.outputs[0].name: torch.zeros(C) for op in pair.upstream_layers} if including_act else {}
        local = {**names, id(scale): 'scale', **{id(a): 'act:' + n for n, a in acts.items()}}
        rec = {'up': [op.name for op in pair.upstream_layers], 'down': [op.name for op in pair.downstream_layers],
               'pair_jobs': _plain(EQ.pair_jobs(pair, scale, 0.5, including_bias, including_act, BIAS_MULTIPLIER, ACT_MULTIPLIER, acts), local)}
        if not CS.is_group_conv(pair): rec['split_tensors'] = _plain(CS.split_tensors(pair), local)
        out.append(rec)
    return out


def _ssd(graph, pairs) -> list:
    from ppq_amd import ssd as SSD
    names = _names(graph)
    return [{'ops': [op.name for op in pair], 'pair_geometry': _plain(SSD.pair_geometry(pair), names)} for pair in pairs]


def record() -> dict:
    from ppq_amd import equalization as EQ
    from ppq_amd import harness
    from ppq_amd import ssd as SSD
    book = {'equalization': {}, 'channel_split': {}, 'ssd': {}}

    def found(g):
        p = EQ.LayerwiseEqualizationPass(iterations=1)
        return p.find_equalization_pair(g, p.interested_operations(g))

    for k, case in enumerate(EC.CASES):
        g = EC.harness_graph(k)
        book['equalization'][case['name']] = _equalization(g, found(g), case['including_bias'], case['including_act'])
    for k, case in enumerate(CC.CASES):
        g = CC.harness_graph(k)
        book['channel_split'][case['name']] = _equalization(g, found(g), case['including_bias'], case['including_act'])
    for k, case in enumerate(SC.CASES):
        g = SC.harness_graph(k, quantize=False)
        book['ssd'][case['name']] = _ssd(g, SSD.SSDEqualizationPass().collect_all_pairs(g))
    g = harness.small_cnn_graph()
    book['equalization']['small_cnn'] = _equalization(g, found(g), True, False)
    book['ssd']['small_cnn'] = _ssd(g, SSD.SSDEqualizationPass().collect_all_pairs(g))

    # a biased transB = 0 Gemm upstream of a MatMul ([in, out]); a transB = 0 Gemm upstream of a transB = 1 one
    for name, ops in (('matmul_down', [('Gemm', 'fc1', (5, 8), 0, True), ('MatMul', 'mm', (8, 3), None, False)]),
                      ('gemm_0_to_1', [('Gemm', 'fc1', (5, 8), 0, True), ('Gemm', 'fc2', (6, 8), 1, True)])):
        g = _linear_graph(name, ops)
        pair = EQ.EqualizationPair([g.operations[ops[0][1]]], [g.operations[ops[1][1]]])
        book['equalization'][name] = _equalization(g, [pair], True, True)
    g = _linear_graph('gemm_0_to_1', [('Gemm', 'fc1', (5, 8), 0, True), ('Gemm', 'fc2', (6, 8), 1, True)])
    book['ssd']['gemm_0_to_1'] = _ssd(g, SSD.SSDEqualizationPass().collect_all_pairs(g))
    for wide in (False, True):
        g = flat_graph(wide)
        book['ssd'][g.name] = _ssd(g, SSD.SSDEqualizationPass().collect_all_pairs(g))
    return book
