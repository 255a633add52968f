"""Host side of the statistical reports (ppq_amd/statistics.py): no GPU needed.

Everything reference-derived comes from tests/golden/statistics.npz / statistics.json (tests/golden/make_statistics.py records
them from the reference's own statistical_analyse and parameter_analyse on the CPU); the case graph is rebuilt from
tests/golden/statistics_cases.py.  The CPU executor and its stand-in fake-quant are those of test_host_analyse.py."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import statistics_cases as C  # noqa: E402
from test_host_analyse import _Counting, _assert_untouched, _cpu_setup, _snapshot  # noqa: E402

GOLD = np.load(os.path.join(HERE, 'golden', 'statistics.npz'))
with open(os.path.join(HERE, 'golden', 'statistics.json')) as _f: BOOK = json.load(_f)


def golden_pairs(device='cpu'):
    """[(operation, variable, x_fp, x_qt)] of the recorded series on the operations and variables of the case graph."""
    graph = C.harness_graph(quantize=False)
    return [(graph.operations[e['Op name']], graph.variables[e['Variable name']],
             torch.from_numpy(GOLD[f'fp_{k}']).to(device), torch.from_numpy(GOLD[f'qt_{k}']).to(device)) for k, e in enumerate(BOOK['records'])]


def test_the_fixture_holds_what_the_tests_lean_on():
    assert BOOK['keys'] == C.KEYS and len(C.KEYS) == 28 and len(BOOK['records']) == 18
    constant = [e for e in BOOK['records'] if e['constant']['Noise']]
    assert constant and all(math.isnan(GOLD['ref_scalars'][k, 0, 2]) for k, e in enumerate(BOOK['records']) if e['constant']['Noise'])
    assert any(e['edges']['Quantized'] > 0 for e in BOOK['records'])
    for k, e in enumerate(BOOK['records']):                                 # the edge cap, recomputed from the series
        series = {'Noise': C.noise_of(GOLD[f'qt_{k}'], GOLD[f'fp_{k}']), 'Quantized': GOLD[f'qt_{k}'], 'Float': GOLD[f'fp_{k}']}
        for kind, x in series.items():
            assert C.edge_samples(x) == e['edges'][kind]
            if not e['constant'][kind]: assert e['edges'][kind] <= C.EDGE_CAP * x.size, (k, kind)


def test_series_statistics_torch_arm_reproduces_the_reference_records():
    """The same fp32 CPU reductions on the same data: Min, Max and Hist are equal, NaN sits where the reference has it, and
    every other value is within its recorded reference-to-float64 deviation plus the same amount again."""
    from ppq_amd.analyse import series_statistics
    records = series_statistics(golden_pairs(), bins=C.BINS, use_kernels=False)
    assert len(records) == len(BOOK['records'])
    worst = 0.0
    for k, (rec, entry) in enumerate(zip(records, BOOK['records'])):
        assert list(rec) == BOOK['keys']
        for key in C.KEYS[:6]: assert rec[key] == entry[key] and type(rec[key]) is type(entry[key]), (k, key)
        for s, kind in enumerate(C.KINDS):
            assert rec[f'{kind} Hist'] == GOLD['ref_hist'][k, s].tolist() and all(type(c) is float for c in rec[f'{kind} Hist'])
            for i, field in enumerate(C.SCALARS):
                got, ref, f64 = rec[f'{kind} {field}'], GOLD['ref_scalars'][k, s, i], GOLD['f64_scalars'][k, s, i]
                assert type(got) is float
                if field in ('Max', 'Min'): assert got == ref, (k, kind, field)
                elif math.isnan(ref): assert math.isnan(got), (k, kind, field)
                else:
                    assert abs(got - ref) <= 2 * abs(ref - f64), (k, kind, field, got, ref, f64)
                    worst = max(worst, abs(got - ref))
        ref, f64 = GOLD['ref_snr'][k], GOLD['f64_snr'][k]
        assert abs(rec['Noise:Signal Power Ratio'] - ref) <= 2 * abs(ref - f64), (k, rec['Noise:Signal Power Ratio'], ref, f64)
    print('largest difference to the recorded reference value', worst)


def _expected_slots(graph):
    from ppq_amd import harness
    return [(op.name, var.name) for op in graph.operations.values()
            if isinstance(op, harness.QuantableOperation) and op.type not in harness.PASSIVE_OPERATIONS
            for var in list(op.inputs) + list(op.outputs)]


def test_statistical_analyse_on_the_cpu_follows_the_reference_protocol():
    from ppq_amd import analyse, harness
    graph, ex, data = _cpu_setup()
    snap = _snapshot(graph)
    loader = _Counting(data)
    steps, batches = 3, 4                                                   # batches 0 .. steps inclusive
    pairs = analyse.collect_samples(graph, 'cpu', loader, steps=steps, executor=ex, use_kernels=False)
    assert loader.taken == 2 * batches and analyse.last_analysis_stats['forwards'] == 2 * batches
    _assert_untouched(graph, snap)
    slots = _expected_slots(graph)
    assert [(op.name, var.name) for op, var, _, _ in pairs] == slots and len(slots) > 6
    assert not any(op.type in harness.PASSIVE_OPERATIONS for op, _, _, _ in pairs)
    index = {}
    for op, var, x_fp, x_qt in pairs:
        assert x_fp.shape == x_qt.shape == (batches * 1024,) and x_fp.device.type == 'cpu'
        if var.is_parameter:                                                # sampled at every batch: the samples repeat
            table = index.setdefault(var.value.numel(), analyse.generate_indexer(1024, var.value.numel(), 10086).long())
            assert torch.equal(x_fp, var.value.flatten().index_select(0, table).repeat(batches))
            assert torch.equal(x_qt.view(batches, 1024)[0], x_qt.view(batches, 1024)[-1])
    # the graph's output in the quantised run is what a plain quantised forward gives
    op, var, _, x_qt = pairs[-1]
    assert var.name in graph.outputs
    for b in range(batches):
        y = ex.forward(inputs=data[b])[list(graph.outputs).index(var.name)].flatten()
        assert torch.equal(x_qt.view(batches, 1024)[b], y.index_select(0, analyse.generate_indexer(1024, y.numel(), 10086).long()))
    assert any(not torch.equal(x_fp, x_qt) for _, var, x_fp, x_qt in pairs if not var.is_parameter)       # quantisation was on in phase 2

    records = analyse.statistical_analyse(graph, 'cpu', _Counting(data), steps=steps, executor=ex, use_kernels=False)
    _assert_untouched(graph, snap)
    assert [(r['Op name'], r['Variable name']) for r in records] == slots
    again = analyse.series_statistics(pairs, use_kernels=False)
    for rec, same, (op, var, x_fp, x_qt) in zip(records, again, pairs):
        assert list(rec) == C.KEYS
        assert json.dumps(rec) == json.dumps(same)                          # (NaN included)
        assert rec['Op type'] == op.type and rec['Is parameter'] == var.is_parameter
        assert rec['Is input'] == (var in op.inputs) and rec['Is output'] == (var in op.outputs)
        for kind in C.KINDS:
            assert len(rec[f'{kind} Hist']) == 32 and sum(rec[f'{kind} Hist']) == batches * 1024
        assert rec['Float Min'] == float(x_fp.min()) and rec['Quantized Max'] == float(x_qt.max())
        f64 = C.float64_series(x_fp.numpy())
        assert abs(rec['Float Mean'] - f64['Mean']) <= 1e-5 * max(1.0, abs(f64['Mean'])) and abs(rec['Float Std'] - f64['Std']) <= 1e-5 * f64['Std']


def test_a_forward_that_raises_leaves_the_graph_as_it_was(monkeypatch):
    from ppq_amd import analyse, harness
    graph, ex, data = _cpu_setup()
    snap = _snapshot(graph)
    real, calls = harness._forward, {'n': 0}

    def failing(op, x):
        calls['n'] += 1
        if calls['n'] > 12: raise RuntimeError('boom')
        return real(op, x)
    monkeypatch.setattr(harness, '_forward', failing)
    with pytest.raises(RuntimeError, match='boom'):
        analyse.statistical_analyse(graph, 'cpu', data, steps=2, executor=ex, use_kernels=False)
    monkeypatch.setattr(harness, '_forward', real)
    _assert_untouched(graph, snap)


def test_the_kernel_arm_refuses_cpu_tensors():
    """No quiet fall-back: with the kernels on, a CPU executor or a CPU series is an error, not a torch run."""
    from ppq_amd import analyse
    graph, ex, data = _cpu_setup()
    snap = _snapshot(graph)
    with pytest.raises(RuntimeError, match='Kernel Failure'):
        analyse.statistical_analyse(graph, 'cpu', data, steps=1, executor=ex)
    _assert_untouched(graph, snap)
    with pytest.raises(RuntimeError, match='Kernel Failure'):
        analyse.series_statistics(golden_pairs()[:2])
    with pytest.raises(RuntimeError, match='Kernel Failure'):
        analyse.variable_analyse(graph, data, list(graph.outputs), running_device='cpu', steps=1, executor=ex)
    _assert_untouched(graph, snap)


def test_parameter_analyse_prints_the_reference_charts(capsys):
    from ppq_amd import analyse
    graph = C.harness_graph()
    snap = _snapshot(graph)
    got = analyse.parameter_analyse(graph)                                  # CPU parameters take the torch arm
    assert capsys.readouterr().out == BOOK['parameter_analyse']['text']
    assert got == BOOK['parameter_analyse']['values'] and list(got) == ['Value Range', 'Value Std', 'Value Mean(Abs)']
    assert analyse.last_analysis_stats['stat_launches'] == 0
    assert analyse.parameter_analyse(graph, verbose=False, use_kernels=False) == got and capsys.readouterr().out == ''
    _assert_untouched(graph, snap)
    # a parameter of one element is skipped, as in the reference
    graph.variables['c1_b'].value = torch.zeros(1)
    assert 'c1_b[c1]' not in analyse.parameter_analyse(graph, verbose=False)['Value Std']
