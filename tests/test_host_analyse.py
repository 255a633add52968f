"""Host side of the error analysis (ppq_amd/analyse.py, ppq_amd/measure.py): no GPU needed.

Everything reference-derived comes from tests/golden/analyse.npz (tests/golden/make_analyse.py records it from the reference's
own code on the CPU); the inputs are regenerated from tests/golden/analyse_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import analyse_cases as C  # noqa: E402

GOLD = np.load(os.path.join(HERE, 'golden', 'analyse.npz'))


def _fn(method):
    from ppq_amd import measure
    return {'snr': measure.torch_snr_error, 'mse': measure.torch_mean_square_error, 'cosine': measure.torch_cosine_similarity}[method]


def _count(shape): return int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])


@pytest.mark.parametrize('k', range(len(C.INDEXER_CASES)))
def test_generate_indexer_equals_the_reference_tables(k):
    from ppq_amd.analyse import generate_indexer
    fetches, elements, seed = C.INDEXER_CASES[k]
    got = generate_indexer(fetches, elements, seed)
    assert got.dtype == torch.int32 and got.device.type == 'cpu' and got.shape == (fetches,)
    assert np.array_equal(got.numpy(), GOLD[f'indexer_{k}'])
    assert torch.equal(generate_indexer(fetches, elements, seed), got)                 # the kept seed chain gives it again


def test_batch_random_fetch_on_the_cpu_equals_the_reference():
    from ppq_amd.analyse import batch_random_fetch
    got = batch_random_fetch(C.measure_tensors(6)[1], fetches_per_batch=50, seed=10086)
    assert np.array_equal(got.numpy(), GOLD['fetch_four_dim'])
    with pytest.raises(ValueError): batch_random_fetch(torch.zeros(2, 3))              # the unseeded form is not provided


@pytest.mark.parametrize('method', C.METHODS)
@pytest.mark.parametrize('k', range(len(C.MEASURE_CASES)))
def test_measures_on_cpu_tensors_match_the_reference(k, method):
    name, shape = C.MEASURE_CASES[k]
    pred, real = C.measure_tensors(k)
    count = _count(shape)
    rows_ref = GOLD[f'measure_{name}_{method}_none']
    got = _fn(method)(pred, real, 'none').numpy()
    assert got.shape == rows_ref.shape == ((shape[0],) if len(shape) > 1 else (1,))
    err = np.abs(got.astype(np.float64) - rows_ref)
    print(name, method, 'max error / bound', float((err / C.measure_bound(method, count, rows_ref)).max()))
    assert (err <= C.measure_bound(method, count, rows_ref)).all()
    for reduction in ('mean', 'sum'):
        want = float(GOLD[f'measure_{name}_{method}_{reduction}'])
        assert abs(float(_fn(method)(pred, real, reduction)) - want) <= C.reduced_bound(method, count, rows_ref, reduction)


def test_measure_argument_checks_and_the_cosine_loss():
    from ppq_amd import measure
    a, b = torch.ones(2, 8), torch.ones(2, 9)
    for method in C.METHODS:
        with pytest.raises(ValueError): _fn(method)(a, b)
        with pytest.raises(ValueError): _fn(method)(a, a, 'median')
        assert _fn(method)(a, a, 'MEAN').ndim == 0                                     # the reduction is lower-cased
        assert np.array_equal(_fn(method)(torch.zeros(2, 64), torch.zeros(2, 64), 'none').numpy(), GOLD[f'measure_zero_{method}_none'])
    pred, real = C.measure_tensors(1)
    assert torch.equal(measure.torch_cosine_similarity_as_loss(pred, real, 'none'), 1 - measure.torch_cosine_similarity(pred, real, 'none'))
    x = pred.clone().requires_grad_(True)
    measure.torch_snr_error(x, real).backward()                                        # tensors with grad keep the torch formula
    assert x.grad is not None and torch.isfinite(x.grad).all()


@pytest.mark.parametrize('method', C.METHODS)
def test_measure_recorder_follows_the_reference_sequence(method):
    from ppq_amd.analyse import MeasureRecorder
    rec, top = MeasureRecorder(measurement=method), MeasureRecorder(measurement=method, reduce='max')
    want_mean, running_max, rows_seen, bound = GOLD[f'recorder_{method}_mean'], 0.0, 0, 0.0
    for i, batch in enumerate(C.RECORDER_BATCHES):
        pred, real = C.recorder_tensors(i)
        rec.update(y_pred=pred, y_real=real); top.update(y_pred=pred, y_real=real)
        rows_ref = GOLD[f'recorder_{method}_rows_{i}']
        # the running mean is a batch-size weighted mean of the per-update results: so is its tolerance
        bound = (bound * rows_seen + C.reduced_bound(method, C.RECORDER_ROW, rows_ref, 'mean') * batch) / (rows_seen + batch)
        rows_seen += batch
        assert rec.num_of_elements == top.num_of_elements == rows_seen
        assert abs(rec.measure - want_mean[i]) <= bound + 1e-12 * abs(want_mean[i])
        # reduce='max': the reference's constructor takes it and its update then fails (recorded); here it is the running
        # maximum of the per-row values, which the reference's own rows give
        assert int(GOLD[f'recorder_{method}_max_raises']) == 1
        running_max = max(running_max, float(rows_ref.max()))
        assert abs(top.measure - running_max) <= C.measure_bound(method, C.RECORDER_ROW, rows_ref).max()
    assert rec.device_reads == 0
    with pytest.raises(ValueError): MeasureRecorder(measurement='psnr')
    with pytest.raises(ValueError): MeasureRecorder(reduce='min')
    with pytest.raises(Exception): rec.update(torch.zeros(2, 4), torch.zeros(3, 4))


@pytest.mark.parametrize('k', range(len(C.PRINTER_CASES)))
def test_measure_printer_prints_the_reference_text(k, capsys):
    from ppq_amd.analyse import MeasurePrinter
    name, data, kwargs = C.PRINTER_CASES[k]
    MeasurePrinter(data, **kwargs).print()
    assert capsys.readouterr().out == str(GOLD[f'printer_{name}'])
    with pytest.raises(ValueError): MeasurePrinter(data, measure='x', order='sideways')


# ---- the two analyses on the CPU: use_kernels=False, a handed-in executor with a stand-in fake-quant function --------------
def _fake_quant(tensor, config):
    """Holds no state of its own: a 1/16 grid where the config is activated, the tensor itself otherwise."""
    from ppq_amd.core import QuantizationStates
    return torch.round(tensor * 16.0) / 16.0 if QuantizationStates.is_activated(config.state) else tensor


def _cpu_setup(batches=6):
    from ppq_amd import harness
    from ppq_amd.core import QuantizationStates
    graph = harness.small_cnn_graph(seed=3)
    harness.quantize_graph(graph, 'minmax')
    for op in graph.operations.values():
        for cfg, _ in getattr(op, 'config_with_variable', []):
            if cfg.state == QuantizationStates.INITIAL: cfg.state = QuantizationStates.ACTIVATED
    ex = harness.TorchExecutor(graph, 'cpu')
    ex._default_quant_fn = _fake_quant
    gen = torch.Generator().manual_seed(0)
    data = [torch.rand(3 if i != 2 else 2, 3, 16, 16, generator=gen) for i in range(batches)]
    return graph, ex, data


class _Counting:
    def __init__(self, data): self.data, self.taken = data, 0

    def __iter__(self):
        for batch in self.data:
            self.taken += 1
            yield batch

    def __len__(self): return len(self.data)


def _snapshot(graph):
    snap = {}
    for op in graph.operations.values():
        for i, (cfg, var) in enumerate(getattr(op, 'config_with_variable', [])):
            snap[(op.name, i)] = (cfg.state, cfg.detail.get('Stored State'), getattr(op, '_dequantized', False))
    for var in graph.variables.values():
        if var.is_parameter:
            snap[var.name] = (var.value.clone(), None if var.stored_value is None else var.stored_value.clone(),
                              var.value.data_ptr())
    return snap


def _assert_untouched(graph, snap):
    now = _snapshot(graph)
    assert now.keys() == snap.keys()
    for key, was in snap.items():
        if isinstance(was[0], torch.Tensor):
            assert torch.equal(now[key][0], was[0]) and now[key][2] == was[2], key
            assert (was[1] is None and now[key][1] is None) or torch.equal(now[key][1], was[1]), key
        else: assert now[key] == was, key


def _reference_two_phase_loop(graph, ex, data, method, steps, fetchs):
    """analyse/graphwise.py:113-164 restated: phase 1 dequantised, samples to the CPU; phase 2 quantised, measured there."""
    from ppq_amd import harness
    from ppq_amd.analyse import MeasureRecorder, generate_indexer

    class Keep:
        def __init__(self): self.fetched = None
        def pre_forward_hook(self, inputs, quant_inputs, quant_configs): return quant_inputs

        def post_forward_hook(self, outputs, quant_outputs, quant_configs):
            rows = quant_outputs[0].flatten(start_dim=1)
            self.fetched = rows.index_select(dim=-1, index=generate_indexer(fetchs, rows.shape[-1], 10086).long())
            return quant_outputs
    ops = [op for op in graph.operations.values() if hasattr(op, 'config') and op.type in harness.COMPUTING_OP]
    hooks = {op.name: Keep() for op in ops}
    recorders = {op.name: MeasureRecorder(measurement=method, use_kernels=False) for op in ops}
    caches = {op.name: [] for op in ops}
    quantable = [op for op in graph.operations.values() if hasattr(op, 'config')]
    for op in quantable: op.dequantize()
    for idx, batch in enumerate(data):
        ex.forward(inputs=batch, hooks=hooks)
        for op in ops: caches[op.name].append(hooks[op.name].fetched)
        if idx >= steps: break
    for op in quantable: op.restore_quantize_state()
    for idx, batch in enumerate(data):
        ex.forward(inputs=batch, hooks=hooks)
        for op in ops: recorders[op.name].update(y_real=caches[op.name][idx], y_pred=hooks[op.name].fetched)
        if idx >= steps: break
    return {op.name: recorders[op.name].measure for op in ops}


@pytest.mark.parametrize('method', C.METHODS)
def test_graphwise_analysis_on_the_cpu_is_the_reference_protocol(method, capsys):
    from ppq_amd import analyse
    graph, ex, data = _cpu_setup()
    snap = _snapshot(graph)
    loader = _Counting(data)
    got = analyse.graphwise_error_analyse(graph, 'cpu', loader, method=method, steps=3, verbose=True, fetchs=256,
                                          executor=ex, use_kernels=False)
    assert list(got) == ['c1', 'c2', 'fc']                                  # the quantable computing operations, graph order
    assert loader.taken == 2 * (3 + 1)                                      # steps + 1 batches in each of the two phases
    assert analyse.last_analysis_stats['forwards'] == 8
    _assert_untouched(graph, snap)
    text = capsys.readouterr().out
    assert analyse._METHOD_TITLES[method] in text and all(name + ':' in text for name in got)
    want = _reference_two_phase_loop(graph, ex, data, method, 3, 256)
    assert got == want                                                      # same operations on the same tensors
    assert all(np.isfinite(v) for v in got.values()) and (method == 'cosine' or max(got.values()) > 0)
    _assert_untouched(graph, snap)
    whole = analyse.graphwise_error_analyse(graph, 'cpu', _Counting(data), method=method, steps=1, verbose=False, fetchs=None,
                                            executor=ex, use_kernels=False)
    assert list(whole) == list(got) and analyse.last_analysis_stats['forwards'] == 4
    _assert_untouched(graph, snap)


def test_layerwise_analysis_on_the_cpu(capsys):
    from ppq_amd import analyse, harness
    graph, ex, data = _cpu_setup()
    snap = _snapshot(graph)
    loader = _Counting(data)
    got = analyse.layerwise_error_analyse(graph, loader, running_device='cpu', method='snr', steps=2, verbose=False, executor=ex,
                                          use_kernels=False)
    assert list(got) == ['c1', 'c2', 'fc'] and loader.taken == 3
    assert analyse.last_analysis_stats['forwards'] == 3 + 3 * 3             # FP32 outputs once per batch, then one per operation
    _assert_untouched(graph, snap)
    # the reference's loop for one operation: everything dequantised but `c2`, the graph output measured
    quantable = [op for op in graph.operations.values() if hasattr(op, 'config')]
    rec = analyse.MeasureRecorder('snr', use_kernels=False)
    for op in quantable: op.dequantize()
    for idx, batch in enumerate(data):
        fp = ex.forward(inputs=batch)
        graph.operations['c2'].restore_quantize_state()
        qt = ex.forward(inputs=batch)
        rec.update(y_pred=qt[0], y_real=fp[0])
        graph.operations['c2'].dequantize()
        if idx >= 2: break
    for op in quantable: op.restore_quantize_state()
    assert got['c2'] == rec.measure and got['c2'] > 0
    _assert_untouched(graph, snap)


@pytest.mark.parametrize('which', ['graphwise', 'graphwise_whole', 'layerwise'])
def test_a_forward_that_raises_leaves_the_graph_as_it_was(which, monkeypatch):
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
        if which == 'layerwise':
            analyse.layerwise_error_analyse(graph, data, running_device='cpu', steps=2, verbose=False, executor=ex, use_kernels=False)
        else:
            analyse.graphwise_error_analyse(graph, 'cpu', data, steps=2, verbose=False, executor=ex, use_kernels=False,
                                            fetchs=None if which == 'graphwise_whole' else 64)
    monkeypatch.setattr(harness, '_forward', real)
    _assert_untouched(graph, snap)


def test_the_kernel_path_refuses_cpu_tensors():
    """No quiet fall-back: with the kernels on, a CPU executor is an error, not a torch run."""
    from ppq_amd import analyse
    graph, ex, data = _cpu_setup()
    snap = _snapshot(graph)
    with pytest.raises(RuntimeError):
        analyse.graphwise_error_analyse(graph, 'cpu', data, steps=1, verbose=False, executor=ex, fetchs=64)
    _assert_untouched(graph, snap)
