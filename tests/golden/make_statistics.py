"""Record what the REFERENCE's statistical_analyse (ppq/quantization/analyse/graphwise.py:186-372) and parameter_analyse
(analyse/layerwise.py:179-203) say, on the CPU, about the case graph of statistics_cases.py.

Run where the reference is importable (oracle/reference_import.find_reference); no test imports the reference:

    python tests/golden/make_statistics.py

The graph is built with the reference's own graph API, quantised and calibrated through oracle/reference_import.py, and both
analyses run unmodified.  The samples are captured by wrapping the module global ``tensor_random_fetch`` of
ppq.quantization.analyse.graphwise, the values of parameter_analyse by wrapping the ``MeasurePrinter`` of analyse.layerwise.

Writes tests/golden/statistics.npz -- per record k the FP32 and the quantised sample series (``fp_{k}`` / ``qt_{k}``, float32
[n]); ``ref_scalars`` [records, 3 kinds, 6] (Mean, Std, Skewness, Kurtosis, Max, Min of Noise / Quantized / Float as the
reference reports them), ``ref_hist`` [records, 3, 32], ``ref_snr`` [records]; ``f64_scalars`` / ``f64_snr``: the same formulas
in float64 on the same series (statistics_cases.float64_series) -- and tests/golden/statistics.json: the keys of a record in
the reference's order, per record its operation, variable and flags, the edge samples of every series, the largest deviation of
the reference's values from float64 per kind of statistic (informative), and parameter_analyse's printout and values.

The conditions the tests lean on are asserted before anything is written; a seed that misses one is refused.
Import shims as in make_ssd.py."""
import contextlib
import importlib.machinery
import io
import json
import math
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
from oracle.reference_import import calibrate, find_reference, load, quantize_reference_graph  # noqa: E402

assert find_reference() is not None, 'the reference is not importable here'
load()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppq import BaseGraph  # noqa: E402
from ppq.core import PPQ_CONFIG, NetworkFramework  # noqa: E402
import ppq.quantization.analyse.graphwise as ref_graphwise  # noqa: E402
import ppq.quantization.analyse.layerwise as ref_layerwise  # noqa: E402

assert PPQ_CONFIG.USING_CUDA_KERNEL is False
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import statistics_cases as C  # noqa: E402


def reference_graph(parameters: dict):
    """The case built with the reference's own graph API."""
    g = BaseGraph(name='statistics_case', built_from=NetworkFramework.ONNX)
    made = {'input': g.create_variable(name='input')}
    for kind, name, inputs, a in C.OPS:
        ins, attrs = [made[n] for n in inputs], {}
        if kind == 'Conv':
            pad = a['k'] // 2
            attrs = {'kernel_shape': [a['k'], a['k']], 'strides': [1, 1], 'pads': [pad] * 4, 'dilations': [1, 1], 'group': 1}
            ins.append(g.create_variable(name=name + '_w', value=parameters[name + '_w'].clone(), is_parameter=True))
            ins.append(g.create_variable(name=name + '_b', value=parameters[name + '_b'].clone(), is_parameter=True))
        elif kind == 'MaxPool': attrs = {'kernel_shape': [a['k'], a['k']], 'strides': [a['k'], a['k']], 'pads': [0] * 4}
        made[name + '_out'] = g.create_variable(name=name + '_out')
        g.create_operation(op_type=kind, name=name, attributes=attrs, inputs=ins, outputs=[made[name + '_out']])
    g.mark_variable_as_graph_input(made['input'])
    for n in C.OUTPUTS: g.mark_variable_as_graph_output(made[n])
    return g


def run_reference():
    batches = C.case_batches()
    g, ex = quantize_reference_graph(reference_graph(C.case_parameters()), 'cpu', batches[0], bins=C.HIST_BINS, method='kl')
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        calibrate(g, ex, batches, method='kl')
    fetched, inner = [], ref_graphwise.tensor_random_fetch

    def capturing(*a, **kw):
        value = inner(*a, **kw)
        fetched.append(value.detach().clone().cpu())
        return value
    ref_graphwise.tensor_random_fetch = capturing
    try:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            records = ref_graphwise.statistical_analyse(g, 'cpu', batches, steps=C.STEPS)
    finally:
        ref_graphwise.tensor_random_fetch = inner
    # parameter_analyse: the printout, and the three dictionaries its MeasurePrinters are handed
    handed, printer = [], ref_layerwise.MeasurePrinter

    def spying(data, *a, **kw):
        handed.append((kw.get('measure'), dict(data)))
        return printer(data, *a, **kw)
    ref_layerwise.MeasurePrinter = spying
    text = io.StringIO()
    try:
        with contextlib.redirect_stdout(text): ref_layerwise.parameter_analyse(g)
    finally:
        ref_layerwise.MeasurePrinter = printer
    return records, fetched, text.getvalue(), handed


def main():
    records, fetched, text, handed = run_reference()
    V, B = len(records), C.BATCHES
    assert list(records[0]) == C.KEYS, list(records[0])
    assert len(fetched) == 2 * B * V, (len(fetched), V)      # the fetch order within a forward is the record order
    out, book = {}, {'keys': C.KEYS, 'records': [], 'seed': C.SEED}
    ref_scalars, ref_hist, ref_snr = np.zeros([V, 3, 6]), np.zeros([V, 3, C.BINS]), np.zeros(V)
    f64_scalars, f64_snr = np.zeros([V, 3, 6]), np.zeros(V)
    deviation = {'Mean relative': 0.0, 'Std relative': 0.0, 'Skewness absolute': 0.0, 'Kurtosis absolute': 0.0, 'Snr relative': 0.0}
    constant_noise = edges_on_quantized = 0
    for k, rec in enumerate(records):
        fp = torch.cat([fetched[b * V + k] for b in range(B)]).numpy()
        qt = torch.cat([fetched[(B + b) * V + k] for b in range(B)]).numpy()
        assert fp.dtype == np.float32 and fp.shape == qt.shape == (B * C.FETCHS,)
        out[f'fp_{k}'], out[f'qt_{k}'] = fp, qt
        series = {'Noise': C.noise_of(qt, fp), 'Quantized': qt, 'Float': fp}
        entry = {key: rec[key] for key in C.KEYS[:6]}
        entry['edges'] = {}
        for s, kind in enumerate(C.KINDS):
            x = series[kind]
            f64 = C.float64_series(x)
            assert float(x.min()) == rec[f'{kind} Min'] and float(x.max()) == rec[f'{kind} Max'], (k, kind)   # the captured series ARE the reference's
            assert sum(rec[f'{kind} Hist']) == x.size, (k, kind)
            ref_hist[k, s] = rec[f'{kind} Hist']
            for i, field in enumerate(C.SCALARS):
                ref_scalars[k, s, i], f64_scalars[k, s, i] = rec[f'{kind} {field}'], f64[field]
            constant = bool(x.min() == x.max())
            edges = C.edge_samples(x)
            entry['edges'][kind] = edges
            entry.setdefault('constant', {})[kind] = constant
            if constant:
                assert math.isnan(rec[f'{kind} Skewness']) and math.isnan(rec[f'{kind} Kurtosis']), (k, kind)
                assert max(rec[f'{kind} Hist']) == x.size, (k, kind)                                       # all n samples in one bin
                constant_noise += int(kind == 'Noise')
                continue
            assert edges <= C.EDGE_CAP * x.size, f'record {k} {kind}: {edges} of {x.size} samples sit on a bin edge: give the case another seed'
            edges_on_quantized += int(kind == 'Quantized' and edges > 0)
            deviation['Mean relative'] = max(deviation['Mean relative'], abs(rec[f'{kind} Mean'] - f64['Mean']) / max(abs(f64['Mean']), 1e-30))
            deviation['Std relative'] = max(deviation['Std relative'], abs(rec[f'{kind} Std'] - f64['Std']) / f64['Std'])
            deviation['Skewness absolute'] = max(deviation['Skewness absolute'], abs(rec[f'{kind} Skewness'] - f64['Skewness']))
            deviation['Kurtosis absolute'] = max(deviation['Kurtosis absolute'], abs(rec[f'{kind} Kurtosis'] - f64['Kurtosis']))
        ref_snr[k], f64_snr[k] = rec['Noise:Signal Power Ratio'], C.float64_snr(qt, fp)
        if f64_snr[k] > 0: deviation['Snr relative'] = max(deviation['Snr relative'], abs(ref_snr[k] - f64_snr[k]) / f64_snr[k])
        book['records'].append(entry)
    # ---- the conditions the tests lean on
    assert constant_noise >= 1, 'no record has a constant noise series: give the case another seed'
    assert edges_on_quantized >= 1, 'no quantised series has a sample on a bin edge: give the case another seed'
    assert [m for m, _ in handed] == ['Value Range', 'Value Std', 'Value Mean(Abs)']
    book['deviation'] = deviation
    book['parameter_analyse'] = {'text': text, 'values': {m: d for m, d in handed}}
    out.update(ref_scalars=ref_scalars, ref_hist=ref_hist, ref_snr=ref_snr, f64_scalars=f64_scalars, f64_snr=f64_snr)
    path = os.path.join(HERE, 'statistics.npz')
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, 'statistics.json'), 'w') as f: json.dump(book, f, indent=1, sort_keys=True)
    worst = max((e['edges'][kind], e['Variable name']) for e in book['records'] for kind in C.KINDS if not e['constant'][kind])
    print(f'{V} records, {constant_noise} constant noise series, {edges_on_quantized} quantised series with edge samples, '
          f'most edge samples of a series that is not constant {worst[0]} of {B * C.FETCHS} ({worst[1]})')
    print('largest deviation of the reference from float64:', {k: float(f'{v:.3g}') for k, v in deviation.items()})
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
