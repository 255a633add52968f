"""Record the REFERENCE's analysis helpers (ppq/utils/fetch.py, ppq/quantization/measure, ppq/quantization/analyse/util) on the
CPU for the cases of analyse_cases.py.

Run where the reference is importable (oracle/reference_import.find_reference); no test imports it:

    python tests/golden/make_analyse.py

Writes tests/golden/analyse.npz: the reference's index tables, its three measures x three reductions per case, the
``MeasureRecorder.measure`` after every update of the recorded sequence, and the text ``MeasurePrinter`` prints.
Import shims as in make_golden.py."""
import contextlib
import importlib.machinery
import io
import os
import sys
from unittest.mock import MagicMock

os.environ['PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION'] = 'python'
sys.dont_write_bytecode = True
for _name in ['onnx', 'onnx.helper', 'onnx.numpy_helper', 'onnx.mapping', 'onnx.onnx_pb', 'onnx.checker',
              'onnx.external_data_helper', 'onnx.shape_inference', 'onnx.version_converter']:
    _m = MagicMock(); _m.__spec__ = importlib.machinery.ModuleSpec(_name, None); _m.__path__ = []
    sys.modules[_name] = _m
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle.reference_import import find_reference  # noqa: E402

assert find_reference() is not None, 'the reference is not importable here'
sys.path.insert(0, find_reference())

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppq.quantization.analyse.util import MeasurePrinter, MeasureRecorder  # noqa: E402
from ppq.quantization.measure.cosine import torch_cosine_similarity  # noqa: E402
from ppq.quantization.measure.norm import torch_mean_square_error, torch_snr_error  # noqa: E402
from ppq.utils.fetch import batch_random_fetch, generate_indexer  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from analyse_cases import (INDEXER_CASES, MEASURE_CASES, METHODS, PRINTER_CASES, RECORDER_BATCHES, REDUCTIONS,  # noqa: E402
                           measure_tensors, recorder_tensors)

FN = {'snr': torch_snr_error, 'mse': torch_mean_square_error, 'cosine': torch_cosine_similarity}


def main():
    out = {}
    for k, (fetches, elements, seed) in enumerate(INDEXER_CASES):
        out[f'indexer_{k}'] = generate_indexer(fetches, elements, seed).numpy()
    out['fetch_four_dim'] = batch_random_fetch(measure_tensors(6)[1], fetches_per_batch=50, seed=10086).numpy()
    for k, (name, _) in enumerate(MEASURE_CASES):
        pred, real = measure_tensors(k)
        for method in METHODS:
            for reduction in REDUCTIONS:
                out[f'measure_{name}_{method}_{reduction}'] = FN[method](pred, real, reduction).numpy()
    zero = torch.zeros(2, 64)
    for method in METHODS: out[f'measure_zero_{method}_none'] = FN[method](zero, zero, 'none').numpy()
    for method in METHODS:
        rec = MeasureRecorder(measurement=method)
        trace = []
        for i in range(len(RECORDER_BATCHES)):
            pred, real = recorder_tensors(i)
            rec.update(y_pred=pred, y_real=real)
            trace.append(rec.measure)
            out[f'recorder_{method}_rows_{i}'] = FN[method](pred, real, 'none').numpy()
        out[f'recorder_{method}_mean'] = np.array(trace, np.float64)
        # reduce='max' is accepted by the reference's constructor and then fails in update (its measures know no 'max')
        rec = MeasureRecorder(measurement=method, reduce='max')
        try:
            rec.update(*recorder_tensors(0)); raised = 0
        except ValueError: raised = 1
        out[f'recorder_{method}_max_raises'] = np.array(raised)
    for name, data, kwargs in PRINTER_CASES:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf): MeasurePrinter(data, **kwargs).print()
        out[f'printer_{name}'] = np.array(buf.getvalue())
    path = os.path.join(HERE, 'analyse.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
