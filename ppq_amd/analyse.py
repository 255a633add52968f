"""Quantization error analysis: what did quantising (and every pass after it) do to the network?

Counterpart of ``ppq/quantization/analyse/`` -- ``graphwise_error_analyse`` (graphwise.py:63-177), ``layerwise_error_analyse``
(layerwise.py:14-133), ``MeasureRecorder`` / ``MeasurePrinter`` (util) -- and of the seeded sample fetch of
``ppq/utils/fetch.py`` on this package's graphs and ``TorchExecutor`` (harness.py).  Names, argument order and defaults
are the reference's.

What differs is where the numbers are made.  The reference copies 4096 samples of every analysed output to the CPU after
every forward (one synchronising copy per operation and batch) and computes the measure there in fp32.  Here the FP32
samples of phase 1 stay in device memory, phase 2 reads the quantised outputs THROUGH the index table while it measures them
against those samples, every analysed output of a forward shares one launch (``csrc/measure.hip``), the sums are
accumulated in double, and ONE copy at the very end brings the per-operation results to the host.
``fetchs=None`` measures whole tensors instead of samples.  ``use_kernels=False`` runs the reference's procedure itself
(torch ``index_select``, a copy per operation, the measure on the CPU): the comparison arm, and the path of a CPU executor.

``statistical_analyse``, ``parameter_analyse`` and ``variable_analyse`` live in ``ppq_amd/statistics.py`` and are re-exported at
the end of this module.
"""
import math
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Union

import numpy as np
import torch

from . import measure as M
from .harness import COMPUTING_OP, BaseGraph, QuantableOperation, TorchExecutor, plan_epilogues

FETCH_SEED = 10086                                 # analyse/graphwise.py:27
_METHOD_TITLES = {'snr': 'NOISE:SIGNAL POWER RATIO', 'cosine': 'COSINE SIMILARITY', 'mse': 'MSE LOSS(UNSCALED)'}

# what the last analysis of this process issued: forwards, launches of each kernel entry point, device-to-host copies
last_analysis_stats: Dict[str, int] = {}


# ---- seeded sampling (utils/fetch.py) -------------------------------------------------------------------------------
_SEED_CHAINS: Dict[tuple, np.ndarray] = {}
_DEVICE_TABLES: Dict[tuple, torch.Tensor] = {}


def _seed_chain(num_of_fetches: int, seed: int) -> np.ndarray:
    """seed_0 = seed, seed_{i+1} = (0x343FD * seed_i + 0x269EC3) mod 2^32 (fetch.py:21-23): independent of the tensor."""
    key = (num_of_fetches, seed)
    chain = _SEED_CHAINS.get(key)
    if chain is None:
        values, s = [], int(seed)
        for _ in range(num_of_fetches):
            values.append(s)
            s = (0x343FD * s + 0x269EC3) % (1 << 32)
        chain = np.array(values, dtype=object if seed >= (1 << 63) or seed < 0 else np.uint64)
        if len(_SEED_CHAINS) >= 16: _SEED_CHAINS.pop(next(iter(_SEED_CHAINS)))
        _SEED_CHAINS[key] = chain
    return chain


def generate_indexer(num_of_fetches: int, num_of_elements: int, seed: int = 0x20211230) -> torch.Tensor:
    """utils/fetch.py:4-24: ``num_of_fetches`` indices below ``num_of_elements``, WITH repetition, as an int32 CPU tensor."""
    if num_of_elements <= 0: raise ValueError('Can not fetch data from empty tensor(0 element).')
    index = (_seed_chain(num_of_fetches, seed) % num_of_elements).astype(np.int64)
    return torch.from_numpy(index).to(torch.int32)


def device_indexer(num_of_fetches: int, num_of_elements: int, seed: int, device) -> torch.Tensor:
    """The table of ``generate_indexer`` on ``device``, made once per (fetches, elements, seed, device) and kept."""
    key = (num_of_fetches, num_of_elements, seed, str(device))
    table = _DEVICE_TABLES.get(key)
    if table is None:
        table = generate_indexer(num_of_fetches, num_of_elements, seed).to(device)
        if len(_DEVICE_TABLES) >= 256: _DEVICE_TABLES.pop(next(iter(_DEVICE_TABLES)))
        _DEVICE_TABLES[key] = table
    return table


def batch_random_fetch(tensor: torch.Tensor, fetches_per_batch: int = 1024, seed: int = None) -> torch.Tensor:
    """utils/fetch.py:98-122, seeded form: ``[batch, fetches_per_batch]`` samples of every batch element, the same positions
    in each.  float32 GPU tensors go through ``ppqhip_fetch_rows_multi``, everything else through ``index_select``."""
    if seed is None: raise ValueError('batch_random_fetch needs a seed here (the unseeded torch.randint form is not provided).')
    rows = tensor.flatten(start_dim=1)
    if rows.shape[-1] <= 0: raise ValueError('Can not fetch data from empty tensor(0 element).')
    if rows.is_cuda and rows.dtype is torch.float32:
        from . import ffi
        return ffi.fetch_rows_multi([(rows.contiguous(), device_indexer(fetches_per_batch, rows.shape[-1], seed, rows.device))])[0]
    index = generate_indexer(fetches_per_batch, rows.shape[-1], seed)
    return rows.index_select(dim=-1, index=index.to(rows.device).long())


# ---- recorder / printer (analyse/util) ------------------------------------------------------------------------------
class MeasureRecorder:
    """Running measure over batches: the batch-size weighted mean, or the maximum, of the per-batch result.

    float32 GPU tensors accumulate ON THE DEVICE (two launches per update, nothing comes back); reading ``measure`` is the
    one synchronising copy.  CPU tensors -- and every tensor when ``use_kernels`` is off -- follow the reference's
    Python running mean literally, one ``.item()`` per update.  A recorder keeps to one of the two."""
    def __init__(self, measurement: str = 'cosine', reduce: str = 'mean', use_kernels: bool = True) -> None:
        if reduce not in {'mean', 'max'}:
            raise ValueError(f'MeasureRecorder reduces by mean or max, {reduce} was given.')
        self.method = str(measurement).lower()
        if self.method not in {'cosine', 'mse', 'snr'}:
            raise ValueError(f'MeasureRecorder measures mse, snr or cosine, {measurement} was given.')
        self.reduce = reduce
        self.use_kernels = use_kernels
        self.num_of_elements = 0
        self.device_reads = 0                      # device-to-host copies this recorder made
        self._measure = 0
        self._acc: Optional[torch.Tensor] = None   # float64 [2] on the device: numerator (or maximum), rows
        self._sums: Dict[int, torch.Tensor] = {}
        self._stale = False

    def bind(self, acc: torch.Tensor) -> 'MeasureRecorder':
        """Accumulate into ``acc`` (zeroed float64 [2] on the device, e.g. one row of a bank shared by many recorders)."""
        self._acc = acc
        return self

    def load(self, host_acc) -> None:
        """Take the state from a host copy of the accumulator (the owner of a shared bank copies it once for all)."""
        numerator, rows = float(host_acc[0]), float(host_acc[1])
        self.num_of_elements = int(rows)
        if self.reduce == 'mean': self._measure = numerator / rows if rows > 0 else 0
        else: self._measure = numerator
        self._stale = False

    def _on_device(self, y_pred: torch.Tensor, y_real: torch.Tensor) -> bool:
        return self.use_kernels and y_pred.ndim > 1 and M.kernel_path(y_pred, y_real)

    def update(self, y_pred: torch.Tensor, y_real: torch.Tensor):
        elements = y_pred.shape[0]
        if elements != y_real.shape[0]:
            raise Exception('Can not update measurement, cause your input data do not share a same batchsize. '
                            f'Shape of y_pred {y_pred.shape} - against shape of y_real {y_real.shape}')
        if y_pred.shape != y_real.shape:
            raise ValueError(f'Can not measure tensors of different shapes ({y_pred.shape} and {y_real.shape}).')
        if self._on_device(y_pred, y_real):
            from . import ffi
            if self._acc is None:
                if self.num_of_elements: raise RuntimeError('this MeasureRecorder has been accumulating on the host')
                self._acc = torch.zeros(2, dtype=torch.float64, device=y_pred.device)
            sums = self._sums.get(elements)
            if sums is None or sums.device != y_pred.device:
                sums = self._sums[elements] = torch.empty([elements, 4], dtype=torch.float64, device=y_pred.device)
            ffi.measure_rows_multi([(y_pred, y_real, None)], [sums])
            ffi.measure_finish_multi([(sums, y_pred.numel() // elements, self._acc, None)], self.method, self.reduce)
            self._stale = True
            return
        if self._acc is not None:
            raise RuntimeError('this MeasureRecorder accumulates on the device: it takes contiguous float32 GPU tensors with a '
                               'batch dimension only (use_kernels=False measures anything with torch)')
        if y_pred.ndim == 1: y_pred, y_real = y_pred.unsqueeze(0), y_real.unsqueeze(0)
        if self.reduce == 'mean':
            result = M.reference_formula(self.method, y_pred, y_real, 'mean').item()
            self._measure = self._measure * self.num_of_elements + result * elements
            self.num_of_elements += elements
            self._measure /= self.num_of_elements
        else:
            result = M.reference_formula(self.method, y_pred, y_real, 'none').max().item()
            self._measure = max(self._measure, result)
            self.num_of_elements += elements
        if y_pred.is_cuda: self.device_reads += 1

    @ property
    def measure(self):
        if self._stale:
            self.device_reads += 1
            self.load(self._acc.cpu())
        return self._measure


class MeasurePrinter:
    """The bar chart of analyse/util: one line per entry, the bar scaled between the smallest and the largest value."""
    def __init__(self, data: Dict[str, float], measure: str, label: str = 'Layer', k: int = None,
                 order: str = 'large_to_small', percentage: bool = False) -> None:
        if order not in {'large_to_small', 'small_to_large', None}:
            raise ValueError('Parameter "order" can only be "large_to_small" or "small_to_large"')
        entries = list(data.items())
        if order is not None:
            entries = sorted(entries, key=lambda e: e[1])
            if order == 'large_to_small': entries = entries[::-1]
        if k is not None: entries = entries[:k]
        self.collection = entries
        if order is None:
            by_value = sorted(entries, key=lambda e: e[1])
            largest, smallest = by_value[-1][1], by_value[0][1]
        elif order == 'large_to_small': largest, smallest = entries[0][1], entries[-1][1]
        else: largest, smallest = entries[-1][1], entries[0][1]
        self.normalized_by = largest - smallest
        self.min = smallest
        self.max_name_length = max([len(label)] + [len(name) for name, _ in entries])
        self.measure_str, self.label, self.percentage = measure, label, percentage

    def print(self, max_blocks: int = 20):
        width = self.max_name_length
        print(f'{self.label}{" " * (width - len(self.label))}  | {self.measure_str} ')
        for name, value in self.collection:
            share = (value - self.min) / (self.normalized_by + 1e-7)
            if math.isnan(value):
                print('\033[31m[Warning] MeasurePrinter found an NaN value in your data.\033[0m')
                share = 0
            blocks = round(share * max_blocks)
            shown = f'{value * 100:.3f}%' if self.percentage else f'{value:.4f}'
            print(f'{name}:{" " * (width - len(name))} | {"█" * blocks}{" " * (max_blocks - blocks)} | {shown}')


def _report(results: Dict[str, float], method: str) -> None:
    MeasurePrinter(results, order='large_to_small', measure=_METHOD_TITLES.get(method, 'MEASUREMENT'),
                   percentage=method in {'snr', 'cosine'}).print()


# ---- the analyses ---------------------------------------------------------------------------------------------------
class OutputKeeper:
    """Runtime hook that keeps the first output of its operation AFTER the output quantisation (``quant_outputs[0]``: what
    the reference's plain RuntimeHook receives, executor/torch.py:541-552) until ``pop``.

    Not a plain ``CalibrationHook``, so ``plan_epilogues`` (rule 4) leaves the operation out of every fused epilogue group and
    nothing writes the kept tensor afterwards; ``clone`` is for an operation whose output a later launch does write in place."""
    def __init__(self, operation, clone: bool = False) -> None:
        self._hook_to = operation
        self.clone = clone
        self.kept: Optional[torch.Tensor] = None

    def pre_forward_hook(self, inputs: list, quant_inputs: list, quant_configs: list) -> list:
        return quant_inputs

    def post_forward_hook(self, outputs: list, quant_outputs: list, quant_configs: list) -> list:
        value = quant_outputs[0]
        assert isinstance(value, torch.Tensor), 'Output of monitoring operation is not a torch.Tensor'
        self.kept = value.clone() if self.clone else value
        return quant_outputs

    def pop(self) -> torch.Tensor:
        value, self.kept = self.kept, None
        return value


def _quantable(graph: BaseGraph) -> List[QuantableOperation]:
    return [op for op in graph.operations.values() if isinstance(op, QuantableOperation)]


def _written_in_place(graph: BaseGraph, hooks: Dict[str, object]) -> set:
    """Operations whose outputs a fused epilogue launch would write in place under these hooks and the current states."""
    groups = plan_epilogues(graph.topological_sort(), hooks, set(graph.outputs))
    return {op.name for grp in groups for op in grp.ops}


def _rows(value: torch.Tensor) -> torch.Tensor:
    """[batch, rest] in the logical (NCHW) order the reference's flatten gives; a copy only for a permuted layout."""
    return value.contiguous().flatten(start_dim=1)


def _batches(dataloader: Iterable, collate_fn: Optional[Callable], steps: int):
    """The reference's loop header: batches 0 .. steps INCLUSIVE (`if idx >= steps: break` comes after the work)."""
    for idx, batch in enumerate(dataloader):
        yield idx, (collate_fn(batch) if collate_fn is not None else batch)
        if idx >= steps: break


@ torch.no_grad()
def graphwise_error_analyse(graph: BaseGraph, running_device: str, dataloader: Iterator, collate_fn: Callable = None,
                            method: str = 'snr', steps: int = 8, verbose: bool = True, fetchs: Optional[int] = 4096, *,
                            executor: TorchExecutor = None, use_kernels: bool = True) -> Dict[str, float]:
    """analyse/graphwise.py:63-177: the difference between the quantised graph and its dequantised self at the (first) output
    of every quantable computing operation, accumulated from the graph's input on: ``{operation name: measure}``.

    Phase 1 runs ``steps + 1`` batches with every operation dequantised and keeps ``fetchs`` seeded samples per batch element
    of every analysed output; phase 2 runs the same batches quantised and measures the same positions against them.
    ``fetchs=None`` (not in the reference) measures WHOLE tensors; the two phases are then interleaved per batch, so that one
    batch of activations is held at a time and the dataloader is walked once.  ``executor``: use this one instead of building
    one on ``running_device``.  ``use_kernels=False``: the reference's procedure with torch operations (module docstring).
    Every operation's quantisation state is put back, also when a forward raises."""
    if executor is None: executor = TorchExecutor(graph=graph, device=running_device)
    interested = [op for op in _quantable(graph) if op.type in COMPUTING_OP]
    if not interested:
        print('Nothing to analyse: the graph has no quantable computing operation.')
        return {}
    for op in interested:
        if len(op.outputs) > 1:
            print(f'\033[31m[Warning] Operation {op.name} has more than 1 output, the first one is analysed.\033[0m')
    quantable = _quantable(graph)
    hooks = {op.name: OutputKeeper(op) for op in interested}
    recorders = {op.name: MeasureRecorder(measurement=method, use_kernels=use_kernels) for op in interested}
    stats = {'forwards': 0, 'fetch_launches': 0, 'measure_launches': 0, 'finish_launches': 0, 'device_reads': 0}

    def set_states(quantised: bool) -> None:
        for op in quantable: op.restore_quantize_state() if quantised else op.dequantize()
        risky = _written_in_place(graph, hooks)
        for name, hook in hooks.items(): hook.clone = name in risky

    def forward(batch) -> List[torch.Tensor]:
        executor.forward(inputs=batch, hooks=hooks)
        stats['forwards'] += 1
        return [_rows(hooks[op.name].pop()) for op in interested]

    bank = None
    if use_kernels:
        from . import ffi
        device = torch.device(executor._device)
        bank = torch.zeros([len(interested), 2], dtype=torch.float64, device=device)
        for k, op in enumerate(interested): recorders[op.name].bind(bank[k])
        sums: Dict[int, List[torch.Tensor]] = {}

        def measure(preds, reals, tables):
            rows = preds[0].shape[0]
            if rows not in sums: sums[rows] = [torch.empty([rows, 4], dtype=torch.float64, device=device) for _ in interested]
            ffi.measure_rows_multi(list(zip(preds, reals, tables)), sums[rows])
            ffi.measure_finish_multi([(s, r.shape[1], bank[k], None) for k, (s, r) in enumerate(zip(sums[rows], reals))], method)
            stats['measure_launches'] += 1; stats['finish_launches'] += 1

        def tables_of(values):
            return [device_indexer(fetchs, v.shape[1], FETCH_SEED, v.device) for v in values]
    else:
        def sample(value):                       # OutputRecorder.post_forward_hook, graphwise.py:23-32
            stats['device_reads'] += int(value.is_cuda)
            if fetchs is None: return value.to('cpu')
            index = generate_indexer(fetchs, value.shape[-1], FETCH_SEED)
            return value.index_select(dim=-1, index=index.to(value.device).long()).to('cpu')

    try:
        if fetchs is None:
            for idx, batch in _batches(dataloader, collate_fn, steps):
                set_states(False)
                reals = forward(batch)
                if not use_kernels: reals = [sample(v) for v in reals]
                set_states(True)
                preds = forward(batch)
                if use_kernels: measure(preds, reals, [None] * len(preds))
                else:
                    for op, p, r in zip(interested, preds, reals): recorders[op.name].update(y_pred=sample(p), y_real=r)
        else:
            caches: List[List[torch.Tensor]] = []
            set_states(False)
            for idx, batch in _batches(dataloader, collate_fn, steps):
                values = forward(batch)
                if use_kernels:
                    caches.append(ffi.fetch_rows_multi(list(zip(values, tables_of(values)))))
                    stats['fetch_launches'] += 1
                else: caches.append([sample(v) for v in values])
            set_states(True)
            for idx, batch in _batches(dataloader, collate_fn, steps):
                values = forward(batch)
                if use_kernels: measure(values, caches[idx], tables_of(values))
                else:
                    for op, p, r in zip(interested, values, caches[idx]): recorders[op.name].update(y_pred=sample(p), y_real=r)
    finally:
        for op in quantable: op.restore_quantize_state()
        for hook in hooks.values(): hook.kept = None

    if bank is not None:
        host = bank.cpu()                         # the one device-to-host copy of the analysis
        stats['device_reads'] += 1
        for k, op in enumerate(interested): recorders[op.name].load(host[k])
    results = {op.name: recorders[op.name].measure for op in interested}
    last_analysis_stats.clear(); last_analysis_stats.update(stats)
    if verbose: _report(results, method)
    return results


@ torch.no_grad()
def layerwise_error_analyse(graph: BaseGraph, dataloader: Iterator, interested_outputs: Union[str, List[str]] = None,
                            collate_fn: Callable = None, running_device: str = 'cuda', method: str = 'snr', steps: int = 8,
                            verbose: bool = True, *, executor: TorchExecutor = None, use_kernels: bool = True) -> Dict[str, float]:
    """analyse/layerwise.py:14-133: ONE quantable computing operation quantised at a time, everything else dequantised; the
    measure is taken on the whole ``interested_outputs`` (default: the graph's outputs): ``{operation name: measure}``.

    The FP32 outputs of a batch do not depend on the operation under test: they are computed once per batch and kept (the
    reference recomputes them for every operation).  The first ``steps + 1`` batches are used.  Every operation's
    quantisation state is put back at the end, also when a forward raises."""
    if interested_outputs is None: interested_outputs = list(graph.outputs)
    if isinstance(interested_outputs, str): interested_outputs = [interested_outputs]
    if executor is None: executor = TorchExecutor(graph=graph, device=running_device)
    quantable = _quantable(graph)
    under_test = [op for op in quantable if op.type in COMPUTING_OP]
    recorders = {op.name: MeasureRecorder(measurement=method, use_kernels=use_kernels) for op in under_test}
    bank = None
    if use_kernels and under_test:
        bank = torch.zeros([len(under_test), 2], dtype=torch.float64, device=torch.device(executor._device))
        for k, op in enumerate(under_test): recorders[op.name].bind(bank[k])
    stats = {'forwards': 0, 'fetch_launches': 0, 'measure_launches': 0, 'finish_launches': 0, 'device_reads': 0}
    try:
        for op in quantable: op.dequantize()
        batches, fp_outputs = [], []
        for idx, batch in _batches(dataloader, collate_fn, steps):
            batches.append(batch)
            fp_outputs.append([y.contiguous() for y in executor.forward(inputs=batch, output_names=interested_outputs)])
            stats['forwards'] += 1
        for op in under_test:
            recorder = recorders[op.name]
            op.restore_quantize_state()
            for batch, fp in zip(batches, fp_outputs):
                qt = executor.forward(inputs=batch, output_names=interested_outputs)
                stats['forwards'] += 1
                for fp_output, qt_output in zip(fp, qt):
                    recorder.update(y_pred=qt_output.contiguous(), y_real=fp_output)
                    stats['measure_launches'] += int(use_kernels); stats['finish_launches'] += int(use_kernels)
            op.dequantize()
    finally:
        for op in quantable: op.restore_quantize_state()
    if bank is not None:
        host = bank.cpu()
        stats['device_reads'] += 1
        for k, op in enumerate(under_test): recorders[op.name].load(host[k])
    results = {op.name: recorders[op.name].measure for op in under_test}
    stats['device_reads'] += sum(r.device_reads for r in recorders.values())
    last_analysis_stats.clear(); last_analysis_stats.update(stats)
    if verbose and results: _report(results, method)
    return results


# ---- the statistical reports (ppq/quantization/analyse: statistical_analyse, parameter_analyse, variable_analyse) ------------
from .statistics import (collect_samples, parameter_analyse, series_statistics, statistical_analyse,  # noqa: E402,F401
                         variable_analyse)
