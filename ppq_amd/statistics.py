"""Statistical reports: what do the values of a quantised network look like, variable by variable?

Counterpart of ``statistical_analyse`` (ppq/quantization/analyse/graphwise.py:186-372), ``parameter_analyse`` and
``variable_analyse`` (analyse/layerwise.py:137-203) on this package's graphs and ``TorchExecutor``; the names are re-exported
from ``ppq_amd.analyse`` next to the two error analyses.  Names, argument order, defaults, record keys and their order are the
reference's.

The reference copies 1024 samples of every input and output of every analysed operation to the CPU in every forward (one
``index_select`` and one synchronising copy per tensor) and then makes each of the 24 numbers of a record with its own small
torch call and ``.item()``.  Here the hook keeps references, ONE fetch launch after a forward gathers the samples of every kept
tensor into device buffers (``ppqhip_fetch_rows_multi``), TWO calls make the statistics of all 3 x V series
(``csrc/stats.hip``: moments, then skewness / kurtosis / histogram from those moments without a host round trip) and ONE copy
brings the packed table back.  ``use_kernels=False`` is the reference's procedure restated with torch: the comparison arm, and
the only path of a CPU executor.
"""
from typing import Callable, Dict, Iterable, Iterator, List, Optional, Tuple, Union

import torch

from . import measure as M
from .harness import PASSIVE_OPERATIONS, BaseGraph, Operation, QuantableOperation, TorchExecutor, Variable

STAT_FETCHS = 1024                                 # DetailedRecorder, analyse/graphwise.py:40-41
KINDS = ('Noise', 'Quantized', 'Float')
FIELDS = ('Mean', 'Std', 'Skewness', 'Kurtosis', 'Hist', 'Max', 'Min')
Pair = Tuple[Operation, Variable, torch.Tensor, torch.Tensor]


def _analyse():
    from . import analyse                          # (analyse re-exports this module's names: imported where it is used)
    return analyse


class DetailedKeeper:
    """Runtime hook that keeps what the reference's DetailedRecorder samples: the inputs its operation is run with
    (``quant_inputs``, parameters included) and its outputs after the output quantisation, until ``pop``.  Not a plain
    ``CalibrationHook``: ``plan_epilogues`` leaves its operation out of every fused epilogue group."""
    def __init__(self, operation: Operation, sample: Callable = None) -> None:
        self._hook_to = operation
        self.sample = sample                       # torch arm: applied to every tensor as it is seen
        self.clone_inputs: List[bool] = [False] * len(operation.inputs)
        self.clone_outputs = False
        self.kept: List[torch.Tensor] = []

    def _keep(self, values: list, clone: List[bool]) -> None:
        for value, c in zip(values, clone):
            assert isinstance(value, torch.Tensor), f'A value of monitoring operation {self._hook_to.name} is not a torch.Tensor'
            if self.sample is not None: value = self.sample(value)
            elif c: value = value.clone()
            self.kept.append(value)

    def pre_forward_hook(self, inputs: list, quant_inputs: list, quant_configs: list) -> list:
        self.kept = []
        self._keep(quant_inputs, self.clone_inputs)
        return quant_inputs

    def post_forward_hook(self, outputs: list, quant_outputs: list, quant_configs: list) -> list:
        self._keep(quant_outputs, [self.clone_outputs] * len(quant_outputs))
        return quant_outputs

    def pop(self) -> List[torch.Tensor]:
        values, self.kept = self.kept, []
        return values


def _interested(graph: BaseGraph) -> List[QuantableOperation]:
    return [op for op in graph.operations.values() if isinstance(op, QuantableOperation) and op.type not in PASSIVE_OPERATIONS]


@ torch.no_grad()
def collect_samples(graph: BaseGraph, running_device: str, dataloader: Iterator, collate_fn: Callable = None, steps: int = 8, *,
                    executor: TorchExecutor = None, use_kernels: bool = True, fetchs: int = STAT_FETCHS) -> List[Pair]:
    """The sampling half of ``statistical_analyse``: ``[(operation, variable, x_fp, x_qt)]``, one entry per input and then per
    output of every quantable operation that is not passive, in ``graph.operations`` order.  ``x_fp`` / ``x_qt``: the
    ``batches * fetchs`` seeded samples (``tensor_random_fetch(seed=10086)`` over the flattened tensor) of the variable in
    the dequantised and in the quantised run of batches 0 .. ``steps`` inclusive.  Parameters are sampled at every batch like
    everything else, so their samples repeat (the count enters the standard deviation).

    Kernel arm: 1-D views of device buffers, filled by one fetch launch per forward.  ``use_kernels=False``: CPU tensors, each
    tensor sampled with ``index_select`` and copied as the hook sees it.  The two arms hold the same bits."""
    A = _analyse()
    if executor is None: executor = TorchExecutor(graph=graph, device=running_device)
    interested = _interested(graph)
    stats = {'forwards': 0, 'fetch_launches': 0, 'stat_launches': 0, 'device_reads': 0}
    A.last_analysis_stats.clear(); A.last_analysis_stats.update(stats)
    if not interested:
        print('Oops. you got nothing to analyse.')
        return []
    quantable = A._quantable(graph)
    slots = [(op, var) for op in interested for var in list(op.inputs) + list(op.outputs)]

    def sample(value: torch.Tensor) -> torch.Tensor:          # DetailedRecorder, graphwise.py:47-57
        stats['device_reads'] += int(value.is_cuda)
        flat = value.flatten()
        index = A.generate_indexer(fetchs, flat.numel(), A.FETCH_SEED)
        return flat.index_select(dim=0, index=index.to(flat.device).long()).to('cpu')

    hooks = {op.name: DetailedKeeper(op, None if use_kernels else sample) for op in interested}
    buffers = None
    if use_kernels:
        from . import ffi
        device = torch.device(executor._device)
        if device.type != 'cuda':
            raise RuntimeError(ffi._KERNEL_FAILURE + 'statistical_analyse: the executor is not on the GPU (ppq_amd has no CPU path; '
                               'use_kernels=False runs the reference\'s procedure with torch)')
        buffers = torch.empty([2, len(slots), steps + 1, fetchs], dtype=torch.float32, device=device)
    kept: List[List[List[torch.Tensor]]] = [[], []]           # torch arm: [phase][batch][slot]

    def set_states(quantised: bool) -> None:
        for op in quantable: op.restore_quantize_state() if quantised else op.dequantize()
        risky = A._written_in_place(graph, hooks)            # operations whose outputs a fused epilogue launch writes in place
        for op in interested:
            hook = hooks[op.name]
            hook.clone_outputs = op.name in risky
            hook.clone_inputs = [v.source_op is not None and v.source_op.name in risky for v in op.inputs]

    def run_phase(phase: int) -> int:
        batches = 0
        for idx, batch in A._batches(dataloader, collate_fn, steps):
            executor.forward(inputs=batch, hooks=hooks)
            stats['forwards'] += 1
            values = [v for op in interested for v in hooks[op.name].pop()]
            if len(values) != len(slots): raise RuntimeError('statistical_analyse: a hooked operation did not run in this forward')
            if use_kernels:
                rows = [v.contiguous().view(1, -1) for v in values]
                ffi.fetch_rows_multi([(r, A.device_indexer(fetchs, r.shape[1], A.FETCH_SEED, r.device)) for r in rows],
                                     [buffers[phase, k, idx].view(1, fetchs) for k in range(len(slots))])
                stats['fetch_launches'] += 1
            else: kept[phase].append(values)
            batches += 1
        return batches

    try:
        set_states(False)
        ran = run_phase(0)
        set_states(True)
        if run_phase(1) != ran: raise RuntimeError('statistical_analyse: the dataloader gave another number of batches in phase 2')
    finally:
        for op in quantable: op.restore_quantize_state()
        for hook in hooks.values(): hook.kept = []
    A.last_analysis_stats.update(stats)
    if use_kernels:
        return [(op, var, buffers[0, k, :ran].reshape(-1), buffers[1, k, :ran].reshape(-1)) for k, (op, var) in enumerate(slots)]
    return [(op, var, torch.cat([b[k] for b in kept[0]], dim=0), torch.cat([b[k] for b in kept[1]], dim=0))
            for k, (op, var) in enumerate(slots)]


def _record(op: Operation, var: Variable, snr: float, columns: Dict[str, dict]) -> dict:
    """One record with the reference's 27 keys in its order (StatisticalErrorAnalyser.stat, graphwise.py:252-285)."""
    record = {'Op name': op.name, 'Op type': op.type, 'Is parameter': var.is_parameter, 'Is input': var in op.inputs,
              'Is output': var in op.outputs, 'Variable name': var.name, 'Noise:Signal Power Ratio': snr}
    for kind in KINDS:
        for field in FIELDS: record[f'{kind} {field}'] = columns[kind][field]
    return record


def _torch_series(x: torch.Tensor, bins: int) -> dict:
    """graphwise.py:227-233 and :287-293 on one series, call by call."""
    mean, std = x.mean().item(), x.std().item()
    return {'Mean': mean, 'Std': std, 'Min': x.min().item(), 'Max': x.max().item(),
            'Skewness': torch.pow((x - mean) / std, 3).mean().item(),
            'Kurtosis': (torch.pow((x - mean) / std, 4).mean() - 3).item(),
            'Hist': torch.histc(x, bins=bins, min=x.min(), max=x.max()).cpu().tolist()}


def series_statistics(pairs: List[Pair], bins: int = 32, use_kernels: bool = True) -> List[dict]:
    """The statistics half of ``statistical_analyse``: one record per ``(operation, variable, x_fp, x_qt)``.

    Kernel arm (float32 series on the GPU): the noise ``x_qt - x_fp``, ``x_qt`` and ``x_fp`` of every pair are three jobs of ONE
    moments call and ONE shape call; one copy brings all records to the host.  The arithmetic is that of ``csrc/stats.hip``:
    sums in double, each elementwise step one fp32 operation; a sample that sits on a histogram bin edge can land in the
    neighbouring bin of what CPU ``torch.histc`` says.  ``use_kernels=False``: the reference's torch calls on the series
    where they are."""
    A = _analyse()
    if not pairs: return []
    if not use_kernels:
        records = []
        for op, var, x_fp, x_qt in pairs:
            A.last_analysis_stats['device_reads'] = A.last_analysis_stats.get('device_reads', 0) + 24 * int(x_fp.is_cuda)
            columns = {'Noise': _torch_series(x_qt - x_fp, bins), 'Quantized': _torch_series(x_qt, bins), 'Float': _torch_series(x_fp, bins)}
            records.append(_record(op, var, M.reference_formula('snr', x_qt.unsqueeze(0), x_fp.unsqueeze(0), 'mean').item(), columns))
        return records
    from . import ffi
    items = []
    for op, var, x_fp, x_qt in pairs:
        if x_fp.shape != x_qt.shape or x_fp.dim() != 1:
            raise ValueError(f'series_statistics: the series of {var.name} are not two 1-D tensors of one length')
        items += [(x_qt, x_fp), (x_qt, None), (x_fp, None)]
    ffi._f32(items[0][0], 'Series')
    table = ffi.stat_table(len(items), bins, items[0][0].device)
    ffi.stat_moments_multi(items, table)
    ffi.stat_shape_multi(items, table)
    host = table.cpu()                             # the one device-to-host copy of the report
    stats = A.last_analysis_stats
    stats['stat_launches'] = stats.get('stat_launches', 0) + 2
    stats['device_reads'] = stats.get('device_reads', 0) + 1
    words, counts = host[:, :ffi.STAT_WORDS].tolist(), ffi.stat_counts(host).tolist()
    records = []
    for k, (op, var, _, _) in enumerate(pairs):
        columns = {}
        for s, kind in enumerate(KINDS):
            w = words[3 * k + s]
            columns[kind] = {'Mean': w[0], 'Std': w[1], 'Min': w[2], 'Max': w[3], 'Skewness': w[4], 'Kurtosis': w[5],
                             'Hist': [float(c) for c in counts[3 * k + s]]}
        records.append(_record(op, var, words[3 * k][6], columns))
    return records


def statistical_analyse(graph: BaseGraph, running_device: str, dataloader: Iterator, collate_fn: Callable = None, steps: int = 8, *,
                        executor: TorchExecutor = None, use_kernels: bool = True, fetchs: int = STAT_FETCHS) -> List[dict]:
    """analyse/graphwise.py:186-372: for every input and output of every quantable operation that is not passive, the mean,
    std, skewness, kurtosis, 32-bin histogram, max and min of its FP32 samples, of its quantised samples and of their
    difference, and the NOISE:SIGNAL power ratio: a list of dicts (``pandas.DataFrame(report)`` reads it).

    ``collect_samples`` then ``series_statistics``; ``last_analysis_stats`` tells what was issued.  Every operation's
    quantisation state is put back, also when a forward raises."""
    pairs = collect_samples(graph, running_device, dataloader, collate_fn, steps, executor=executor, use_kernels=use_kernels,
                            fetchs=fetchs)
    return series_statistics(pairs, bins=32, use_kernels=use_kernels)


def parameter_analyse(graph: BaseGraph, *, verbose: bool = True, use_kernels: bool = True) -> Dict[str, Dict[str, float]]:
    """analyse/layerwise.py:179-203: range, std and |mean| of every parameter with more than one element, printed as the
    reference's three charts (``verbose``) and returned as ``{'Value Range': {...}, 'Value Std': {...}, 'Value Mean(Abs)': {...}}``
    keyed ``'{variable}[{operation}]'``.

    Kernel arm: every float32 GPU parameter is one job of ONE moments call (one read of each parameter) and one copy brings
    all of them back; any other parameter takes the reference's four torch calls."""
    A = _analyse()
    ranges, stds, means = {}, {}, {}
    jobs: List[Tuple[str, torch.Tensor]] = []
    stats = {'forwards': 0, 'fetch_launches': 0, 'stat_launches': 0, 'device_reads': 0}
    for operation in graph.operations.values():
        for var in operation.parameters:
            value = var.value
            assert isinstance(value, torch.Tensor), f'Invaild parameter value type, expect torch.Tensor, however {type(value)} was given.'
            if value.numel() <= 1: continue
            label = f'{var.name}[{operation.name}]'
            ranges[label] = stds[label] = means[label] = 0                     # (keeps the reference's insertion order)
            if use_kernels and value.is_cuda and value.dtype is torch.float32:
                jobs.append((label, value.contiguous().view(-1)))
                continue
            _min, _max, _std, _mean = 0, 0, 0, 0
            try:
                _min, _max, _std, _mean = value.min().item(), value.max().item(), value.std().item(), value.mean().item()
                stats['device_reads'] += 4 * int(value.is_cuda)
            except Exception: pass
            ranges[label], stds[label], means[label] = _max - _min, _std, abs(_mean)
    if jobs:
        from . import ffi
        table = ffi.stat_table(len(jobs), 0, jobs[0][1].device)
        ffi.stat_moments_multi([(x, None) for _, x in jobs], table)
        host = table.cpu().tolist()
        stats['stat_launches'] += 1; stats['device_reads'] += 1
        for (label, _), w in zip(jobs, host):
            ranges[label], stds[label], means[label] = w[3] - w[2], w[1], abs(w[0])
    A.last_analysis_stats.clear(); A.last_analysis_stats.update(stats)
    if verbose and ranges:
        A.MeasurePrinter(ranges, order='large_to_small', measure='Value Range').print()
        A.MeasurePrinter(stds, order='large_to_small', measure='Value Std').print()
        A.MeasurePrinter(means, order='large_to_small', measure='Value Mean(Abs)').print()
    return {'Value Range': ranges, 'Value Std': stds, 'Value Mean(Abs)': means}


@ torch.no_grad()
def variable_analyse(graph: BaseGraph, dataloader: Iterable, interested_outputs: Union[str, List[str]], collate_fn: Callable = None,
                     running_device: str = 'cuda', samples_per_step: int = 65536, steps: int = 8, dequantize: bool = False, *,
                     seed: Optional[int] = None, show: bool = False, executor: TorchExecutor = None) -> Dict[str, tuple]:
    """analyse/layerwise.py:137-176: ``samples_per_step`` samples of every interested variable in each of batches 0 .. ``steps``
    and their 64-bin histogram between their minimum and maximum: ``{name: (counts[64], lo, hi)}`` (the reference draws it;
    here it is drawn only with ``show=True`` and matplotlib installed).  ``seed=None`` draws each index table with
    ``torch.randint`` as the reference does; a seed gives the table of ``generate_indexer``."""
    from . import ffi
    A = _analyse()
    if isinstance(interested_outputs, str): interested_outputs = [interested_outputs]
    if executor is None: executor = TorchExecutor(graph=graph, device=running_device)
    quantable = A._quantable(graph) if dequantize else []
    device = torch.device(executor._device)
    buffers = torch.empty([len(interested_outputs), steps + 1, samples_per_step], dtype=torch.float32, device=device)
    ran = 0
    try:
        for op in quantable: op.dequantize()
        for idx, batch in A._batches(dataloader, collate_fn, steps):
            outputs = executor.forward(inputs=batch, output_names=interested_outputs)
            rows = [y.contiguous().view(1, -1) for y in outputs]
            tables = [A.device_indexer(samples_per_step, r.shape[1], seed, r.device) if seed is not None else
                      torch.randint(low=0, high=r.shape[1], size=[samples_per_step]).to(torch.int32).to(r.device) for r in rows]
            ffi.fetch_rows_multi(list(zip(rows, tables)), [buffers[k, idx].view(1, -1) for k in range(len(rows))])
            ran += 1
    finally:
        for op in quantable: op.restore_quantize_state()
    if ran == 0: return {}
    items = [(buffers[k, :ran].reshape(-1), None) for k in range(len(interested_outputs))]
    table = ffi.stat_table(len(items), 64, device)
    ffi.stat_moments_multi(items, table)
    ffi.stat_shape_multi(items, table)
    host = table.cpu()
    words, counts = host[:, :ffi.STAT_WORDS].tolist(), ffi.stat_counts(host).tolist()
    result = {name: (counts[k], words[k][2], words[k][3]) for k, name in enumerate(interested_outputs)}
    if show:
        try: from matplotlib import pyplot as plt
        except ImportError: plt = None
        for name, (count, lo, hi) in result.items() if plt is not None else ():
            width = (hi - lo) / 64 if hi > lo else 2 / 64
            left = lo if hi > lo else lo - 1
            plt.figure(figsize=[12, 8])
            plt.title(f'Histogram Result of Variable {name}:')
            plt.bar([left + (b + 0.5) * width for b in range(64)], count, width=width)
            plt.show()
    return result
