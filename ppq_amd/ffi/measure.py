"""Error analysis and statistical reports (include/ppq_hip.h ppqhip_fetch_rows_multi / ppqhip_measure_rows_multi /
ppqhip_measure_finish_multi / ppqhip_fq_measure_rows_multi / ppqhip_stat_moments_multi / ppqhip_stat_shape_multi)."""
from typing import List

import numpy as np
import torch

from .._lib import lib
from ._base import _KERNEL_FAILURE, JobTable, _DeviceOf, _f32, _geometry, _ptr, _raise, _stream
from .abi import FETCH_JOB, FINISH_JOB, FQ_MEASURE_JOB, MEASURE_JOB, STAT_JOB

# the four error-analysis builders are written out, not built on JobTable: the frame costs them 0.15 - 0.4 us per item (profiles/ffi_tables.txt)
MEASURE_METHODS = {'snr': 0, 'mse': 1, 'cosine': 2}
MEASURE_REDUCES = {'mean': 0, 'max': 1}


def _rows_of(t: torch.Tensor, name: str):
    """(rows, row_len) of a batched tensor read as [shape[0], rest], which must be float32, on the GPU and contiguous."""
    _f32(t, name)
    if not t.is_contiguous(): raise RuntimeError(_KERNEL_FAILURE + f'{name} is not contiguous')
    if t.dim() < 1: raise RuntimeError(_KERNEL_FAILURE + f'{name} has no batch dimension')
    return t.shape[0], t.numel() // t.shape[0]


def _index_of(index: torch.Tensor, row_len: int, dev) -> int:
    if index.dtype != torch.int32 or not index.is_cuda or not index.is_contiguous() or index.dim() != 1 or index.numel() == 0:
        raise RuntimeError(_KERNEL_FAILURE + 'Index must be a contiguous 1-D int32 tensor on the GPU')
    if index.device != dev: raise RuntimeError(_KERNEL_FAILURE + 'Index is on another device')
    return index.numel()


def fq_measure_rows_multi(items, sums=None) -> List[torch.Tensor]:
    """The row sums ``[rows, 4]`` of :func:`measure_rows_multi` between ``fake_quant(y)`` and ``r`` for every item, the
    fake-quant done in registers: ONE launch, y and r read once, nothing else written, bit-identical to ``LinearQuantize_T/C``
    into a buffer followed by ``measure_rows_multi``.  items[k] = (y, r, scale, offset, channel_axis, quant_min, quant_max,
    rounding): a linear config, ``channel_axis`` None (per tensor) or 1 (the axis behind the batch axis)."""
    if not items: return []
    dev = items[0][0].device
    if sums is None: sums = [torch.empty([it[0].shape[0], 4], dtype=torch.float64, device=dev) for it in items]
    jobs = np.zeros(len(items), dtype=FQ_MEASURE_JOB)
    for k, ((y, r, scale, offset, axis, qmin, qmax, rounding), out) in enumerate(zip(items, sums)):
        rows, count = _rows_of(y, 'Value')
        if _rows_of(r, 'Real') != (rows, count): raise RuntimeError(_KERNEL_FAILURE + f'fq measure: item {k}: Value {tuple(y.shape)} and Real {tuple(r.shape)} do not match')
        _f32(scale, 'Scale'); _f32(offset, 'Offset')
        if axis is None: C, epc = 1, count
        else:
            if axis % y.dim() != 1: raise RuntimeError(_KERNEL_FAILURE + f'fq measure: item {k}: channel_axis must be 1, {axis} was given')
            C, epc = _geometry(y.shape, 1)
        if scale.numel() != C or offset.numel() != C or not scale.is_contiguous() or not offset.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + f'fq measure: item {k}: Scale / Offset must be contiguous with {C} element(s)')
        if any(t.device != dev for t in (y, r, scale, offset, out)): raise RuntimeError(_KERNEL_FAILURE + f'fq measure: item {k} is on another device')
        if out.dtype != torch.float64 or out.numel() != rows * 4 or not out.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + f'fq measure: item {k}: Sums must be a contiguous float64 [{rows}, 4]')
        jobs[k] = (y.data_ptr(), r.data_ptr(), scale.data_ptr(), offset.data_ptr(), out.data_ptr(), rows, count, C, epc,
                   int(qmin), int(qmax), int(rounding), 0)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_fq_measure_rows_multi(jobs.ctypes.data, len(items), _stream()))
    return sums


def fetch_rows_multi(items, outs=None) -> List[torch.Tensor]:
    """``batch_random_fetch`` (ppq/utils/fetch.py:98-122) of every ``(x, index)`` item in ONE launch:
    ``out[b, i] = x[b].flatten()[index[i]]``; ``index`` is a device int32 table with values below ``x[0].numel()``."""
    if not items: return []
    dev = items[0][0].device
    if outs is None: outs = [torch.empty([x.shape[0], index.numel()], dtype=torch.float32, device=dev) for x, index in items]
    jobs = np.zeros(len(items), dtype=FETCH_JOB)
    for k, ((x, index), out) in enumerate(zip(items, outs)):
        rows, row_len = _rows_of(x, 'Value')
        count = _index_of(index, row_len, dev)
        if x.device != dev or out.device != dev: raise RuntimeError(_KERNEL_FAILURE + f'fetch: item {k} is on another device')
        if _rows_of(out, 'Out') != (rows, count): raise RuntimeError(_KERNEL_FAILURE + f'fetch: item {k}: Out is not [{rows}, {count}]')
        jobs[k] = (x.data_ptr(), index.data_ptr(), out.data_ptr(), rows, row_len, count)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_fetch_rows_multi(jobs.ctypes.data, len(items), _stream()))
    return outs


def measure_rows_multi(items, sums=None) -> List[torch.Tensor]:
    """The row sums ``[rows, 4]`` (float64: noise, signal, pp, pr) of every ``(p, r, index)`` item in ONE launch.  ``index``
    None: p and r have one shape.  Otherwise r is ``[rows, index.numel()]`` and p is read through the table (the fetch fused)."""
    if not items: return []
    dev = items[0][0].device
    if sums is None: sums = [torch.empty([p.shape[0], 4], dtype=torch.float64, device=dev) for p, _, _ in items]
    jobs = np.zeros(len(items), dtype=MEASURE_JOB)
    for k, ((p, r, index), out) in enumerate(zip(items, sums)):
        rows, row_len = _rows_of(p, 'Pred')
        r_rows, count = _rows_of(r, 'Real')
        if p.device != dev or r.device != dev or out.device != dev:
            raise RuntimeError(_KERNEL_FAILURE + f'measure: item {k} is on another device')
        if r_rows != rows or (index is None and count != row_len) or (index is not None and _index_of(index, row_len, dev) != count):
            raise RuntimeError(_KERNEL_FAILURE + f'measure: item {k}: Pred {tuple(p.shape)} and Real {tuple(r.shape)} do not match')
        if out.dtype != torch.float64 or out.numel() != rows * 4 or not out.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + f'measure: item {k}: Sums must be a contiguous float64 [{rows}, 4]')
        jobs[k] = (p.data_ptr(), r.data_ptr(), 0 if index is None else index.data_ptr(), out.data_ptr(), rows, row_len, count)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_measure_rows_multi(jobs.ctypes.data, len(items), _stream()))
    return sums


def measure_finish_multi(items, method: str, reduce: str = 'mean') -> None:
    """Per ``(sums, count, acc, row_out)`` item: the per-row measure of ``sums`` ([rows, 4] float64 of a row of ``count``
    elements) in fp32, written to ``row_out`` (float32 [rows] or None) and folded into ``acc`` (float64 [2]: running
    numerator and row count of one MeasureRecorder, or None).  ONE launch; the ``acc`` of the items must be distinct."""
    if not items: return
    jobs = np.zeros(len(items), dtype=FINISH_JOB)
    m, rd = MEASURE_METHODS[method], MEASURE_REDUCES[reduce]
    for k, (sums, count, acc, row_out) in enumerate(items):
        rows = sums.numel() // 4
        for name, t, dt, n in (('Sums', sums, torch.float64, rows * 4), ('Acc', acc, torch.float64, 2), ('RowOut', row_out, torch.float32, rows)):
            if t is None: continue
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.numel() != n or n == 0 or t.device != sums.device:
                raise RuntimeError(_KERNEL_FAILURE + f'measure finish: item {k}: {name} must be a contiguous {dt} tensor of {n} on the GPU')
        jobs[k] = (sums.data_ptr(), 0 if acc is None else acc.data_ptr(), 0 if row_out is None else row_out.data_ptr(),
                   rows, int(count), m, rd)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_measure_finish_multi(jobs.ctypes.data, len(items), _stream()))


# ---- statistical reports --------------------------------------------------------------------------------------------------------
STAT_WORDS = 8                                     # words of a record in front of its histogram counts
STAT_MAX_BINS = 64


def stat_table(num_series: int, bins: int, device) -> torch.Tensor:
    """The records of ``num_series`` series: float32 ``[num_series, 8 + bins]``; row k is mean, std, min, max, skewness,
    kurtosis, NOISE:SIGNAL, 0 and then the ``bins`` histogram counts as int32 bit patterns (``stat_counts`` reads them)."""
    if not 0 <= bins <= STAT_MAX_BINS: raise RuntimeError(_KERNEL_FAILURE + f'statistics: {bins} bins (at most {STAT_MAX_BINS})')
    return torch.zeros([num_series, STAT_WORDS + bins], dtype=torch.float32, device=device)


def stat_counts(table: torch.Tensor) -> torch.Tensor:
    """The histogram counts of a record table (device or host copy) as int32 ``[num_series, bins]``."""
    return table.view(torch.int32)[:, STAT_WORDS:]


def _stat_jobs(items, table: torch.Tensor) -> JobTable:
    if table.dtype != torch.float32 or not table.is_cuda or not table.is_contiguous() or table.dim() != 2 \
            or table.shape[0] != len(items) or not STAT_WORDS <= table.shape[1] <= STAT_WORDS + STAT_MAX_BINS:
        raise RuntimeError(_KERNEL_FAILURE + f'statistics: Table must be a contiguous float32 [{len(items)}, 8 + bins] tensor on the GPU')
    jobs = JobTable(STAT_JOB, 'statistics', len(items))
    jobs.tensor(table, 'Table', 0)                                  # the records' device is the series'
    words = table.shape[1]
    for k, (p, r) in enumerate(items):
        jobs.tensor(p, 'Series', k)
        if r is not None: jobs.tensor(r, 'Real', k, numel=p.numel())
        jobs.jobs[k] = (p.data_ptr(), _ptr(r), table.data_ptr() + 4 * words * k, p.numel(), words - STAT_WORDS, 0)
    return jobs


def stat_moments_multi(items, table: torch.Tensor) -> torch.Tensor:
    """Mean, std (n - 1), min, max of every ``(p, r)`` series in ONE call -- ``r`` None: the series is ``p``, otherwise
    ``p - r`` and the record also gets ``torch_snr_error(p, r)`` -- into words 0..3 and 6 of row k of ``table`` (``stat_table``)."""
    if items: _stat_jobs(items, table).launch(lib.ppqhip_stat_moments_multi)
    return table


def stat_shape_multi(items, table: torch.Tensor) -> torch.Tensor:
    """Skewness, kurtosis and the ``table.shape[1] - 8``-bin histogram of every series from the mean, std, min and max that
    ``stat_moments_multi`` left in ``table`` (read on the device), into words 4, 5 and 8.. of its row.  ONE call."""
    if items: _stat_jobs(items, table).launch(lib.ppqhip_stat_shape_multi)
    return table
