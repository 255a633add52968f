"""The quantize plans: MANY tensors fake-quantised with ONE launch per call into one resident arena (include/ppq_hip.h
ppqhip_fq_linear_multi / ppqhip_fq_float_multi); the MX plans of ``mx.py`` carve their arenas the same way."""
from itertools import accumulate
from typing import List

import torch

from .._lib import lib
from ._base import _KERNEL_FAILURE, JobTable, _dense, _geometry
from .abi import FQ_FLOAT_JOB, FQ_JOB


def _carve(sizes, dtype, device):
    """One resident buffer and its pieces of ``sizes`` elements in turn, every piece starting 16-B aligned."""
    unit = 16 // dtype.itemsize
    starts = list(accumulate(((n + unit - 1) // unit * unit for n in sizes), initial=0))
    buffer = torch.empty(starts[-1], dtype=dtype, device=device)
    return buffer, [buffer[at: at + n] for at, n in zip(starts, sizes)]


class _ArenaPlan:
    """What ``LinearQuantizePlan`` and ``FloatingQuantizePlan`` share; a subclass supplies the record (``_record``), the columns
    behind ``elem_per_channel`` (``_tail``) and the name of its C function (``_entry``; ``<_entry>_table_bytes`` sizes its table)."""
    @ staticmethod
    def accepts(value, scale, offset, axis) -> bool:
        """True when the plan can point at these tensors themselves (no layout copy needed)."""
        return _dense(value, axis) is value and scale.is_contiguous() and offset.is_contiguous()

    def __init__(self, items, rounding: int = 0):
        name = type(self).__name__
        if not items: raise ValueError(f'{name} needs at least one item')
        table = self._jobs = JobTable(self._record, name, len(items))          # keeps the tensors the device table points at
        tails = []
        for k, (value, scale, offset, axis, *tail) in enumerate(items):
            for what, t in (('Value', value), ('Scale', scale), ('Offset', offset)): table.tensor(t, what, k, contiguous=False)
            if not self.accepts(value, scale, offset, axis):
                raise RuntimeError(_KERNEL_FAILURE + f'{name}: value must be dense in storage order and '
                                   'scale / offset contiguous (a private copy would go stale); see accepts()')
            tails.append(self._tail(*tail))
        self._arena, pieces = _carve([it[0].numel() for it in items], torch.float32, table.dev)
        self._outs = []
        for k, (v, scale, offset, axis, *_) in enumerate(items):
            sc, of = scale.reshape(-1), offset.reshape(-1)          # views: accepts() guarantees contiguity
            C, epc = (1, v.numel()) if axis is None else _geometry(v.shape, axis)
            if sc.numel() != C or of.numel() != C: table.refuse(k, f'needs {C} scales / offsets')
            out = pieces[k].as_strided(v.shape, v.stride())          # same memory format as the input
            self._outs.append(out)
            table.jobs[k] = (v.data_ptr(), sc.data_ptr(), of.data_ptr(), out.data_ptr(), v.numel(), C, epc, *tails[k])
        self._rounding = int(getattr(rounding, 'value', rounding))
        self._table = torch.empty(int(getattr(lib, self._entry + '_table_bytes')(len(items))), dtype=torch.uint8, device=table.dev)
        self._uploaded = False
        self.bytes = 8 * sum(it[0].numel() for it in items)

    def run(self) -> List[torch.Tensor]:
        self._jobs.launch(getattr(lib, self._entry), self._rounding, self._table.data_ptr(), 0 if self._uploaded else 1)
        self._uploaded = True
        return self._outs


class LinearQuantizePlan(_ArenaPlan):
    """Fake-quantise MANY tensors with ONE launch per call (``ppqhip_fq_linear_multi``): the weights of
    a graph, which the executor quantises again on every forward.  Built once from
    ``(value, scale, offset, channel_axis | None, quant_min, quant_max)`` items that share a rounding
    policy; ``run()`` re-quantises all of them into one resident arena and returns views shaped like
    the inputs -- values identical to ``CUDA.LinearQuantize_C`` / ``_T`` per item.  The device job
    table holds POINTERS to the callers' tensors and is uploaded by the first ``run()``: in-place updates
    of a value / scale / offset are seen by later runs, a REPLACED tensor needs a new plan (the owner keys
    on ``data_ptr()``, harness._fused_parameters).  An item whose value is not dense in storage order, or
    whose scale / offset is not contiguous, would need a private copy that later in-place updates never
    reach: such items are refused (``accepts()``) and go through the per-tensor entry points instead."""
    _record, _entry = FQ_JOB, 'ppqhip_fq_linear_multi'

    @ staticmethod
    def _tail(qmin, qmax): return int(qmin), int(qmax)


class FloatingQuantizePlan(_ArenaPlan):
    """The FP8 twin of LinearQuantizePlan (``ppqhip_fq_float_multi``): items are
    ``(value, scale, offset, channel_axis | None, exponent, mantissa, clip_min, clip_max)`` sharing a rounding policy --
    the per-channel FP8 weights the TRT_FP8 policy fake-quantises again on every forward (ViT-B/16: 50 of them).
    Values identical to ``CUDA.FloatingQuantize_C`` / ``_T`` per item; same pointer / accepts() rules."""
    _record, _entry = FQ_FLOAT_JOB, 'ppqhip_fq_float_multi'

    @ staticmethod
    def _tail(exponent, mantissa, clip_min, clip_max):
        if exponent <= 0: raise ValueError('Floating Quantization requires exponent > 0')          # the reference's ffi.py:283
        return int(exponent), int(mantissa), float(clip_min), float(clip_max)
