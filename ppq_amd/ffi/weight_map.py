"""The weight maps: AdaRound and round tuning (include/ppq_hip.h ppqhip_adaround_*_multi / ppqhip_roundtune_fwd_multi)."""
from typing import List

import numpy as np
import torch

from .._lib import lib
from ._base import _KERNEL_FAILURE, _DeviceOf, _f32, _geometry, _raise, _stream
from .abi import ADAROUND_JOB, ROUNDTUNE_JOB


def _weight_map_table(label, dtype, items, outs, dys=None):
    """items[k] = (w, rounding, scale, offset, channel_axis or None, quant_min, quant_max): w (round tuning: the pre-floored
    weight), the rounding variable (AdaRound's V, round tuning's R) and outs[k] (and dys[k]) contiguous float32 CUDA tensors of
    one shape on one device, scale / offset contiguous float32 with one element per channel.  ``dtype``: ADAROUND_JOB (with
    its ``dy`` column, 0 in the forward) or ROUNDTUNE_JOB."""
    n = len(items)
    if len(outs) != n or (dys is not None and len(dys) != n):
        raise RuntimeError(_KERNEL_FAILURE + f'{label}: argument lists differ in length')
    jobs = np.zeros(n, dtype=dtype)
    dev = items[0][0].device
    for k, (w, v, s, o, axis, qmin, qmax) in enumerate(items):
        ts = [('Value', w), ('Rounding', v), ('Scale', s), ('Offset', o), ('Out', outs[k])] + ([('Dy', dys[k])] if dys is not None else [])
        for name, t in ts:
            _f32(t, name)
            if t.device != dev: raise RuntimeError(_KERNEL_FAILURE + f'{label}: item {k}: {name} is on another device')
            if not t.is_contiguous(): raise RuntimeError(_KERNEL_FAILURE + f'{label}: item {k}: {name} is not contiguous')
        for name, t in ts[1:2] + ts[4:]:
            if t.shape != w.shape: raise RuntimeError(_KERNEL_FAILURE + f'{label}: item {k}: {name} is not shaped like the weight')
        C, epc = _geometry(w.shape, axis) if axis is not None else (1, w.numel())
        if s.numel() != C or o.numel() != C:
            raise RuntimeError(_KERNEL_FAILURE + f'{label}: item {k}: scale / offset need {C} elements')
        ptrs = [t.data_ptr() for _, t in ts[:5]]
        if 'dy' in dtype.names: ptrs.append(dys[k].data_ptr() if dys is not None else 0)
        jobs[k] = (*ptrs, w.numel(), C, epc, int(qmin), int(qmax))
    return jobs


def adaround_forward_multi(items, outs=None) -> List[torch.Tensor]:
    """AdaRoundDelegator.__call__ (ppq/quantization/optim/legacy.py:122-132) for every item in ONE launch; ``outs`` (optional,
    caller-owned) receive the fake-quantised weights.  The job table travels in the kernel arguments: capturable."""
    if not items: return []
    if outs is None: outs = [torch.empty_like(it[0]) for it in items]
    jobs = _weight_map_table('AdaRound', ADAROUND_JOB, items, outs)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_adaround_fwd_multi(jobs.ctypes.data, len(items), _stream()))
    return outs


def adaround_backward_multi(items, dys, reg: torch.Tensor, dvs=None) -> List[torch.Tensor]:
    """dV of every item in ONE launch: torch autograd's gradient through AdaRoundDelegator.__call__ plus, when ``reg[0]`` != 0,
    the gradient of gamma * AdaroundRegTerm (legacy.py:58-64).  ``reg``: float32 CUDA tensor {k, beta, beta - 1}."""
    if not items: return []
    _f32(reg, 'Reg')
    if reg.numel() != 3 or not reg.is_contiguous() or reg.device != items[0][0].device:
        raise RuntimeError(_KERNEL_FAILURE + 'AdaRound: reg must be a contiguous float32[3] on the weights\' device')
    if dvs is None: dvs = [torch.empty_like(it[0]) for it in items]
    jobs = _weight_map_table('AdaRound', ADAROUND_JOB, items, dvs, dys)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_adaround_bwd_multi(jobs.ctypes.data, len(items), reg.data_ptr(), _stream()))
    return dvs


def roundtune_forward_multi(items, outs=None) -> List[torch.Tensor]:
    """RoundTruningDelegator.__call__ (ppq/quantization/algorithm/training.py:490-527, :580-590) for every item in ONE launch;
    ``outs`` (optional, caller-owned) receive the fake-quantised weights.  The job table travels in the kernel arguments:
    capturable.  The reference's backward is the identity, so there is nothing else to launch."""
    if not items: return []
    if outs is None: outs = [torch.empty_like(it[0]) for it in items]
    jobs = _weight_map_table('RoundTuning', ROUNDTUNE_JOB, items, outs)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_roundtune_fwd_multi(jobs.ctypes.data, len(items), _stream()))
    return outs
