"""Layerwise equalization, channelwise split and SSD equalization (include/ppq_hip.h ppqhip_equalize_*_multi, ppqhip_split_*_multi,
ppqhip_ssd_*_multi): the kernel families whose jobs describe their tensors with ``ppqhip_equalize_segment`` records."""
import numpy as np
import torch

from .._lib import lib
from ._base import JobTable
from .abi import EQ_APPLY_JOB, EQ_SCALE_JOB, EQ_SEGMENT, SPLIT_APPLY_JOB, SPLIT_PLAN_JOB, SSD_APPLY_JOB, SSD_SCALES_JOB

EqualizeTable = JobTable     # built once, launched every iteration: the jobs hold POINTERS, the pass changes its tensors in place


def _segment_record(table: JobTable, segment, k: int, what: str = 'Value') -> tuple:
    """One ``ppqhip_equalize_segment`` of item ``k`` from (tensor, div, a, b, outer, stride, run, multiplier, downstream): the
    tensor contiguous float32 on the table's device (its numel is the extent the library checks against)."""
    t, div, a, b, outer, stride, run, mult, down = segment
    table.tensor(t, what, k)
    return (t.data_ptr(), t.numel(), int(div), int(a), int(b), int(outer), int(stride), int(run), float(mult), 1 if down else 0)


def _segment_table(dtype, label, entry, items, head) -> JobTable:
    """A table whose job k owns a run of segment records: ``items[k] = (..., value_threshold, segments)`` and ``head(table, k,
    item)`` checks what stands in front and returns its addresses and the channel count.  The records of all jobs share one array."""
    table = JobTable(dtype, label, len(items), entry)
    segs = np.zeros(sum(len(it[-1]) for it in items), dtype=EQ_SEGMENT)
    records = []
    for k, item in enumerate(items):
        ptrs, C = head(table, k, item)
        table.jobs[k] = (segs.ctypes.data + len(records) * EQ_SEGMENT.itemsize, *ptrs, len(item[-1]), C, float(item[-2]), 0)
        records += [_segment_record(table, segment, k) for segment in item[-1]]
    segs[:] = records                                                     # one assignment: element-wise ones cost a microsecond each
    table.keep.append(segs)                                               # the jobs point into it
    return table


# ---- layerwise equalization -----------------------------------------------------------------------------------------------------
def _scale_head(table, k, item):
    scale = table.tensor(item[0], 'Scale', k)
    return (scale.data_ptr(),), scale.numel()


def equalize_scale_table(items) -> EqualizeTable:
    """items[k] = (scale, value_threshold, segments): ``scale`` a contiguous float32[C] CUDA tensor that receives the pair's
    scale; segments[t] = (tensor, div, a, b, outer, stride, run, multiplier, downstream) as ``ppqhip_equalize_segment``
    describes them, ``tensor`` contiguous float32 on the same device (its numel is the extent the library checks against)."""
    return _segment_table(EQ_SCALE_JOB, 'Equalization', lib.ppqhip_equalize_scale_multi, items, _scale_head)


def equalize_apply_table(items) -> EqualizeTable:
    """items[k] = (x, scale, run, inner, group_out, divide) as ``ppqhip_equalize_apply_job`` describes them: ``x`` is changed in
    place.  The tensors of one table must not overlap (the library refuses)."""
    table = JobTable(EQ_APPLY_JOB, 'Equalization', len(items), lib.ppqhip_equalize_apply_multi)
    for k, (x, scale, run, inner, group_out, divide) in enumerate(items):
        table.tensor(x, 'Value', k); table.tensor(scale, 'Scale', k)
        table.jobs[k] = (x.data_ptr(), scale.data_ptr(), x.numel(), int(run), int(inner), int(group_out), scale.numel(), 1 if divide else 0, 0)
    return table


def _run_table(items, build) -> None:
    (items if isinstance(items, JobTable) else build(items)).run()


def equalize_scale_multi(items) -> None:
    """EqualizationPair.calculate_scale over reduce_by_axis (ppq/quantization/algorithm/equalization.py:419-436) for every item
    (an :class:`EqualizeTable` or the items of :func:`equalize_scale_table`) in ONE launch."""
    _run_table(items, equalize_scale_table)


def equalize_apply_multi(items) -> None:
    """EqualizationHelper.scale_to_upstream / scale_to_downstream (:139-198) for every item in ONE launch, in place."""
    _run_table(items, equalize_apply_table)


# ---- channelwise split ----------------------------------------------------------------------------------------------------------
SPLIT_MAX_JOBS, SPLIT_MAX_SEGMENTS = 32, 72        # what one launch holds (csrc/split.hip kSpMaxJobs / kSpApMaxJobs, kEqMaxSegs)
SPLIT_BIT = -0x80000000                            # bit 31 of an int32 plan entry: the channel is one half of a split


def _plan_head(table, k, item):
    src_of, count = item[0], item[1]
    if src_of.numel() % 2: table.refuse(k, 'SrcOf must hold 2 x C entries')
    table.tensor(src_of, 'SrcOf', k, torch.int32); table.tensor(count, 'Count', k, torch.int32, numel=1)
    return (src_of.data_ptr(), count.data_ptr()), src_of.numel() // 2


def split_plan_table(items) -> EqualizeTable:
    """items[k] = (src_of, count, value_threshold, segments): ``src_of`` a contiguous int32[2 C] CUDA tensor that receives the
    pair's plan, ``count`` an int32[1] tensor (a view into one buffer per level: one copy reads them all) that receives the new
    channel count; segments as in :func:`equalize_scale_table`."""
    return _segment_table(SPLIT_PLAN_JOB, 'Channel split', lib.ppqhip_split_plan_multi, items, _plan_head)


def split_apply_table(items) -> EqualizeTable:
    """items[k] = (x, out, src_of, num_channel, count, run): ``x`` viewed as [outer, num_channel, run] is gathered into ``out``
    [outer, count, run] as ``ppqhip_split_apply_job`` describes; ``count`` is the host's copy of what the plan wrote."""
    table = JobTable(SPLIT_APPLY_JOB, 'Channel split', len(items), lib.ppqhip_split_apply_multi)
    for k, (x, out, src_of, C, count, run) in enumerate(items):
        table.tensor(x, 'Value', k); table.tensor(out, 'Out', k); table.tensor(src_of, 'SrcOf', k, torch.int32)
        C, count, run = int(C), int(count), int(run)
        if C > 0 and run > 0 and x.numel() % (C * run) == 0 and C <= count <= 2 * C:       # else the library says what is wrong
            if out.numel() != x.numel() // C * count or src_of.numel() < count:
                table.refuse(k, f'Out must hold {x.numel() // C * count} floats and SrcOf {count} entries')
        table.jobs[k] = (x.data_ptr(), out.data_ptr(), src_of.data_ptr(), x.numel(), run, C, count)
    return table


def split_plan_launches(items) -> int:
    """Kernel launches of :func:`split_plan_multi` on these items: two (mask, scan) per chunk of at most 32 jobs / 72 segments."""
    chunks = jobs = segs = 0
    for it in items:
        n = len(it[3])
        if jobs == 0 or jobs == SPLIT_MAX_JOBS or segs + n > SPLIT_MAX_SEGMENTS: chunks, jobs, segs = chunks + 1, 0, 0
        jobs, segs = jobs + 1, segs + n
    return 2 * chunks


def split_apply_launches(items) -> int:
    return (len(items) + SPLIT_MAX_JOBS - 1) // SPLIT_MAX_JOBS


def split_plan_multi(items) -> None:
    """The split plan of EqualizationPair.channel_split (ppq/quantization/algorithm/equalization.py:361-393) for every item (an
    :class:`EqualizeTable` or the items of :func:`split_plan_table`): keys and mask in one launch, the scan in another."""
    _run_table(items, split_plan_table)


def split_apply_multi(items) -> None:
    """ChannelSplitHelper.split_by_mask (:203-220) for every item in ONE launch, out of place."""
    _run_table(items, split_apply_table)


# ---- SSD equalization -----------------------------------------------------------------------------------------------------------
def ssd_scales_multi(items) -> None:
    """The four candidate scales of every pair of ``items`` in ONE call (ppq/quantization/optim/ssd.py:288-320 without the
    write-back).  items[k] = (first, last, act_range, channel_ratio, scales, ranges): ``first`` / ``last`` are segments
    (tensor, div, a, b, outer, stride, run) as ``ppqhip_equalize_segment`` describes them -- the rows of output channel c of the
    pair's first weight and the slices of input channel c of its last weight; ``act_range`` float32 [C]; ``scales`` float32
    [4, C] and ``ranges`` float32 [2, C] are overwritten.  Everything contiguous float32 on one device."""
    table = JobTable(SSD_SCALES_JOB, 'SSD scales', len(items))
    for k, (first, last, act, ratio, scales, ranges) in enumerate(items):
        C = act.numel()
        table.tensor(act, 'ActRange', k); table.tensor(scales, 'Scales', k, numel=4 * C); table.tensor(ranges, 'Ranges', k, numel=2 * C)
        segs = [_segment_record(table, tuple(seg) + (1.0, False), k, what) for what, seg in (('First', first), ('Last', last))]
        table.jobs[k] = (segs[0], segs[1], act.data_ptr(), scales.data_ptr(), ranges.data_ptr(), C, float(ratio))
    table.launch(lib.ppqhip_ssd_scales_multi)


def ssd_apply_multi(items) -> None:
    """write_back (ssd.py:212-262) of all four candidates of every tensor of ``items`` in ONE launch, out of place.
    items[k] = (x, out, scales, run, inner, group_out, divide): ``out`` float32 [4, *x.shape] receives x * s_k (or the IEEE
    quotient x / s_k) for the four rows s_k of ``scales`` [4, C]; geometry as in :func:`equalize_apply_table`.  x is not
    written."""
    table = JobTable(SSD_APPLY_JOB, 'SSD apply', len(items))
    for k, (x, out, scales, run, inner, group_out, divide) in enumerate(items):
        table.tensor(x, 'Value', k); table.tensor(out, 'Out', k, numel=4 * x.numel()); table.tensor(scales, 'Scales', k)
        if scales.numel() % 4: table.refuse(k, 'Scales must be [4, C]')
        table.jobs[k] = (x.data_ptr(), out.data_ptr(), scales.data_ptr(), x.numel(), int(run), int(inner), int(group_out),
                         scales.numel() // 4, 1 if divide else 0, 0)
    table.launch(lib.ppqhip_ssd_apply_multi)
