"""The drop-in seam: ``ppq.core.ffi`` rebuilt over the C-ABI HIP library.

Reference: ppq/core/ffi.py.  Two objects are provided.

``HIP_EXTENSION`` presents the 20 callables of the reference's pybind module ``PPQ_Cuda_Impls``
(ppq/csrc/export.cc:8-34) with the same names and positional arguments, so it can be assigned to
``ppq.core.ffi.CUDA_COMPLIER.__CUDA_EXTENTION__`` (see :func:`install_into_ppq` / INTEGRATION.md)
and every ``ppq.core.ffi.CUDA.*`` wrapper of an unmodified PPQ then lands in our kernels.

``CUDA`` mirrors the reference's static-method class of the same name (ffi.py:56-350): same method
names, argument names, defaults and order, for code that wants the operator surface without PPQ.
It adds the MI355X-native entries that have no twin in the reference (``MinMax_T/C``, ``KLLosses``,
``MseSearch``, the persistent-row / multi-tensor statistics launches).

All tensor arguments must live on the GPU.  There is no CPU path: a CPU tensor raises.
Errors follow the reference's convention as seen from Python: the C++ ``ValueTypeException`` /
``InvalidValueException`` (common.cuh:32-48) surface as ``RuntimeError``.
"""
import math
import threading
import weakref
from typing import List

import numpy as np
import torch

from . import _lib
from ._lib import lib

_KERNEL_FAILURE = 'Kernel Failure, '


_raw_stream = torch._C._cuda_getCurrentRawStream     # hipStream_t of torch's current stream, no Stream object
_get_device = torch._C._cuda_getDevice


def _stream() -> int:
    return _raw_stream(_get_device())


def _check(t: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    """CheckTensor, ppq/csrc/cuda/common.cuh:78-86."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a torch.Tensor, got {type(t)}')
    if t.dtype != dtype:
        raise RuntimeError(_KERNEL_FAILURE + 'Invalid dtype of Input tensor: ' + name)
    if t.numel() == 0:
        raise RuntimeError(_KERNEL_FAILURE + 'Tensor is empty: ' + name)
    if not t.is_cuda:
        raise RuntimeError(_KERNEL_FAILURE + f'{name} is not on the GPU (ppq_amd has no CPU path)')


_F32 = torch.float32


def _f32(t, name):
    # fast path of _check: one expression when everything is in order (the common case)
    try:
        if t.dtype is _F32 and t.is_cuda and t.numel() > 0: return
    except AttributeError:
        pass
    _check(t, torch.float32, name + '(Expect to be FP32)')


def _dense(t: torch.Tensor, channel_axis=None) -> torch.Tensor:
    """The tensor the kernels stream, WITHOUT a layout copy where none is needed: per-tensor kernels are
    order agnostic, so a dense channels-last tensor (MIOpen's preferred activation layout on MI355X) is
    read in storage order; per-channel kernels may do the same when the channel axis is the outermost
    one (conv weights [O, I, H, W] in channels-last keep one contiguous I*H*W chunk per output channel).
    Everything else falls back to ``.contiguous()`` like the reference (linear.cu:106,207)."""
    if t.is_contiguous(): return t
    if channel_axis is None or channel_axis % t.dim() == 0:
        if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last): return t
        if t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d): return t
    return t.contiguous()


def _raise(status: int) -> None:
    if status != 0:
        raise RuntimeError(_KERNEL_FAILURE + _lib.last_error())


def _geometry(shape, channel_axis: int):
    """num_channel = sizes[axis]; elem_per_channel = contiguous stride of the axis (linear.cu:213-214)
    == product of the trailing dims (floating.cu:118-122)."""
    ndim = len(shape)
    if channel_axis < 0: channel_axis += ndim
    if not 0 <= channel_axis < ndim:
        raise RuntimeError(_KERNEL_FAILURE + f'channel_axis {channel_axis} out of range for a {ndim}-d tensor')
    epc = 1
    for d in shape[channel_axis + 1:]:
        epc *= int(d)
    return int(shape[channel_axis]), epc


class _DeviceOf:
    """Make the tensor's device current while launching (the library launches on the current device)."""
    __slots__ = ('idx', 'prev')

    def __init__(self, t: torch.Tensor):
        self.idx = t.device.index
        self.prev = None

    def __enter__(self):
        if self.idx is not None and self.idx != _get_device():
            self.prev = _get_device()
            torch.cuda.set_device(self.idx)

    def __exit__(self, *a):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)


_workspaces = {}
_MAX_WORKSPACES = 16


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Per-(device, stream) scratch buffer for the kernels' two-stage reductions, grown on demand and
    allocated by torch's caching allocator -- so it is also valid while the current stream is being
    captured into a HIP graph (it then comes from the graph's private pool and lives as long as this
    cache holds it).  Launches that use it are ordered on the current stream."""
    key = (device.index, _stream())
    ws = _workspaces.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
    _workspaces[key] = ws                       # most recently used last
    while len(_workspaces) > _MAX_WORKSPACES:   # streams come and go (side streams, graph capture): drop the oldest;
        _workspaces.pop(next(iter(_workspaces)))    # the caching allocator frees it once queued work on its stream is done
    return ws


# host-side job records of the multi-tensor entry points (struct layouts of include/ppq_hip.h)
_MINMAX_JOB = np.dtype([('x', '<u8'), ('slots', '<u8'), ('n', '<i8')])
_FQ_JOB = np.dtype([('x', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('out', '<u8'), ('n', '<i8'),
                    ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('clip_min', '<i4'), ('clip_max', '<i4')])
_FQ_FLOAT_JOB = np.dtype([('x', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('out', '<u8'), ('n', '<i8'),
                          ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('exponent', '<i4'), ('mantissa', '<i4'),
                          ('clip_min', '<f4'), ('clip_max', '<f4')])
_FLOAT_SEARCH_JOB = np.dtype([('x', '<u8'), ('rows', '<i8'), ('row_len', '<i8'), ('exponent', '<i4'), ('mantissa', '<i4'),
                              ('clip_min', '<f4'), ('clip_max', '<f4')])
_LSQ_JOB = np.dtype([('x', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('grad_y', '<u8'), ('grad_x', '<u8'), ('grad_s', '<u8'),
                     ('n', '<i8'), ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('clip_min', '<i4'), ('clip_max', '<i4')])
_LSQ_FINISH_JOB = np.dtype([('partial', '<u8'), ('grad_s', '<u8'), ('n', '<i8'), ('clip_min', '<i4'), ('clip_max', '<i4')])
_MINMAX_C_JOB = np.dtype([('x', '<u8'), ('mins', '<u8'), ('maxs', '<u8'), ('n', '<i8'), ('num_channel', '<i8'),
                          ('elem_per_channel', '<i8'), ('fresh', '<i4'), ('reserved', '<i4')])
_QUANTILE_JOB = np.dtype([('x', '<u8'), ('dest', '<u8'), ('hint', '<u8'), ('n', '<i8')])

# Quantile_T(source, q) is stateless in the reference, but calibration calls it batch after batch from the same observer on
# the same activation.  A caller that wants the speed-up hands the entry point a threshold hint (include/ppq_hip.h:
# ppqhip_quantile_t): either explicitly (``Quantile_T(source, q, hint=...)``, what this package's percentile observer does) or
# by declaring itself the OWNER of the calls it is about to make -- ``with quantile_hint_owner(observer): ...`` -- which is
# what ``install_into_ppq()`` wraps around the reference's ``TorchPercentileObserver.observe``.  The owner's hints are kept per
# (device, numel, q) and die with it (weak keys): keyed by shape alone, one layer's thresholds would be handed to every other
# layer of that size (a CNN repeats its shapes), and a misplaced hint costs the exact passes.  No hint and no owner: every
# call samples its thresholds (``hint=None`` is the stateless default).  A hint only ever changes how much the kernels read,
# never the result.  (Round 3 found the owner by walking the caller's stack frames for a ``self``; a wrapper, a lambda or a
# functools.partial in between silently turned every call cold -- VERDICT r3.)
_owner_hints = weakref.WeakKeyDictionary()
_hint_owner = threading.local()


def quantile_hint(device: torch.device) -> torch.Tensor:
    """A fresh (zeroed) threshold hint for one stream of similar tensors: int32[8] on ``device``."""
    return torch.zeros(8, dtype=torch.int32, device=device)


class quantile_hint_owner:
    """Context manager: ``Quantile_T`` calls made (on this thread) inside the block use hints owned by ``owner`` -- one per
    (device, numel, q), created on first use, dropped when ``owner`` is garbage collected.  Nestable; ``owner`` must be weakly
    referenceable (any ordinary object)."""
    __slots__ = ('owner', 'prev')

    def __init__(self, owner):
        self.owner, self.prev = owner, None

    def __enter__(self):
        self.prev = getattr(_hint_owner, 'current', None)
        _hint_owner.current = self.owner
        return self

    def __exit__(self, *a):
        _hint_owner.current = self.prev


def _owner_quantile_hint(device: torch.device, numel: int, q: float):
    owner = getattr(_hint_owner, 'current', None)
    if owner is None: return None
    try: per = _owner_hints.setdefault(owner, {})
    except TypeError: return None                           # not weakly referenceable
    key = (device.index, int(numel), float(q))
    h = per.get(key)
    if h is None: h = per[key] = quantile_hint(device)
    return h


_HIST_JOB = np.dtype([('x', '<u8'), ('rows', '<u8'), ('n', '<i8'), ('p0', '<f4'), ('p1', '<f4')])


# ---- convolution epilogues (include/ppq_hip.h ppqhip_bias_act / ppqhip_bias_add_act) ---------------------------------
def _epilogue_geometry(ts, bias_list):
    """(num_channel, elem_per_channel) when every tensor of `ts` is a float32 CUDA 4-D tensor of one shape and one dense
    layout (contiguous -> (C, H*W), channels-last -> (C, 1), by _dense's rules) and every bias a contiguous float32 CUDA
    vector of C elements on the same device; None otherwise (the caller runs the unfused ops: nothing is copied)."""
    t0 = ts[0]
    if not isinstance(t0, torch.Tensor) or t0.dtype is not _F32 or not t0.is_cuda or t0.dim() != 4 or t0.numel() == 0:
        return None
    shape, strides, dev = t0.shape, t0.stride(), t0.device
    for t in ts[1:]:
        if not isinstance(t, torch.Tensor) or t.dtype is not _F32 or t.device != dev or t.shape != shape or t.stride() != strides:
            return None
    C = int(shape[1])
    for bias in bias_list:
        if (not isinstance(bias, torch.Tensor) or bias.dtype is not _F32 or bias.device != dev or bias.dim() != 1
                or bias.numel() != C or not bias.is_contiguous()):
            return None
    if t0.is_contiguous(): return C, int(shape[2]) * int(shape[3])
    if t0.is_contiguous(memory_format=torch.channels_last): return C, 1
    return None


def _pool_launch(y: torch.Tensor, geo, pool):
    """``(pooled, arguments)`` of a pooled launch (``ppqhip_bias_act_pool*``): the empty ``[N, C, OH, OW]`` result and the shape /
    window arguments behind the three pointers; None when `y` is not contiguous NCHW or ``pool = (kernel, stride, pad)`` has no
    output.  Whether the kernel has a path for the window is its own decision (PPQHIP_NOT_FUSED)."""
    k, s, p = (int(v) for v in pool)
    if geo is None or not y.is_contiguous() or k < 1 or s < 1 or p < 0: return None
    N, C, H, W = (int(v) for v in y.shape)
    if H + 2 * p < k or W + 2 * p < k: return None
    pooled = torch.empty((N, C, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1), dtype=_F32, device=y.device)
    return pooled, (y.numel(), C, H, W), (k, s, p, 1, 0)


def _run_epilogue(ts, biases, relu, kind=None, jobs=(), elide=0, pool=None, store=True):
    """What the six functions below share: the one call of a ``ppqhip_bias_[add_]act[_pool][_stats[2]|_hist]`` entry point.
    ``ts``: ``[y]``, or ``[a, b]`` with ``biases = [bias_a, bias_b or None]``; ``kind``: what the sinks take, ``'minmax'`` or
    ``'hist_rows'``, with one job (or None) per tensor the launch stores; ``elide`` / ``pool`` / ``store`` as the callers document
    them.  Returns None when NOTHING was launched -- operands that are not fusable (a residual that is its own operand: both
    would be written), a job for ``b`` without ``bias_b``, a job of another kind, no job at all or rules that differ, a window
    without output, PPQHIP_NOT_FUSED; else ``out`` of the residual form, the pooled tensor, or True."""
    a, resid = ts[0], len(ts) == 2
    geo = _epilogue_geometry(ts, biases if biases[-1] is not None else biases[:1])
    if geo is None or (resid and a.data_ptr() == ts[1].data_ptr()): return None
    name, sinks = 'ppqhip_bias_add_act' if resid else 'ppqhip_bias_act', ()
    if kind is not None:
        if resid and biases[1] is None and jobs[1] is not None: return None
        try:
            if kind == 'minmax':
                sinks = [_sink_slots(job, a.device) for job in jobs]
                if not any(sinks): return None
            else:
                sinks = [v for job in jobs for v in _sink_rows(job, a.device)]
                rule = _hist_rule(jobs)
                if rule is None: return None
                sinks += (rule[0], int(rule[1]), int(rule[2]))
        except ValueError: return None
    if resid:
        done = torch.empty_like(a)
        ptrs = (a.data_ptr(), biases[0].data_ptr(), ts[1].data_ptr(), 0 if biases[1] is None else biases[1].data_ptr(),
                done.data_ptr(), a.numel(), geo[0], geo[1], 1 if relu else 0)
        if kind == 'hist_rows': name, sinks = name + '_hist', (*sinks, int(elide))
        elif kind == 'minmax' and elide: name, sinks = name + '_stats2', (*sinks, int(elide))
        elif kind == 'minmax': name += '_stats'                            # (takes no elide: ppq_hip.h)
    elif pool is not None:
        launch = _pool_launch(a, geo, pool)
        if launch is None: return None
        done = launch[0]
        ptrs = (a.data_ptr(), biases[0].data_ptr(), done.data_ptr(), *launch[1], 1 if relu else 0, *launch[2])
        name += '_pool'
        if kind is not None: name, sinks = name + ('_stats' if kind == 'minmax' else '_hist'), (*sinks, 1 if store else 0)
    else:
        done = True
        ptrs = (a.data_ptr(), biases[0].data_ptr(), a.numel(), geo[0], geo[1], 1 if relu else 0)
        if kind is not None: name += '_stats' if kind == 'minmax' else '_hist'
    with _DeviceOf(a):
        return done if _fused_or_raise(getattr(lib, name)(*ptrs, *sinks, _stream())) else None


def bias_act_(y: torch.Tensor, bias: torch.Tensor, relu: bool, pool=None):
    """In place ``y = act(y + bias.view(1, C, 1, 1))`` with act = F.relu when `relu`, one launch; bitwise
    ``F.relu(F.conv2d(x, w, None) + b)``'s elementwise tail.  False (nothing done) when the operands are not fusable.
    ``pool = (kernel, stride, pad)``: the same launch also pools what it stores (``ppqhip_bias_act_pool``) and the call returns
    ``F.max_pool2d(y, kernel, stride, pad)`` bit for bit, or None when NOTHING was launched."""
    done = _run_epilogue([y], [bias], relu, pool=pool)
    return done if pool is not None else done is not None


def bias_add_act(a: torch.Tensor, bias_a: torch.Tensor, b: torch.Tensor, bias_b, relu: bool):
    """``a += bias_a``, ``b += bias_b`` (when given, else b is only read), returns ``act(a + b)`` in a new tensor of a's
    layout: the conv bias(es), the graph's Add(a, b) and F.relu in one launch.  None (nothing done) when not fusable."""
    return _run_epilogue([a, b], [bias_a, bias_b], relu)


def conv1x1(x: torch.Tensor, w: torch.Tensor, bias, stride: int = 1):
    """``F.conv2d(x, w, bias, stride=stride)`` for a 1x1 kernel on contiguous NCHW float32 operands as ONE native launch
    (``ppqhip_conv1x1``: FP32-input MFMA, every output the ascending-k fmaf chain from +0, then ``+ bias``; include/ppq_hip.h).
    ``w``: ``[O, C, 1, 1]`` or ``[O, C]``; ``bias``: ``[O]`` or None.  Returns the new ``[N, O, HO, WO]`` tensor, or None when
    NOTHING was launched because the kernel has no path for the operands (PPQHIP_NOT_FUSED); anything else that is wrong raises."""
    _f32(x, 'x'); _f32(w, 'w')
    if x.dim() != 4 or not x.is_contiguous() or not w.is_contiguous() or w.dim() not in (2, 4) or w.numel() != w.shape[0] * w.shape[1]:
        raise RuntimeError(_KERNEL_FAILURE + 'conv1x1: x must be contiguous NCHW and w a contiguous [O, C, 1, 1] or [O, C]')
    N, C, H, W = (int(v) for v in x.shape)
    O = int(w.shape[0])
    if int(w.shape[1]) != C or w.device != x.device: raise RuntimeError(_KERNEL_FAILURE + 'conv1x1: w does not match x')
    if bias is not None:
        _f32(bias, 'bias')
        if bias.dim() != 1 or bias.numel() != O or not bias.is_contiguous() or bias.device != x.device:
            raise RuntimeError(_KERNEL_FAILURE + 'conv1x1: bias must be a contiguous [O] vector on the device of x')
    stride = int(stride)
    y = torch.empty((N, O, (H - 1) // max(stride, 1) + 1, (W - 1) // max(stride, 1) + 1), dtype=_F32, device=x.device)
    with _DeviceOf(x):
        ok = _fused_or_raise(lib.ppqhip_conv1x1(x.data_ptr(), w.data_ptr(), 0 if bias is None else bias.data_ptr(), y.data_ptr(),
                                                N, C, H, W, O, stride, _stream()))
    return y if ok else None


def _sink_slots(job, dev) -> int:
    """Device address of the slots of an observer's ``('minmax', slots)`` job (``BaseTensorObserver.stat_job``), 0 for no job.
    Raises ValueError for a job the epilogue kernels have no sink for (the caller then does not fuse)."""
    if job is None: return 0
    slots = job[1]
    if (job[0] != 'minmax' or slots.dtype is not _F32 or slots.device != dev or not slots.is_contiguous()
            or slots.numel() != 2 * lib.ppqhip_minmax_slots()): raise ValueError('no sink for this job')
    return slots.data_ptr()


def _fused_or_raise(status: int) -> bool:
    if status == _lib.NOT_FUSED: return False
    _raise(status)
    return True


def bias_act_stats_(y: torch.Tensor, bias: torch.Tensor, relu: bool, job, pool=None, store: bool = True):
    """``bias_act_`` that also folds the stored ``y`` into the slots of ``job`` (an observer's ``('minmax', slots)``) from the
    registers it is stored from (``ppqhip_bias_act_stats``).  False: NOTHING was launched (operands or job not fusable) --
    the caller runs ``bias_act_`` and observes ``y`` as usual.
    ``pool = (kernel, stride, pad)``: the pooled form (``ppqhip_bias_act_pool_stats``), which returns the pooled tensor, or None
    when nothing was launched; with ``store=False`` it folds and pools ``act(y + bias)`` but leaves ``y`` as it was."""
    done = _run_epilogue([y], [bias], relu, 'minmax', [job], pool=pool, store=store)
    return done if pool is not None else done is not None


ELIDE_A, ELIDE_B = 1, 2          # PPQHIP_ELIDE_A / PPQHIP_ELIDE_B: the tensors a statistics epilogue computes, feeds, and does NOT store


def bias_add_act_stats(a: torch.Tensor, bias_a: torch.Tensor, b: torch.Tensor, bias_b, relu: bool, job_a, job_b, job_out,
                       elide: int = 0):
    """``bias_add_act`` that also folds the stored ``a``, ``b`` (only with ``bias_b``) and the returned ``out`` into the slots
    of their ``('minmax', slots)`` jobs (None: that tensor is not folded) (``ppqhip_bias_add_act_stats``).  ``elide``
    (ELIDE_A | ELIDE_B): those tensors are folded but not stored -- their memory keeps the convolution output
    (``ppqhip_bias_add_act_stats2``; each needs a job).
    None: NOTHING was launched -- the caller runs ``bias_add_act`` and observes as usual."""
    return _run_epilogue([a, b], [bias_a, bias_b], relu, 'minmax', [job_a, job_b, job_out], elide)


def _sink_rows(job, dev) -> tuple:
    """(rows address, p0, p1) of an observer's ``('hist_rows', rows, asymmetric, p0, p1, clip)`` job, (0, 0, 0) for no job.
    Raises ValueError for a job the histogram sinks do not take."""
    if job is None: return 0, 0.0, 0.0
    if job[0] != 'hist_rows': raise ValueError('no sink for this job')
    rows = job[1]
    if (rows.dtype is not torch.int32 or rows.device != dev or rows.dim() != 2 or not rows.is_contiguous()
            or rows.shape[0] != lib.ppqhip_hist_rows()): raise ValueError('no sink for this job')
    return rows.data_ptr(), float(job[3]), float(job[4])


def _hist_rule(jobs):
    """(bins, asymmetric, clip) shared by the jobs of one launch; None when they differ or there is none."""
    rules = {(int(j[1].shape[1]), bool(j[2]), bool(j[5])) for j in jobs if j is not None}
    return next(iter(rules)) if len(rules) == 1 else None


def bias_act_hist_(y: torch.Tensor, bias: torch.Tensor, relu: bool, job, pool=None, store: bool = True):
    """``bias_act_`` that also counts the stored ``y`` into the rows of ``job`` (an observer's ``('hist_rows', rows,
    asymmetric, p0, p1, clip)``) from the registers it is stored from (``ppqhip_bias_act_hist``).  False: NOTHING was
    launched -- the caller runs ``bias_act_`` and observes ``y`` as usual.
    ``pool`` / ``store``: the pooled form (``ppqhip_bias_act_pool_hist``), as in ``bias_act_stats_``."""
    done = _run_epilogue([y], [bias], relu, 'hist_rows', [job], pool=pool, store=store)
    return done if pool is not None else done is not None


def bias_add_act_hist(a: torch.Tensor, bias_a: torch.Tensor, b: torch.Tensor, bias_b, relu: bool, job_a, job_b, job_out,
                      elide: int = 0):
    """``bias_add_act`` that also counts ``a``, ``b`` (only with ``bias_b``) and the returned ``out`` into the rows of their
    ``'hist_rows'`` jobs (None: not counted), with ``elide`` as in ``bias_add_act_stats`` (``ppqhip_bias_add_act_hist``).
    None: NOTHING was launched -- the caller runs ``bias_add_act`` and observes as usual."""
    return _run_epilogue([a, b], [bias_a, bias_b], relu, 'hist_rows', [job_a, job_b, job_out], elide)


SINK_MINMAX, SINK_HIST = 1, 2    # PPQHIP_SINK_MINMAX / PPQHIP_SINK_HIST


def conv1x1_epilogue(x: torch.Tensor, w: torch.Tensor, stride: int, bias_a: torch.Tensor, resid, bias_b, relu: bool, job_a, job_r,
                     job_out, max_workgroups: int = 0):
    """``conv1x1`` with its whole epilogue group and the group's calibration sinks in the GEMM's store, one launch
    (``ppqhip_conv1x1_epilogue``).  ``resid`` None (P1): returns ``act(conv(x, w) + bias_a)``; with ``resid`` of the output's shape:
    ``act((conv(x, w) + bias_a) + r)`` with ``r = resid + bias_b`` (P2b) or ``r = resid`` (``bias_b`` None, P2) -- bit for bit
    ``conv1x1(x, w, None, stride)`` followed by ``bias_act_`` / ``bias_add_act``.  ``job_a`` / ``job_r`` / ``job_out``: the
    observers' ``('minmax', slots)`` or ``('hist_rows', ...)`` jobs for ``conv + bias_a``, the biased ``r`` and the result (None: not
    fed; P1 has ``job_out`` alone); neither of the first two tensors is ever stored.  ``max_workgroups``: a cap on the grid (0: none).
    Returns the new ``[N, O, HO, WO]`` tensor, or None when NOTHING was launched: no job, jobs of two kinds or rules, a job the
    sinks do not take, a residual that is no contiguous float32 tensor of the output's shape, PPQHIP_NOT_FUSED."""
    _f32(x, 'x'); _f32(w, 'w'); _f32(bias_a, 'bias_a')
    if x.dim() != 4 or not x.is_contiguous() or not w.is_contiguous() or w.dim() not in (2, 4) or w.numel() != w.shape[0] * w.shape[1]:
        raise RuntimeError(_KERNEL_FAILURE + 'conv1x1_epilogue: x must be contiguous NCHW and w a contiguous [O, C, 1, 1] or [O, C]')
    N, C, H, W = (int(v) for v in x.shape)
    O, dev = int(w.shape[0]), x.device
    if int(w.shape[1]) != C or w.device != dev: raise RuntimeError(_KERNEL_FAILURE + 'conv1x1_epilogue: w does not match x')
    for bias in (bias_a, bias_b):
        if bias is None: continue
        _f32(bias, 'bias')
        if bias.dim() != 1 or bias.numel() != O or not bias.is_contiguous() or bias.device != dev:
            raise RuntimeError(_KERNEL_FAILURE + 'conv1x1_epilogue: a bias must be a contiguous [O] vector on the device of x')
    stride = int(stride)
    shape = (N, O, (H - 1) // max(stride, 1) + 1, (W - 1) // max(stride, 1) + 1)
    if resid is None and bias_b is not None: raise RuntimeError(_KERNEL_FAILURE + 'conv1x1_epilogue: bias_b without a residual')
    if resid is not None and not (isinstance(resid, torch.Tensor) and resid.dtype is _F32 and resid.device == dev
                                  and tuple(resid.shape) == shape and resid.is_contiguous()): return None
    jobs = [job_a, job_r, job_out]
    kinds = {job[0] for job in jobs if job is not None}
    if len(kinds) != 1: return None
    try:
        if kinds == {'minmax'}:
            kind, dst, rule = SINK_MINMAX, [_sink_slots(job, dev) for job in jobs], (0, 0, 0)
            ps = [0.0] * 6
        else:
            rows = [_sink_rows(job, dev) for job in jobs]
            rule = _hist_rule(jobs)
            if rule is None: return None
            kind, dst, ps = SINK_HIST, [r[0] for r in rows], [v for r in rows for v in r[1:]]
    except ValueError: return None
    out = torch.empty(shape, dtype=_F32, device=dev)
    with _DeviceOf(x):
        ok = _fused_or_raise(lib.ppqhip_conv1x1_epilogue(
            x.data_ptr(), w.data_ptr(), bias_a.data_ptr(), 0 if resid is None else resid.data_ptr(),
            0 if bias_b is None else bias_b.data_ptr(), out.data_ptr(), N, C, H, W, O, stride, 1 if relu else 0, kind, *dst, *ps,
            int(rule[0]), int(rule[1]), int(rule[2]), int(max_workgroups), _stream()))
    return out if ok else None


# ---- the weight maps: AdaRound and round tuning (include/ppq_hip.h ppqhip_adaround_*_multi / ppqhip_roundtune_fwd_multi) ------
_ADAROUND_JOB = np.dtype([('w', '<u8'), ('v', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('out', '<u8'), ('dy', '<u8'),
                          ('n', '<i8'), ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('qmin', '<i4'), ('qmax', '<i4')])
_ROUNDTUNE_JOB = np.dtype([('w', '<u8'), ('r', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('out', '<u8'),
                           ('n', '<i8'), ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('qmin', '<i4'), ('qmax', '<i4')])


def _weight_map_table(label, dtype, items, outs, dys=None):
    """items[k] = (w, rounding, scale, offset, channel_axis or None, quant_min, quant_max): w (round tuning: the pre-floored
    weight), the rounding variable (AdaRound's V, round tuning's R) and outs[k] (and dys[k]) contiguous float32 CUDA tensors of
    one shape on one device, scale / offset contiguous float32 with one element per channel.  ``dtype``: _ADAROUND_JOB (with
    its ``dy`` column, 0 in the forward) or _ROUNDTUNE_JOB."""
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
    jobs = _weight_map_table('AdaRound', _ADAROUND_JOB, items, outs)
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
    jobs = _weight_map_table('AdaRound', _ADAROUND_JOB, items, dvs, dys)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_adaround_bwd_multi(jobs.ctypes.data, len(items), reg.data_ptr(), _stream()))
    return dvs


def roundtune_forward_multi(items, outs=None) -> List[torch.Tensor]:
    """RoundTruningDelegator.__call__ (ppq/quantization/algorithm/training.py:490-527, :580-590) for every item in ONE launch;
    ``outs`` (optional, caller-owned) receive the fake-quantised weights.  The job table travels in the kernel arguments:
    capturable.  The reference's backward is the identity, so there is nothing else to launch."""
    if not items: return []
    if outs is None: outs = [torch.empty_like(it[0]) for it in items]
    jobs = _weight_map_table('RoundTuning', _ROUNDTUNE_JOB, items, outs)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_roundtune_fwd_multi(jobs.ctypes.data, len(items), _stream()))
    return outs


# ---- layerwise equalization (include/ppq_hip.h ppqhip_equalize_scale_multi / ppqhip_equalize_apply_multi) --------------------
_EQ_SEGMENT = np.dtype([('base', '<u8'), ('extent', '<i8'), ('div', '<i8'), ('a', '<i8'), ('b', '<i8'), ('outer', '<i8'),
                        ('stride', '<i8'), ('run', '<i8'), ('multiplier', '<f4'), ('downstream', '<i4')])
_EQ_SCALE_JOB = np.dtype([('segments', '<u8'), ('scale', '<u8'), ('num_segments', '<i4'), ('num_channel', '<i4'),
                          ('value_threshold', '<f4'), ('reserved', '<i4')])
_EQ_APPLY_JOB = np.dtype([('x', '<u8'), ('scale', '<u8'), ('n', '<i8'), ('run', '<i8'), ('inner', '<i8'), ('group_out', '<i8'),
                          ('num_scale', '<i8'), ('divide', '<i4'), ('reserved', '<i4')])


def _eq_tensor(t, what: str, k: int, dev):
    _f32(t, what)
    if t.device != dev: raise RuntimeError(_KERNEL_FAILURE + f'Equalization: item {k}: {what} is on another device')
    if not t.is_contiguous(): raise RuntimeError(_KERNEL_FAILURE + f'Equalization: item {k}: {what} is not contiguous')


def _segment_record(segment, k: int, dev, what: str = 'Value') -> tuple:
    """One ``ppqhip_equalize_segment`` of item ``k`` from (tensor, div, a, b, outer, stride, run, multiplier, downstream): the
    tensor contiguous float32 on ``dev`` (its numel is the extent the library checks against)."""
    t, div, a, b, outer, stride, run, mult, down = segment
    _eq_tensor(t, what, k, dev)
    return (t.data_ptr(), t.numel(), int(div), int(a), int(b), int(outer), int(stride), int(run), float(mult), 1 if down else 0)


class EqualizeTable:
    """The host job table of one equalization launch, built once and launched every iteration: the jobs hold POINTERS and the
    pass changes its tensors in place.  Keeps the tensors (and the segment array the jobs point into) alive."""
    __slots__ = ('jobs', 'segments', 'keep', 'entry')

    def __init__(self, jobs, segments, keep, entry):
        self.jobs, self.segments, self.keep, self.entry = jobs, segments, keep, entry

    def __len__(self) -> int: return len(self.jobs)

    def run(self) -> None:
        if len(self.jobs) == 0: return
        with _DeviceOf(self.keep[0]):
            _raise(self.entry(self.jobs.ctypes.data, len(self.jobs), _stream()))


def equalize_scale_table(items) -> EqualizeTable:
    """items[k] = (scale, value_threshold, segments): ``scale`` a contiguous float32[C] CUDA tensor that receives the pair's
    scale; segments[t] = (tensor, div, a, b, outer, stride, run, multiplier, downstream) as ``ppqhip_equalize_segment``
    describes them, ``tensor`` contiguous float32 on the same device (its numel is the extent the library checks against)."""
    jobs = np.zeros(len(items), dtype=_EQ_SCALE_JOB)
    segs = np.zeros(sum(len(it[2]) for it in items), dtype=_EQ_SEGMENT)
    keep, records = [], []
    dev = items[0][0].device if items else None
    for k, (scale, threshold, segments) in enumerate(items):
        _eq_tensor(scale, 'Scale', k, dev)
        keep.append(scale)
        jobs[k] = (segs.ctypes.data + len(records) * _EQ_SEGMENT.itemsize, scale.data_ptr(), len(segments), scale.numel(), float(threshold), 0)
        for segment in segments:
            records.append(_segment_record(segment, k, dev))
            keep.append(segment[0])
    segs[:] = records                                                     # one assignment: element-wise ones cost a microsecond each
    return EqualizeTable(jobs, segs, keep, lib.ppqhip_equalize_scale_multi)


def equalize_apply_table(items) -> EqualizeTable:
    """items[k] = (x, scale, run, inner, group_out, divide) as ``ppqhip_equalize_apply_job`` describes them: ``x`` is changed in
    place.  The tensors of one table must not overlap (the library refuses)."""
    jobs = np.zeros(len(items), dtype=_EQ_APPLY_JOB)
    keep = []
    dev = items[0][0].device if items else None
    for k, (x, scale, run, inner, group_out, divide) in enumerate(items):
        _eq_tensor(x, 'Value', k, dev); _eq_tensor(scale, 'Scale', k, dev)
        keep += [x, scale]
        jobs[k] = (x.data_ptr(), scale.data_ptr(), x.numel(), int(run), int(inner), int(group_out), scale.numel(), 1 if divide else 0, 0)
    return EqualizeTable(jobs, None, keep, lib.ppqhip_equalize_apply_multi)


def equalize_scale_multi(items) -> None:
    """EqualizationPair.calculate_scale over reduce_by_axis (ppq/quantization/algorithm/equalization.py:419-436) for every item
    (an :class:`EqualizeTable` or the items of :func:`equalize_scale_table`) in ONE launch."""
    (items if isinstance(items, EqualizeTable) else equalize_scale_table(items)).run()


def equalize_apply_multi(items) -> None:
    """EqualizationHelper.scale_to_upstream / scale_to_downstream (:139-198) for every item in ONE launch, in place."""
    (items if isinstance(items, EqualizeTable) else equalize_apply_table(items)).run()


# ---- channelwise split (include/ppq_hip.h ppqhip_split_plan_multi / ppqhip_split_apply_multi) --------------------------------
_SPLIT_PLAN_JOB = np.dtype([('segments', '<u8'), ('src_of', '<u8'), ('count', '<u8'), ('num_segments', '<i4'), ('num_channel', '<i4'),
                            ('value_threshold', '<f4'), ('reserved', '<i4')])
_SPLIT_APPLY_JOB = np.dtype([('x', '<u8'), ('out', '<u8'), ('src_of', '<u8'), ('n', '<i8'), ('run', '<i8'), ('num_channel', '<i4'),
                             ('count', '<i4')])
SPLIT_MAX_JOBS, SPLIT_MAX_SEGMENTS = 32, 72        # what one launch holds (csrc/split.hip kSpMaxJobs / kSpApMaxJobs, kEqMaxSegs)
SPLIT_BIT = -0x80000000                            # bit 31 of an int32 plan entry: the channel is one half of a split


def _i32(t, what: str, k: int, dev, numel: int):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == numel):
        raise RuntimeError(_KERNEL_FAILURE + f'Channel split: item {k}: {what} must be a contiguous int32 tensor of {numel}')
    if not t.is_cuda: raise RuntimeError(_KERNEL_FAILURE + f'Channel split: item {k}: {what} is not on the GPU')
    if t.device != dev: raise RuntimeError(_KERNEL_FAILURE + f'Channel split: item {k}: {what} is on another device')


def split_plan_table(items) -> EqualizeTable:
    """items[k] = (src_of, count, value_threshold, segments): ``src_of`` a contiguous int32[2 C] CUDA tensor that receives the
    pair's plan, ``count`` an int32[1] tensor (a view into one buffer per level: one copy reads them all) that receives the new
    channel count; segments as in :func:`equalize_scale_table`."""
    jobs = np.zeros(len(items), dtype=_SPLIT_PLAN_JOB)
    segs = np.zeros(sum(len(it[3]) for it in items), dtype=_EQ_SEGMENT)
    keep, records = [], []
    dev = items[0][0].device if items else None
    for k, (src_of, count, threshold, segments) in enumerate(items):
        if src_of.numel() % 2: raise RuntimeError(_KERNEL_FAILURE + f'Channel split: item {k}: SrcOf must hold 2 x C entries')
        _i32(src_of, 'SrcOf', k, dev, src_of.numel()); _i32(count, 'Count', k, dev, 1)
        keep += [src_of, count]
        jobs[k] = (segs.ctypes.data + len(records) * _EQ_SEGMENT.itemsize, src_of.data_ptr(), count.data_ptr(), len(segments), src_of.numel() // 2,
                   float(threshold), 0)
        for segment in segments:
            records.append(_segment_record(segment, k, dev))
            keep.append(segment[0])
    segs[:] = records                                                     # one assignment: element-wise ones cost a microsecond each
    return EqualizeTable(jobs, segs, keep, lib.ppqhip_split_plan_multi)


def split_apply_table(items) -> EqualizeTable:
    """items[k] = (x, out, src_of, num_channel, count, run): ``x`` viewed as [outer, num_channel, run] is gathered into ``out``
    [outer, count, run] as ``ppqhip_split_apply_job`` describes; ``count`` is the host's copy of what the plan wrote."""
    jobs = np.zeros(len(items), dtype=_SPLIT_APPLY_JOB)
    keep = []
    dev = items[0][0].device if items else None
    for k, (x, out, src_of, C, count, run) in enumerate(items):
        _eq_tensor(x, 'Value', k, dev); _eq_tensor(out, 'Out', k, dev)
        _i32(src_of, 'SrcOf', k, dev, src_of.numel())
        C, count, run = int(C), int(count), int(run)
        if C > 0 and run > 0 and x.numel() % (C * run) == 0 and C <= count <= 2 * C:       # else the library says what is wrong
            if out.numel() != x.numel() // C * count or src_of.numel() < count:
                raise RuntimeError(_KERNEL_FAILURE + f'Channel split: item {k}: Out must hold {x.numel() // C * count} floats and SrcOf {count} entries')
        keep += [x, out, src_of]
        jobs[k] = (x.data_ptr(), out.data_ptr(), src_of.data_ptr(), x.numel(), run, C, count)
    return EqualizeTable(jobs, None, keep, lib.ppqhip_split_apply_multi)


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
    (items if isinstance(items, EqualizeTable) else split_plan_table(items)).run()


def split_apply_multi(items) -> None:
    """ChannelSplitHelper.split_by_mask (:203-220) for every item in ONE launch, out of place."""
    (items if isinstance(items, EqualizeTable) else split_apply_table(items)).run()


# ---- SSD equalization (include/ppq_hip.h ppqhip_ssd_scales_multi / ppqhip_ssd_apply_multi / ppqhip_fq_measure_rows_multi) ----
_SSD_SCALES_JOB = np.dtype([('first', _EQ_SEGMENT), ('last', _EQ_SEGMENT), ('act_range', '<u8'), ('scales', '<u8'), ('ranges', '<u8'),
                            ('num_channel', '<i4'), ('channel_ratio', '<f4')])
_SSD_APPLY_JOB = np.dtype([('x', '<u8'), ('out', '<u8'), ('scales', '<u8'), ('n', '<i8'), ('run', '<i8'), ('inner', '<i8'),
                           ('group_out', '<i8'), ('num_channel', '<i8'), ('divide', '<i4'), ('reserved', '<i4')])
_FQ_MEASURE_JOB = np.dtype([('y', '<u8'), ('r', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('sums', '<u8'), ('rows', '<i8'),
                            ('count', '<i8'), ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('clip_min', '<i4'),
                            ('clip_max', '<i4'), ('rounding', '<i4'), ('reserved', '<i4')])


def ssd_scales_multi(items) -> None:
    """The four candidate scales of every pair of ``items`` in ONE call (ppq/quantization/optim/ssd.py:288-320 without the
    write-back).  items[k] = (first, last, act_range, channel_ratio, scales, ranges): ``first`` / ``last`` are segments
    (tensor, div, a, b, outer, stride, run) as ``ppqhip_equalize_segment`` describes them -- the rows of output channel c of the
    pair's first weight and the slices of input channel c of its last weight; ``act_range`` float32 [C]; ``scales`` float32
    [4, C] and ``ranges`` float32 [2, C] are overwritten.  Everything contiguous float32 on one device."""
    if not items: return
    jobs = np.zeros(len(items), dtype=_SSD_SCALES_JOB)
    dev = items[0][2].device
    for k, (first, last, act, ratio, scales, ranges) in enumerate(items):
        C = act.numel()
        for what, t, n in (('ActRange', act, C), ('Scales', scales, 4 * C), ('Ranges', ranges, 2 * C)):
            _eq_tensor(t, what, k, dev)
            if t.numel() != n: raise RuntimeError(_KERNEL_FAILURE + f'SSD scales: item {k}: {what} must hold {n} floats')
        segs = [_segment_record(tuple(seg) + (1.0, False), k, dev, what) for what, seg in (('First', first), ('Last', last))]
        jobs[k] = (segs[0], segs[1], act.data_ptr(), scales.data_ptr(), ranges.data_ptr(), C, float(ratio))
    with _DeviceOf(items[0][2]):
        _raise(lib.ppqhip_ssd_scales_multi(jobs.ctypes.data, len(items), _stream()))


def ssd_apply_multi(items) -> None:
    """write_back (ssd.py:212-262) of all four candidates of every tensor of ``items`` in ONE launch, out of place.
    items[k] = (x, out, scales, run, inner, group_out, divide): ``out`` float32 [4, *x.shape] receives x * s_k (or the IEEE
    quotient x / s_k) for the four rows s_k of ``scales`` [4, C]; geometry as in :func:`equalize_apply_table`.  x is not
    written."""
    if not items: return
    jobs = np.zeros(len(items), dtype=_SSD_APPLY_JOB)
    dev = items[0][0].device
    for k, (x, out, scales, run, inner, group_out, divide) in enumerate(items):
        _eq_tensor(x, 'Value', k, dev); _eq_tensor(out, 'Out', k, dev); _eq_tensor(scales, 'Scales', k, dev)
        if out.numel() != 4 * x.numel(): raise RuntimeError(_KERNEL_FAILURE + f'SSD apply: item {k}: Out must hold 4 x {x.numel()} floats')
        if scales.numel() % 4: raise RuntimeError(_KERNEL_FAILURE + f'SSD apply: item {k}: Scales must be [4, C]')
        jobs[k] = (x.data_ptr(), out.data_ptr(), scales.data_ptr(), x.numel(), int(run), int(inner), int(group_out),
                   scales.numel() // 4, 1 if divide else 0, 0)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_ssd_apply_multi(jobs.ctypes.data, len(items), _stream()))


def fq_measure_rows_multi(items, sums=None) -> List[torch.Tensor]:
    """The row sums ``[rows, 4]`` of :func:`measure_rows_multi` between ``fake_quant(y)`` and ``r`` for every item, the
    fake-quant done in registers: ONE launch, y and r read once, nothing else written, bit-identical to ``LinearQuantize_T/C``
    into a buffer followed by ``measure_rows_multi``.  items[k] = (y, r, scale, offset, channel_axis, quant_min, quant_max,
    rounding): a linear config, ``channel_axis`` None (per tensor) or 1 (the axis behind the batch axis)."""
    if not items: return []
    dev = items[0][0].device
    if sums is None: sums = [torch.empty([it[0].shape[0], 4], dtype=torch.float64, device=dev) for it in items]
    jobs = np.zeros(len(items), dtype=_FQ_MEASURE_JOB)
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


# ---- error analysis (include/ppq_hip.h ppqhip_fetch_rows_multi / ppqhip_measure_rows_multi / ppqhip_measure_finish_multi) ----
_FETCH_JOB = np.dtype([('x', '<u8'), ('index', '<u8'), ('out', '<u8'), ('rows', '<i8'), ('row_len', '<i8'), ('count', '<i8')])
_MEASURE_JOB = np.dtype([('p', '<u8'), ('r', '<u8'), ('index', '<u8'), ('sums', '<u8'), ('rows', '<i8'), ('row_len', '<i8'),
                         ('count', '<i8')])
_FINISH_JOB = np.dtype([('sums', '<u8'), ('acc', '<u8'), ('row_out', '<u8'), ('rows', '<i8'), ('count', '<i8'),
                        ('method', '<i4'), ('reduce', '<i4')])
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


def fetch_rows_multi(items, outs=None) -> List[torch.Tensor]:
    """``batch_random_fetch`` (ppq/utils/fetch.py:98-122) of every ``(x, index)`` item in ONE launch:
    ``out[b, i] = x[b].flatten()[index[i]]``; ``index`` is a device int32 table with values below ``x[0].numel()``."""
    if not items: return []
    dev = items[0][0].device
    if outs is None: outs = [torch.empty([x.shape[0], index.numel()], dtype=torch.float32, device=dev) for x, index in items]
    jobs = np.zeros(len(items), dtype=_FETCH_JOB)
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
    jobs = np.zeros(len(items), dtype=_MEASURE_JOB)
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
    jobs = np.zeros(len(items), dtype=_FINISH_JOB)
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


# ---- statistical reports (include/ppq_hip.h ppqhip_stat_moments_multi / ppqhip_stat_shape_multi) ----
_STAT_JOB = np.dtype([('p', '<u8'), ('r', '<u8'), ('rec', '<u8'), ('n', '<i8'), ('bins', '<i4'), ('reserved', '<i4')])
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


def _stat_jobs(items, table: torch.Tensor) -> np.ndarray:
    if table.dtype != torch.float32 or not table.is_cuda or not table.is_contiguous() or table.dim() != 2 \
            or table.shape[0] != len(items) or not STAT_WORDS <= table.shape[1] <= STAT_WORDS + STAT_MAX_BINS:
        raise RuntimeError(_KERNEL_FAILURE + f'statistics: Table must be a contiguous float32 [{len(items)}, 8 + bins] tensor on the GPU')
    jobs = np.zeros(len(items), dtype=_STAT_JOB)
    words = table.shape[1]
    for k, (p, r) in enumerate(items):
        _f32(p, 'Series')
        if not p.is_contiguous(): raise RuntimeError(_KERNEL_FAILURE + f'statistics: item {k}: Series is not contiguous')
        if p.device != table.device: raise RuntimeError(_KERNEL_FAILURE + f'statistics: item {k} is on another device')
        if r is not None:
            _f32(r, 'Real')
            if not r.is_contiguous() or r.numel() != p.numel() or r.device != table.device:
                raise RuntimeError(_KERNEL_FAILURE + f'statistics: item {k}: Real must be contiguous, on the same device and as long as Series')
        jobs[k] = (p.data_ptr(), 0 if r is None else r.data_ptr(), table.data_ptr() + 4 * words * k, p.numel(), words - STAT_WORDS, 0)
    return jobs


def stat_moments_multi(items, table: torch.Tensor) -> torch.Tensor:
    """Mean, std (n - 1), min, max of every ``(p, r)`` series in ONE call -- ``r`` None: the series is ``p``, otherwise
    ``p - r`` and the record also gets ``torch_snr_error(p, r)`` -- into words 0..3 and 6 of row k of ``table`` (``stat_table``)."""
    if not items: return table
    jobs = _stat_jobs(items, table)
    with _DeviceOf(table):
        _raise(lib.ppqhip_stat_moments_multi(jobs.ctypes.data, len(items), _stream()))
    return table


def stat_shape_multi(items, table: torch.Tensor) -> torch.Tensor:
    """Skewness, kurtosis and the ``table.shape[1] - 8``-bin histogram of every series from the mean, std, min and max that
    ``stat_moments_multi`` left in ``table`` (read on the device), into words 4, 5 and 8.. of its row.  ONE call."""
    if not items: return table
    jobs = _stat_jobs(items, table)
    with _DeviceOf(table):
        _raise(lib.ppqhip_stat_shape_multi(jobs.ctypes.data, len(items), _stream()))
    return table


class LinearQuantizePlan:
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
    @ staticmethod
    def accepts(value, scale, offset, axis) -> bool:
        """True when the plan can point at these tensors themselves (no layout copy needed)."""
        return _dense(value, axis) is value and scale.is_contiguous() and offset.is_contiguous()

    def __init__(self, items, rounding: int = 0):
        if not items: raise ValueError('LinearQuantizePlan needs at least one item')
        self._keep = []                       # the tensors the device table points at
        dev = items[0][0].device
        total = 0
        for value, scale, offset, axis, qmin, qmax in items:
            _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
            if value.device != dev or scale.device != dev or offset.device != dev:
                raise RuntimeError(_KERNEL_FAILURE + 'LinearQuantizePlan: every tensor must live on one device')
            if not LinearQuantizePlan.accepts(value, scale, offset, axis):
                raise RuntimeError(_KERNEL_FAILURE + 'LinearQuantizePlan: value must be dense in storage order and '
                                   'scale / offset contiguous (a private copy would go stale); see accepts()')
            total += (value.numel() + 3) // 4 * 4
        self._arena = torch.empty(total, dtype=torch.float32, device=dev)
        self._jobs = np.zeros(len(items), dtype=_FQ_JOB)
        self._outs = []
        at = 0
        for k, (value, scale, offset, axis, qmin, qmax) in enumerate(items):
            v = value
            sc, of = scale.reshape(-1), offset.reshape(-1)          # views: accepts() guarantees contiguity
            if axis is None: C, epc = 1, v.numel()
            else: C, epc = _geometry(v.shape, axis)
            if sc.numel() != C or of.numel() != C:
                raise RuntimeError(_KERNEL_FAILURE + f'LinearQuantizePlan: item {k} needs {C} scales / offsets')
            out = self._arena[at: at + v.numel()].as_strided(v.shape, v.stride())     # same memory format as the input
            at += (v.numel() + 3) // 4 * 4          # every output starts 16-B aligned
            self._keep.append((v, sc, of))
            self._outs.append(out)
            self._jobs[k] = (v.data_ptr(), sc.data_ptr(), of.data_ptr(), out.data_ptr(), v.numel(), C, epc, int(qmin), int(qmax))
        self._rounding = int(getattr(rounding, 'value', rounding))
        self._table = torch.empty(int(lib.ppqhip_fq_linear_multi_table_bytes(len(items))), dtype=torch.uint8, device=dev)
        self._uploaded = False
        self.bytes = 8 * sum(v.numel() for v, _, _ in self._keep)

    def run(self) -> List[torch.Tensor]:
        with _DeviceOf(self._arena):
            _raise(lib.ppqhip_fq_linear_multi(self._jobs.ctypes.data, len(self._jobs), self._rounding,
                                              self._table.data_ptr(), 0 if self._uploaded else 1, _stream()))
        self._uploaded = True
        return self._outs


class FloatingQuantizePlan:
    """The FP8 twin of LinearQuantizePlan (``ppqhip_fq_float_multi``): items are
    ``(value, scale, offset, channel_axis | None, exponent, mantissa, clip_min, clip_max)`` sharing a rounding policy --
    the per-channel FP8 weights the TRT_FP8 policy fake-quantises again on every forward (ViT-B/16: 50 of them).
    Values identical to ``CUDA.FloatingQuantize_C`` / ``_T`` per item; same pointer / accepts() rules."""
    accepts = staticmethod(LinearQuantizePlan.accepts)

    def __init__(self, items, rounding: int = 0):
        if not items: raise ValueError('FloatingQuantizePlan needs at least one item')
        self._keep = []
        dev = items[0][0].device
        total = 0
        for value, scale, offset, axis, *_ in items:
            _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
            if value.device != dev or scale.device != dev or offset.device != dev:
                raise RuntimeError(_KERNEL_FAILURE + 'FloatingQuantizePlan: every tensor must live on one device')
            if not self.accepts(value, scale, offset, axis):
                raise RuntimeError(_KERNEL_FAILURE + 'FloatingQuantizePlan: value must be dense in storage order and '
                                   'scale / offset contiguous (a private copy would go stale); see accepts()')
            total += (value.numel() + 3) // 4 * 4
        self._arena = torch.empty(total, dtype=torch.float32, device=dev)
        self._jobs = np.zeros(len(items), dtype=_FQ_FLOAT_JOB)
        self._outs = []
        at = 0
        for k, (v, scale, offset, axis, exponent, mantissa, clip_min, clip_max) in enumerate(items):
            if exponent <= 0: raise ValueError('Floating Quantization requires exponent > 0')          # ffi.py:283
            sc, of = scale.reshape(-1), offset.reshape(-1)
            if axis is None: C, epc = 1, v.numel()
            else: C, epc = _geometry(v.shape, axis)
            if sc.numel() != C or of.numel() != C:
                raise RuntimeError(_KERNEL_FAILURE + f'FloatingQuantizePlan: item {k} needs {C} scales / offsets')
            out = self._arena[at: at + v.numel()].as_strided(v.shape, v.stride())
            at += (v.numel() + 3) // 4 * 4
            self._keep.append((v, sc, of))
            self._outs.append(out)
            self._jobs[k] = (v.data_ptr(), sc.data_ptr(), of.data_ptr(), out.data_ptr(), v.numel(), C, epc, int(exponent),
                             int(mantissa), float(clip_min), float(clip_max))
        self._rounding = int(getattr(rounding, 'value', rounding))
        self._table = torch.empty(int(lib.ppqhip_fq_float_multi_table_bytes(len(items))), dtype=torch.uint8, device=dev)
        self._uploaded = False
        self.bytes = 8 * sum(v.numel() for v, _, _ in self._keep)

    def run(self) -> List[torch.Tensor]:
        with _DeviceOf(self._arena):
            _raise(lib.ppqhip_fq_float_multi(self._jobs.ctypes.data, len(self._jobs), self._rounding,
                                             self._table.data_ptr(), 0 if self._uploaded else 1, _stream()))
        self._uploaded = True
        return self._outs


# ---- OCP Microscaling (include/ppq_hip.h ppqhip_mx_fq / ppqhip_mx_fq_multi) ----
_MX_JOB = np.dtype([('x', '<u8'), ('y', '<u8'), ('scale_codes', '<u8'), ('outer', '<i8'), ('axis_len', '<i8'), ('inner', '<i8'),
                    ('format', '<i4'), ('reserved', '<i4')])
MX_BLOCK = 32
MX_FORMATS = {'MXFP8_E4M3': 0, 'MXFP8_E5M2': 1, 'MXFP6_E3M2': 2, 'MXFP6_E2M3': 3, 'MXFP4_E2M1': 4, 'MXINT8': 5}      # PPQHIP_MX*


def mx_format_id(format) -> int:
    """The library's id of an MX format given as ``ppq_amd.mx.MXFormat``, its name or the id itself."""
    key = getattr(format, 'name', format)
    if isinstance(key, str) and key in MX_FORMATS: return MX_FORMATS[key]
    if isinstance(key, int) and not isinstance(key, bool) and key in MX_FORMATS.values(): return key
    raise ValueError(f'unknown MX format {format!r}: expected one of {", ".join(MX_FORMATS)}')


MX_SCALE_RULES = {'FLOOR': 0, 'CEIL': 1, 'EVEN': 2, 'MSE': 3}      # PPQHIP_MX_FLOOR .. PPQHIP_MX_MSE
MX_RULE_SHIFT = 8                                                   # PPQHIP_MX_RULE_SHIFT


def mx_rule_id(rule) -> int:
    """The library's id of an MX scale rule given as ``ppq_amd.mx.MXScaleRule``, its name or the id itself; None is FLOOR."""
    if rule is None: return MX_SCALE_RULES['FLOOR']
    key = getattr(rule, 'name', rule)
    if isinstance(key, str) and key in MX_SCALE_RULES: return MX_SCALE_RULES[key]
    if isinstance(key, int) and not isinstance(key, bool) and key in MX_SCALE_RULES.values(): return key
    raise ValueError(f'unknown MX scale rule {rule!r}: expected one of {", ".join(MX_SCALE_RULES)}')


def mx_format_arg(format, scale_rule=None) -> int:
    """The ``format`` argument of the entry points that make scales: ``format | rule << 8`` (FLOOR: the format's id as it is)."""
    return mx_format_id(format) | (mx_rule_id(scale_rule) << MX_RULE_SHIFT)


def _mx_item(item):
    """``(value, format, axis)`` or ``(value, format, axis, scale_rule)`` of a plan as (value, format, axis, rule id)."""
    if len(item) not in (3, 4): raise ValueError(f'an MX plan item is (value, format, axis[, scale_rule]), got {len(item)} entries')
    return item[0], item[1], item[2], mx_rule_id(item[3] if len(item) == 4 else None)


def _mx_axis(ndim: int, axis: int) -> int:
    if not isinstance(axis, int) or not -ndim <= axis < ndim:
        raise RuntimeError(_KERNEL_FAILURE + f'axis {axis} out of range for a {ndim}-d tensor')
    return axis % ndim


def _mx_channels_last(t: torch.Tensor, axis: int) -> bool:
    """A dense 4-D channels-last tensor quantised along its channels: the blocks are contiguous in storage as they are."""
    return t.dim() == 4 and axis == 1 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def _mx_geometry(t: torch.Tensor, axis: int):
    """(outer, axis_len, inner) of the storage of ``t`` (contiguous, or channels-last with axis 1) and the shape of its scale codes."""
    shape = list(t.shape)
    codes = shape[:axis] + [(shape[axis] + MX_BLOCK - 1) // MX_BLOCK] + shape[axis + 1:]
    if _mx_channels_last(t, axis): return t.numel() // shape[1], shape[1], 1, codes
    inner = 1
    for d in shape[axis + 1:]: inner *= int(d)
    return t.numel() // (shape[axis] * inner), shape[axis], inner, codes


def _mx_dense(t: torch.Tensor, axis: int) -> torch.Tensor:
    return t if t.is_contiguous() or _mx_channels_last(t, axis) else t.contiguous()


def _mx_codes_like(v: torch.Tensor, axis: int, shape) -> torch.Tensor:
    fmt = torch.channels_last if _mx_channels_last(v, axis) else torch.contiguous_format
    return torch.empty(shape, dtype=torch.uint8, device=v.device, memory_format=fmt)


class MXQuantizePlan:
    """MX fake-quant of MANY tensors with ONE launch per call (``ppqhip_mx_fq_multi``): the MX weights of a graph.  Built once from
    ``(value, format, axis)`` items; ``run()`` re-quantises all of them into one resident arena and returns views shaped like the
    inputs -- bits identical to ``CUDA.MXQuantize`` per item.  The job table travels in the kernel arguments and holds POINTERS to
    the callers' tensors: in-place updates are seen by later runs, a REPLACED tensor needs a new plan.  A value that is not dense
    (contiguous, or 4-D channels-last along axis 1) would need a private copy that later updates never reach: refused
    (``accepts()``).  ``with_codes``: also keep every item's E8M0 scale codes (``codes``).  An item may carry a fourth entry, its
    scale rule (``ppq_amd.mx.MXScaleRule``; default FLOOR): one launch serves any mix of rules and formats."""
    @ staticmethod
    def accepts(value, axis) -> bool:
        return value.dim() > 0 and -value.dim() <= axis < value.dim() and _mx_dense(value, axis % value.dim()) is value

    def __init__(self, items, with_codes: bool = False):
        if not items: raise ValueError('MXQuantizePlan needs at least one item')
        items = [_mx_item(item) for item in items]
        dev = items[0][0].device
        total = 0
        for value, format, axis, _ in items:
            _f32(value, 'Value')
            if value.device != dev: raise RuntimeError(_KERNEL_FAILURE + 'MXQuantizePlan: every tensor must live on one device')
            if not MXQuantizePlan.accepts(value, _mx_axis(value.dim(), axis)):
                raise RuntimeError(_KERNEL_FAILURE + 'MXQuantizePlan: value must be dense in storage order (a private copy would go stale); see accepts()')
            total += (value.numel() + 3) // 4 * 4
        self._arena = torch.empty(total, dtype=torch.float32, device=dev)
        self._jobs = np.zeros(len(items), dtype=_MX_JOB)
        self._keep, self._outs, self.codes = [], [], []
        at = 0
        for k, (v, format, axis, rule) in enumerate(items):
            axis = _mx_axis(v.dim(), axis)
            outer, length, inner, codes_shape = _mx_geometry(v, axis)
            out = self._arena[at: at + v.numel()].as_strided(v.shape, v.stride())     # same memory format as the input
            at += (v.numel() + 3) // 4 * 4                                             # every output starts 16-B aligned
            codes = _mx_codes_like(v, axis, codes_shape) if with_codes else None
            self._keep.append(v); self._outs.append(out); self.codes.append(codes)
            self._jobs[k] = (v.data_ptr(), out.data_ptr(), codes.data_ptr() if with_codes else 0, outer, length, inner,
                             mx_format_arg(format, rule), 0)
        self.bytes = 8 * sum(v.numel() for v in self._keep)

    def run(self) -> List[torch.Tensor]:
        with _DeviceOf(self._arena):
            _raise(lib.ppqhip_mx_fq_multi(self._jobs.ctypes.data, len(self._jobs), _stream()))
        return self._outs


# ---- round tuning on the MX grid (include/ppq_hip.h ppqhip_mx_round_split_multi / ppqhip_mx_round_fwd_multi) ----
_MX_ROUND_SPLIT_JOB = np.dtype([('w', '<u8'), ('floored', '<u8'), ('rounding', '<u8'), ('scale_codes', '<u8'), ('outer', '<i8'),
                                ('axis_len', '<i8'), ('inner', '<i8'), ('format', '<i4'), ('reserved', '<i4')])
_MX_ROUND_FWD_JOB = np.dtype([('floored', '<u8'), ('rounding', '<u8'), ('scale_codes', '<u8'), ('out', '<u8'), ('outer', '<i8'),
                              ('axis_len', '<i8'), ('inner', '<i8'), ('format', '<i4'), ('reserved', '<i4')])


def mx_round_split_multi(items) -> List[tuple]:
    """The split of MX round tuning for every item in ONE launch (``ppqhip_mx_round_split_multi``).  items[k] = ``(w, format, axis)`` or
    ``(w, format, axis, scale_rule)``: ``w`` a float32 CUDA tensor (a non-contiguous one is copied).  Returns
    ``[(floored, rounding, scale_codes)]``: two contiguous float32 tensors shaped like ``w`` and the uint8 E8M0 codes (the axis replaced
    by ceil(len / 32))."""
    if not items: return []
    items = [_mx_item(item) for item in items]
    dev = items[0][0].device
    jobs = np.zeros(len(items), dtype=_MX_ROUND_SPLIT_JOB)
    keep, results = [], []
    for k, (w, format, axis, rule) in enumerate(items):
        _f32(w, 'Value')
        if w.device != dev: raise RuntimeError(_KERNEL_FAILURE + f'MXRoundSplit: item {k} is on another device')
        axis = _mx_axis(w.dim(), axis)
        v = w.detach().contiguous()
        outer, length, inner, codes_shape = _mx_geometry(v, axis)
        floored, rounding = torch.empty_like(v), torch.empty_like(v)
        codes = torch.empty(codes_shape, dtype=torch.uint8, device=dev)
        keep.append(v); results.append((floored, rounding, codes))
        jobs[k] = (v.data_ptr(), floored.data_ptr(), rounding.data_ptr(), codes.data_ptr(), outer, length, inner, mx_format_arg(format, rule), 0)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_mx_round_split_multi(jobs.ctypes.data, len(jobs), _stream()))
    return results


def mx_round_forward_jobs(items, outs) -> np.ndarray:
    """The job table of ``mx_round_forward_multi``: it holds POINTERS, so a caller whose tensors stay where they are (a group
    that is launched every step) builds it once."""
    if len(outs) != len(items): raise RuntimeError(_KERNEL_FAILURE + 'MXRoundForward: argument lists differ in length')
    jobs = np.zeros(len(items), dtype=_MX_ROUND_FWD_JOB)
    dev = items[0][0].device
    for k, (floored, rounding, codes, format, axis) in enumerate(items):
        ts = [('Value', floored), ('Rounding', rounding), ('Out', outs[k])]
        for name, t in ts:
            _f32(t, name)
            if t.device != dev: raise RuntimeError(_KERNEL_FAILURE + f'MXRoundForward: item {k}: {name} is on another device')
            if not t.is_contiguous(): raise RuntimeError(_KERNEL_FAILURE + f'MXRoundForward: item {k}: {name} is not contiguous')
            if t.shape != floored.shape: raise RuntimeError(_KERNEL_FAILURE + f'MXRoundForward: item {k}: {name} is not shaped like the weight')
        axis = _mx_axis(floored.dim(), axis)
        outer, length, inner, codes_shape = _mx_geometry(floored, axis)
        _check(codes, torch.uint8, 'Scale codes(Expect to be UINT8)')
        if list(codes.shape) != codes_shape or not codes.is_contiguous() or codes.device != dev:
            raise RuntimeError(_KERNEL_FAILURE + f'MXRoundForward: item {k}: scale_codes must be a contiguous uint8 tensor of shape {codes_shape} on the weight\'s device')
        jobs[k] = (floored.data_ptr(), rounding.data_ptr(), codes.data_ptr(), outs[k].data_ptr(), outer, length, inner, mx_format_id(format), 0)
    return jobs


def mx_round_forward_multi(items, outs=None, jobs=None) -> List[torch.Tensor]:
    """The forward of MX round tuning for every item in ONE launch (``ppqhip_mx_round_fwd_multi``).  items[k] =
    ``(floored, rounding, scale_codes, format, axis)``: contiguous float32 CUDA tensors of one shape and the uint8 codes of the split;
    ``outs`` (optional, caller-owned) receive the weights; ``jobs``: the table ``mx_round_forward_jobs`` built from the same items and
    outs.  The job table travels in the kernel arguments: capturable.  The backward is the identity: nothing else to launch."""
    if not items: return []
    if outs is None: outs = [torch.empty_like(it[0]) for it in items]
    if jobs is None: jobs = mx_round_forward_jobs(items, outs)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_mx_round_fwd_multi(jobs.ctypes.data, len(jobs), _stream()))
    return outs


# ---- packed MX export (include/ppq_hip.h ppqhip_mx_pack / ppqhip_mx_unpack and their _multi forms) ----
_MX_PACK_JOB = np.dtype([('x', '<u8'), ('elements', '<u8'), ('scales', '<u8'), ('outer', '<i8'), ('axis_len', '<i8'), ('inner', '<i8'),
                         ('format', '<i4'), ('reserved', '<i4')])
_MX_UNPACK_JOB = np.dtype([('elements', '<u8'), ('scales', '<u8'), ('y', '<u8'), ('outer', '<i8'), ('axis_len', '<i8'), ('inner', '<i8'),
                           ('format', '<i4'), ('reserved', '<i4')])
MX_BLOCK_BYTES = {'MXFP8_E4M3': 32, 'MXFP8_E5M2': 32, 'MXFP6_E3M2': 24, 'MXFP6_E2M3': 24, 'MXFP4_E2M1': 16, 'MXINT8': 32}
_MX_BLOCK_BYTES_BY_ID = {MX_FORMATS[k]: v for k, v in MX_BLOCK_BYTES.items()}


def mx_block_bytes(format) -> int:
    """Bytes of one packed block of 32 elements: 32 (MXFP8, MXINT8), 24 (MXFP6), 16 (MXFP4)."""
    return _MX_BLOCK_BYTES_BY_ID[mx_format_id(format)]


def mx_packed_shapes(shape, axis: int, format):
    """(shape of ``elements``, shape of ``scales``) of a tensor of ``shape`` packed along ``axis`` (not negative): the shape without
    the axis, plus [nb * B] resp. [nb] -- the block axis is last."""
    shape = [int(d) for d in shape]
    nb = (shape[axis] + MX_BLOCK - 1) // MX_BLOCK
    lead = shape[:axis] + shape[axis + 1:]
    return lead + [nb * mx_block_bytes(format)], lead + [nb]


def _ptr(t) -> int: return t.data_ptr() if t is not None else 0                          # the address of a tensor, 0 for None


def _mx_operand_args(rank, size, operands, shapes, bias):
    """The operand checks of the MX MFMA bindings at rank 2 (matmul) or 4 (conv).  ``operands``: (name, elements, scales, format id)
    each; ``shapes()``: their logical shapes, packed along axis 1, whose length ``size`` names (``'k'``) -- asked for once dtype,
    rank and device are known.  The bias has one entry per row of the last operand.  Returns the tensors as the kernel takes them,
    [elements, scales] of each operand in turn, the bias and the shapes."""
    dev = operands[0][1].device
    for op, e, s, _ in operands:
        for kind, t in (('elements', e), ('scales', s)):
            if isinstance(t, torch.Tensor) and t.dtype is torch.uint8 and t.is_cuda and t.dim() == rank and t.device == dev and t.numel(): continue
            _check(t, torch.uint8, f'{op} {kind}(Expect to be UINT8)')                   # not the common case: name what is wrong
            if t.dim() != rank: raise RuntimeError(_KERNEL_FAILURE + f'{op} {kind} must be {rank}-d, got {list(t.shape)}')
            if t.device != dev: raise RuntimeError(_KERNEL_FAILURE + f'{op} {kind} is on another device')
    shapes, out = shapes(), []
    for (name, e, s, fmt), shape in zip(operands, shapes):
        eshape, sshape = mx_packed_shapes(shape, 1, fmt)
        if list(e.shape) != eshape or list(s.shape) != sshape:
            raise RuntimeError(_KERNEL_FAILURE + f'{name}: elements / scales of shape {list(e.shape)} / {list(s.shape)}, expected {eshape} / {sshape} for {size} = {shape[1]}')
        e = e.contiguous()
        out += [e.clone() if e.data_ptr() % 16 else e, s.contiguous()]                   # the kernel's 16-byte loads; the allocator aligns
    if bias is not None:
        n = shapes[-1][0]
        _f32(bias, 'Bias')
        if list(bias.shape) != [n]: raise RuntimeError(_KERNEL_FAILURE + f'bias of shape {list(bias.shape)}, expected [{n}]')
        if bias.device != dev: raise RuntimeError(_KERNEL_FAILURE + 'bias is on another device')
        bias = bias.contiguous()
    return out, bias, shapes


def _mx_matmul_args(a_elements, a_scales, a_format, b_elements, b_scales, b_format, k, bias):
    """The checks of ``CUDA.MXMatmul`` / ``MXMatmulFused``; returns the tensors as the kernel takes them, the format ids, k, M and N."""
    fa, fb = mx_format_id(a_format), mx_format_id(b_format)
    k = int(k)
    if k <= 0: raise RuntimeError(_KERNEL_FAILURE + f'k must be positive, got {k}')
    (a_elements, a_scales, b_elements, b_scales), bias, ((m, _), (n, _)) = _mx_operand_args(
        2, 'k', (('A', a_elements, a_scales, fa), ('B', b_elements, b_scales, fb)),
        lambda: ([a_elements.shape[0], k], [b_elements.shape[0], k]), bias)
    return a_elements, a_scales, fa, b_elements, b_scales, fb, k, bias, m, n


def _mx_conv_args(x_elements, x_scales, x_format, w_elements, w_scales, w_format, c, bias, stride, padding, dilation):
    """The checks of ``CUDA.MXConv2d`` / ``MXConv2dFused``; returns the tensors as the kernel takes them, the format ids and
    ``geo = (n, c, h, w, o, kh, kw, sh, sw, ph, pw, dh, dw, oh, ow)``: the entry point's sizes, then the output's."""
    fx, fw = mx_format_id(x_format), mx_format_id(w_format)
    c = int(c)
    if c <= 0: raise RuntimeError(_KERNEL_FAILURE + f'c must be positive, got {c}')
    (x_elements, x_scales, w_elements, w_scales), bias, ((n, _, h, w), (o, _, kh, kw)) = _mx_operand_args(
        4, 'c', (('x', x_elements, x_scales, fx), ('w', w_elements, w_scales, fw)),
        lambda: [[v[0], c, v[1], v[2]] for v in (x_scales.shape, w_scales.shape)], bias)
    (sh, sw), (ph, pw), (dh, dw) = ([int(v) for v in pair] for pair in (stride, padding, dilation))
    if min(sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise RuntimeError(_KERNEL_FAILURE + f'stride {(sh, sw)} and dilation {(dh, dw)} must be at least 1, padding {(ph, pw)} at least 0')
    oh, ow = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if oh < 1 or ow < 1:
        raise RuntimeError(_KERNEL_FAILURE + f'a {kh} x {kw} kernel with dilation {(dh, dw)} does not fit an input of {h} x {w} padded by {(ph, pw)}')
    return x_elements, x_scales, fx, w_elements, w_scales, fw, bias, (n, c, h, w, o, kh, kw, sh, sw, ph, pw, dh, dw, oh, ow)


def _mx_fused_args(out_format, out_float, residual, shape, device):
    """The checks the fused bindings add: returns the id of ``out_format`` (a float format; without one nothing is packed and the id
    is a placeholder) and the residual, float32 of ``shape`` on ``device``."""
    fo = mx_format_id(out_format) if out_format is not None else MX_FORMATS['MXFP8_E4M3']
    if fo == MX_FORMATS['MXINT8']: raise RuntimeError(_KERNEL_FAILURE + 'out_format MXINT8 is not a format the fused epilogue packs')
    if out_format is None and not out_float: raise RuntimeError(_KERNEL_FAILURE + 'no output: out_format is None and out_float is False')
    if residual is not None:
        _f32(residual, 'Residual')
        if list(residual.shape) != list(shape): raise RuntimeError(_KERNEL_FAILURE + f'residual of shape {list(residual.shape)}, expected {list(shape)}')
        if residual.device != device: raise RuntimeError(_KERNEL_FAILURE + 'residual is on another device')
        if len(shape) == 2: residual = residual.contiguous()
    return fo, residual


def _mx_fused_outputs(shape, fo, out_format, out_float, device):
    """The outputs of a fused binding for a result of ``shape`` packed along axis 1: the float32 tensor with that axis last, or
    None, and the packed pair, or None, None."""
    out = torch.empty(shape[:1] + shape[2:] + shape[1:2], dtype=torch.float32, device=device) if out_float else None
    if out_format is None: return out, None, None
    eshape, sshape = mx_packed_shapes(shape, 1, fo)
    return out, torch.empty(eshape, dtype=torch.uint8, device=device), torch.empty(sshape, dtype=torch.uint8, device=device)


class MXPackPlan:
    """The sibling of ``MXQuantizePlan`` for the packed export: MANY tensors packed with ONE launch per call
    (``ppqhip_mx_pack_multi``).  Built once from ``(value, format, axis)`` items; ``run()`` packs all of them into one resident
    uint8 arena (every ``elements`` and every ``scales`` starts 16-B aligned) and returns ``[(elements, scales)]`` -- bytes identical
    to ``CUDA.MXPack`` per item.  The table holds POINTERS to the callers' tensors: in-place updates are seen by later runs; a value
    that is not dense in storage order is refused (``MXQuantizePlan.accepts``).  An item may carry its scale rule as a fourth entry."""
    accepts = staticmethod(MXQuantizePlan.accepts)

    def __init__(self, items):
        if not items: raise ValueError('MXPackPlan needs at least one item')
        items = [_mx_item(item) for item in items]
        dev = items[0][0].device
        geometry, total = [], 0
        for value, format, axis, _ in items:
            _f32(value, 'Value')
            if value.device != dev: raise RuntimeError(_KERNEL_FAILURE + 'MXPackPlan: every tensor must live on one device')
            axis = _mx_axis(value.dim(), axis)
            if not MXQuantizePlan.accepts(value, axis):
                raise RuntimeError(_KERNEL_FAILURE + 'MXPackPlan: value must be dense in storage order (a private copy would go stale); see accepts()')
            eshape, sshape = mx_packed_shapes(value.shape, axis, format)
            geometry.append((axis, eshape, sshape))
            total += (math.prod(eshape) + 15) // 16 * 16 + (math.prod(sshape) + 15) // 16 * 16
        self._arena = torch.empty(total, dtype=torch.uint8, device=dev)
        self._jobs = np.zeros(len(items), dtype=_MX_PACK_JOB)
        self._keep, self._outs = [], []
        at = 0
        for k, ((v, format, _, rule), (axis, eshape, sshape)) in enumerate(zip(items, geometry)):
            outer, length, inner, _ = _mx_geometry(v, axis)
            ne, ns = math.prod(eshape), math.prod(sshape)
            elements = self._arena[at: at + ne].view(eshape)
            at += (ne + 15) // 16 * 16
            scales = self._arena[at: at + ns].view(sshape)
            at += (ns + 15) // 16 * 16
            self._keep.append(v); self._outs.append((elements, scales))
            self._jobs[k] = (v.data_ptr(), elements.data_ptr(), scales.data_ptr(), outer, length, inner, mx_format_arg(format, rule), 0)
        self.bytes = sum(4 * v.numel() + e.numel() + s.numel() for v, (e, s) in zip(self._keep, self._outs))

    def run(self):
        with _DeviceOf(self._arena):
            _raise(lib.ppqhip_mx_pack_multi(self._jobs.ctypes.data, len(self._jobs), _stream()))
        return self._outs


def mx_unpack_multi(items) -> None:
    """``ppqhip_mx_unpack_multi``: every ``(elements, scales, y, format, axis)`` item in ONE call (one launch per 40 live jobs).
    ``y`` is the float32 tensor the packed pair unpacks INTO, dense in storage order (``MXQuantizePlan.accepts``); nothing is
    copied, the library checks pointers, sizes and overlaps."""
    if not items: return
    jobs = np.zeros(len(items), dtype=_MX_UNPACK_JOB)
    for k, (elements, scales, y, format, axis) in enumerate(items):
        if y.numel() == 0:                                                                # an empty job: sizes 0, nothing launched for it
            jobs[k]['format'] = mx_format_id(format)
            continue
        _check(elements, torch.uint8, 'Elements(Expect to be UINT8)'); _check(scales, torch.uint8, 'Scales(Expect to be UINT8)'); _f32(y, 'Out')
        axis = _mx_axis(y.dim(), axis)
        if not MXQuantizePlan.accepts(y, axis): raise RuntimeError(_KERNEL_FAILURE + f'mx_unpack_multi: item {k}: Out must be dense in storage order')
        outer, length, inner, _ = _mx_geometry(y, axis)
        jobs[k] = (elements.data_ptr(), scales.data_ptr(), y.data_ptr(), outer, length, inner, mx_format_id(format), 0)
    with _DeviceOf(items[0][0]):
        _raise(lib.ppqhip_mx_unpack_multi(jobs.ctypes.data, len(jobs), _stream()))


class _HipExtension:
    """Same callables as the pybind module built from ppq/csrc/export.cc:8-34."""
    __name__ = 'PPQ_Hip_Impls'

    # ---- linear ------------------------------------------------------------------------------
    @ staticmethod
    def QuantizeTensor_LT(value, scale, offset, clip_min: int, clip_max: int, rounding: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
        v = _dense(value)
        out = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_linear_t(v.data_ptr(), scale.data_ptr(), offset.data_ptr(), out.data_ptr(),
                                          v.numel(), int(clip_min), int(clip_max), int(rounding), _stream()))
        return out

    @ staticmethod
    def QuantizeTensor_LC(value, scale, offset, clip_min: int, clip_max: int, channel_axis: int,
                          rounding: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
        v = _dense(value, channel_axis)
        C, epc = _geometry(v.shape, channel_axis)
        if scale.numel() < C or offset.numel() < C:
            raise RuntimeError(_KERNEL_FAILURE + f'scale/offset need {C} elements for channel axis {channel_axis}')
        out = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_linear_c(v.data_ptr(), scale.contiguous().data_ptr(), offset.contiguous().data_ptr(),
                                          out.data_ptr(), v.numel(), C, epc, int(clip_min), int(clip_max),
                                          int(rounding), _stream()))
        return out

    @ staticmethod
    def QuantizeTensor_ToInt(value, scale, offset, clip_min: int, clip_max: int, rounding: int, channel_axis,
                             dtype: torch.dtype) -> torch.Tensor:
        """PPQLinearQuant_toInt's arithmetic (qfunction/linear.py:218-238) as one kernel: quantise only, integer output
        (``dtype``: torch.int8 / torch.uint8 / torch.int32), element order of ``value.contiguous()``."""
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
        code = {torch.int8: 0, torch.uint8: 1, torch.int32: 2}.get(dtype)
        if code is None: raise RuntimeError(_KERNEL_FAILURE + f'unsupported integer dtype {dtype}')
        v = value.contiguous()
        out = torch.empty(v.shape, dtype=dtype, device=v.device)
        sc, of = scale.contiguous(), offset.contiguous()
        with _DeviceOf(v):
            if channel_axis is None:
                _raise(lib.ppqhip_to_int_t(v.data_ptr(), sc.data_ptr(), of.data_ptr(), out.data_ptr(), v.numel(), int(clip_min),
                                           int(clip_max), int(rounding), code, _stream()))
            else:
                C, epc = _geometry(v.shape, channel_axis)
                if sc.numel() < C or of.numel() < C:
                    raise RuntimeError(_KERNEL_FAILURE + f'scale/offset need {C} elements for channel axis {channel_axis}')
                _raise(lib.ppqhip_to_int_c(v.data_ptr(), sc.data_ptr(), of.data_ptr(), out.data_ptr(), v.numel(), C, epc,
                                           int(clip_min), int(clip_max), int(rounding), code, _stream()))
        return out

    @ staticmethod
    def QuantizeTensor_LT_B(value, scale, offset, grad_y, clip_min: int, clip_max: int,
                            rounding: int) -> List[torch.Tensor]:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset'); _f32(grad_y, 'Gard')
        v = value.contiguous(); g = grad_y.contiguous()
        grad_x = torch.empty_like(g); grad_s = torch.empty_like(scale)
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_linear_t_bwd(v.data_ptr(), scale.data_ptr(), offset.data_ptr(), g.data_ptr(),
                                              grad_x.data_ptr(), grad_s.data_ptr(), v.numel(), int(clip_min),
                                              int(clip_max), int(rounding), _stream()))
        return [grad_x, grad_s]

    @ staticmethod
    def lsq_t_partials(numel: int) -> int:
        """Floats ``QuantizeTensor_LT_B_Main`` writes into ``partial`` for a tensor of ``numel`` elements."""
        return int(lib.ppqhip_fq_linear_t_bwd_partials(int(numel)))

    @ staticmethod
    def QuantizeTensor_LT_B_Main(value, scale, offset, grad_y, clip_min: int, clip_max: int, rounding: int, partial) -> torch.Tensor:
        """First half of ``QuantizeTensor_LT_B`` (``ppqhip_fq_linear_t_bwd_main``): returns grad_x and leaves the per-workgroup
        partial sums of the scale gradient in the caller-owned float32 ``partial`` (>= ``lsq_t_partials(numel)`` elements);
        ``LSQ_Finish_Multi`` turns the partials of many tensors into their grad_s in ONE launch."""
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset'); _f32(grad_y, 'Gard'); _f32(partial, 'Partial')
        v = value.contiguous(); g = grad_y.contiguous()
        if partial.numel() < int(lib.ppqhip_fq_linear_t_bwd_partials(v.numel())) or not partial.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + 'QuantizeTensor_LT_B_Main: partial is too small (see lsq_t_partials)')
        grad_x = torch.empty_like(g)
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_linear_t_bwd_main(v.data_ptr(), scale.data_ptr(), offset.data_ptr(), g.data_ptr(), grad_x.data_ptr(),
                                                   partial.data_ptr(), v.numel(), int(clip_min), int(clip_max), int(rounding), _stream()))
        return grad_x

    @ staticmethod
    def LSQ_Finish_Multi(partials, numels, clip_mins, clip_maxs, grad_ss) -> None:
        """Second half for MANY tensors (``ppqhip_lsq_finish_multi``): ``grad_ss[k][0]`` = the scale gradient of tensor k, bit
        for bit what ``QuantizeTensor_LT_B`` returns."""
        n = len(partials)
        if n == 0: return
        if not (len(numels) == len(clip_mins) == len(clip_maxs) == len(grad_ss) == n):
            raise RuntimeError(_KERNEL_FAILURE + 'LSQ_Finish_Multi: argument lists differ in length')
        jobs = np.empty(n, dtype=_LSQ_FINISH_JOB)
        for k in range(n):
            _f32(partials[k], 'Partial'); _f32(grad_ss[k], 'Grad_s')
            if partials[k].device != partials[0].device or grad_ss[k].device != partials[0].device:
                raise RuntimeError(_KERNEL_FAILURE + 'LSQ_Finish_Multi: one device per call')
            if partials[k].numel() < int(lib.ppqhip_fq_linear_t_bwd_partials(int(numels[k]))) or grad_ss[k].numel() < 1:
                raise RuntimeError(_KERNEL_FAILURE + f'LSQ_Finish_Multi: item {k}: partial / grad_s too small')
            jobs[k] = (partials[k].data_ptr(), grad_ss[k].data_ptr(), int(numels[k]), int(clip_mins[k]), int(clip_maxs[k]))
        with _DeviceOf(partials[0]):
            _raise(lib.ppqhip_lsq_finish_multi(jobs.ctypes.data, n, _stream()))

    @ staticmethod
    def QuantizeTensor_LC_B(value, scale, offset, grad_y, clip_min: int, clip_max: int, rounding: int,
                            channel_axis: int) -> List[torch.Tensor]:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset'); _f32(grad_y, 'Gard')
        v = value.contiguous(); g = grad_y.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        grad_x = torch.empty_like(g); grad_s = torch.empty_like(scale.contiguous())
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_linear_c_bwd(v.data_ptr(), scale.contiguous().data_ptr(),
                                              offset.contiguous().data_ptr(), g.data_ptr(), grad_x.data_ptr(),
                                              grad_s.data_ptr(), v.numel(), C, epc, int(clip_min), int(clip_max),
                                              int(rounding), _stream()))
        return [grad_x, grad_s]

    @ staticmethod
    def QuantizeTensor_LC_B_Multi(values, scales, offsets, grad_ys, clip_mins, clip_maxs, rounding: int, channel_axes,
                                  grad_xs=None, grad_ss=None):
        """``QuantizeTensor_LC_B`` for MANY per-channel tensors in ONE launch (``ppqhip_fq_linear_c_bwd_multi``): all the
        weights of a block in a block-wise LSQ step.  Returns ``(grad_xs, grad_ss)``; pass preallocated lists to have them
        written in place (they are what the caller installs as ``.grad``).  Per item the results are those of
        ``QuantizeTensor_LC_B`` (grad_x bit for bit; grad_s bit for bit when the per-tensor path itself sums in a fixed
        order, see include/ppq_hip.h)."""
        n = len(values)
        if n == 0: return [], []
        if not (len(scales) == len(offsets) == len(grad_ys) == len(clip_mins) == len(clip_maxs) == len(channel_axes) == n):
            raise RuntimeError(_KERNEL_FAILURE + 'QuantizeTensor_LC_B_Multi: argument lists differ in length')
        dev = values[0].device
        jobs = np.empty(n, dtype=_LSQ_JOB)
        keep, gxs, gss = [], [], []
        for k in range(n):
            _f32(values[k], 'Value'); _f32(scales[k], 'Scale'); _f32(offsets[k], 'Offset'); _f32(grad_ys[k], 'Gard')
            if values[k].device != dev or grad_ys[k].device != dev:
                raise RuntimeError(_KERNEL_FAILURE + 'QuantizeTensor_LC_B_Multi: one device per call')
            v = values[k].contiguous(); g = grad_ys[k].contiguous()
            sc, of = scales[k].contiguous(), offsets[k].contiguous()
            C, epc = _geometry(v.shape, channel_axes[k])
            if sc.numel() != C or of.numel() != C:
                raise RuntimeError(_KERNEL_FAILURE + f'QuantizeTensor_LC_B_Multi: item {k} needs {C} scales / offsets')
            gx = torch.empty_like(g) if grad_xs is None else grad_xs[k]
            gs = torch.empty_like(sc) if grad_ss is None else grad_ss[k]
            if grad_xs is not None and (gx.shape != g.shape or not gx.is_contiguous() or gx.dtype != _F32):
                raise RuntimeError(_KERNEL_FAILURE + f'QuantizeTensor_LC_B_Multi: grad_xs[{k}] must be a contiguous float32 tensor shaped like the value')
            if grad_ss is not None and (gs.numel() != C or not gs.is_contiguous() or gs.dtype != _F32):
                raise RuntimeError(_KERNEL_FAILURE + f'QuantizeTensor_LC_B_Multi: grad_ss[{k}] must be a contiguous float32[{C}]')
            keep.append((v, g, sc, of)); gxs.append(gx); gss.append(gs)
            jobs[k] = (v.data_ptr(), sc.data_ptr(), of.data_ptr(), g.data_ptr(), gx.data_ptr(), gs.data_ptr(), v.numel(), C, epc,
                       int(clip_mins[k]), int(clip_maxs[k]))
        with _DeviceOf(values[0]):
            _raise(lib.ppqhip_fq_linear_c_bwd_multi(jobs.ctypes.data, n, int(rounding), _stream()))
        return gxs, gss

    # ---- floating ----------------------------------------------------------------------------
    @ staticmethod
    def QuantizeTensor_FT(value, scale, offset, exponent: int, mantissa: int, clip_min: float, clip_max: float,
                          rounding: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
        v = _dense(value)
        out = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_float_t(v.data_ptr(), scale.data_ptr(), offset.data_ptr(), out.data_ptr(),
                                         v.numel(), int(exponent), int(mantissa), float(clip_min), float(clip_max),
                                         int(rounding), _stream()))
        return out

    @ staticmethod
    def QuantizeTensor_FC(value, scale, offset, exponent: int, mantissa: int, clip_min: float, clip_max: float,
                          channel_axis: int, rounding: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
        v = value.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        out = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_float_c(v.data_ptr(), scale.contiguous().data_ptr(), offset.contiguous().data_ptr(),
                                         out.data_ptr(), v.numel(), C, epc, int(exponent), int(mantissa),
                                         float(clip_min), float(clip_max), int(rounding), _stream()))
        return out

    @ staticmethod
    def QuantizeTensor_FT_B(value, scales, offsets, grad_y, exponent: int, mantissa: int, clip_min: float,
                            clip_max: float, rounding: int) -> List[torch.Tensor]:
        _f32(value, 'Value'); _f32(scales, 'Scale'); _f32(offsets, 'Offset'); _f32(grad_y, 'Gard')
        v = value.contiguous(); g = grad_y.contiguous()
        grad_x = torch.empty_like(g); grad_s = torch.empty_like(scales)
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_float_c_bwd(v.data_ptr(), scales.data_ptr(), offsets.data_ptr(), g.data_ptr(),
                                             grad_x.data_ptr(), grad_s.data_ptr(), v.numel(), 1, v.numel(),
                                             int(exponent), int(mantissa), float(clip_min), float(clip_max),
                                             int(rounding), _stream()))
        return [grad_x, grad_s]

    @ staticmethod
    def QuantizeTensor_FC_B(value, scales, offsets, grad_y, exponent: int, mantissa: int, clip_min: float,
                            clip_max: float, rounding: int, channel_axis: int) -> List[torch.Tensor]:
        _f32(value, 'Value'); _f32(scales, 'Scale'); _f32(offsets, 'Offset'); _f32(grad_y, 'Gard')
        v = value.contiguous(); g = grad_y.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        grad_x = torch.empty_like(g); grad_s = torch.empty_like(scales.contiguous())
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_float_c_bwd(v.data_ptr(), scales.contiguous().data_ptr(),
                                             offsets.contiguous().data_ptr(), g.data_ptr(), grad_x.data_ptr(),
                                             grad_s.data_ptr(), v.numel(), C, epc, int(exponent), int(mantissa),
                                             float(clip_min), float(clip_max), int(rounding), _stream()))
        return [grad_x, grad_s]

    # ---- histograms / order statistics -------------------------------------------------------
    @ staticmethod
    def _check_hist(hist):
        _check(hist, torch.int32, 'Histogram(Expect to be INT32)')
        if not hist.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + 'Histogram must be contiguous (it is accumulated in place)')

    @ staticmethod
    def Histogram_T(value, hist_scale: float, clip_outliers: bool, hist) -> None:
        _f32(value, 'Value'); _HipExtension._check_hist(hist)
        v = _dense(value)
        with _DeviceOf(v):
            ws = _workspace(v.device, lib.ppqhip_hist_workspace_bytes(v.numel(), hist.numel()))
            _raise(lib.ppqhip_hist_sym_t(v.data_ptr(), v.numel(), float(hist_scale), int(bool(clip_outliers)),
                                         hist.data_ptr(), hist.numel(), ws.data_ptr(), _stream()))

    @ staticmethod
    def Histogram_Asymmetric_T(min: float, max: float, value, clip_outliers: bool, hist) -> None:
        _f32(value, 'Value'); _HipExtension._check_hist(hist)
        v = _dense(value)
        with _DeviceOf(v):
            ws = _workspace(v.device, lib.ppqhip_hist_workspace_bytes(v.numel(), hist.numel()))
            _raise(lib.ppqhip_hist_asym_t(v.data_ptr(), v.numel(), float(min), float(max),
                                          int(bool(clip_outliers)), hist.data_ptr(), hist.numel(), ws.data_ptr(),
                                          _stream()))

    @ staticmethod
    def Histogram_C(value, channel_axis: int, hist_scale: float, clip_outliers: bool, hist) -> None:
        _f32(value, 'Value'); _HipExtension._check_hist(hist)
        v = value.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        if hist.numel() % C != 0:
            raise RuntimeError(_KERNEL_FAILURE + 'Histogram shape is invalid.')
        with _DeviceOf(v):
            _raise(lib.ppqhip_hist_sym_c(v.data_ptr(), v.numel(), C, epc, float(hist_scale),
                                         int(bool(clip_outliers)), hist.data_ptr(), hist.numel() // C, _stream()))

    @ staticmethod
    def Histogram_C_Scales(value, channel_axis: int, hist_scales, clip_outliers: bool, hist) -> None:
        """Per-channel histogram with one hist_scale per channel (device float32 [C]); hist int32 [C, bins]."""
        _f32(value, 'Value'); _f32(hist_scales, 'Hist scales'); _HipExtension._check_hist(hist)
        v = value.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        if hist.numel() % C != 0 or hist_scales.numel() != C or not hist.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + 'Histogram shape is invalid.')
        with _DeviceOf(v):
            _raise(lib.ppqhip_hist_sym_c_scales(v.data_ptr(), v.numel(), C, epc, hist_scales.contiguous().data_ptr(),
                                                int(bool(clip_outliers)), hist.data_ptr(), hist.numel() // C, _stream()))

    @ staticmethod
    def Histogram_Asymmetric_C_Ranges(value, channel_axis: int, mins, maxs, clip_outliers: bool, hist) -> None:
        """Per-channel asymmetric histogram, one (min, max) per channel (device float32 [C]); hist int32 [C, bins]."""
        _f32(value, 'Value'); _f32(mins, 'Mins'); _f32(maxs, 'Maxs'); _HipExtension._check_hist(hist)
        v = value.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        if hist.numel() % C != 0 or mins.numel() != C or maxs.numel() != C:
            raise RuntimeError(_KERNEL_FAILURE + 'Histogram shape is invalid.')
        with _DeviceOf(v):
            _raise(lib.ppqhip_hist_asym_c_ranges(v.data_ptr(), v.numel(), C, epc, mins.contiguous().data_ptr(),
                                                 maxs.contiguous().data_ptr(), int(bool(clip_outliers)), hist.data_ptr(),
                                                 hist.numel() // C, _stream()))

    @ staticmethod
    def Quantile_T(source, q: float, hint='auto') -> torch.Tensor:
        """``hint``: 'auto' (the hint of the declared owner of this call, ``quantile_hint_owner``; none declared -> None),
        None (stateless: every call estimates its thresholds from a sample), or an int32[8] device tensor from
        ``quantile_hint`` owned by the caller."""
        _f32(source, 'Value')
        v = _dense(source)
        dest = torch.empty(2, dtype=torch.float32, device=v.device)
        if isinstance(hint, str): hint = _owner_quantile_hint(v.device, v.numel(), q)
        with _DeviceOf(v):
            ws = _workspace(v.device, lib.ppqhip_quantile_workspace_bytes(v.numel()))
            _raise(lib.ppqhip_quantile_t(v.data_ptr(), v.numel(), float(q), dest.data_ptr(),
                                         _HipExtension._hint_ptr(hint, v.device), ws.data_ptr(), _stream()))
        return dest

    @ staticmethod
    def _hint_ptr(hint, device) -> int:
        if hint is None: return 0
        if hint.dtype != torch.int32 or hint.numel() != 8 or not hint.is_contiguous() or hint.device != device:
            raise RuntimeError(_KERNEL_FAILURE + 'a quantile hint is a contiguous int32[8] on the tensor\'s device')
        return hint.data_ptr()

    @ staticmethod
    def Quantile_T_Multi(sources, q: float, dests=None, hints=None) -> list:
        """One launch sequence for many tensors; each result as Quantile_T.  ``dests``: optional list of
        preallocated float32[2] device tensors to fill; ``hints``: optional list (entries may be None) of
        ``quantile_hint`` tensors, one per source."""
        if not sources: return []
        vs = []
        for v in sources:
            _f32(v, 'Value')
            if v.device != sources[0].device: raise RuntimeError(_KERNEL_FAILURE + 'Quantile_T_Multi: one device per call')
            vs.append(_dense(v))
        if dests is None: dests = [torch.empty(2, dtype=torch.float32, device=vs[0].device) for _ in vs]
        if len(dests) != len(vs): raise RuntimeError(_KERNEL_FAILURE + 'sources / dests length mismatch')
        for d in dests:
            _f32(d, 'Dest')
            if d.numel() != 2 or not d.is_contiguous(): raise RuntimeError(_KERNEL_FAILURE + 'dest must be a contiguous float32[2]')
        if hints is None: hints = [None] * len(vs)
        if len(hints) != len(vs): raise RuntimeError(_KERNEL_FAILURE + 'sources / hints length mismatch')
        jobs = np.empty(len(vs), dtype=_QUANTILE_JOB)
        jobs['x'] = [v.data_ptr() for v in vs]
        jobs['dest'] = [d.data_ptr() for d in dests]
        jobs['hint'] = [_HipExtension._hint_ptr(h, vs[0].device) for h in hints]
        jobs['n'] = [v.numel() for v in vs]
        with _DeviceOf(vs[0]):
            ws = _workspace(vs[0].device, lib.ppqhip_quantile_multi_workspace_bytes(len(vs), sum(v.numel() for v in vs)))
            _raise(lib.ppqhip_quantile_t_multi(jobs.ctypes.data, len(vs), float(q), ws.data_ptr(), _stream()))
        return dests

    @ staticmethod
    def Isotone_T(source) -> torch.Tensor:
        _f32(source, 'Value')
        v = source.contiguous()
        dest = torch.empty(4, dtype=torch.float32, device=v.device)
        with _DeviceOf(v):
            ws = _workspace(v.device, lib.ppqhip_quantile_workspace_bytes(v.numel()))
            _raise(lib.ppqhip_isotone_t(v.data_ptr(), v.numel(), dest.data_ptr(), ws.data_ptr(), _stream()))
        return dest

    # ---- training helpers (no caller in ppq) --------------------------------------------------
    @ staticmethod
    def TensorClip_T(value, reference, limit) -> torch.Tensor:
        _f32(value, 'Value'); _f32(reference, 'Reference'); _f32(limit, 'Limit')
        v = value.contiguous(); r = reference.contiguous()
        out = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_tensor_clip_t(v.data_ptr(), r.data_ptr(), limit.data_ptr(), out.data_ptr(), v.numel(),
                                            _stream()))
        return out

    @ staticmethod
    def TensorClip_C(value, reference, limit, channel_axis: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(reference, 'Reference'); _f32(limit, 'Limit')
        v = value.contiguous(); r = reference.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        out = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_tensor_clip_c(v.data_ptr(), r.data_ptr(), limit.contiguous().data_ptr(), out.data_ptr(),
                                            v.numel(), C, epc, _stream()))
        return out

    @ staticmethod
    def RoundingLoss_LT(value, scale, offset, clip_min: int, clip_max: int, rounding: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
        v = value.contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=v.device)
        with _DeviceOf(v):
            _raise(lib.ppqhip_rounding_loss(v.data_ptr(), scale.data_ptr(), offset.data_ptr(), loss.data_ptr(),
                                            v.numel(), 0, 1, int(clip_min), int(clip_max), int(rounding), _stream()))
        return loss

    @ staticmethod
    def RoundingLoss_LC(value, scale, offset, clip_min: int, clip_max: int, channel_axis: int,
                        rounding: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
        v = value.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        loss = torch.empty(1, dtype=torch.float32, device=v.device)
        with _DeviceOf(v):
            _raise(lib.ppqhip_rounding_loss(v.data_ptr(), scale.contiguous().data_ptr(),
                                            offset.contiguous().data_ptr(), loss.data_ptr(), v.numel(), C, epc,
                                            int(clip_min), int(clip_max), int(rounding), _stream()))
        return loss

    @ staticmethod
    def RoundingLoss_LT_B(value, dy, scale, offset, clip_min: int, clip_max: int, rounding: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset'); _f32(dy, 'Gard')
        v = value.contiguous()
        dx = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_rounding_loss_bwd(v.data_ptr(), dy.data_ptr(), scale.data_ptr(), offset.data_ptr(),
                                                dx.data_ptr(), v.numel(), 0, 1, int(clip_min), int(clip_max),
                                                int(rounding), _stream()))
        return dx

    @ staticmethod
    def RoundingLoss_LC_B(value, dy, scale, offset, clip_min: int, clip_max: int, channel_axis: int,
                          rounding: int) -> torch.Tensor:
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset'); _f32(dy, 'Gard')
        v = value.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        dx = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_rounding_loss_bwd(v.data_ptr(), dy.data_ptr(), scale.contiguous().data_ptr(),
                                                offset.contiguous().data_ptr(), dx.data_ptr(), v.numel(), C, epc,
                                                int(clip_min), int(clip_max), int(rounding), _stream()))
        return dx

    @ staticmethod
    def compute_mse_loss(hist: list, start: int, step: int, end: int) -> float:
        import ctypes
        arr = (ctypes.c_int64 * len(hist))(*[int(v) for v in hist])
        return float(lib.ppqhip_mse_loss_host(arr, len(hist), int(start), int(step), int(end)))

    # ---- MI355X-native additions (no twin in export.cc) -----------------------------------------
    @ staticmethod
    def MinMax_T(value, minmax) -> None:
        """minmax: float32[2] on the GPU, accumulated in place; seed with [+inf, -inf]."""
        _f32(value, 'Value'); _f32(minmax, 'MinMax')
        v = _dense(value)
        with _DeviceOf(v):
            ws = _workspace(v.device, lib.ppqhip_minmax_workspace_bytes(v.numel()))
            _raise(lib.ppqhip_minmax_t(v.data_ptr(), v.numel(), minmax.data_ptr(), ws.data_ptr(), _stream()))

    @ staticmethod
    def MinMax_T_Slots(value, slots) -> None:
        """slots: float32 [minmax_slots(), 2] seeded with (+inf, -inf); one slot per workgroup, no
        per-launch reduction.  Fold with MinMax_Slots_Finish when the range is needed."""
        _f32(value, 'Value'); _f32(slots, 'Slots')
        if slots.numel() != 2 * lib.ppqhip_minmax_slots() or not slots.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + f'slots must be a contiguous [{lib.ppqhip_minmax_slots()}, 2] tensor')
        v = _dense(value)
        with _DeviceOf(v):
            _raise(lib.ppqhip_minmax_t_slots(v.data_ptr(), v.numel(), slots.data_ptr(), _stream()))

    @ staticmethod
    def MinMax_T_Slots_Multi(values, slots) -> None:
        """One launch for many (value, slots) pairs; each pair as MinMax_T_Slots.  All on one device."""
        if len(values) != len(slots): raise RuntimeError(_KERNEL_FAILURE + 'values / slots length mismatch')
        if not values: return
        S = 2 * lib.ppqhip_minmax_slots()
        vs = []
        for v, sl in zip(values, slots):
            _f32(v, 'Value'); _f32(sl, 'Slots')
            if sl.numel() != S or not sl.is_contiguous() or sl.device != values[0].device or v.device != values[0].device:
                raise RuntimeError(_KERNEL_FAILURE + 'slots must be contiguous [minmax_slots(), 2] tensors on the values\' device')
            vs.append(_dense(v))
        jobs = np.empty(len(vs), dtype=_MINMAX_JOB)
        jobs['x'] = [v.data_ptr() for v in vs]
        jobs['slots'] = [sl.data_ptr() for sl in slots]
        jobs['n'] = [v.numel() for v in vs]
        with _DeviceOf(vs[0]):
            _raise(lib.ppqhip_minmax_t_slots_multi(jobs.ctypes.data, len(vs), _stream()))

    @ staticmethod
    def Histogram_T_Rows_Multi(values, rows, p0, p1, asymmetric: bool, clip_outliers: bool) -> None:
        """One launch for many (value, rows) pairs sharing the bin count: symmetric jobs take
        p0 = hist_scale, asymmetric ones p0 = min, p1 = max; each pair as Histogram_[Asymmetric_]T_Rows."""
        if not (len(values) == len(rows) == len(p0)) or (asymmetric and len(p1) != len(values)):
            raise RuntimeError(_KERNEL_FAILURE + 'values / rows / parameter length mismatch')
        if not values: return
        R, bins = lib.ppqhip_hist_rows(), rows[0].shape[-1]
        vs = []
        for v, r in zip(values, rows):
            _f32(v, 'Value'); _check(r, torch.int32, 'Rows(Expect to be INT32)')
            if (r.ndim != 2 or r.shape[0] != R or r.shape[1] != bins or not r.is_contiguous()
                    or r.device != values[0].device or v.device != values[0].device):
                raise RuntimeError(_KERNEL_FAILURE + f'rows must be contiguous [{R}, {bins}] tensors on the values\' device')
            vs.append(_dense(v))
        jobs = np.empty(len(vs), dtype=_HIST_JOB)
        jobs['x'] = [v.data_ptr() for v in vs]
        jobs['rows'] = [r.data_ptr() for r in rows]
        jobs['n'] = [v.numel() for v in vs]
        jobs['p0'] = np.asarray(p0, dtype=np.float32)
        jobs['p1'] = np.asarray(p1, dtype=np.float32) if asymmetric else 0.0
        with _DeviceOf(vs[0]):
            _raise(lib.ppqhip_hist_t_rows_multi(jobs.ctypes.data, len(vs), int(bool(asymmetric)),
                                                int(bool(clip_outliers)), bins, _stream()))

    @ staticmethod
    def MinMax_Slots_Finish(slots, minmax) -> None:
        _f32(slots, 'Slots'); _f32(minmax, 'MinMax')
        with _DeviceOf(slots):
            _raise(lib.ppqhip_minmax_slots_finish(slots.data_ptr(), minmax.data_ptr(), _stream()))

    @ staticmethod
    def Histogram_T_Rows(value, hist_scale: float, clip_outliers: bool, rows) -> None:
        """rows: int32 [hist_rows(), bins], zero-initialised; see include/ppq_hip.h."""
        _f32(value, 'Value'); _check(rows, torch.int32, 'Rows(Expect to be INT32)')
        R = lib.ppqhip_hist_rows()
        if rows.ndim != 2 or rows.shape[0] != R or not rows.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + f'rows must be a contiguous [{R}, bins] tensor')
        v = _dense(value)
        with _DeviceOf(v):
            _raise(lib.ppqhip_hist_sym_t_rows(v.data_ptr(), v.numel(), float(hist_scale), int(bool(clip_outliers)),
                                              rows.data_ptr(), rows.shape[1], _stream()))

    @ staticmethod
    def Histogram_Asymmetric_T_Rows(min: float, max: float, value, clip_outliers: bool, rows) -> None:
        _f32(value, 'Value'); _check(rows, torch.int32, 'Rows(Expect to be INT32)')
        R = lib.ppqhip_hist_rows()
        if rows.ndim != 2 or rows.shape[0] != R or not rows.is_contiguous():
            raise RuntimeError(_KERNEL_FAILURE + f'rows must be a contiguous [{R}, bins] tensor')
        v = _dense(value)
        with _DeviceOf(v):
            _raise(lib.ppqhip_hist_asym_t_rows(v.data_ptr(), v.numel(), float(min), float(max),
                                               int(bool(clip_outliers)), rows.data_ptr(), rows.shape[1], _stream()))

    @ staticmethod
    def Histogram_Rows_Finish(rows, hist) -> None:
        _check(rows, torch.int32, 'Rows(Expect to be INT32)'); _HipExtension._check_hist(hist)
        with _DeviceOf(rows):
            _raise(lib.ppqhip_hist_rows_finish(rows.data_ptr(), rows.shape[1], hist.data_ptr(), _stream()))

    @ staticmethod
    def MinMax_C(value, channel_axis: int, mins, maxs) -> None:
        _f32(value, 'Value'); _f32(mins, 'Mins'); _f32(maxs, 'Maxs')
        v = _dense(value, channel_axis)
        C, epc = _geometry(v.shape, channel_axis)
        if mins.numel() != C or maxs.numel() != C:
            raise RuntimeError(_KERNEL_FAILURE + f'mins / maxs need {C} elements')
        with _DeviceOf(v):
            _raise(lib.ppqhip_minmax_c(v.data_ptr(), v.numel(), C, epc, mins.data_ptr(), maxs.data_ptr(), _stream()))

    @ staticmethod
    def MinMax_C_Multi(values, channel_axes, mins, maxs, fresh: bool = False):
        """``MinMax_C`` for MANY tensors in ONE launch (``ppqhip_minmax_c_multi``): every weight ParameterQuantizePass observes.
        ``mins[k]`` / ``maxs[k]``: contiguous float32[C_k]; accumulated into (seed with +-inf) unless ``fresh``: then they are
        OVERWRITTEN, allowed for tensors whose channel axis is the outermost one with at most 8192 elements per channel
        (one wave per channel; ``minmax_c_fresh_ok``).  ``fresh`` may be a list with one flag per item; as a single True it
        applies to the items that qualify, the others must have been seeded by the caller and are accumulated.
        The job table travels in the kernel arguments: nothing is uploaded, the launch can be captured into a HIP graph."""
        n = len(values)
        if n == 0: return
        if not (len(channel_axes) == len(mins) == len(maxs) == n):
            raise RuntimeError(_KERNEL_FAILURE + 'MinMax_C_Multi: argument lists differ in length')
        dev = values[0].device
        jobs = np.empty(n, dtype=_MINMAX_C_JOB)
        keep = []
        for k in range(n):
            _f32(values[k], 'Value'); _f32(mins[k], 'Mins'); _f32(maxs[k], 'Maxs')
            if values[k].device != dev: raise RuntimeError(_KERNEL_FAILURE + 'MinMax_C_Multi: one device per call')
            v = _dense(values[k], channel_axes[k])
            C, epc = _geometry(v.shape, channel_axes[k])
            if mins[k].numel() != C or maxs[k].numel() != C or not mins[k].is_contiguous() or not maxs[k].is_contiguous():
                raise RuntimeError(_KERNEL_FAILURE + f'MinMax_C_Multi: item {k} needs contiguous float32[{C}] mins / maxs')
            owns = bool(fresh[k] if isinstance(fresh, (list, tuple)) else fresh)
            if owns and not (v.numel() == C * epc and epc <= 8192):
                if isinstance(fresh, (list, tuple)):
                    raise RuntimeError(_KERNEL_FAILURE + f'MinMax_C_Multi: item {k} cannot be `fresh` (see minmax_c_fresh_ok)')
                owns = False
            keep.append(v)
            jobs[k] = (v.data_ptr(), mins[k].data_ptr(), maxs[k].data_ptr(), v.numel(), C, epc, 1 if owns else 0, 0)
        with _DeviceOf(values[0]):
            _raise(lib.ppqhip_minmax_c_multi(jobs.ctypes.data, n, _stream()))

    @ staticmethod
    def minmax_c_outer_is_one(value, channel_axis: int) -> bool:
        """True for parameter-shaped tensors: the channel axis is the outermost one that is not 1 (one row per channel)."""
        C, epc = _geometry(value.shape, channel_axis)      # a shape question: no layout copy of a non-contiguous tensor for it
        return value.numel() == C * epc

    @ staticmethod
    def minmax_c_fresh_ok(value, channel_axis: int) -> bool:
        """True when ``MinMax_C_Multi(fresh=True)`` will OVERWRITE this item's mins / maxs (see there)."""
        C, epc = _geometry(value.shape, channel_axis)
        return value.numel() == C * epc and epc <= 8192

    @ staticmethod
    def ChannelSum(value, channel_axis: int, sums) -> None:
        """sums (float64 [C]) += per-channel sum of value; deterministic double accumulation."""
        _f32(value, 'Value'); _check(sums, torch.float64, 'Sums(Expect to be FP64)')
        v = value.contiguous()
        C, epc = _geometry(v.shape, channel_axis)
        if sums.numel() != C: raise RuntimeError(_KERNEL_FAILURE + f'sums needs {C} elements')
        with _DeviceOf(v):
            _raise(lib.ppqhip_channel_sum(v.data_ptr(), v.numel(), C, epc, sums.data_ptr(), _stream()))

    @ staticmethod
    def FloatScaleSearch(items, candidates, rounding: int = 0) -> torch.Tensor:
        """ppqhip_float_scale_search: `items` = [(values [rows, row_len] contiguous float32, exponent, mantissa, clip_min,
        clip_max)]; returns float64 [total rows, len(candidates)]: the squared fake-quant error sums of every row under
        every candidate scale, rows numbered over the items in order.  One launch per 128 items."""
        if not items: raise ValueError('FloatScaleSearch needs at least one item')
        dev = items[0][0].device
        jobs = np.zeros(len(items), dtype=_FLOAT_SEARCH_JOB)
        keep, total = [], 0
        for k, (v, e, m, lo, hi) in enumerate(items):
            _f32(v, 'Value')
            if v.ndim != 2 or not v.is_contiguous() or v.device != dev:
                raise RuntimeError(_KERNEL_FAILURE + 'FloatScaleSearch: values must be contiguous [rows, row_len] tensors on one device')
            if e <= 0: raise ValueError('Floating Quantization requires exponent > 0')
            keep.append(v)
            jobs[k] = (v.data_ptr(), v.shape[0], v.shape[1], int(e), int(m), float(lo), float(hi))
            total += v.shape[0]
        cand = np.asarray(candidates, dtype=np.float32)
        out = torch.empty(total, len(cand), dtype=torch.float64, device=dev)
        table = _workspace(dev, int(lib.ppqhip_float_scale_search_table_bytes(len(items))))
        with _DeviceOf(out):
            _raise(lib.ppqhip_float_scale_search(jobs.ctypes.data, len(jobs), cand.ctypes.data, len(cand),
                                                 int(getattr(rounding, 'value', rounding)), table.data_ptr(), out.data_ptr(), _stream()))
        return out

    @ staticmethod
    def KL_Losses(hist, num_of_bits: int) -> torch.Tensor:
        """hist: int32 [num_hist, bins] (or [bins]) -> float64 [num_hist, candidates]."""
        _check(hist, torch.int32, 'Histogram(Expect to be INT32)')
        h = hist.contiguous().reshape(-1, hist.shape[-1])
        ncand = lib.ppqhip_kl_num_candidates(h.shape[1], int(num_of_bits))
        if ncand <= 0:
            raise RuntimeError(_KERNEL_FAILURE + 'histogram length must be a multiple of 2^(num_of_bits-1)')
        losses = torch.empty((h.shape[0], ncand), dtype=torch.float64, device=h.device)
        with _DeviceOf(h):
            _raise(lib.ppqhip_kl_losses(h.data_ptr(), h.shape[0], h.shape[1], int(num_of_bits), losses.data_ptr(),
                                        _stream()))
        return losses

    @ staticmethod
    def MSE_Search(hist, hist_scale, min_value, quant_min: int, quant_max: int, symmetrical: bool) -> torch.Tensor:
        """hist: int32 [num_hist, bins]; hist_scale / min_value: float64 [num_hist] on the GPU.
        Returns int32 [num_hist, 4] = (start, end, step, candidate index) of the first minimum."""
        _check(hist, torch.int32, 'Histogram(Expect to be INT32)')
        _check(hist_scale, torch.float64, 'HistScale(Expect to be FP64)')
        _check(min_value, torch.float64, 'Min(Expect to be FP64)')
        h = hist.contiguous().reshape(-1, hist.shape[-1])
        best = torch.empty((h.shape[0], 4), dtype=torch.int32, device=h.device)
        with _DeviceOf(h):
            ws = _workspace(h.device, lib.ppqhip_mse_search_workspace_bytes(h.shape[0]))
            _raise(lib.ppqhip_mse_search(h.data_ptr(), h.shape[0], h.shape[1], hist_scale.contiguous().data_ptr(),
                                         min_value.contiguous().data_ptr(), int(quant_min), int(quant_max),
                                         int(bool(symmetrical)), best.data_ptr(), ws.data_ptr(), _stream()))
        return best


HIP_EXTENSION = _HipExtension()


class ComplieHelper:
    """Counterpart of ppq.core.ffi.ComplieHelper (ffi.py:16-49): nothing is JIT-compiled here, the
    library is built ahead of time (``__graft_entry__.build()``) and loaded by ``ppq_amd._lib``."""
    def __init__(self) -> None:
        self.__CUDA_EXTENTION__ = HIP_EXTENSION

    def complie(self):
        self.__CUDA_EXTENTION__ = HIP_EXTENSION

    @ property
    def CUDA_EXTENSION(self):
        return self.__CUDA_EXTENTION__


CUDA_COMPLIER = ComplieHelper()


class ENABLE_CUDA_KERNEL:
    """ppq/api/interface.py:915-935 for code written against this package alone: inside the block
    ``PPQ_CONFIG.USING_CUDA_KERNEL`` is True (it always is here -- there is no torch arithmetic branch to fall back to), the
    previous value comes back on exit."""
    def __init__(self) -> None:
        CUDA_COMPLIER.complie()
        self._state = False

    def __enter__(self):
        from .core import PPQ_CONFIG
        self._state = PPQ_CONFIG.USING_CUDA_KERNEL
        PPQ_CONFIG.USING_CUDA_KERNEL = True

    def __exit__(self, *args):
        from .core import PPQ_CONFIG
        PPQ_CONFIG.USING_CUDA_KERNEL = self._state


def install_into_ppq(fast_observers: bool = False) -> None:
    """Route an importable, unmodified PPQ through these kernels: the two lines a PPQ user adds.  ``CUDA_COMPLIER.complie()``
    -- which would JIT-build ppq/csrc with nvcc -- is shadowed on the singleton, so ``with ENABLE_CUDA_KERNEL():`` keeps
    working in scripts written for the reference.

    ``fast_observers=True`` (opt-in, still no reference file touched): the reference's ``TorchMinMaxObserver.observe`` --
    also phase 1 of its histogram / MSE observers -- reads every per-tensor activation TWICE with torch (``value.min()``,
    ``value.max()``, observer/range.py:86-98) and appends two 1-element tensors per batch; wrapped, it accumulates both into one
    float32[2] with ONE pass of ``ppqhip_minmax_t`` and hands the collectors views of that accumulator once.  The rendered
    range is the same number (min / max are exact and order independent); the one difference: a NaN in an activation is
    ignored instead of poisoning the range.  INTEGRATION.md section 3 has the measured effect."""
    from ppq.core import PPQ_CONFIG as REF_CONFIG
    from ppq.core.ffi import CUDA_COMPLIER as REF_COMPLIER
    REF_COMPLIER.__CUDA_EXTENTION__ = HIP_EXTENSION
    REF_CONFIG.USING_CUDA_KERNEL = True
    # existing scripts wrap their calls in ``with ENABLE_CUDA_KERNEL():`` (api/interface.py:915-935), whose constructor calls
    # CUDA_COMPLIER.complie(): shadow the method ON THE SINGLETON INSTANCE so that it re-selects this library instead of
    # JIT-building ppq/csrc (no reference file is touched; uninstall_from_ppq removes the shadow)
    def complie() -> None:
        REF_COMPLIER.__CUDA_EXTENTION__ = HIP_EXTENSION
    REF_COMPLIER.complie = complie
    # the reference's percentile observer calls the stateless CUDA.Quantile(value, q) once per batch (observer/range.py:349):
    # declare the observer the owner of those calls, so that batch k + 1 filters with the thresholds that worked for batch k
    from ppq.quantization.observer.range import TorchPercentileObserver as RefPercentile
    if 'percentile_observe' not in _SAVED_KERNEL_STATE:
        original = RefPercentile.observe
        _SAVED_KERNEL_STATE['percentile_observe'] = original

        def observe(self, value):
            with quantile_hint_owner(self): return original(self, value)
        observe.__wrapped__ = original
        RefPercentile.observe = observe
    if fast_observers and 'minmax_observe' not in _SAVED_KERNEL_STATE:
        from ppq.core import QuantizationProperty as RefProperty, QuantizationStates as RefStates
        from ppq.quantization.observer.range import TorchMinMaxObserver as RefMinMax
        original_mm = RefMinMax.observe
        _SAVED_KERNEL_STATE['minmax_observe'] = original_mm

        def observe_minmax(self, value):
            cfg = self._quant_cfg
            if (isinstance(value, torch.Tensor) and value.is_cuda and value.dtype == torch.float32 and value.numel() > 0
                    and cfg.state == RefStates.INITIAL and cfg.policy.has_property(RefProperty.PER_TENSOR)):
                acc = getattr(self, '_ppq_amd_minmax', None)
                if acc is None or acc.device != value.device or not self._min_val_collector:
                    acc = self._ppq_amd_minmax = torch.tensor([float('inf'), float('-inf')], dtype=torch.float32, device=value.device)
                    self._min_val_collector.append(acc[0:1]); self._max_val_collector.append(acc[1:2])    # views: later batches land in them
                HIP_EXTENSION.MinMax_T(value, acc)
                return
            return original_mm(self, value)
        observe_minmax.__wrapped__ = original_mm
        RefMinMax.observe = observe_minmax


_SAVED_PLUGIN_STATE: dict = {}       # what install_plugins_into_ppq(observers=True) replaced, for uninstall_from_ppq
_SAVED_KERNEL_STATE: dict = {}       # what install_into_ppq() wrapped (the percentile observer's observe)


def uninstall_from_ppq() -> None:
    """Undo :func:`install_into_ppq` AND :func:`install_plugins_into_ppq`: PPQ is back on its own torch path
    (USING_CUDA_KERNEL False, no extension), its ``OBSERVER_TABLE`` holds its own observer classes again (entries this
    package added are removed) and ``optim.calibration``'s two-phase type test points at its own classes.  The two ABC
    registrations (hook, pass base class) cannot be withdrawn (``ABCMeta.register`` has no inverse) and are harmless:
    they only make ``isinstance`` accept this package's objects."""
    from ppq.core import PPQ_CONFIG as REF_CONFIG
    from ppq.core.ffi import CUDA_COMPLIER as REF_COMPLIER
    REF_COMPLIER.__CUDA_EXTENTION__ = None
    REF_CONFIG.USING_CUDA_KERNEL = False
    REF_COMPLIER.__dict__.pop('complie', None)           # the class's own complie() is visible again
    if 'percentile_observe' in _SAVED_KERNEL_STATE:
        from ppq.quantization.observer.range import TorchPercentileObserver as RefPercentile
        RefPercentile.observe = _SAVED_KERNEL_STATE.pop('percentile_observe')
    if 'minmax_observe' in _SAVED_KERNEL_STATE:
        from ppq.quantization.observer.range import TorchMinMaxObserver as RefMinMax
        RefMinMax.observe = _SAVED_KERNEL_STATE.pop('minmax_observe')
    from . import observer as _observer
    _observer.SIBLING_PREFETCH = False
    if _SAVED_PLUGIN_STATE:
        import ppq.quantization.observer as ref_observer
        import ppq.quantization.optim.calibration as ref_calibration
        table = _SAVED_PLUGIN_STATE.pop('table')
        ref_observer.OBSERVER_TABLE.clear()
        ref_observer.OBSERVER_TABLE.update(table)
        ref_calibration.TorchHistObserver = _SAVED_PLUGIN_STATE.pop('hist')
        ref_calibration.TorchMSEObserver = _SAVED_PLUGIN_STATE.pop('mse')


def install_plugins_into_ppq(observers: bool = True) -> None:
    """The higher seams (last row), on top of :func:`install_into_ppq`: make this package's observers and
    passes first-class citizens of an importable, UNMODIFIED PPQ -- nothing of PPQ is edited, only its own registration
    points are used:

    * ``ppq.executor.base.QuantOPRuntimeHook`` is an ABC and PPQ's executor admits a hook by ``isinstance``
      (executor/torch.py:525-531): this package's ``CalibrationHook`` is registered as a virtual subclass, so
      ``ppq.TorchExecutor.forward(hooks=...)`` fires it;
    * ``ppq.quantization.optim.base.QuantizationOptimizationPass`` is an ABC and PPQ's pipeline admits a pass by
      ``isinstance`` (optim/base.py:60-82): this package's pass base class is registered, so
      ``ppq_amd.calibration.RuntimeCalibrationPass`` (and the parameter / LSQ / bias-correction passes) go into
      ``ppq.lib.Pipeline``; ``TorchQuantizeDelegator`` likewise admits this package's ``LSQDelegator``, ``AdaRoundDelegator`` and
      ``RoundTuningDelegator`` to
      ``TorchExecutor.register_quantize_delegate``;
    * with ``observers=True`` PPQ's ``OBSERVER_TABLE`` (observer/__init__.py:15-23) is updated with the HIP-backed
      observers, so PPQ's OWN ``RuntimeCalibrationPass`` builds them; its two-phase test is by exact type
      (optim/calibration.py:196: ``type(ob) not in {TorchHistObserver, TorchMSEObserver}``), so the two names that module
      imported are re-bound to the classes now in the table (the per-channel extensions 'kl_channel' / 'mse_channel'
      are two-phase too and therefore need this package's pass).  PPQ's pass renders the observers one by one; with
      ``observer.SIBLING_PREFETCH`` (switched on here) the first of those renders fetches the ranges of ALL live observers with one
      copy and searches all their histograms with one launch per group, the others finish on host values -- same numbers."""
    install_into_ppq()
    from ppq.executor.base import QuantOPRuntimeHook
    from ppq.quantization.optim.base import QuantizationOptimizationPass as RefPass

    from ppq.executor.torch import TorchQuantizeDelegator

    from . import adaround, calibration, lsq, mx_roundtune, observer, roundtune
    QuantOPRuntimeHook.register(observer.CalibrationHook)
    RefPass.register(calibration.QuantizationOptimizationPass)
    TorchQuantizeDelegator.register(lsq.LSQDelegator)      # register_quantize_delegate admits by isinstance (torch.py:317-320)
    TorchQuantizeDelegator.register(adaround.AdaRoundDelegator)
    TorchQuantizeDelegator.register(roundtune.RoundTuningDelegator)
    TorchQuantizeDelegator.register(mx_roundtune.MXRoundTuningDelegator)
    if observers:
        import ppq.quantization.observer as ref_observer
        import ppq.quantization.optim.calibration as ref_calibration
        if not _SAVED_PLUGIN_STATE:                                     # keep the ORIGINAL state across repeated installs
            _SAVED_PLUGIN_STATE.update(table=dict(ref_observer.OBSERVER_TABLE), hist=ref_calibration.TorchHistObserver,
                                       mse=ref_calibration.TorchMSEObserver)
        ref_observer.OBSERVER_TABLE.update(observer.OBSERVER_TABLE)
        ref_calibration.TorchHistObserver = observer.TorchHistObserver
        ref_calibration.TorchMSEObserver = observer.TorchMSEObserver
        # PPQ's pass renders observer by observer: let the first render fetch what all of them need (observer.SIBLING_PREFETCH)
        observer.SIBLING_PREFETCH = True


class CUDA:
    """Mirror of ppq.core.ffi.CUDA (ffi.py:51-350): same names, argument order and defaults."""

    @ staticmethod
    def LinearQuantize_T(tensor, scales, offsets, minimum: int = -128, maximum: int = 127, rounding: int = 0):
        return HIP_EXTENSION.QuantizeTensor_LT(tensor, scales, offsets, minimum, maximum, rounding)

    @ staticmethod
    def LinearQuantize_C(tensor, scales, offsets, channel_axis: int, minimum: int = -128, maximum: int = 127,
                         rounding: int = 0):
        return HIP_EXTENSION.QuantizeTensor_LC(tensor, scales, offsets, minimum, maximum, channel_axis, rounding)

    @ staticmethod
    def LinearQuantize_ToInt(tensor, scales, offsets, minimum: int, maximum: int, rounding: int, channel_axis, dtype):
        """MI355X-native addition (the reference does this step with torch ops): see HIP_EXTENSION.QuantizeTensor_ToInt."""
        return HIP_EXTENSION.QuantizeTensor_ToInt(tensor, scales, offsets, minimum, maximum, rounding, channel_axis, dtype)

    @ staticmethod
    def LinearQuantize_T_B(tensor, scales, offsets, dy, minimum: int, maximum: int, rounding: int):
        return HIP_EXTENSION.QuantizeTensor_LT_B(tensor, scales, offsets, dy, minimum, maximum, rounding)

    @ staticmethod
    def LinearQuantize_C_B(tensor, scales, offsets, dy, minimum: int, maximum: int, channel_axis: int, rounding: int):
        return HIP_EXTENSION.QuantizeTensor_LC_B(tensor, scales, offsets, dy, minimum, maximum, rounding, channel_axis)

    @ staticmethod
    def lsq_t_partials(numel: int) -> int:
        return HIP_EXTENSION.lsq_t_partials(numel)

    @ staticmethod
    def LinearQuantize_T_B_Main(tensor, scales, offsets, dy, minimum: int, maximum: int, rounding: int, partial):
        return HIP_EXTENSION.QuantizeTensor_LT_B_Main(tensor, scales, offsets, dy, minimum, maximum, rounding, partial)

    @ staticmethod
    def LSQ_Finish_Multi(partials, numels, minimums, maximums, grad_ss) -> None:
        return HIP_EXTENSION.LSQ_Finish_Multi(partials, numels, minimums, maximums, grad_ss)

    @ staticmethod
    def LinearQuantize_C_B_Multi(tensors, scales, offsets, dys, minimums, maximums, channel_axes, rounding: int,
                                 grad_xs=None, grad_ss=None):
        return HIP_EXTENSION.QuantizeTensor_LC_B_Multi(tensors, scales, offsets, dys, minimums, maximums, rounding, channel_axes,
                                                       grad_xs, grad_ss)

    @ staticmethod
    def Histogram_T(tensor, histogram, scale: float, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_T(tensor, scale, clip_outliers, histogram)
        return histogram

    @ staticmethod
    def Histogram_Asymmetric_T(min_value: float, max_value: float, tensor, histogram, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_Asymmetric_T(min_value, max_value, tensor, clip_outliers, histogram)
        return histogram

    @ staticmethod
    def Histogram_C(tensor, channel_axis: int, histogram, scale: float, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_C(tensor, channel_axis, scale, clip_outliers, histogram)
        return histogram

    @ staticmethod
    def Histogram_C_Scales(tensor, channel_axis: int, histogram, scales, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_C_Scales(tensor, channel_axis, scales, clip_outliers, histogram)
        return histogram

    @ staticmethod
    def Histogram_Asymmetric_C_Ranges(tensor, channel_axis: int, histogram, mins, maxs, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_Asymmetric_C_Ranges(tensor, channel_axis, mins, maxs, clip_outliers, histogram)
        return histogram

    @ staticmethod
    def Quantile(tensor, q: float):
        return HIP_EXTENSION.Quantile_T(tensor, q)

    @ staticmethod
    def Quantile_Hinted(tensor, q: float, hint):
        """CUDA.Quantile with the caller's threshold hint (``quantile_hint``), or None for none at all."""
        return HIP_EXTENSION.Quantile_T(tensor, q, hint)

    @ staticmethod
    def Quantile_Multi(tensors, q: float, dests=None, hints=None):
        return HIP_EXTENSION.Quantile_T_Multi(tensors, q, dests, hints)

    @ staticmethod
    def Isotone(tensor):
        return HIP_EXTENSION.Isotone_T(tensor)

    @ staticmethod
    def TensorClip_T(tensor, reference, limit):
        return HIP_EXTENSION.TensorClip_T(tensor, reference, limit)

    @ staticmethod
    def TensorClip_C(tensor, reference, limit, channel_axis: int):
        return HIP_EXTENSION.TensorClip_C(tensor, reference, limit, channel_axis)

    @ staticmethod
    def RoundingLoss_LT(tensor, scales, offsets, minimum: int = -128, maximum: int = 127, rounding: int = 0):
        return HIP_EXTENSION.RoundingLoss_LT(tensor, scales, offsets, minimum, maximum, rounding)

    @ staticmethod
    def RoundingLoss_LT_B(tensor, dy, scales, offsets, minimum: int = -128, maximum: int = 127, rounding: int = 0):
        return HIP_EXTENSION.RoundingLoss_LT_B(tensor, dy, scales, offsets, minimum, maximum, rounding)

    @ staticmethod
    def RoundingLoss_LC(tensor, scales, offsets, channel_axis: int, minimum: int = -128, maximum: int = 127,
                        rounding: int = 0):
        return HIP_EXTENSION.RoundingLoss_LC(tensor, scales, offsets, minimum, maximum, channel_axis, rounding)

    @ staticmethod
    def RoundingLoss_LC_B(tensor, dy, scales, offsets, channel_axis: int, minimum: int = -128, maximum: int = 127,
                          rounding: int = 0):
        return HIP_EXTENSION.RoundingLoss_LC_B(tensor, dy, scales, offsets, minimum, maximum, channel_axis, rounding)

    @ staticmethod
    def OrderPreservingObserve(tensor):
        """ppq/core/ffi.py:257-261, kept for surface completeness: the reference wires this name to ``RoundingLoss_LC_B`` with ONE
        argument, so every call fails in the extension's argument check (pybind: TypeError) -- nothing in ppq calls it.  Same
        wiring, same outcome here."""
        if not tensor.is_contiguous(): tensor = tensor.contiguous()
        return CUDA_COMPLIER.CUDA_EXTENSION.RoundingLoss_LC_B(tensor)

    @ staticmethod
    def compute_mse_loss(histogram: list, start: int, step: int, end: int) -> float:
        return HIP_EXTENSION.compute_mse_loss(histogram, start, step, end)

    @ staticmethod
    def FloatingQuantize_T(tensor, scales, offsets, exponent: int = 4, mantissa: int = 3, minimum: float = -448,
                           maximum: float = +448, rounding: int = 0):
        if exponent <= 0: raise ValueError('Floating Quantization requires exponent > 0')
        return HIP_EXTENSION.QuantizeTensor_FT(tensor, scales, offsets, exponent, mantissa, minimum, maximum, rounding)

    @ staticmethod
    def FloatingQuantize_C(tensor, scales, offsets, channel_axis: int, exponent: int = 4, mantissa: int = 3,
                           minimum: float = -448, maximum: float = +448, rounding: int = 0):
        if exponent <= 0: raise ValueError('Floating Quantization requires exponent > 0')
        return HIP_EXTENSION.QuantizeTensor_FC(tensor, scales, offsets, exponent, mantissa, minimum, maximum,
                                               channel_axis, rounding)

    @ staticmethod
    def FloatingQuantize_T_B(tensor, scales, offsets, dy, exponent: int, mantissa: int, minimum: float,
                             maximum: float, rounding: int):
        return HIP_EXTENSION.QuantizeTensor_FT_B(tensor, scales, offsets, dy, exponent, mantissa, minimum, maximum,
                                                 rounding)

    @ staticmethod
    def FloatingQuantize_C_B(tensor, scales, offsets, dy, exponent: int, mantissa: int, minimum: float,
                             maximum: float, channel_axis: int, rounding: int):
        return HIP_EXTENSION.QuantizeTensor_FC_B(tensor, scales, offsets, dy, exponent, mantissa, minimum, maximum,
                                                 rounding, channel_axis)

    # ---- additions ------------------------------------------------------------------------------
    @ staticmethod
    def MinMax_T(tensor, minmax):
        HIP_EXTENSION.MinMax_T(tensor, minmax)
        return minmax

    @ staticmethod
    def MinMax_C(tensor, channel_axis: int, mins, maxs):
        HIP_EXTENSION.MinMax_C(tensor, channel_axis, mins, maxs)
        return mins, maxs

    @ staticmethod
    def MinMax_C_Multi(tensors, channel_axes, mins, maxs, fresh: bool = False):
        return HIP_EXTENSION.MinMax_C_Multi(tensors, channel_axes, mins, maxs, fresh)

    @ staticmethod
    def minmax_c_fresh_ok(tensor, channel_axis: int) -> bool:
        return HIP_EXTENSION.minmax_c_fresh_ok(tensor, channel_axis)

    @ staticmethod
    def minmax_c_outer_is_one(tensor, channel_axis: int) -> bool:
        return HIP_EXTENSION.minmax_c_outer_is_one(tensor, channel_axis)

    @ staticmethod
    def ChannelSum(tensor, channel_axis: int, sums):
        HIP_EXTENSION.ChannelSum(tensor, channel_axis % tensor.ndim, sums)
        return sums

    @ staticmethod
    def ChannelMean(tensor, channel_axis: int) -> torch.Tensor:
        """float32 [C]: mean over every dim but channel_axis -- collect_bias of BiasCorrectionPass
        (ppq/quantization/optim/training.py:438-448) without the reduce-over-dims temporaries."""
        axis = channel_axis % tensor.ndim
        sums = torch.zeros(tensor.shape[axis], dtype=torch.float64, device=tensor.device)
        HIP_EXTENSION.ChannelSum(tensor, axis, sums)
        return (sums / (tensor.numel() // tensor.shape[axis])).to(torch.float32)

    # persistent accumulators (one row / slot per workgroup, folded on demand) ---------------------
    @ staticmethod
    def minmax_slots() -> int: return int(lib.ppqhip_minmax_slots())

    @ staticmethod
    def hist_rows() -> int: return int(lib.ppqhip_hist_rows())

    @ staticmethod
    def MinMax_T_Slots(tensor, slots):
        HIP_EXTENSION.MinMax_T_Slots(tensor, slots)
        return slots

    @ staticmethod
    def MinMax_Slots_Finish(slots, minmax):
        HIP_EXTENSION.MinMax_Slots_Finish(slots, minmax)
        return minmax

    @ staticmethod
    def MinMax_T_Slots_Multi(tensors, slots):
        HIP_EXTENSION.MinMax_T_Slots_Multi(tensors, slots)
        return slots

    @ staticmethod
    def Histogram_T_Rows_Multi(tensors, rows, scales, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_T_Rows_Multi(tensors, rows, scales, None, False, clip_outliers)
        return rows

    @ staticmethod
    def Histogram_Asymmetric_T_Rows_Multi(min_values, max_values, tensors, rows, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_T_Rows_Multi(tensors, rows, min_values, max_values, True, clip_outliers)
        return rows

    @ staticmethod
    def Histogram_T_Rows(tensor, rows, scale: float, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_T_Rows(tensor, scale, clip_outliers, rows)
        return rows

    @ staticmethod
    def Histogram_Asymmetric_T_Rows(min_value: float, max_value: float, tensor, rows, clip_outliers: bool = True):
        HIP_EXTENSION.Histogram_Asymmetric_T_Rows(min_value, max_value, tensor, clip_outliers, rows)
        return rows

    @ staticmethod
    def Histogram_Rows_Finish(rows, histogram):
        HIP_EXTENSION.Histogram_Rows_Finish(rows, histogram)
        return histogram

    @ staticmethod
    def FloatScaleSearch(items, candidates, rounding: int = 0):
        return HIP_EXTENSION.FloatScaleSearch(items, candidates, rounding)

    @ staticmethod
    def KLLosses(histogram, num_of_bits: int = 8):
        return HIP_EXTENSION.KL_Losses(histogram, num_of_bits)

    @ staticmethod
    def MseSearch(histogram, hist_scale, min_value, quant_min: int, quant_max: int, symmetrical: bool):
        return HIP_EXTENSION.MSE_Search(histogram, hist_scale, min_value, quant_min, quant_max, symmetrical)

    @ staticmethod
    def MXQuantize(tensor, format, axis: int, block_size: int = MX_BLOCK, scale_codes=None, scale_rule=None):
        """OCP Microscaling fake quant (MI355X-native; the contract is DESIGN.md section 9): blocks of 32 along ``axis`` share one
        power-of-two scale, elements are cast to ``format`` (``ppq_amd.mx.MXFormat``, its name or id).  ``scale_codes``: an
        optional uint8 tensor with the input's shape, the axis replaced by ceil(len / 32), that receives the E8M0 codes.
        A 4-D channels-last tensor quantised along axis 1 is read in storage order; any other non-contiguous one is copied.
        ``scale_rule``: how a block's scale is made from its values (``ppq_amd.mx.MXScaleRule``, its name or id; DESIGN.md section
        9.17) -- FLOOR (the default), CEIL, EVEN or MSE."""
        if block_size != MX_BLOCK: raise ValueError(f'MX block size is {MX_BLOCK}, got {block_size}')
        fmt = mx_format_arg(format, scale_rule)
        _f32(tensor, 'Value')
        axis = _mx_axis(tensor.dim(), axis)
        v = _mx_dense(tensor, axis)
        outer, length, inner, codes_shape = _mx_geometry(v, axis)
        codes = None
        if scale_codes is not None:
            if not (isinstance(scale_codes, torch.Tensor) and scale_codes.dtype == torch.uint8 and list(scale_codes.shape) == codes_shape):
                raise RuntimeError(_KERNEL_FAILURE + f'scale_codes must be a uint8 tensor of shape {codes_shape}')
            if scale_codes.device != v.device: raise RuntimeError(_KERNEL_FAILURE + 'scale_codes is on another device')
            codes = scale_codes if scale_codes.stride() == _mx_codes_like(v, axis, codes_shape).stride() else _mx_codes_like(v, axis, codes_shape)
        out = torch.empty_like(v)
        with _DeviceOf(v):
            _raise(lib.ppqhip_mx_fq(v.data_ptr(), out.data_ptr(), _ptr(codes), outer, length, inner,
                                    fmt, _stream()))
        if codes is not None and codes is not scale_codes: scale_codes.copy_(codes)
        return out

    @ staticmethod
    def MXRoundSplit(tensor, format, axis: int, scale_rule=None):
        """The split of MX round tuning: ``(floored, rounding, scale_codes)`` -- the element value just
        below every element on its block's grid, the element's position between that value and the one above in [0, 1), and the
        blocks' E8M0 codes, those of ``MXQuantize`` under ``scale_rule``."""
        return mx_round_split_multi([(tensor, format, axis, scale_rule)])[0]

    @ staticmethod
    def MXRoundForward(floored, rounding, scale_codes, format, axis: int):
        """The forward of MX round tuning: ``rounding > .5`` takes the element value above ``floored`` on its block's grid
        (``scale_codes``: the split's), anything else ``floored`` itself."""
        return mx_round_forward_multi([(floored, rounding, scale_codes, format, axis)])[0]

    @ staticmethod
    def MXPack(tensor, format, axis: int, block_size: int = MX_BLOCK, scale_rule=None):
        """Packed OCP Microscaling export: ``(elements, scales)``, two uint8 tensors with the block axis
        LAST -- the input's shape without ``axis`` plus ``[nb * B]`` resp. ``[nb]`` (nb = ceil(len / 32); B = 32 / 24 / 16 bytes per
        block for 8 / 6 / 4-bit elements).  Blocks, scales and rounding are those of ``MXQuantize``.  A 4-D channels-last tensor packed
        along axis 1 is read in storage order; any other non-contiguous one is copied.  ``scale_rule``: as for ``MXQuantize``."""
        if block_size != MX_BLOCK: raise ValueError(f'MX block size is {MX_BLOCK}, got {block_size}')
        fmt = mx_format_arg(format, scale_rule)
        _f32(tensor, 'Value')
        axis = _mx_axis(tensor.dim(), axis)
        v = _mx_dense(tensor, axis)
        outer, length, inner, _ = _mx_geometry(v, axis)
        eshape, sshape = mx_packed_shapes(v.shape, axis, format)
        elements = torch.empty(eshape, dtype=torch.uint8, device=v.device)
        scales = torch.empty(sshape, dtype=torch.uint8, device=v.device)
        with _DeviceOf(v):
            _raise(lib.ppqhip_mx_pack(v.data_ptr(), elements.data_ptr(), scales.data_ptr(), outer, length, inner, fmt, _stream()))
        return elements, scales

    @ staticmethod
    def MXUnpack(elements, scales, format, shape, axis: int):
        """The inverse of ``MXPack``: a contiguous float32 tensor of ``shape`` whose blocks along ``axis`` are
        value(code) * 2^(scale - 127); scale 0xFF and the NaN codes of MXFP8 give NaN, the tail padding is dropped."""
        fmt = mx_format_id(format)
        shape = [int(d) for d in shape]
        axis = _mx_axis(len(shape), axis)
        _check(elements, torch.uint8, 'Elements(Expect to be UINT8)'); _check(scales, torch.uint8, 'Scales(Expect to be UINT8)')
        eshape, sshape = mx_packed_shapes(shape, axis, fmt)
        if list(elements.shape) != eshape or list(scales.shape) != sshape:
            raise RuntimeError(_KERNEL_FAILURE + f'elements / scales of shape {list(elements.shape)} / {list(scales.shape)}, expected {eshape} / {sshape}')
        if scales.device != elements.device: raise RuntimeError(_KERNEL_FAILURE + 'scales is on another device')
        elements, scales = elements.contiguous(), scales.contiguous()
        out = torch.empty(shape, dtype=torch.float32, device=elements.device)
        outer, length, inner, _ = _mx_geometry(out, axis)
        with _DeviceOf(out):
            _raise(lib.ppqhip_mx_unpack(elements.data_ptr(), scales.data_ptr(), out.data_ptr(), outer, length, inner, fmt, _stream()))
        return out

    @ staticmethod
    def MXMatmul(a_elements, a_scales, a_format, b_elements, b_scales, b_format, k: int, bias=None):
        """``A[M, k] . B[N, k]^T (+ bias[N])`` as float32 ``[M, N]`` on the block-scaled MFMA.  Both operands
        are packed along their last axis as ``MXPack`` leaves them: ``elements [rows, nb * B]`` and ``scales [rows, nb]``, uint8,
        nb = ceil(k / 32).  The five float formats in any combination; MXINT8 is refused.  Non-contiguous inputs are copied, and so is an ``elements`` tensor whose
        data does not start on a 16-byte boundary (a row slice of a 6-bit operand with an odd nb: the row pitch is 24 nb)."""
        a_elements, a_scales, fa, b_elements, b_scales, fb, k, bias, m, n = _mx_matmul_args(a_elements, a_scales, a_format, b_elements, b_scales, b_format, k, bias)
        out = torch.empty([m, n], dtype=torch.float32, device=a_elements.device)
        with _DeviceOf(out):
            _raise(lib.ppqhip_mx_gemm(a_elements.data_ptr(), a_scales.data_ptr(), fa, b_elements.data_ptr(), b_scales.data_ptr(), fb,
                                      _ptr(bias), out.data_ptr(), m, n, k, _stream()))
        return out

    @ staticmethod
    def MXMatmulFused(a_elements, a_scales, a_format, b_elements, b_scales, b_format, k: int, bias=None, residual=None, relu: bool = False,
                      out_format=None, out_float: bool = True):
        """``MXMatmul`` with the fused epilogue: ``v = A . B^T (+ bias) (+ residual[M, N])``, then the ReLU
        (``v > 0 ? v : +0``, NaN kept), in ONE launch.  Returns ``(c, elements, scales)``: ``c`` the float32 ``[M, N]`` (None with
        ``out_float=False``), ``elements [M, nbo * B]`` / ``scales [M, nbo]`` ``v`` packed along its last axis in ``out_format``
        exactly as ``MXPack`` packs it (None, None without ``out_format``).  ``out_format``: one of the five float formats."""
        a_elements, a_scales, fa, b_elements, b_scales, fb, k, bias, m, n = _mx_matmul_args(a_elements, a_scales, a_format, b_elements, b_scales, b_format, k, bias)
        fo, residual = _mx_fused_args(out_format, out_float, residual, [m, n], a_elements.device)
        out, elements, scales = _mx_fused_outputs([m, n], fo, out_format, out_float, a_elements.device)
        with _DeviceOf(a_elements):
            _raise(lib.ppqhip_mx_gemm_fused(a_elements.data_ptr(), a_scales.data_ptr(), fa, b_elements.data_ptr(), b_scales.data_ptr(), fb,
                                            _ptr(bias), _ptr(residual), 1 if relu else 0, _ptr(out), _ptr(elements), _ptr(scales),
                                            fo, m, n, k, _stream()))
        return out, elements, scales

    @ staticmethod
    def MXConv2d(x_elements, x_scales, x_format, w_elements, w_scales, w_format, c: int, bias=None, stride=(1, 1), padding=(0, 0),
                 dilation=(1, 1)):
        """``conv2d(x[N, c, H, W], w[O, c, kh, kw]) (+ bias[O])`` as float32 ``[N, O, OH, OW]`` with channels-last strides, on the
        block-scaled MFMA as an implicit GEMM.  Both operands are packed along axis 1 as ``MXPack`` leaves
        them: x ``elements [N, H, W, nbc * B]`` / ``scales [N, H, W, nbc]``, w ``elements [O, kh, kw, nbc * B]`` / ``scales
        [O, kh, kw, nbc]``, uint8, nbc = ceil(c / 32).  The five float formats in any combination; MXINT8 is refused.  ``stride``,
        ``padding`` (symmetric) and ``dilation`` are (h, w) pairs.  Non-contiguous inputs are copied, and so is an ``elements`` tensor
        whose data does not start on a 16-byte boundary."""
        x_elements, x_scales, fx, w_elements, w_scales, fw, bias, geo = _mx_conv_args(x_elements, x_scales, x_format, w_elements, w_scales, w_format, c, bias, stride, padding, dilation)
        n, _, _, _, o, _, _ = geo[:7]
        out = torch.empty([n, geo[-2], geo[-1], o], dtype=torch.float32, device=x_elements.device)
        with _DeviceOf(out):
            _raise(lib.ppqhip_mx_conv2d(x_elements.data_ptr(), x_scales.data_ptr(), fx, w_elements.data_ptr(), w_scales.data_ptr(), fw,
                                        _ptr(bias), out.data_ptr(), *geo[:13], _stream()))
        return out.permute(0, 3, 1, 2)

    @ staticmethod
    def MXConv2dFused(x_elements, x_scales, x_format, w_elements, w_scales, w_format, c: int, bias=None, stride=(1, 1), padding=(0, 0),
                      dilation=(1, 1), residual=None, relu: bool = False, out_format=None, out_float: bool = True):
        """``MXConv2d`` with the fused epilogue: ``v = conv2d(x, w) (+ bias) (+ residual)``, then the ReLU
        (``v > 0 ? v : +0``, NaN kept), in ONE launch.  ``residual`` is ``[N, O, OH, OW]``; a tensor that is not channels-last is
        copied into that layout.  Returns ``(y, elements, scales)``: ``y`` the float32 ``[N, O, OH, OW]`` with channels-last strides
        (None with ``out_float=False``), ``elements [N, OH, OW, nbo * B]`` / ``scales [N, OH, OW, nbo]`` ``v`` packed along axis 1 in
        ``out_format`` exactly as ``MXPack`` packs it -- the x of the next ``MXConv2d`` -- (None, None without ``out_format``)."""
        x_elements, x_scales, fx, w_elements, w_scales, fw, bias, geo = _mx_conv_args(x_elements, x_scales, x_format, w_elements, w_scales, w_format, c, bias, stride, padding, dilation)
        n, o, oh, ow = geo[0], geo[4], geo[-2], geo[-1]
        dev = x_elements.device
        fo, residual = _mx_fused_args(out_format, out_float, residual, [n, o, oh, ow], dev)
        if residual is not None: residual = residual.permute(0, 2, 3, 1).contiguous()               # no copy when it is channels-last
        out, elements, scales = _mx_fused_outputs([n, o, oh, ow], fo, out_format, out_float, dev)
        with _DeviceOf(x_elements):
            _raise(lib.ppqhip_mx_conv2d_fused(x_elements.data_ptr(), x_scales.data_ptr(), fx, w_elements.data_ptr(), w_scales.data_ptr(), fw,
                                              _ptr(bias), _ptr(residual), 1 if relu else 0, _ptr(out), _ptr(elements), _ptr(scales),
                                              fo, *geo[:13], _stream()))
        return (out.permute(0, 3, 1, 2) if out is not None else None), elements, scales

    @ staticmethod
    def Sync():
        """Synchronize device (ffi.py:347-350)."""
        torch.cuda.synchronize()
