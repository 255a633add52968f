"""The convolution epilogues and the native 1x1 convolution (include/ppq_hip.h ppqhip_bias_act / ppqhip_bias_add_act and their
sinks, ppqhip_conv1x1 / ppqhip_conv1x1_epilogue).  No job table: every launch takes its operands as arguments."""
import torch

from .. import _lib
from .._lib import lib
from ._base import _F32, _KERNEL_FAILURE, _DeviceOf, _f32, _raise, _stream


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
