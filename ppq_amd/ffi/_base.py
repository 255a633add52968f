"""What every binding module shares: stream, tensor checks, layout and channel geometry, device guard, workspaces, the job table."""
import numpy as np
import torch

from .. import _lib

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
        self.idx = t.device.index if t is not None else None
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


def _ptr(t) -> int: return t.data_ptr() if t is not None else 0                          # the address of a tensor, 0 for None


def _same_length(label: str, n: int, *lists) -> None:
    if any(len(v) != n for v in lists): raise RuntimeError(_KERNEL_FAILURE + f'{label}: argument lists differ in length')


_EXPECT = {torch.float32: '(Expect to be FP32)', torch.float64: '(Expect to be FP64)', torch.int32: '(Expect to be INT32)',
           torch.uint8: '(Expect to be UINT8)'}


class JobTable:
    """The host half of one ``_multi`` launch: ``n`` records of ``dtype`` (``abi.py``), the tensors whose addresses went into them
    (kept alive for as long as the table is) and the one device all of them live on.  A builder checks each tensor with
    ``tensor()``, writes row k (``table.jobs[k] = (...)``, or a column at a time) and calls ``launch()``; a table that is built once
    and launched every iteration (``EqualizeTable``) carries its ``entry`` and is ``run()``.  The records hold POINTERS."""
    __slots__ = ('jobs', 'label', 'entry', 'keep', 'dev')

    def __init__(self, dtype, label: str, n: int, entry=None):
        self.jobs = np.zeros(n, dtype=dtype)
        self.label, self.entry = label, entry
        self.keep, self.dev = [], None

    def __len__(self) -> int: return len(self.jobs)

    def refuse(self, k: int, what: str):
        raise RuntimeError(_KERNEL_FAILURE + f'{self.label}: item {k}: {what}')

    def tensor(self, t, name: str, k: int, dtype=_F32, numel=None, like=None, contiguous=True):
        """``t`` of item ``k`` as the kernels take it: a non-empty GPU tensor of ``dtype`` on the table's device (the first tensor
        pins it), contiguous, with ``numel`` elements / the shape of ``like`` where given.  Returns ``t``, now kept alive."""
        try:                                    # one expression when everything is in order, as in _f32
            ok = t.dtype is dtype and t.is_cuda and t.numel() > 0
        except AttributeError:
            ok = False
        if not ok: _check(t, dtype, name + _EXPECT[dtype])
        if t.device != self.dev:
            if self.dev is not None: self.refuse(k, f'{name} is on another device')
            self.dev = t.device
        if contiguous and not t.is_contiguous(): self.refuse(k, f'{name} is not contiguous')
        if like is not None and t.shape != like.shape: self.refuse(k, f'{name} is not shaped like the weight')
        if numel is not None and t.numel() != numel: self.refuse(k, f'{name} must hold {numel} elements')
        self.keep.append(t)
        return t

    def launch(self, entry, *extra) -> None:
        """``entry(jobs, n, *extra, stream)`` on the table's device; an empty table launches nothing."""
        if len(self.jobs) == 0: return
        with _DeviceOf(self.keep[0] if self.keep else None):        # no tensor at all: nothing to launch for, any device does
            _raise(entry(self.jobs.ctypes.data, len(self.jobs), *extra, _stream()))

    def run(self) -> None: self.launch(self.entry)      # a table that carries its entry point
