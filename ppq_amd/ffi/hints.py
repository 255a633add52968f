"""Who owns the threshold hints of ``Quantile_T``: the part of the calibration seam (``seam.py``) that ``extension.py`` reads."""
import threading
import weakref

import torch

# Quantile_T(source, q) is stateless in the reference, but calibration calls it batch after batch on the same activation.  A caller
# hands it a threshold hint (include/ppq_hip.h: ppqhip_quantile_t) explicitly, or declares itself the OWNER of the calls it is about
# to make, which ``install_into_ppq()`` wraps around the reference's percentile observer.  Keyed by the owner, not by shape alone:
# a CNN repeats its shapes, and a misplaced hint costs the exact passes.  A hint changes how much the kernels read, never the result.
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
