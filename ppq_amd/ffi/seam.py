"""The calibration seam: the reference's ``ComplieHelper`` / ``ENABLE_CUDA_KERNEL`` and the installers into an unmodified PPQ."""
import torch

from .extension import HIP_EXTENSION
from .hints import quantile_hint_owner


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
        from ..core import PPQ_CONFIG
        self._state = PPQ_CONFIG.USING_CUDA_KERNEL
        PPQ_CONFIG.USING_CUDA_KERNEL = True

    def __exit__(self, *args):
        from ..core import PPQ_CONFIG
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
    from .. import observer as _observer
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

    from .. import adaround, calibration, lsq, mx_roundtune, observer, roundtune
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
