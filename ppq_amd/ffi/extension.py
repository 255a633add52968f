"""``HIP_EXTENSION``: the callables of the reference's pybind module over the C-ABI library, and the MI355X-native additions."""
from typing import List

import numpy as np
import torch

from .._lib import lib
from ._base import _F32, _KERNEL_FAILURE, JobTable, _DeviceOf, _check, _dense, _f32, _geometry, _raise, _same_length, _stream, _workspace
from .abi import FLOAT_SEARCH_JOB, HIST_JOB, LSQ_FINISH_JOB, LSQ_JOB, MINMAX_C_JOB, MINMAX_JOB, QUANTILE_JOB
from .hints import _owner_quantile_hint


def _rows_are(rows, R: int) -> None:
    """What ``Histogram_T_Rows`` and ``Histogram_Asymmetric_T_Rows`` ask of ``rows`` beyond its dtype: a contiguous [hist_rows(), bins]."""
    if rows.ndim != 2 or rows.shape[0] != R or not rows.is_contiguous():
        raise RuntimeError(_KERNEL_FAILURE + f'rows must be a contiguous [{R}, bins] tensor')


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
        _same_length('LSQ_Finish_Multi', n, numels, clip_mins, clip_maxs, grad_ss)
        table = JobTable(LSQ_FINISH_JOB, 'LSQ_Finish_Multi', n)
        for k in range(n):
            partial, grad_s = table.tensor(partials[k], 'Partial', k, contiguous=False), table.tensor(grad_ss[k], 'Grad_s', k, contiguous=False)
            if partial.numel() < int(lib.ppqhip_fq_linear_t_bwd_partials(int(numels[k]))): table.refuse(k, 'partial is too small (see lsq_t_partials)')
            table.jobs[k] = (partial.data_ptr(), grad_s.data_ptr(), int(numels[k]), int(clip_mins[k]), int(clip_maxs[k]))
        table.launch(lib.ppqhip_lsq_finish_multi)

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
        _same_length('QuantizeTensor_LC_B_Multi', n, scales, offsets, grad_ys, clip_mins, clip_maxs, channel_axes)
        table = JobTable(LSQ_JOB, 'QuantizeTensor_LC_B_Multi', n)
        gxs, gss = [], []
        for k in range(n):
            v, sc, of, g = (table.tensor(t, name, k, contiguous=False).contiguous() for name, t in
                            (('Value', values[k]), ('Scale', scales[k]), ('Offset', offsets[k]), ('Gard', grad_ys[k])))
            C, epc = _geometry(v.shape, channel_axes[k])
            if sc.numel() != C or of.numel() != C: table.refuse(k, f'needs {C} scales / offsets')
            gx = torch.empty_like(g) if grad_xs is None else grad_xs[k]
            gs = torch.empty_like(sc) if grad_ss is None else grad_ss[k]
            if grad_xs is not None and (gx.shape != g.shape or not gx.is_contiguous() or gx.dtype != _F32):
                raise RuntimeError(_KERNEL_FAILURE + f'QuantizeTensor_LC_B_Multi: grad_xs[{k}] must be a contiguous float32 tensor shaped like the value')
            if grad_ss is not None and (gs.numel() != C or not gs.is_contiguous() or gs.dtype != _F32):
                raise RuntimeError(_KERNEL_FAILURE + f'QuantizeTensor_LC_B_Multi: grad_ss[{k}] must be a contiguous float32[{C}]')
            table.keep += (v, g, sc, of, gx, gs); gxs.append(gx); gss.append(gs)      # the contiguous copies, where one was made
            table.jobs[k] = (v.data_ptr(), sc.data_ptr(), of.data_ptr(), g.data_ptr(), gx.data_ptr(), gs.data_ptr(), v.numel(), C, epc,
                             int(clip_mins[k]), int(clip_maxs[k]))
        table.launch(lib.ppqhip_fq_linear_c_bwd_multi, int(rounding))
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
    def _float_bwd(value, scales, offsets, grad_y, exponent, mantissa, clip_min, clip_max, rounding, channel_axis=None):
        """``ppqhip_fq_float_c_bwd`` along ``channel_axis``, or with the whole tensor as its one channel."""
        _f32(value, 'Value'); _f32(scales, 'Scale'); _f32(offsets, 'Offset'); _f32(grad_y, 'Gard')
        v = value.contiguous(); g = grad_y.contiguous()
        sc, of = scales.contiguous(), offsets.contiguous()
        C, epc = (1, v.numel()) if channel_axis is None else _geometry(v.shape, channel_axis)
        grad_x = torch.empty_like(g); grad_s = torch.empty_like(sc)
        with _DeviceOf(v):
            _raise(lib.ppqhip_fq_float_c_bwd(v.data_ptr(), sc.data_ptr(), of.data_ptr(), g.data_ptr(), grad_x.data_ptr(),
                                             grad_s.data_ptr(), v.numel(), C, epc, int(exponent), int(mantissa),
                                             float(clip_min), float(clip_max), int(rounding), _stream()))
        return [grad_x, grad_s]

    @ staticmethod
    def QuantizeTensor_FT_B(value, scales, offsets, grad_y, exponent: int, mantissa: int, clip_min: float, clip_max: float, rounding: int) -> List[torch.Tensor]:
        return _HipExtension._float_bwd(value, scales, offsets, grad_y, exponent, mantissa, clip_min, clip_max, rounding)

    @ staticmethod
    def QuantizeTensor_FC_B(value, scales, offsets, grad_y, exponent: int, mantissa: int, clip_min: float, clip_max: float, rounding: int,
                            channel_axis: int) -> List[torch.Tensor]:
        return _HipExtension._float_bwd(value, scales, offsets, grad_y, exponent, mantissa, clip_min, clip_max, rounding, channel_axis)

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
        vs = []                                 # written out, not built on JobTable: the frame costs it 5 % (profiles/ffi_tables.txt)
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
        jobs = np.empty(len(vs), dtype=QUANTILE_JOB)
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
    def _tensor_clip(value, reference, limit, channel_axis=None) -> torch.Tensor:
        _f32(value, 'Value'); _f32(reference, 'Reference'); _f32(limit, 'Limit')
        v = value.contiguous(); r = reference.contiguous()
        geometry = () if channel_axis is None else _geometry(v.shape, channel_axis)
        out = torch.empty_like(v)
        with _DeviceOf(v):
            _raise((lib.ppqhip_tensor_clip_c if geometry else lib.ppqhip_tensor_clip_t)(
                v.data_ptr(), r.data_ptr(), limit.contiguous().data_ptr(), out.data_ptr(), v.numel(), *geometry, _stream()))
        return out

    @ staticmethod
    def TensorClip_T(value, reference, limit) -> torch.Tensor: return _HipExtension._tensor_clip(value, reference, limit)

    @ staticmethod
    def TensorClip_C(value, reference, limit, channel_axis: int) -> torch.Tensor:
        return _HipExtension._tensor_clip(value, reference, limit, channel_axis)

    @ staticmethod
    def _rounding_loss(value, dy, scale, offset, clip_min, clip_max, rounding, channel_axis=None):
        """``ppqhip_rounding_loss`` (``dy`` None: returns the loss) or ``ppqhip_rounding_loss_bwd`` (returns dx), per channel along
        ``channel_axis`` or per tensor, which the library takes as ``(num_channel, elem_per_channel) = (0, 1)``."""
        _f32(value, 'Value'); _f32(scale, 'Scale'); _f32(offset, 'Offset')
        if dy is not None: _f32(dy, 'Gard')
        v = value.contiguous()
        C, epc = (0, 1) if channel_axis is None else _geometry(v.shape, channel_axis)
        sc, of = scale.contiguous(), offset.contiguous()
        out = torch.empty(1, dtype=torch.float32, device=v.device) if dy is None else torch.empty_like(v)
        tail = (sc.data_ptr(), of.data_ptr(), out.data_ptr(), v.numel(), C, epc, int(clip_min), int(clip_max), int(rounding))
        with _DeviceOf(v):
            if dy is None: _raise(lib.ppqhip_rounding_loss(v.data_ptr(), *tail, _stream()))
            else: _raise(lib.ppqhip_rounding_loss_bwd(v.data_ptr(), dy.data_ptr(), *tail, _stream()))
        return out

    @ staticmethod
    def RoundingLoss_LT(value, scale, offset, clip_min: int, clip_max: int, rounding: int) -> torch.Tensor:
        return _HipExtension._rounding_loss(value, None, scale, offset, clip_min, clip_max, rounding)

    @ staticmethod
    def RoundingLoss_LC(value, scale, offset, clip_min: int, clip_max: int, channel_axis: int, rounding: int) -> torch.Tensor:
        return _HipExtension._rounding_loss(value, None, scale, offset, clip_min, clip_max, rounding, channel_axis)

    @ staticmethod
    def RoundingLoss_LT_B(value, dy, scale, offset, clip_min: int, clip_max: int, rounding: int) -> torch.Tensor:
        return _HipExtension._rounding_loss(value, dy, scale, offset, clip_min, clip_max, rounding)

    @ staticmethod
    def RoundingLoss_LC_B(value, dy, scale, offset, clip_min: int, clip_max: int, channel_axis: int, rounding: int) -> torch.Tensor:
        return _HipExtension._rounding_loss(value, dy, scale, offset, clip_min, clip_max, rounding, channel_axis)

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
        jobs = np.empty(len(vs), dtype=MINMAX_JOB)
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
        jobs = np.empty(len(vs), dtype=HIST_JOB)
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
        _f32(value, 'Value'); _check(rows, torch.int32, 'Rows(Expect to be INT32)'); _rows_are(rows, lib.ppqhip_hist_rows())
        v = _dense(value)
        with _DeviceOf(v):
            _raise(lib.ppqhip_hist_sym_t_rows(v.data_ptr(), v.numel(), float(hist_scale), int(bool(clip_outliers)),
                                              rows.data_ptr(), rows.shape[1], _stream()))

    @ staticmethod
    def Histogram_Asymmetric_T_Rows(min: float, max: float, value, clip_outliers: bool, rows) -> None:
        _f32(value, 'Value'); _check(rows, torch.int32, 'Rows(Expect to be INT32)'); _rows_are(rows, lib.ppqhip_hist_rows())
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
        _same_length('MinMax_C_Multi', n, channel_axes, mins, maxs)
        table = JobTable(MINMAX_C_JOB, 'MinMax_C_Multi', n)
        for k in range(n):
            v = _dense(table.tensor(values[k], 'Value', k, contiguous=False), channel_axes[k])
            C, epc = _geometry(v.shape, channel_axes[k])
            table.tensor(mins[k], 'Mins', k, numel=C); table.tensor(maxs[k], 'Maxs', k, numel=C)
            owns = bool(fresh[k] if isinstance(fresh, (list, tuple)) else fresh)
            if owns and not (v.numel() == C * epc and epc <= 8192):
                if isinstance(fresh, (list, tuple)): table.refuse(k, 'cannot be `fresh` (see minmax_c_fresh_ok)')
                owns = False
            table.keep.append(v)                                        # the dense copy, where one was made
            table.jobs[k] = (v.data_ptr(), mins[k].data_ptr(), maxs[k].data_ptr(), v.numel(), C, epc, 1 if owns else 0, 0)
        table.launch(lib.ppqhip_minmax_c_multi)

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
        table, total = JobTable(FLOAT_SEARCH_JOB, 'FloatScaleSearch', len(items)), 0
        for k, (v, e, m, lo, hi) in enumerate(items):
            table.tensor(v, 'Value', k)
            if v.ndim != 2: table.refuse(k, 'values must be contiguous [rows, row_len] tensors')
            if e <= 0: raise ValueError('Floating Quantization requires exponent > 0')
            table.jobs[k] = (v.data_ptr(), v.shape[0], v.shape[1], int(e), int(m), float(lo), float(hi))
            total += v.shape[0]
        cand = np.asarray(candidates, dtype=np.float32)
        out = torch.empty(total, len(cand), dtype=torch.float64, device=table.dev)
        device_table = _workspace(table.dev, int(lib.ppqhip_float_scale_search_table_bytes(len(items))))
        table.launch(lib.ppqhip_float_scale_search, cand.ctypes.data, len(cand), int(getattr(rounding, 'value', rounding)),
                     device_table.data_ptr(), out.data_ptr())
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
