"""``CUDA``: the reference's operator surface, forwarded to ``HIP_EXTENSION``, plus the MI355X-native MX entries."""
import torch

from .. import ffi as _package     # public entry points are called through the package: a replaced one is seen here too
from .._lib import lib
from ._base import _KERNEL_FAILURE, _DeviceOf, _check, _f32, _ptr, _raise, _stream
from .extension import HIP_EXTENSION
from .mx import (MX_BLOCK, _mx_axis, _mx_codes_like, _mx_conv_args, _mx_dense, _mx_fused_args, _mx_fused_outputs, _mx_geometry,
                 _mx_matmul_args, mx_format_arg, mx_format_id, mx_packed_shapes)
from .seam import CUDA_COMPLIER


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
        return _package.mx_round_split_multi([(tensor, format, axis, scale_rule)])[0]

    @ staticmethod
    def MXRoundForward(floored, rounding, scale_codes, format, axis: int):
        """The forward of MX round tuning: ``rounding > .5`` takes the element value above ``floored`` on its block's grid
        (``scale_codes``: the split's), anything else ``floored`` itself."""
        return _package.mx_round_forward_multi([(floored, rounding, scale_codes, format, axis)])[0]

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
