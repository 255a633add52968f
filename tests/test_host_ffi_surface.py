"""The surface of ``ppq_amd.ffi``, pinned: the names below were read off the single-module ``ppq_amd/ffi.py`` before it became a
package -- every public module-level name, every method of ``_HipExtension`` and ``CUDA`` with its signature, and the underscore
names that tests, tools and bench.py reach for.  The package must still offer each one, the methods with the same signature."""
import inspect

import pytest

from ppq_amd import ffi

MODULE_NAMES = ['CUDA', 'CUDA_COMPLIER', 'ComplieHelper', 'ELIDE_A', 'ELIDE_B', 'ENABLE_CUDA_KERNEL', 'EqualizeTable', 'FloatingQuantizePlan',
 'HIP_EXTENSION', 'LinearQuantizePlan', 'MEASURE_METHODS', 'MEASURE_REDUCES', 'MXPackPlan', 'MXQuantizePlan', 'MX_BLOCK',
 'MX_BLOCK_BYTES', 'MX_FORMATS', 'MX_RULE_SHIFT', 'MX_SCALE_RULES', 'SINK_HIST', 'SINK_MINMAX', 'SPLIT_BIT', 'SPLIT_MAX_JOBS',
 'SPLIT_MAX_SEGMENTS', 'STAT_MAX_BINS', 'STAT_WORDS', 'adaround_backward_multi', 'adaround_forward_multi', 'bias_act_',
 'bias_act_hist_', 'bias_act_stats_', 'bias_add_act', 'bias_add_act_hist', 'bias_add_act_stats', 'conv1x1', 'conv1x1_epilogue',
 'equalize_apply_multi', 'equalize_apply_table', 'equalize_scale_multi', 'equalize_scale_table', 'fetch_rows_multi',
 'fq_measure_rows_multi', 'install_into_ppq', 'install_plugins_into_ppq', 'lib', 'measure_finish_multi', 'measure_rows_multi',
 'mx_block_bytes', 'mx_format_arg', 'mx_format_id', 'mx_packed_shapes', 'mx_round_forward_jobs', 'mx_round_forward_multi',
 'mx_round_split_multi', 'mx_rule_id', 'mx_unpack_multi', 'quantile_hint', 'quantile_hint_owner', 'roundtune_forward_multi',
 'split_apply_launches', 'split_apply_multi', 'split_apply_table', 'split_plan_launches', 'split_plan_multi', 'split_plan_table',
 'ssd_apply_multi', 'ssd_scales_multi', 'stat_counts', 'stat_moments_multi', 'stat_shape_multi', 'stat_table',
 'uninstall_from_ppq']

UNDERSCORE_NAMES = ['_ADAROUND_JOB', '_EQ_APPLY_JOB', '_EQ_SCALE_JOB', '_EQ_SEGMENT', '_FETCH_JOB', '_FINISH_JOB', '_FLOAT_SEARCH_JOB',
 '_FQ_FLOAT_JOB', '_FQ_JOB', '_FQ_MEASURE_JOB', '_HIST_JOB', '_KERNEL_FAILURE', '_LSQ_FINISH_JOB', '_LSQ_JOB', '_MEASURE_JOB',
 '_MINMAX_C_JOB', '_MINMAX_JOB', '_MX_JOB', '_MX_PACK_JOB', '_MX_ROUND_FWD_JOB', '_MX_ROUND_SPLIT_JOB', '_MX_UNPACK_JOB',
 '_QUANTILE_JOB', '_ROUNDTUNE_JOB', '_SPLIT_APPLY_JOB', '_SPLIT_PLAN_JOB', '_SSD_APPLY_JOB', '_SSD_SCALES_JOB', '_STAT_JOB',
 '_dense', '_f32', '_mx_dense', '_mx_geometry', '_owner_hints', '_owner_quantile_hint', '_stream', '_workspaces']

HIP_EXTENSION_METHODS = [('ChannelSum', '(value, channel_axis: int, sums) -> None'),
 ('FloatScaleSearch', '(items, candidates, rounding: int = 0) -> torch.Tensor'),
 ('Histogram_Asymmetric_C_Ranges', '(value, channel_axis: int, mins, maxs, clip_outliers: bool, hist) -> None'),
 ('Histogram_Asymmetric_T', '(min: float, max: float, value, clip_outliers: bool, hist) -> None'),
 ('Histogram_Asymmetric_T_Rows', '(min: float, max: float, value, clip_outliers: bool, rows) -> None'),
 ('Histogram_C', '(value, channel_axis: int, hist_scale: float, clip_outliers: bool, hist) -> None'),
 ('Histogram_C_Scales', '(value, channel_axis: int, hist_scales, clip_outliers: bool, hist) -> None'),
 ('Histogram_Rows_Finish', '(rows, hist) -> None'),
 ('Histogram_T', '(value, hist_scale: float, clip_outliers: bool, hist) -> None'),
 ('Histogram_T_Rows', '(value, hist_scale: float, clip_outliers: bool, rows) -> None'),
 ('Histogram_T_Rows_Multi', '(values, rows, p0, p1, asymmetric: bool, clip_outliers: bool) -> None'),
 ('Isotone_T', '(source) -> torch.Tensor'),
 ('KL_Losses', '(hist, num_of_bits: int) -> torch.Tensor'),
 ('LSQ_Finish_Multi', '(partials, numels, clip_mins, clip_maxs, grad_ss) -> None'),
 ('MSE_Search', '(hist, hist_scale, min_value, quant_min: int, quant_max: int, symmetrical: bool) -> torch.Tensor'),
 ('MinMax_C', '(value, channel_axis: int, mins, maxs) -> None'),
 ('MinMax_C_Multi', '(values, channel_axes, mins, maxs, fresh: bool = False)'),
 ('MinMax_Slots_Finish', '(slots, minmax) -> None'),
 ('MinMax_T', '(value, minmax) -> None'),
 ('MinMax_T_Slots', '(value, slots) -> None'),
 ('MinMax_T_Slots_Multi', '(values, slots) -> None'),
 ('Quantile_T', "(source, q: float, hint='auto') -> torch.Tensor"),
 ('Quantile_T_Multi', '(sources, q: float, dests=None, hints=None) -> list'),
 ('QuantizeTensor_FC',
  '(value, scale, offset, exponent: int, mantissa: int, clip_min: float, clip_max: float, channel_axis: int, rounding: int) -> '
  'torch.Tensor'),
 ('QuantizeTensor_FC_B',
  '(value, scales, offsets, grad_y, exponent: int, mantissa: int, clip_min: float, clip_max: float, rounding: int, channel_axis: '
  'int) -> List[torch.Tensor]'),
 ('QuantizeTensor_FT',
  '(value, scale, offset, exponent: int, mantissa: int, clip_min: float, clip_max: float, rounding: int) -> torch.Tensor'),
 ('QuantizeTensor_FT_B',
  '(value, scales, offsets, grad_y, exponent: int, mantissa: int, clip_min: float, clip_max: float, rounding: int) -> '
  'List[torch.Tensor]'),
 ('QuantizeTensor_LC', '(value, scale, offset, clip_min: int, clip_max: int, channel_axis: int, rounding: int) -> torch.Tensor'),
 ('QuantizeTensor_LC_B',
  '(value, scale, offset, grad_y, clip_min: int, clip_max: int, rounding: int, channel_axis: int) -> List[torch.Tensor]'),
 ('QuantizeTensor_LC_B_Multi',
  '(values, scales, offsets, grad_ys, clip_mins, clip_maxs, rounding: int, channel_axes, grad_xs=None, grad_ss=None)'),
 ('QuantizeTensor_LT', '(value, scale, offset, clip_min: int, clip_max: int, rounding: int) -> torch.Tensor'),
 ('QuantizeTensor_LT_B', '(value, scale, offset, grad_y, clip_min: int, clip_max: int, rounding: int) -> List[torch.Tensor]'),
 ('QuantizeTensor_LT_B_Main',
  '(value, scale, offset, grad_y, clip_min: int, clip_max: int, rounding: int, partial) -> torch.Tensor'),
 ('QuantizeTensor_ToInt',
  '(value, scale, offset, clip_min: int, clip_max: int, rounding: int, channel_axis, dtype: torch.dtype) -> torch.Tensor'),
 ('RoundingLoss_LC', '(value, scale, offset, clip_min: int, clip_max: int, channel_axis: int, rounding: int) -> torch.Tensor'),
 ('RoundingLoss_LC_B',
  '(value, dy, scale, offset, clip_min: int, clip_max: int, channel_axis: int, rounding: int) -> torch.Tensor'),
 ('RoundingLoss_LT', '(value, scale, offset, clip_min: int, clip_max: int, rounding: int) -> torch.Tensor'),
 ('RoundingLoss_LT_B', '(value, dy, scale, offset, clip_min: int, clip_max: int, rounding: int) -> torch.Tensor'),
 ('TensorClip_C', '(value, reference, limit, channel_axis: int) -> torch.Tensor'),
 ('TensorClip_T', '(value, reference, limit) -> torch.Tensor'),
 ('_check_hist', '(hist)'),
 ('_hint_ptr', '(hint, device) -> int'),
 ('compute_mse_loss', '(hist: list, start: int, step: int, end: int) -> float'),
 ('lsq_t_partials', '(numel: int) -> int'),
 ('minmax_c_fresh_ok', '(value, channel_axis: int) -> bool'),
 ('minmax_c_outer_is_one', '(value, channel_axis: int) -> bool')]

CUDA_METHODS = [('ChannelMean', '(tensor, channel_axis: int) -> torch.Tensor'),
 ('ChannelSum', '(tensor, channel_axis: int, sums)'),
 ('FloatScaleSearch', '(items, candidates, rounding: int = 0)'),
 ('FloatingQuantize_C',
  '(tensor, scales, offsets, channel_axis: int, exponent: int = 4, mantissa: int = 3, minimum: float = -448, maximum: float = '
  '448, rounding: int = 0)'),
 ('FloatingQuantize_C_B',
  '(tensor, scales, offsets, dy, exponent: int, mantissa: int, minimum: float, maximum: float, channel_axis: int, rounding: '
  'int)'),
 ('FloatingQuantize_T',
  '(tensor, scales, offsets, exponent: int = 4, mantissa: int = 3, minimum: float = -448, maximum: float = 448, rounding: int = '
  '0)'),
 ('FloatingQuantize_T_B',
  '(tensor, scales, offsets, dy, exponent: int, mantissa: int, minimum: float, maximum: float, rounding: int)'),
 ('Histogram_Asymmetric_C_Ranges', '(tensor, channel_axis: int, histogram, mins, maxs, clip_outliers: bool = True)'),
 ('Histogram_Asymmetric_T', '(min_value: float, max_value: float, tensor, histogram, clip_outliers: bool = True)'),
 ('Histogram_Asymmetric_T_Rows', '(min_value: float, max_value: float, tensor, rows, clip_outliers: bool = True)'),
 ('Histogram_Asymmetric_T_Rows_Multi', '(min_values, max_values, tensors, rows, clip_outliers: bool = True)'),
 ('Histogram_C', '(tensor, channel_axis: int, histogram, scale: float, clip_outliers: bool = True)'),
 ('Histogram_C_Scales', '(tensor, channel_axis: int, histogram, scales, clip_outliers: bool = True)'),
 ('Histogram_Rows_Finish', '(rows, histogram)'),
 ('Histogram_T', '(tensor, histogram, scale: float, clip_outliers: bool = True)'),
 ('Histogram_T_Rows', '(tensor, rows, scale: float, clip_outliers: bool = True)'),
 ('Histogram_T_Rows_Multi', '(tensors, rows, scales, clip_outliers: bool = True)'),
 ('Isotone', '(tensor)'),
 ('KLLosses', '(histogram, num_of_bits: int = 8)'),
 ('LSQ_Finish_Multi', '(partials, numels, minimums, maximums, grad_ss) -> None'),
 ('LinearQuantize_C', '(tensor, scales, offsets, channel_axis: int, minimum: int = -128, maximum: int = 127, rounding: int = 0)'),
 ('LinearQuantize_C_B', '(tensor, scales, offsets, dy, minimum: int, maximum: int, channel_axis: int, rounding: int)'),
 ('LinearQuantize_C_B_Multi',
  '(tensors, scales, offsets, dys, minimums, maximums, channel_axes, rounding: int, grad_xs=None, grad_ss=None)'),
 ('LinearQuantize_T', '(tensor, scales, offsets, minimum: int = -128, maximum: int = 127, rounding: int = 0)'),
 ('LinearQuantize_T_B', '(tensor, scales, offsets, dy, minimum: int, maximum: int, rounding: int)'),
 ('LinearQuantize_T_B_Main', '(tensor, scales, offsets, dy, minimum: int, maximum: int, rounding: int, partial)'),
 ('LinearQuantize_ToInt', '(tensor, scales, offsets, minimum: int, maximum: int, rounding: int, channel_axis, dtype)'),
 ('MXConv2d',
  '(x_elements, x_scales, x_format, w_elements, w_scales, w_format, c: int, bias=None, stride=(1, 1), padding=(0, 0), '
  'dilation=(1, 1))'),
 ('MXConv2dFused',
  '(x_elements, x_scales, x_format, w_elements, w_scales, w_format, c: int, bias=None, stride=(1, 1), padding=(0, 0), '
  'dilation=(1, 1), residual=None, relu: bool = False, out_format=None, out_float: bool = True)'),
 ('MXMatmul', '(a_elements, a_scales, a_format, b_elements, b_scales, b_format, k: int, bias=None)'),
 ('MXMatmulFused',
  '(a_elements, a_scales, a_format, b_elements, b_scales, b_format, k: int, bias=None, residual=None, relu: bool = False, '
  'out_format=None, out_float: bool = True)'),
 ('MXPack', '(tensor, format, axis: int, block_size: int = 32, scale_rule=None)'),
 ('MXQuantize', '(tensor, format, axis: int, block_size: int = 32, scale_codes=None, scale_rule=None)'),
 ('MXRoundForward', '(floored, rounding, scale_codes, format, axis: int)'),
 ('MXRoundSplit', '(tensor, format, axis: int, scale_rule=None)'),
 ('MXUnpack', '(elements, scales, format, shape, axis: int)'),
 ('MinMax_C', '(tensor, channel_axis: int, mins, maxs)'),
 ('MinMax_C_Multi', '(tensors, channel_axes, mins, maxs, fresh: bool = False)'),
 ('MinMax_Slots_Finish', '(slots, minmax)'),
 ('MinMax_T', '(tensor, minmax)'),
 ('MinMax_T_Slots', '(tensor, slots)'),
 ('MinMax_T_Slots_Multi', '(tensors, slots)'),
 ('MseSearch', '(histogram, hist_scale, min_value, quant_min: int, quant_max: int, symmetrical: bool)'),
 ('OrderPreservingObserve', '(tensor)'),
 ('Quantile', '(tensor, q: float)'),
 ('Quantile_Hinted', '(tensor, q: float, hint)'),
 ('Quantile_Multi', '(tensors, q: float, dests=None, hints=None)'),
 ('RoundingLoss_LC', '(tensor, scales, offsets, channel_axis: int, minimum: int = -128, maximum: int = 127, rounding: int = 0)'),
 ('RoundingLoss_LC_B',
  '(tensor, dy, scales, offsets, channel_axis: int, minimum: int = -128, maximum: int = 127, rounding: int = 0)'),
 ('RoundingLoss_LT', '(tensor, scales, offsets, minimum: int = -128, maximum: int = 127, rounding: int = 0)'),
 ('RoundingLoss_LT_B', '(tensor, dy, scales, offsets, minimum: int = -128, maximum: int = 127, rounding: int = 0)'),
 ('Sync', '()'),
 ('TensorClip_C', '(tensor, reference, limit, channel_axis: int)'),
 ('TensorClip_T', '(tensor, reference, limit)'),
 ('compute_mse_loss', '(histogram: list, start: int, step: int, end: int) -> float'),
 ('hist_rows', '() -> int'),
 ('lsq_t_partials', '(numel: int) -> int'),
 ('minmax_c_fresh_ok', '(tensor, channel_axis: int) -> bool'),
 ('minmax_c_outer_is_one', '(tensor, channel_axis: int) -> bool'),
 ('minmax_slots', '() -> int')]


@pytest.mark.parametrize('name', MODULE_NAMES + UNDERSCORE_NAMES)
def test_the_package_offers_the_name(name):
    assert hasattr(ffi, name), name


def _methods(cls):
    found = {}
    for name, value in vars(cls).items():
        function = value.__func__ if isinstance(value, staticmethod) else value
        if not name.startswith('__') and callable(function): found[name] = str(inspect.signature(function))
    return found


@pytest.mark.parametrize('cls, expected', [(ffi._HipExtension, HIP_EXTENSION_METHODS), (ffi.CUDA, CUDA_METHODS)], ids=['HIP_EXTENSION', 'CUDA'])
def test_methods_keep_their_signatures(cls, expected):
    found = _methods(cls)
    assert [(name, found.get(name)) for name, _ in expected] == expected


def test_shared_state_is_one_object():
    """The mutable module state is re-exported, not copied."""
    from ppq_amd.ffi import _base, hints, seam
    assert ffi._workspaces is _base._workspaces and ffi._owner_hints is hints._owner_hints
    assert ffi._SAVED_KERNEL_STATE is seam._SAVED_KERNEL_STATE and ffi._SAVED_PLUGIN_STATE is seam._SAVED_PLUGIN_STATE
    assert type(ffi.HIP_EXTENSION) is ffi._HipExtension and ffi.CUDA_COMPLIER.CUDA_EXTENSION is ffi.HIP_EXTENSION
