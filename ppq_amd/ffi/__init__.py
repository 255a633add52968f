"""The drop-in seam: ``ppq.core.ffi`` rebuilt over the C-ABI HIP library.

Reference: ppq/core/ffi.py.  Two objects are provided.

``HIP_EXTENSION`` presents the 20 callables of the reference's pybind module ``PPQ_Cuda_Impls`` (ppq/csrc/export.cc:8-34) with the same
names and positional arguments, so it can be assigned to ``ppq.core.ffi.CUDA_COMPLIER.__CUDA_EXTENTION__`` (see :func:`install_into_ppq` /
INTEGRATION.md) and every ``ppq.core.ffi.CUDA.*`` wrapper of an unmodified PPQ then lands in our kernels.

``CUDA`` mirrors the reference's static-method class of the same name (ffi.py:56-350): same method names, argument names, defaults and
order, for code that wants the operator surface without PPQ.  It adds the MI355X-native entries that have no twin in the reference
(``MinMax_T/C``, ``KLLosses``, ``MseSearch``, the persistent-row / multi-tensor statistics launches).

All tensor arguments must live on the GPU.  There is no CPU path: a CPU tensor raises.  Errors follow the reference's convention as seen
from Python: the C++ ``ValueTypeException`` / ``InvalidValueException`` (common.cuh:32-48) surface as ``RuntimeError``.

One module per kernel family over ``_base.py`` (checks, the job table) and ``abi.py`` (the header's records); every name is re-exported
here and the rest of ``ppq_amd`` imports from here alone, so a caller that replaces ``ppq_amd.ffi.bias_act_`` is seen by every user.
"""
from .._lib import lib
from . import abi
from ._base import (_DeviceOf, _F32, _KERNEL_FAILURE, JobTable, _check, _dense, _f32, _geometry, _ptr, _raise, _stream, _workspace,
                    _workspaces)
from .cuda import CUDA
from .epilogue import (ELIDE_A, ELIDE_B, SINK_HIST, SINK_MINMAX, _run_epilogue, bias_act_, bias_act_hist_, bias_act_stats_, bias_add_act,
                       bias_add_act_hist, bias_add_act_stats, conv1x1, conv1x1_epilogue)
from .equalize import (SPLIT_BIT, SPLIT_MAX_JOBS, SPLIT_MAX_SEGMENTS, EqualizeTable, equalize_apply_multi, equalize_apply_table,
                       equalize_scale_multi, equalize_scale_table, split_apply_launches, split_apply_multi, split_apply_table,
                       split_plan_launches, split_plan_multi, split_plan_table, ssd_apply_multi, ssd_scales_multi)
from .extension import HIP_EXTENSION, _HipExtension
from .hints import _hint_owner, _owner_hints, _owner_quantile_hint, quantile_hint, quantile_hint_owner
from .measure import (MEASURE_METHODS, MEASURE_REDUCES, STAT_MAX_BINS, STAT_WORDS, fetch_rows_multi, fq_measure_rows_multi,
                      measure_finish_multi, measure_rows_multi, stat_counts, stat_moments_multi, stat_shape_multi, stat_table)
from .mx import (MX_BLOCK, MX_BLOCK_BYTES, MX_FORMATS, MX_RULE_SHIFT, MX_SCALE_RULES, MXPackPlan, MXQuantizePlan, _mx_axis,
                 _mx_channels_last, _mx_codes_like, _mx_dense, _mx_geometry, mx_block_bytes, mx_format_arg, mx_format_id, mx_packed_shapes,
                 mx_round_forward_jobs, mx_round_forward_multi, mx_round_split_multi, mx_rule_id, mx_unpack_multi)
from .plans import FloatingQuantizePlan, LinearQuantizePlan
from .seam import (_SAVED_KERNEL_STATE, _SAVED_PLUGIN_STATE, CUDA_COMPLIER, ENABLE_CUDA_KERNEL, ComplieHelper, install_into_ppq,
                   install_plugins_into_ppq, uninstall_from_ppq)
from .weight_map import adaround_backward_multi, adaround_forward_multi, roundtune_forward_multi

from .abi import JOB_LAYOUTS

# the records under the names they had when they stood next to their builders, ``_MX_JOB`` for ``abi.MX_JOB`` (tests and tools use these)
globals().update({'_' + name: record for name, record in vars(abi).items() if name.isupper() and name != 'JOB_LAYOUTS'})
