"""ppq_amd -- MI355X-native (gfx950) implementation of PPQ's quantization-simulation hot path:
fake-quant kernels, calibration statistics (min/max, histograms, quantiles) and the KL / MSE /
percentile clipping searches of ``RuntimeCalibrationPass``, behind PPQ's own ``ppq.core.ffi.CUDA``
operator surface.  Importing this package loads ``libppq_hip.so`` and fails loudly if it is absent.
"""
from . import _lib  # noqa: F401  (raises ImportError when the HIP library has not been built)
from .core import (PPQ_CONFIG, FloatingQuantizationConfig, LinearQuantizationConfig, QuantizationPolicy,
                   QuantizationProperty, QuantizationStates, RoundingPolicy, TensorQuantizationConfig)
from .ffi import (CUDA, CUDA_COMPLIER, ENABLE_CUDA_KERNEL, HIP_EXTENSION, install_into_ppq, install_plugins_into_ppq,
                  uninstall_from_ppq)
from .mx import (MXDelegator, MXDeployment, MXFormat, MXScaleRule, MXTensor, deploy_graph_mx, export_graph_mx, mx_conv2d, mx_conv2d_packed, mx_dequantize,
                 mx_fake_quant, mx_linear, mx_matmul, mx_quantize, quantize_graph_mx)
from .mx_roundtune import MXRoundTuningDelegator, MXRoundTuningGroup, MXRoundTuningPass, mx_round_forward, mx_round_split

__all__ = ['MXFormat', 'MXScaleRule', 'MXDelegator', 'MXTensor', 'mx_fake_quant', 'mx_quantize', 'mx_dequantize', 'mx_matmul', 'mx_linear', 'mx_conv2d', 'mx_conv2d_packed', 'quantize_graph_mx', 'export_graph_mx', 'deploy_graph_mx', 'MXDeployment', 'mx_round_split', 'mx_round_forward', 'MXRoundTuningDelegator', 'MXRoundTuningGroup', 'MXRoundTuningPass', 'CUDA', 'CUDA_COMPLIER', 'ENABLE_CUDA_KERNEL', 'HIP_EXTENSION', 'install_into_ppq', 'install_plugins_into_ppq', 'uninstall_from_ppq', 'PPQ_CONFIG', 'RoundingPolicy',
           'QuantizationProperty', 'QuantizationPolicy', 'QuantizationStates', 'TensorQuantizationConfig',
           'LinearQuantizationConfig', 'FloatingQuantizationConfig']
