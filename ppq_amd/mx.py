"""OCP Microscaling (MX) block-scaled fake quant: MXFP8 (E4M3 / E5M2), MXFP6 (E3M2 / E2M3), MXFP4 (E2M1) and MXINT8.

32 consecutive values along one axis share a power-of-two E8M0 scale taken from the block itself -- nothing is calibrated.  The
reference has no MX: the contract (restated by ``tests/mx_reference.py``) is this package's own.  Per block

    amax = max |v| over the finite elements;  se = clamp(floor(log2(amax)) - emax, -127, 127), -127 when amax == 0;  X = 2^se
    y = cast(v / X) * X       cast: nearest element value, ties to the even encoding, saturating at the largest normal

NaN passes through, +-Inf saturates, zero keeps its sign, float32 subnormals are honoured.  Every step is exact in float32, so the
HIP kernels (``ppq_amd/csrc/mx.hip``, ``use_kernels=True``) and the torch restatement below (``use_kernels=False``, any device)
give identical bits.  That ``se`` is the OCP floor rule, ``MXScaleRule.FLOOR`` and the default everywhere; ``scale_rule=`` chooses
``CEIL``, ``EVEN`` or ``MSE`` instead (restated by ``tests/mx_scale_reference.py``), in the same one launch.

``mx_quantize`` / ``mx_dequantize`` are the export: the element codes and E8M0 scales a block-scaled GEMM or a checkpoint stores
(``MXTensor``; the packed contract is DESIGN.md section 9.13, restated by ``tests/mx_pack_reference.py``), cut from the same rounded
patterns as the fake quant, so that ``mx_dequantize(mx_quantize(x))`` has the bits of ``mx_fake_quant(x)``.  ``export_graph_mx`` packs
every MX weight of a graph in one launch.  ``mx_matmul`` / ``mx_linear`` multiply two packed tensors on the block-scaled MFMA
(``ppq_amd/csrc/mx_gemm.hip``), ``mx_conv2d`` / ``mx_conv2d_packed`` convolve them (``mx_conv.hip``, an implicit
GEMM; section 9.15): the hardware in the loop of both the simulation and the export.  ``deploy_graph_mx`` puts the Conv / Gemm /
MatMul of a ``quantize_graph_mx`` graph on those kernels through the executor's operation overrides.

``quantize_graph_mx`` puts MX on the inputs of Conv / Gemm / MatMul of a harness graph through the executor's delegator seam
(``TorchExecutor.register_quantize_delegate``): ``MXDelegator`` follows the reference's delegator protocol
(``delegator(tensor, config)``, ppq/executor/torch.py:296-323) and works in its executor unchanged.
"""
from enum import Enum
from typing import Dict, List, Optional

import torch
from torch.autograd import Function

from .core import (FloatingQuantizationConfig, LinearQuantizationConfig, QuantizationStates)
from .ffi import CUDA, MX_BLOCK, MX_FORMATS, MX_SCALE_RULES, MXPackPlan, MXQuantizePlan, mx_format_id, mx_packed_shapes, mx_rule_id

# name -> (exponent bits, mantissa bits, smallest normal exponent, emax, largest normal); MXINT8: k / 64 with |k| <= 127
_SPEC = {
    'MXFP8_E4M3': (4, 3, -6, 8, 448.0),
    'MXFP8_E5M2': (5, 2, -14, 15, 57344.0),
    'MXFP6_E3M2': (3, 2, -2, 4, 28.0),
    'MXFP6_E2M3': (2, 3, 0, 2, 7.5),
    'MXFP4_E2M1': (2, 1, 0, 2, 6.0),
    'MXINT8': (0, 6, None, 0, 127.0 / 64.0),
}


class MXFormat(Enum):
    """The element formats of OCP MX v1.0; the value is the id the HIP library knows the format by."""
    MXFP8_E4M3 = MX_FORMATS['MXFP8_E4M3']
    MXFP8_E5M2 = MX_FORMATS['MXFP8_E5M2']
    MXFP6_E3M2 = MX_FORMATS['MXFP6_E3M2']
    MXFP6_E2M3 = MX_FORMATS['MXFP6_E2M3']
    MXFP4_E2M1 = MX_FORMATS['MXFP4_E2M1']
    MXINT8 = MX_FORMATS['MXINT8']

    @ property
    def exponent_bits(self) -> int: return _SPEC[self.name][0]

    @ property
    def mantissa_bits(self) -> int: return _SPEC[self.name][1]

    @ property
    def emax(self) -> int: return _SPEC[self.name][3]

    @ property
    def max_normal(self) -> float: return _SPEC[self.name][4]

    @ property
    def is_float(self) -> bool: return self is not MXFormat.MXINT8

    @ classmethod
    def of(cls, format) -> 'MXFormat':
        """``format`` as a member: a member, its name, or the library's id."""
        if isinstance(format, cls): return format
        return cls(mx_format_id(format))


class MXScaleRule(Enum):
    """How a block's E8M0 scale is made from its values; the value is the id the HIP library knows the
    rule by.  With ``code_f`` the floor code ``max(exponent(amax) - emax, 0)`` and every code clamped to 254:
    ``FLOOR`` -- ``code_f``, the OCP rule: amax / X may lie above the largest normal and saturate;
    ``CEIL`` -- ``code_f + 1`` when amax / X would saturate: the largest element is never clipped;
    ``EVEN`` -- the floor code of amax rounded to the element's precision: one more only when amax rounds up into the next binade;
    ``MSE`` -- of ``code_f`` and ``code_f + 1`` the one with the smaller squared error over the block (a tie keeps ``code_f``)."""
    FLOOR = MX_SCALE_RULES['FLOOR']
    CEIL = MX_SCALE_RULES['CEIL']
    EVEN = MX_SCALE_RULES['EVEN']
    MSE = MX_SCALE_RULES['MSE']

    @ classmethod
    def of(cls, rule) -> 'MXScaleRule':
        """``rule`` as a member: a member, its name, the library's id, or None (FLOOR)."""
        if isinstance(rule, cls): return rule
        return cls(mx_rule_id(rule))


def _bits_to_float(bits: torch.Tensor) -> torch.Tensor:
    return bits.to(torch.int32).view(torch.float32)


def _pow2(biased: torch.Tensor) -> torch.Tensor:
    """2^(biased - 127) for 0 <= biased <= 254 (2^-127 is the subnormal 0x00400000)."""
    return _bits_to_float(torch.where(biased > 0, biased << 23, torch.full_like(biased, 0x00400000)))


def _mx_round(umag: torch.Tensor, format: MXFormat) -> torch.Tensor:
    """The cast of |u| on its float32 pattern (``mx_round`` of mx_common.hpp): the pattern of the nearest element value, ties to
    the even encoding, saturating at the largest normal.  A NaN pattern gives a pattern nobody may use."""
    _, m, emin, _, max_normal = _SPEC[format.name]
    max_bits = int(torch.tensor(max_normal, dtype=torch.float32).view(torch.int32))
    if format.is_float:
        shift = 23 - m
        finite = torch.where(umag > 0x7f800000, torch.zeros_like(umag), umag)                         # a NaN pattern plus the rounding add would wrap
        normal = (finite + ((1 << (shift - 1)) - 1) + ((finite >> shift) & 1)) & ~((1 << shift) - 1)  # RNE on the mantissa
        grid = (torch.round(_bits_to_float(umag) * 2.0 ** (m - emin)) * 2.0 ** (emin - m)).view(torch.int32)
        r = torch.where(umag < ((emin + 127) << 23), grid, normal)
    else:
        r = (torch.round(_bits_to_float(umag) * 64.0) * 0.015625).view(torch.int32)
    return torch.minimum(r, torch.full_like(r, max_bits))


def _mx_values(x: torch.Tensor, code: torch.Tensor, format: MXFormat) -> torch.Tensor:
    """cast(x / X) * X for X = 2^(code - 127); a NaN keeps its bits."""
    ubits = (x * _pow2(254 - code)).view(torch.int32)
    umag = ubits & 0x7fffffff
    y = _bits_to_float(_mx_round(umag, format) | (ubits & -0x80000000)) * _pow2(code)
    return torch.where(umag > 0x7f800000, x, y)


def _mx_scale_code(x: torch.Tensor, format: MXFormat, rule: MXScaleRule) -> torch.Tensor:
    """The E8M0 code (int32, ``[..., nb, 1]``) of every block of ``x`` ``[..., nb, 32]`` under ``rule``: ``mx_rule_code`` and ``MxMse``
    of mx_common.hpp in torch ops."""
    _, m, _, emax, max_normal = _SPEC[format.name]
    mag = x.view(torch.int32) & 0x7fffffff
    finite = mag < 0x7f800000
    amax = torch.where(finite, mag, torch.zeros_like(mag)).amax(dim=-1, keepdim=True)
    floor_code = ((amax >> 23) - emax).clamp_(min=0)
    if rule is MXScaleRule.FLOOR: return floor_code
    if rule is MXScaleRule.CEIL:
        max_bits = int(torch.tensor(max_normal, dtype=torch.float32).view(torch.int32))
        scaled = (_bits_to_float(amax) * _pow2(254 - floor_code)).view(torch.int32)              # exact: a power of two
        return (floor_code + (scaled > max_bits).to(torch.int32)).clamp_(max=254)
    if rule is MXScaleRule.EVEN:
        return (((amax + (1 << (22 - m))) >> 23) - emax).clamp_(min=0, max=254)
    c0, c1 = floor_code, (floor_code + 1).clamp_(max=254)
    errors = []
    for c in (c0, c1):                                 # the same ops in the same order: equal candidates give equal sums
        d = _mx_values(x, c, format) - x               # exact in float32
        d = torch.where(finite, d, torch.zeros_like(d)).to(torch.float64)
        errors.append((d * d).sum(dim=-1, keepdim=True))
    return torch.where(errors[1] < errors[0], c1, c0)


def _mx_torch(tensor: torch.Tensor, format: MXFormat, axis: int, scale_codes: Optional[torch.Tensor],
              scale_rule: MXScaleRule = MXScaleRule.FLOOR) -> torch.Tensor:
    """The contract in torch ops, on the tensor's device: integer arithmetic on the float32 patterns, exact float32 products."""
    length = tensor.shape[axis]
    nb = (length + MX_BLOCK - 1) // MX_BLOCK
    x = tensor.movedim(axis, -1)
    lead = list(x.shape[:-1])
    x = x.contiguous()
    if nb * MX_BLOCK != length:                       # zeros take no part in amax; the padding is cut off again below
        x = torch.nn.functional.pad(x, (0, nb * MX_BLOCK - length))
    x = x.reshape(lead + [nb, MX_BLOCK])
    code = _mx_scale_code(x, format, scale_rule)
    y = _mx_values(x, code, format)                   # NaN: the input's own bits
    y = y.reshape(lead + [nb * MX_BLOCK])[..., :length].movedim(-1, axis)
    if scale_codes is not None:
        scale_codes.copy_(code.reshape(lead + [nb]).movedim(-1, axis).to(torch.uint8))
    return y.contiguous()


def _check_codes(tensor: torch.Tensor, axis: int, scale_codes) -> None:
    if scale_codes is None: return
    want = list(tensor.shape)
    want[axis] = (want[axis] + MX_BLOCK - 1) // MX_BLOCK
    if not (isinstance(scale_codes, torch.Tensor) and scale_codes.dtype == torch.uint8 and list(scale_codes.shape) == want):
        raise RuntimeError(f'scale_codes must be a uint8 tensor of shape {want}')


def _check_input(tensor, axis) -> int:
    """The argument checks of ``mx_fake_quant`` and ``mx_quantize``; returns the axis counted from the front."""
    if not isinstance(tensor, torch.Tensor): raise TypeError(f'expected a torch.Tensor, got {type(tensor)}')
    if tensor.dtype != torch.float32: raise RuntimeError('Kernel Failure, Invalid dtype of Input tensor: Value(Expect to be FP32)')
    if tensor.dim() == 0 or not isinstance(axis, int) or not -tensor.dim() <= axis < tensor.dim():
        raise RuntimeError(f'Kernel Failure, axis {axis} out of range for a {tensor.dim()}-d tensor')
    if tensor.numel() == 0: raise RuntimeError('Kernel Failure, Tensor is empty: Value')
    return axis % tensor.dim()


class _MXFakeQuant(Function):
    @ staticmethod
    def forward(ctx, tensor, format, axis, scale_codes, use_kernels, scale_rule):
        if use_kernels: return CUDA.MXQuantize(tensor, format, axis, MX_BLOCK, scale_codes, scale_rule)
        return _mx_torch(tensor, format, axis, scale_codes, scale_rule)

    @ staticmethod
    def backward(ctx, dy: torch.Tensor):
        return dy, None, None, None, None, None


def mx_fake_quant(tensor: torch.Tensor, format, axis: int = -1, scale_codes: torch.Tensor = None, use_kernels: bool = True,
                  scale_rule=MXScaleRule.FLOOR) -> torch.Tensor:
    """MX fake quant of ``tensor`` with blocks of 32 along ``axis``; straight-through backward (``dy`` as it is).
    ``scale_codes``: optional uint8 tensor (the input's shape, the axis replaced by ceil(len / 32)) that receives the E8M0 codes.
    ``use_kernels=True``: the HIP kernels (the tensor must be on the GPU).  ``False``: the torch restatement of the same contract
    on whatever device the tensor lives on -- identical bits.  ``scale_rule``: how the block's scale is made (``MXScaleRule``, its
    name or id): FLOOR, the OCP rule, by default."""
    format, scale_rule = MXFormat.of(format), MXScaleRule.of(scale_rule)
    axis = _check_input(tensor, axis)
    _check_codes(tensor, axis, scale_codes)
    return _MXFakeQuant.apply(tensor, format, axis, scale_codes, use_kernels, scale_rule)


# ---- the packed export ------------------------------------------------------------------------------------
def _element_bits(format: MXFormat) -> int:
    return 8 if format is MXFormat.MXINT8 else 1 + format.exponent_bits + format.mantissa_bits


def _mx_pack_torch(tensor: torch.Tensor, format: MXFormat, axis: int, scale_rule: MXScaleRule = MXScaleRule.FLOOR):
    """The packed contract in torch ops, on the tensor's device: the rounded pattern of ``_mx_torch``, then the code read off it."""
    _, m, emin, _, _ = _SPEC[format.name]
    width, fp8 = _element_bits(format), format in (MXFormat.MXFP8_E4M3, MXFormat.MXFP8_E5M2)
    length = tensor.shape[axis]
    nb = (length + MX_BLOCK - 1) // MX_BLOCK
    x = tensor.movedim(axis, -1)
    lead = list(x.shape[:-1])
    x = x.contiguous()
    if nb * MX_BLOCK != length: x = torch.nn.functional.pad(x, (0, nb * MX_BLOCK - length))      # +0: code 0
    x = x.reshape(lead + [nb, MX_BLOCK])
    bits = x.view(torch.int32)
    mag = bits & 0x7fffffff
    sign = (bits >> 31) & 1
    isnan = mag > 0x7f800000
    scale = _mx_scale_code(x, format, scale_rule)
    umag = (x * _pow2(254 - scale)).view(torch.int32) & 0x7fffffff
    r = _mx_round(umag, format)
    if format.is_float:
        shift = 23 - m
        index = (_bits_to_float(r) * 2.0 ** (m - emin)).to(torch.int32)                            # the grid's index: exact
        code = torch.where(r < ((emin + 127) << 23), index, (r >> shift) - ((emin + 126) << m))     # emin + 126 = 127 - bias
        if fp8: code = torch.where(isnan, torch.full_like(code, 0x7f), code)
        code = code | (sign << (width - 1))
    else:
        k = (_bits_to_float(r) * 64.0).to(torch.int32)
        code = torch.where(sign == 1, -k, k) & 0xff
    if not fp8:                                        # no NaN encoding: the block is NaN as a whole
        dead = isnan.any(dim=-1, keepdim=True)
        code = torch.where(dead, torch.zeros_like(code), code)
        scale = torch.where(dead, torch.full_like(scale, 0xff), scale)
    if width == 4:
        packed = code[..., 0::2] | (code[..., 1::2] << 4)
    elif width == 6:                                   # four codes, three bytes
        c = code.reshape(lead + [nb, MX_BLOCK // 4, 4])
        packed = torch.stack([c[..., 0] | (c[..., 1] << 6), (c[..., 1] >> 2) | (c[..., 2] << 4), (c[..., 2] >> 4) | (c[..., 3] << 2)], dim=-1) & 0xff
    else:
        packed = code
    elements = packed.reshape(lead + [nb * 4 * width]).to(torch.uint8)
    return elements, scale.reshape(lead + [nb]).to(torch.uint8)


def _mx_unpack_torch(elements: torch.Tensor, scales: torch.Tensor, format: MXFormat, shape, axis: int) -> torch.Tensor:
    """value(code) * 2^(scale - 127) in torch ops, on the tensors' device."""
    _, m, emin, _, _ = _SPEC[format.name]
    width, fp8 = _element_bits(format), format in (MXFormat.MXFP8_E4M3, MXFormat.MXFP8_E5M2)
    lead, nb = list(scales.shape[:-1]), scales.shape[-1]
    e = elements.to(torch.int32)
    if width == 4:
        code = torch.stack([e & 15, e >> 4], dim=-1)
    elif width == 6:
        b = e.reshape(lead + [nb * MX_BLOCK // 4, 3])
        code = torch.stack([b[..., 0], (b[..., 0] >> 6) | (b[..., 1] << 2), (b[..., 1] >> 4) | (b[..., 2] << 4), b[..., 2] >> 2], dim=-1) & 63
    else:
        code = e
    code = code.reshape(lead + [nb, MX_BLOCK])
    s = scales.to(torch.int32).unsqueeze(-1)
    X = _pow2(s.clamp(max=254))
    nan = (s == 0xff).expand_as(code)
    nan_bits = torch.full_like(code, 0x7fc00000)
    if format.is_float:
        shift = 23 - m
        sign = ((code >> (width - 1)) & 1) << 31
        mag = code & ((1 << (width - 1)) - 1)
        field, man = mag >> m, mag & ((1 << m) - 1)
        sub = (man.to(torch.float32) * 2.0 ** (emin - m)).view(torch.int32)
        y = _bits_to_float(torch.where(field > 0, (mag << shift) + ((emin + 126) << 23), sub) | sign) * X
        if format is MXFormat.MXFP8_E4M3: nan = nan | (mag == 0x7f)
        if format is MXFormat.MXFP8_E5M2:
            nan = nan | ((field == 31) & (man != 0))
            y = torch.where((field == 31) & (man == 0), _bits_to_float(sign | 0x7f800000), y)
        if fp8: nan_bits = nan_bits | sign
    else:
        y = torch.where(code >= 128, code - 256, code).to(torch.float32) * 0.015625 * X
    y = torch.where(nan, _bits_to_float(nan_bits), y)
    return y.reshape(lead + [nb * MX_BLOCK])[..., :shape[axis]].movedim(-1, axis).contiguous()


class MXTensor:
    """A tensor in packed MX form: ``elements`` (uint8, ``shape`` without ``axis`` plus ``[nb * B]``) and ``scales`` (uint8 E8M0
    codes, ``shape`` without ``axis`` plus ``[nb]``) -- the block axis is last; ``format`` is an ``MXFormat``, ``shape`` the shape of
    the float tensor and ``axis`` (counted from the front) the axis its blocks run along."""
    def __init__(self, format, shape, axis: int, elements: torch.Tensor, scales: torch.Tensor):
        self.format = MXFormat.of(format)
        self.shape = tuple(int(d) for d in shape)
        if not isinstance(axis, int) or isinstance(axis, bool) or not self.shape or not -len(self.shape) <= axis < len(self.shape):
            raise ValueError(f'MXTensor: axis {axis!r} out of range for shape {list(self.shape)}')
        self.axis = axis % len(self.shape)
        eshape, sshape = mx_packed_shapes(self.shape, self.axis, self.format)
        for name, t, want in (('elements', elements, eshape), ('scales', scales, sshape)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8: raise ValueError(f'MXTensor: {name} must be a uint8 tensor')
            if list(t.shape) != want:
                raise ValueError(f'MXTensor: {name} of shape {list(t.shape)}, but {self.format.name} of {list(self.shape)} along axis {self.axis} has {want}')
        if elements.device != scales.device: raise ValueError('MXTensor: elements and scales live on different devices')
        self.elements, self.scales = elements, scales

    @ property
    def nbytes(self) -> int: return self.elements.numel() + self.scales.numel()

    @ property
    def device(self): return self.elements.device

    def to(self, device) -> 'MXTensor':
        return MXTensor(self.format, self.shape, self.axis, self.elements.to(device), self.scales.to(device))

    def dequantize(self, use_kernels: bool = True) -> torch.Tensor:
        """The float32 tensor of ``shape``: value(code) * 2^(scale - 127).  ``use_kernels=True``: the HIP kernel (the tensors must
        be on the GPU); ``False``: torch ops on whatever device they live on -- identical bits."""
        if use_kernels: return CUDA.MXUnpack(self.elements, self.scales, self.format, self.shape, self.axis)
        return _mx_unpack_torch(self.elements, self.scales, self.format, self.shape, self.axis)

    def matmul(self, other: 'MXTensor', bias: torch.Tensor = None, use_kernels: bool = True) -> torch.Tensor:
        """``mx_matmul(self, other, bias, use_kernels)``: ``self . other^T`` in float32."""
        return mx_matmul(self, other, bias, use_kernels)

    def conv2d(self, weight: 'MXTensor', bias: torch.Tensor = None, stride=1, padding=0, dilation=1, use_kernels: bool = True) -> torch.Tensor:
        """``mx_conv2d_packed(self, weight, bias, stride, padding, dilation, use_kernels)``: ``self`` is the activation."""
        return mx_conv2d_packed(self, weight, bias, stride, padding, dilation, use_kernels)

    def to_dict(self) -> dict:
        """Tensors, ints and the format's name only: ``torch.save`` round-trips it (``from_dict``)."""
        return {'format': self.format.name, 'shape': torch.tensor(self.shape, dtype=torch.int64), 'axis': self.axis,
                'elements': self.elements, 'scales': self.scales}

    @ classmethod
    def from_dict(cls, d: dict) -> 'MXTensor':
        """The inverse of ``to_dict``; dtype and shapes are checked against format, shape and axis (ValueError)."""
        missing = [k for k in ('format', 'shape', 'axis', 'elements', 'scales') if k not in d]
        if missing: raise ValueError(f'MXTensor.from_dict: missing {missing}')
        return cls(d['format'], [int(v) for v in d['shape']], d['axis'], d['elements'], d['scales'])

    def __repr__(self) -> str:
        return f'MXTensor({self.format.name}, shape={list(self.shape)}, axis={self.axis}, {self.nbytes} bytes on {self.device})'


def mx_quantize(tensor: torch.Tensor, format, axis: int = -1, use_kernels: bool = True, scale_rule=MXScaleRule.FLOOR) -> MXTensor:
    """``tensor`` in packed MX form, blocks of 32 along ``axis``: the blocks, scales and roundings of ``mx_fake_quant``, stored as
    element codes and E8M0 scale codes.  ``use_kernels=True``: the HIP kernel (the tensor must be on the GPU); ``False``: the torch
    restatement on whatever device the tensor lives on -- identical bytes.  ``scale_rule``: as for ``mx_fake_quant``; the rule is
    not part of the packed tensor, whose scales say all a reader needs."""
    format, scale_rule = MXFormat.of(format), MXScaleRule.of(scale_rule)
    axis = _check_input(tensor, axis)
    if use_kernels: elements, scales = CUDA.MXPack(tensor, format, axis, MX_BLOCK, scale_rule)
    else: elements, scales = _mx_pack_torch(tensor.detach(), format, axis, scale_rule)
    return MXTensor(format, tensor.shape, axis, elements, scales)


def mx_dequantize(mxt: MXTensor, use_kernels: bool = True) -> torch.Tensor:
    """``mxt`` as float32.  Without NaN in the source, ``mx_dequantize(mx_quantize(x))`` has the bits of ``mx_fake_quant(x)``
    (MXINT8: -0 comes back as +0)."""
    if not isinstance(mxt, MXTensor): raise TypeError(f'expected an MXTensor, got {type(mxt)}')
    return mxt.dequantize(use_kernels)


# ---- the fused epilogue of the GEMM and the convolution ------------------------------------------------------
def relu_positive_zero(v: torch.Tensor) -> torch.Tensor:
    """The ReLU of the fused epilogue in torch ops: ``v > 0 ? v : +0`` with a NaN staying the NaN it is.  Unlike ``F.relu`` it never
    returns -0: the sign of a zero is a bit of the packed code."""
    return torch.where(v > 0, v, torch.where(v != v, v, torch.zeros_like(v)))


def _check_fused(what: str, like, shape, residual, relu, out_format, out_float):
    """The checks of the keywords ``residual`` / ``relu`` / ``out_format`` / ``out_float``; ``like`` is an operand (for the device),
    ``shape`` the result's.  Returns (fused, out_format as a member or None, out_float as a bool)."""
    fused = residual is not None or bool(relu) or out_format is not None or out_float is not None
    if not fused: return False, None, True
    if out_format is not None:
        out_format = MXFormat.of(out_format)
        if not out_format.is_float: raise RuntimeError(f'{what}: out_format {out_format.name} is not a format the fused epilogue packs')
    if out_float is None: out_float = out_format is None
    if out_format is None and not out_float: raise RuntimeError(f'{what}: no output: out_format is None and out_float is False')
    if residual is not None:
        if not isinstance(residual, torch.Tensor) or residual.dtype != torch.float32: raise RuntimeError(f'{what}: residual must be a float32 tensor')
        if list(residual.shape) != list(shape): raise RuntimeError(f'{what}: residual of shape {list(residual.shape)}, expected {list(shape)}')
        if residual.device != like.device: raise RuntimeError(f'{what}: residual is on {residual.device}, the operands on {like.device}')
    return True, out_format, bool(out_float)


def _fused_torch(y: torch.Tensor, residual, relu, out_format, out_float, axis: int):
    """The torch arm of the fused epilogue on the float32 result ``y`` of the reference: the same order of operations."""
    if residual is not None: y = y + residual
    if relu: y = relu_positive_zero(y)
    if out_format is None: return y
    packed = mx_quantize(y, out_format, axis, use_kernels=False)
    return (y, packed) if out_float else packed


def _fused_result(y, packed, out_float):
    if packed is None: return y
    return (y, packed) if out_float else packed


# ---- GEMM on the packed tensors ---------------------------------------------------------------------------
def _check_matmul(a, b, bias):
    """The argument checks of ``mx_matmul``; returns (lead shape of a, N, K)."""
    for name, t in (('a', a), ('b', b)):
        if not isinstance(t, MXTensor): raise TypeError(f'mx_matmul: {name}: expected an MXTensor, got {type(t)}')
        if not t.format.is_float: raise RuntimeError(f'mx_matmul: {name} is {t.format.name}, which is not an operand type of the scaled MFMA')
        if t.axis != len(t.shape) - 1:
            raise RuntimeError(f'mx_matmul: {name} of shape {list(t.shape)} is packed along axis {t.axis}, not along its last axis')
    if len(b.shape) != 2: raise RuntimeError(f'mx_matmul: b must be 2-d [N, K], got shape {list(b.shape)}')
    if a.shape[-1] != b.shape[-1]: raise RuntimeError(f'mx_matmul: K mismatch: a has {a.shape[-1]}, b has {b.shape[-1]}')
    if a.device != b.device: raise RuntimeError(f'mx_matmul: a is on {a.device}, b on {b.device}')
    n = b.shape[0]
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32: raise RuntimeError('mx_matmul: bias must be a float32 tensor')
        if list(bias.shape) != [n]: raise RuntimeError(f'mx_matmul: bias of shape {list(bias.shape)}, expected [{n}]')
    return list(a.shape[:-1]), n, a.shape[-1]


def mx_matmul(a: MXTensor, b: MXTensor, bias: torch.Tensor = None, use_kernels: bool = True, residual: torch.Tensor = None,
              relu: bool = False, out_format=None, out_float: bool = None):
    """``a . b^T (+ bias)`` in float32: ``a`` is ``lead + [K]``, ``b`` is ``[N, K]`` (a Gemm weight [out, in], as ``export_graph_mx``
    leaves it), both packed along their last axis in any of the five float formats; the result is ``lead + [N]``.
    ``use_kernels=True``: the packed bytes go to the block-scaled MFMA as they are (``CUDA.MXMatmul``; the tensors must be on the
    GPU).  ``False``: the readable reference on any device -- ``mx_dequantize`` of both, the product in float64, rounded to float32.
    The two are NOT bit-identical: the kernel accumulates in float32 in the hardware's order (DESIGN.md section 9.14 bounds the
    difference by K 2^-23 sum |a_k| |b_k|); they agree exactly on an output of one non-zero term, subnormal results included.
    The fused epilogue, all in the ONE launch: ``residual`` (float32, the result's shape) is added after the
    bias; ``relu`` is ``v > 0 ? v : +0`` with NaN kept; ``out_format`` (a float MX format) returns the result as an ``MXTensor`` packed
    along its last axis -- the bytes of ``mx_quantize`` of the float result --, ``out_format`` with ``out_float=True`` returns
    ``(tensor, MXTensor)``; ``relu`` / ``residual`` alone return the float tensor.  With the defaults this is the plain kernel."""
    lead, n, k = _check_matmul(a, b, bias)
    fused, out_format, out_float = _check_fused('mx_matmul', a, lead + [n], residual, relu, out_format, out_float)
    if use_kernels:
        e = a.elements.reshape(-1, a.elements.shape[-1])
        s = a.scales.reshape(-1, a.scales.shape[-1])
        if not fused: return CUDA.MXMatmul(e, s, a.format, b.elements, b.scales, b.format, k, bias).reshape(lead + [n])
        y, oe, os_ = CUDA.MXMatmulFused(e, s, a.format, b.elements, b.scales, b.format, k, bias, residual.reshape(-1, n) if residual is not None else None,
                                        relu, out_format, out_float)
        if y is not None: y = y.reshape(lead + [n])
        packed = MXTensor(out_format, lead + [n], len(lead), oe.reshape(lead + [oe.shape[-1]]), os_.reshape(lead + [os_.shape[-1]])) if oe is not None else None
        return _fused_result(y, packed, out_float)
    x, w = a.dequantize(use_kernels=False).to(torch.float64), b.dequantize(use_kernels=False).to(torch.float64)
    y = x.reshape(-1, k) @ w.t()
    if bias is not None: y = y + bias.to(torch.float64)
    y = y.to(torch.float32).reshape(lead + [n])
    return _fused_torch(y, residual, relu, out_format, out_float, -1) if fused else y


def mx_linear(x: torch.Tensor, weight: MXTensor, activation_format, bias: torch.Tensor = None, use_kernels: bool = True,
              residual: torch.Tensor = None, relu: bool = False, out_format=None, out_float: bool = None, scale_rule=MXScaleRule.FLOOR):
    """A linear layer on an MX weight as it runs in deployment: ``mx_quantize(x, activation_format, -1)``, then ``mx_matmul`` with
    ``weight`` ``[N, K]`` -- two launches, the bias added in the GEMM's epilogue (one float32 add per output).  ``residual``, ``relu``,
    ``out_format`` and ``out_float`` are ``mx_matmul``'s; ``scale_rule`` is the rule of the activation's quantisation (``out_format``
    is packed by FLOOR)."""
    return mx_matmul(mx_quantize(x, activation_format, -1, use_kernels=use_kernels, scale_rule=scale_rule), weight, bias, use_kernels, residual, relu, out_format, out_float)


# ---- convolution on the packed tensors --------------------------------------------------------------------
def _pair(value, name: str, least: int):
    """An int or a pair of ints (h, w), each at least ``least``."""
    pair = (value, value) if isinstance(value, int) and not isinstance(value, bool) else tuple(value)
    if len(pair) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in pair):
        raise RuntimeError(f'mx_conv2d: {name} must be an int or a pair of ints, got {value!r}')
    if min(pair) < least: raise RuntimeError(f'mx_conv2d: {name} must be at least {least}, got {value!r}')
    return pair


def _check_conv(x, w, bias, stride, padding, dilation):
    """The argument checks of ``mx_conv2d_packed``; returns (stride, padding, dilation, (OH, OW)), each a pair."""
    for name, t in (('x', x), ('w', w)):
        if not isinstance(t, MXTensor): raise TypeError(f'mx_conv2d: {name}: expected an MXTensor, got {type(t)}')
        if not t.format.is_float: raise RuntimeError(f'mx_conv2d: {name} is {t.format.name}, which is not an operand type of the scaled MFMA')
        if len(t.shape) != 4: raise RuntimeError(f'mx_conv2d: {name} must be 4-d, got shape {list(t.shape)}')
        if t.axis != 1: raise RuntimeError(f'mx_conv2d: {name} of shape {list(t.shape)} is packed along axis {t.axis}, not along its channels (axis 1)')
    if x.shape[1] != w.shape[1]:
        raise RuntimeError(f'mx_conv2d: C mismatch: x has {x.shape[1]} channels, w has {w.shape[1]} (groups must be 1)')
    if x.device != w.device: raise RuntimeError(f'mx_conv2d: x is on {x.device}, w on {w.device}')
    if 0 in x.shape or 0 in w.shape: raise RuntimeError(f'mx_conv2d: empty operand: x {list(x.shape)}, w {list(w.shape)}')
    stride, padding, dilation = _pair(stride, 'stride', 1), _pair(padding, 'padding', 0), _pair(dilation, 'dilation', 1)
    out = tuple((x.shape[2 + i] + 2 * padding[i] - dilation[i] * (w.shape[2 + i] - 1) - 1) // stride[i] + 1 for i in range(2))
    if min(out) < 1:
        raise RuntimeError(f'mx_conv2d: a {w.shape[2]} x {w.shape[3]} kernel with dilation {dilation} does not fit an input of '
                           f'{x.shape[2]} x {x.shape[3]} padded by {padding}')
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32: raise RuntimeError('mx_conv2d: bias must be a float32 tensor')
        if list(bias.shape) != [w.shape[0]]: raise RuntimeError(f'mx_conv2d: bias of shape {list(bias.shape)}, expected [{w.shape[0]}]')
    return stride, padding, dilation, out


def mx_conv2d_packed(x: MXTensor, w: MXTensor, bias: torch.Tensor = None, stride=1, padding=0, dilation=1, use_kernels: bool = True,
                     residual: torch.Tensor = None, relu: bool = False, out_format=None, out_float: bool = None):
    """``conv2d(x, w) (+ bias)`` in float32: ``x`` is ``[N, C, H, W]``, ``w`` is ``[O, C, kh, kw]`` (a Conv weight as
    ``export_graph_mx`` leaves it), both packed along axis 1 in any of the five float formats; ``stride``, ``padding`` (symmetric, as
    ``F.conv2d`` takes it) and ``dilation`` are ints or (h, w) pairs, groups is 1.  The result is ``[N, O, OH, OW]``.
    ``use_kernels=True``: the packed bytes go to the block-scaled MFMA as they are, the rows of the implicit GEMM gathered by address
    (``CUDA.MXConv2d``; the tensors must be on the GPU); the result has channels-last strides.  ``False``: the readable reference
    on any device -- ``mx_dequantize`` of both, the windows gathered by slicing, the product in float64, rounded to float32.
    As for ``mx_matmul`` the two are not bit-identical (K 2^-23 sum |x| |w| with K = kh kw 32 ceil(C / 32));
    the kernel has the bits of ``mx_matmul`` on the gathered rows.
    The fused epilogue, all in the ONE launch: ``residual`` (float32 ``[N, O, OH, OW]``; channels-last is
    read in place, anything else is copied) is added after the bias; ``relu`` is ``v > 0 ? v : +0`` with NaN kept; ``out_format`` (a
    float MX format) returns the result as an ``MXTensor`` ``[N, O, OH, OW]`` packed along axis 1 -- the bytes of ``mx_quantize`` of
    the float result, and what this function takes as ``x`` --, ``out_format`` with ``out_float=True`` returns ``(tensor, MXTensor)``;
    ``relu`` / ``residual`` alone return the float tensor.  With the defaults this is the plain kernel."""
    (sh, sw), (ph, pw), (dh, dw), (oh, ow) = _check_conv(x, w, bias, stride, padding, dilation)
    shape = [x.shape[0], w.shape[0], oh, ow]
    fused, out_format, out_float = _check_fused('mx_conv2d', x, shape, residual, relu, out_format, out_float)
    if use_kernels:
        if not fused:
            return CUDA.MXConv2d(x.elements, x.scales, x.format, w.elements, w.scales, w.format, x.shape[1], bias, (sh, sw), (ph, pw), (dh, dw))
        y, oe, os_ = CUDA.MXConv2dFused(x.elements, x.scales, x.format, w.elements, w.scales, w.format, x.shape[1], bias, (sh, sw), (ph, pw), (dh, dw),
                                        residual, relu, out_format, out_float)
        return _fused_result(y, MXTensor(out_format, shape, 1, oe, os_) if oe is not None else None, out_float)
    n, c, _, _ = x.shape
    o, _, kh, kw = w.shape
    xf = torch.nn.functional.pad(x.dequantize(use_kernels=False).to(torch.float64), (pw, pw, ph, ph))
    wf = w.dequantize(use_kernels=False).to(torch.float64)
    taps = [xf[:, :, ky * dh: ky * dh + (oh - 1) * sh + 1: sh, kx * dw: kx * dw + (ow - 1) * sw + 1: sw] for ky in range(kh) for kx in range(kw)]
    cols = torch.stack(taps, dim=1).permute(0, 3, 4, 1, 2).reshape(n * oh * ow, kh * kw * c)          # rows (n, oy, ox), K (ky, kx, c)
    y = cols @ wf.permute(0, 2, 3, 1).reshape(o, kh * kw * c).t()
    if bias is not None: y = y + bias.to(torch.float64)
    y = y.to(torch.float32).reshape(n, oh, ow, o).permute(0, 3, 1, 2)
    return _fused_torch(y, residual, relu, out_format, out_float, 1) if fused else y


def mx_conv2d(x: torch.Tensor, weight: MXTensor, activation_format, bias: torch.Tensor = None, stride=1, padding=0, dilation=1,
              groups: int = 1, use_kernels: bool = True, residual: torch.Tensor = None, relu: bool = False, out_format=None,
              out_float: bool = None, scale_rule=MXScaleRule.FLOOR):
    """A convolution on an MX weight as it runs in deployment: ``mx_quantize(x, activation_format, 1)`` -- ``x`` ``[N, C, H, W]``,
    contiguous or channels-last --, then ``mx_conv2d_packed`` with ``weight`` ``[O, C, kh, kw]``: two launches, the bias added in the
    kernel's epilogue (one float32 add per output).  ``residual``, ``relu``, ``out_format`` and ``out_float`` are ``mx_conv2d_packed``'s;
    ``scale_rule`` is the rule of the activation's quantisation (``out_format`` is packed by FLOOR)."""
    if groups != 1: raise RuntimeError(f'mx_conv2d: groups must be 1, got {groups}')
    if isinstance(x, torch.Tensor) and x.dim() != 4: raise RuntimeError(f'mx_conv2d: x must be 4-d [N, C, H, W], got shape {list(x.shape)}')
    return mx_conv2d_packed(mx_quantize(x, activation_format, 1, use_kernels=use_kernels, scale_rule=scale_rule), weight, bias, stride, padding, dilation, use_kernels,
                            residual, relu, out_format, out_float)


def _activated(config) -> bool:
    return config is None or QuantizationStates.is_activated(config.state)


class MXWeightGroup:
    """The MX weights of one graph as ONE launch (``ffi.MXQuantizePlan`` -> ``ppqhip_mx_fq_multi``), shared by their delegators.
    The arena is refilled when a member is asked for and ITS weight is not the one the arena was filled from: another tensor
    (``data_ptr``, shape or strides changed: the plan is rebuilt) or the same one written in place (``_version``).  One refill
    serves every member, so a forward over unchanged weights launches nothing, and a step that updated all of them launches once."""
    def __init__(self, members):
        self.members = [tuple(m[:3]) for m in members]                                 # [(variable, format, axis)]
        self.rules = [MXScaleRule.of(m[3] if len(m) > 3 else None) for m in members]   # each member's scale rule (an optional fourth entry)
        self.plan = None
        self.stamps: List[tuple] = [None] * len(members)
        self.outputs = None
        self.launches = 0

    @ staticmethod
    def eligible(var, axis: int) -> bool:
        v = var.value
        return (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.numel() > 0 and not v.requires_grad
                and MXQuantizePlan.accepts(v, axis))

    @ staticmethod
    def _stamp(v: torch.Tensor) -> tuple:
        return (v.data_ptr(), v._version, tuple(v.shape), v.stride())

    def output(self, slot: int) -> torch.Tensor:
        if self.stamps[slot] != self._stamp(self.members[slot][0].value): self.refresh()
        return self.outputs[slot]

    def refresh(self) -> None:
        stamps = [self._stamp(var.value) for var, _, _ in self.members]
        same = self.plan is not None and all(a is not None and a[0] == b[0] and a[2:] == b[2:] for a, b in zip(self.stamps, stamps))
        if not same: self.plan = MXQuantizePlan([(var.value, fmt, axis, rule) for (var, fmt, axis), rule in zip(self.members, self.rules)])
        self.outputs = self.plan.run()
        self.stamps = stamps
        self.launches += 1


class MXDelegator:
    """``delegator(tensor, config)`` for ``TorchExecutor.register_quantize_delegate`` (this package's harness and the reference's
    executor alike): MX fake quant of the tensor with blocks along ``axis``.  A config that is not activated (a dequantised
    operation) passes the tensor through, as the default quantize function does.  ``scale_rule``: the ``MXScaleRule`` of the blocks'
    scales (FLOOR by default)."""
    def __init__(self, format, axis: int, use_kernels: bool = True, scale_rule=MXScaleRule.FLOOR):
        self.format = MXFormat.of(format)
        self.scale_rule = MXScaleRule.of(scale_rule)
        self.axis = axis
        self.use_kernels = use_kernels
        self.group, self.slot, self.var = None, None, None     # set by quantize_graph_mx: this weight rides the graph's one launch

    def __call__(self, tensor: torch.Tensor, config=None) -> torch.Tensor:
        if not _activated(config): return tensor
        if self.group is not None and tensor is self.var.value and MXWeightGroup.eligible(self.var, self.axis):
            return self.group.output(self.slot)
        return mx_fake_quant(tensor, self.format, self.axis, use_kernels=self.use_kernels, scale_rule=self.scale_rule)


def _config_rule(config) -> MXScaleRule:
    """The scale rule recorded in a config's detail; an absent entry means FLOOR."""
    return MXScaleRule.of(getattr(config, 'detail', {}).get('MX_SCALE_RULE'))


def _mx_config(format: MXFormat, device, scale_rule: MXScaleRule = MXScaleRule.FLOOR):
    """An ACTIVATED config that describes the element format to every report that reads configs; scale 1, offset 0 (the block
    scales live in the data, not in the config)."""
    if format.is_float:
        c = FloatingQuantizationConfig(exponent=format.exponent_bits, mantissa=format.mantissa_bits, quant_min=-format.max_normal,
                                       quant_max=format.max_normal, calibration='mx')
    else:
        c = LinearQuantizationConfig(symmetrical=True, power_of_2=True, quant_min=-127, quant_max=127, num_of_bits=8, calibration='mx')
    c.scale = torch.ones(1, dtype=torch.float32, device=device)
    c.offset = torch.zeros(1, dtype=torch.float32, device=device)
    c.state = QuantizationStates.ACTIVATED
    c.detail['MX_FORMAT'] = format.name
    if scale_rule is not MXScaleRule.FLOOR: c.detail['MX_SCALE_RULE'] = scale_rule.name
    return c


MX_OPERATIONS = ('Conv', 'Gemm', 'MatMul')


def mx_block_axis(op_type: str, input_index: int) -> int:
    """The axis MX blocks run along for input ``input_index`` of a Conv / Gemm / MatMul: the reduction axis, along which the scaled
    MFMA shares a scale.  Conv: channels (axis 1) of activation and weight; Gemm: the last axis of the activation and of the
    harness's [out, in] weight; MatMul: the last axis of the left operand, the second to last of the right one (axis 0 of a 2-D
    [in, out] weight)."""
    if op_type == 'Conv': return 1
    if op_type == 'MatMul' and input_index == 1: return -2
    return -1


def quantize_graph_mx(graph, executor, weight_format, activation_format, operations=None, use_kernels: bool = True,
                      weight_scale_rule=MXScaleRule.FLOOR, activation_scale_rule=MXScaleRule.FLOOR) -> dict:
    """The policy of ``harness.quantize_graph_fp8`` with MX formats: only the inputs of Conv / Gemm / MatMul are quantised, weights
    with ``weight_format`` and activations with ``activation_format``, blocks along the reduction
    axis (``mx_block_axis``); bias and everything else stay FP32.  Each quantised input gets an ACTIVATED config and an
    ``MXDelegator`` registered on ``executor``; with ``use_kernels`` all weights share one ``MXWeightGroup``.  ``operations``: names
    of the operations to quantise (default: all).  ``weight_scale_rule`` / ``activation_scale_rule``: the ``MXScaleRule`` of the
    weights' resp. the activations' block scales, kept on the delegator and, where it is not FLOOR, as
    ``config.detail['MX_SCALE_RULE']``.  Returns config -> delegator."""
    from .harness import OperationQuantizationConfig, QuantableOperation
    wfmt, afmt = MXFormat.of(weight_format), MXFormat.of(activation_format)
    wrule, arule = MXScaleRule.of(weight_scale_rule), MXScaleRule.of(activation_scale_rule)
    device = getattr(executor, '_device', 'cuda')
    delegators, weights = {}, []

    def fp32():
        c = LinearQuantizationConfig()
        c.state = QuantizationStates.FP32
        return c

    for name, op in list(graph.operations.items()):
        if operations is not None and name not in operations: continue
        in_cfgs = []
        for i, v in enumerate(op.inputs):
            fmt = None
            if op.type in MX_OPERATIONS and i < 2: fmt = wfmt if v.is_parameter else afmt
            if fmt is None:
                in_cfgs.append(fp32())
                continue
            rule = wrule if v.is_parameter else arule
            c = _mx_config(fmt, device, rule)
            d = MXDelegator(fmt, mx_block_axis(op.type, i), use_kernels, rule)
            if v.is_parameter: weights.append((d, v))
            in_cfgs.append(c)
            delegators[c] = d
        qop = QuantableOperation(op, OperationQuantizationConfig(in_cfgs, [fp32() for _ in op.outputs]))
        for v in qop.inputs: v.dest_ops[v.dest_ops.index(op)] = qop
        for v in qop.outputs: v.source_op = qop
        graph.operations[name] = qop
    for c, d in delegators.items(): executor.register_quantize_delegate(c, d)
    if use_kernels and weights:
        group = MXWeightGroup([(v, d.format, d.axis, d.scale_rule) for d, v in weights])
        for k, (d, v) in enumerate(weights): d.group, d.slot, d.var = group, k, v
    return delegators


def export_graph_mx(graph, delegators=None, use_kernels: bool = True) -> Dict[str, MXTensor]:
    """Every parameter ``quantize_graph_mx`` put an MX config on, in packed form, keyed by the variable's name.  The format is the
    ``MXDelegator``'s (``delegators``: what ``quantize_graph_mx`` returned) or, without delegators, ``config.detail['MX_FORMAT']``;
    the axis is ``mx_block_axis``; the scale rule is read where the format is read (the delegator's ``scale_rule`` resp.
    ``config.detail['MX_SCALE_RULE']``, absent: FLOOR).  With ``use_kernels`` all of them are packed by ONE launch (``ffi.MXPackPlan``)."""
    from .harness import QuantableOperation
    names, items = [], []
    for op in graph.operations.values():
        if not isinstance(op, QuantableOperation) or op.type not in MX_OPERATIONS: continue
        for i, (v, c) in enumerate(zip(op.inputs, op.config.input_quantization_config)):
            if not v.is_parameter or i >= 2 or v.name in names: continue
            if delegators is not None:
                d = delegators.get(c)
                if not isinstance(d, MXDelegator): continue
                fmt, rule = d.format, d.scale_rule
            elif 'MX_FORMAT' in getattr(c, 'detail', {}): fmt, rule = MXFormat.of(c.detail['MX_FORMAT']), _config_rule(c)
            else: continue
            value = v.value
            _check_input(value, mx_block_axis(op.type, i))
            names.append(v.name)
            items.append((value.detach(), fmt, mx_block_axis(op.type, i) % value.dim(), rule))
    if not items: return {}
    if not use_kernels:
        return {n: mx_quantize(v, fmt, axis, use_kernels=False, scale_rule=rule) for n, (v, fmt, axis, rule) in zip(names, items)}
    items = [(v if MXPackPlan.accepts(v, axis) else v.contiguous(), fmt, axis, rule) for v, fmt, axis, rule in items]
    packed = MXPackPlan(items).run()
    return {n: MXTensor(fmt, v.shape, axis, e, s) for n, (v, fmt, axis, _), (e, s) in zip(names, items, packed)}


# ---- the graph on the hardware path (DESIGN.md sections 9.15, 9.16) ------------------------------------------------------------------
class MXFusedGroup:
    """One fused launch of ``deploy_graph_mx(fuse=True)``: ``members`` -- the deployed operation, then the Add and / or Relu of its
    tail --, ``residual`` -- the name of the Add's other operand --, ``relu``, ``output`` -- the name of the last tensor --,
    ``out_format`` -- the format it leaves the launch packed in, or None -- and ``notes``: why an Add was not fused or the output
    is float only."""
    def __init__(self, members):
        self.members: List[str] = list(members)
        self.residual: Optional[str] = None
        self.relu = False
        self.output: Optional[str] = None
        self.out_format: Optional[MXFormat] = None
        self.notes: List[str] = []

    def __repr__(self) -> str:
        tail = (f' + {self.residual}' if self.residual else '') + (' relu' if self.relu else '')
        return f'MXFusedGroup({" -> ".join(self.members)}{tail}; {self.out_format.name if self.out_format else "float"}{"; " + "; ".join(self.notes) if self.notes else ""})'


def _handed(op, x: MXTensor, format: MXFormat, axis: int) -> MXTensor:
    """The activation a fused producer handed over packed, checked against what this operation would have quantised itself."""
    if x.format is not format or x.axis != axis:
        raise RuntimeError(f'{op.name}: its activation arrived packed as {x.format.name} along axis {x.axis}, expected {format.name} along axis {axis}')
    return x


class MXDeployment:
    """What ``deploy_graph_mx`` did: ``deployed`` -- the names of the operations that run on the block-scaled MFMA --, ``skipped`` --
    name -> reason for every MX operation that stays on the simulated path --, ``weights`` -- the packed weights
    (``export_graph_mx``).  ``refresh()`` packs the weights again after they changed; ``remove()`` drops the overrides, after which
    the executor runs the simulation again."""
    def __init__(self, graph, executor, delegators=None, use_kernels: bool = True, fuse: bool = False):
        self.graph, self.executor, self.delegators, self.use_kernels, self.fuse = graph, executor, delegators, use_kernels, fuse
        self.deployed: List[str] = []
        self.skipped: Dict[str, str] = {}
        self.groups: Dict[str, MXFusedGroup] = {}     # fuse=True: first operation's name -> what its one launch covers
        self.weights: Dict[str, MXTensor] = {}
        self._operands: Dict[str, MXTensor] = {}      # operation name -> its weight as the kernel takes it
        self._runs: Dict[str, object] = {}            # operation name -> its override
        self.refresh()

    def _format(self, config) -> Optional[MXFormat]:
        if self.delegators is not None:
            d = self.delegators.get(config)
            return d.format if isinstance(d, MXDelegator) else None
        name = getattr(config, 'detail', {}).get('MX_FORMAT')
        return MXFormat.of(name) if name is not None else None

    def _rule(self, config) -> MXScaleRule:
        """The scale rule of a config, read where ``_format`` reads the format."""
        if self.delegators is not None:
            d = self.delegators.get(config)
            return d.scale_rule if isinstance(d, MXDelegator) else MXScaleRule.FLOOR
        return _config_rule(config)

    def _plan(self, op):
        """(run, operand) of an eligible operation, or the reason it is not one; None for an operation without MX inputs."""
        cfgs = op.config.input_quantization_config
        formats = [self._format(c) for c in cfgs[:2]]
        if len(formats) < 2 or all(f is None for f in formats): return None
        x_var, w_var = op.inputs[0], op.inputs[1]
        if x_var.is_parameter or not w_var.is_parameter: return 'the operands are not an activation and a parameter'
        afmt, wfmt = formats
        arule = self._rule(cfgs[0])
        if afmt is None or wfmt is None: return 'only one operand carries an MX format'
        if not (afmt.is_float and wfmt.is_float): return 'MXINT8 is not an operand type of the scaled MFMA'
        if not (_activated(cfgs[0]) and _activated(cfgs[1])): return 'an MX config is not activated'
        packed = self.weights.get(w_var.name)
        if packed is None: return 'export_graph_mx left the weight out'
        use_kernels = self.use_kernels
        if op.type == 'Conv':
            a = op.attributes
            if a.get('group', 1) != 1: return 'a grouped convolution'
            if len(packed.shape) != 4: return f'a {len(packed.shape)}-d Conv weight'
            stride, padding, operand = a.get('strides', 1), a.get('pads', 0), packed

            def run(op, x, **tail):
                bias = x[2] if len(x) > 2 else None
                if isinstance(x[0], MXTensor):         # handed over packed by the producer's fused launch: nothing to quantise
                    return mx_conv2d_packed(_handed(op, x[0], afmt, 1), self._operands[op.name], bias, stride, padding, use_kernels=use_kernels, **tail)
                return mx_conv2d(x[0], self._operands[op.name], afmt, bias, stride, padding, use_kernels=use_kernels, scale_rule=arule, **tail)
        else:
            if len(packed.shape) != 2: return f'a {len(packed.shape)}-d {op.type} weight'
            # a MatMul weight [in, out] is packed along axis 0: its bytes are those of [out, in] packed along axis 1
            operand = packed if op.type == 'Gemm' else MXTensor(packed.format, packed.shape[::-1], 1, packed.elements, packed.scales)

            def run(op, x, **tail):
                bias = x[2] if len(x) > 2 else None
                if isinstance(x[0], MXTensor):
                    return mx_matmul(_handed(op, x[0], afmt, len(x[0].shape) - 1), self._operands[op.name], bias, use_kernels, **tail)
                return mx_linear(x[0], self._operands[op.name], afmt, bias, use_kernels=use_kernels, scale_rule=arule, **tail)
        return run, operand

    def refresh(self) -> None:
        """Pack the weights as they are now and (re)register the overrides."""
        from .harness import QuantableOperation
        self.remove()
        self.weights = export_graph_mx(self.graph, self.delegators, self.use_kernels)
        for name, op in self.graph.operations.items():
            if not isinstance(op, QuantableOperation) or op.type not in MX_OPERATIONS: continue
            plan = self._plan(op)
            if plan is None: continue
            if isinstance(plan, str):
                self.skipped[name] = plan
                continue
            run, self._operands[name] = plan
            self._runs[name] = run
            self.executor.register_operation_override(name, run, takes_packed=self.fuse)
            self.deployed.append(name)
        if self.fuse: self._plan_groups()

    def _plan_groups(self) -> None:
        """A tail behind every deployed operation -- an optional Add whose other operand is a float activation computed earlier,
        then an optional Relu, every intermediate feeding only the next member and being no graph output, every config on the way
        passing through -- and whether the tail's last tensor leaves the launch packed: when every deployed consumer reads it as
        its activation, in one format, along the axis the launch packs (Conv -> Conv, Gemm / MatMul -> Gemm / MatMul)."""
        from .harness import QuantableOperation
        order = self.graph.topological_sort()
        at = {op.name: i for i, op in enumerate(order)}
        outputs, claimed = set(self.graph.outputs), set()

        delegates = getattr(self.executor, '_delegates', {})

        def passes(c) -> bool:                         # the rule of the executor's epilogue plan: not activated and not delegated
            return not _activated(c) and c not in delegates

        def through(op) -> bool:                       # nothing is applied to the tensors the launch does not write one by one
            if not isinstance(op, QuantableOperation): return True
            return all(passes(c) for c in (*op.config.input_quantization_config, *op.config.output_quantization_config))

        def sole_consumer(v, op_type: str):
            if v.name in outputs or len(v.dest_ops) != 1 or v.dest_ops[0].type != op_type: return None
            return v.dest_ops[0]

        for op in order:
            if op.name not in self._runs: continue
            group = MXFusedGroup([op.name])
            t = op.outputs[0]
            if len(op.outputs) != 1 or not all(passes(c) for c in op.config.output_quantization_config):
                group.notes.append('the output config is activated or delegated: no tail, float output')
                self.groups[op.name] = group
                continue
            add = sole_consumer(t, 'Add')
            if add is not None:
                other = [v for v in add.inputs if v is not t]
                why = None
                if len(add.inputs) != 2 or len(other) != 1 or len(add.outputs) != 1: why = 'the Add does not add this output to one other tensor'
                elif add.name in claimed: why = 'the Add belongs to another group'
                elif other[0].is_parameter: why = 'the other operand of the Add is a parameter'
                elif other[0].source_op is not None and at[other[0].source_op.name] > at[op.name]: why = 'the other operand of the Add is computed later'
                elif at[add.name] < at[op.name] or not through(add): why = 'a config of the Add is activated or delegated'
                if why is None:
                    group.members.append(add.name); group.residual = other[0].name
                    claimed.add(add.name)
                    t = add.outputs[0]
                else: group.notes.append(f'Add {add.name} not fused: {why}')
            if add is None or group.residual is not None:
                relu = sole_consumer(t, 'Relu')
                if relu is not None and len(relu.inputs) == 1 and len(relu.outputs) == 1 and through(relu) and relu.name not in claimed:
                    group.members.append(relu.name); group.relu = True
                    claimed.add(relu.name)
                    t = relu.outputs[0]
            group.output = t.name
            takers = [d for d in t.dest_ops if d.name in self._runs]
            kind = (lambda o: 'Conv' if o.type == 'Conv' else 'Gemm')
            if not takers: group.notes.append('float output: no deployed consumer')
            elif any(d.inputs[0] is not t or sum(1 for x in d.inputs if x is t) != 1 for d in takers): group.notes.append('float output: a deployed consumer does not read it as its activation')
            elif any(kind(d) != kind(op) for d in takers): group.notes.append('float output: a deployed consumer packs along another axis')
            elif len({self._format(d.config.input_quantization_config[0]) for d in takers}) != 1: group.notes.append('float output: the deployed consumers read it in different formats')
            elif any(self._rule(d.config.input_quantization_config[0]) is not MXScaleRule.FLOOR for d in takers):
                rules = sorted({self._rule(d.config.input_quantization_config[0]).name for d in takers} - {'FLOOR'})
                group.notes.append(f'float output: a deployed consumer makes its scales by {" / ".join(rules)}, the fused epilogue packs by FLOOR')
            else: group.out_format = self._format(takers[0].config.input_quantization_config[0])
            self.groups[op.name] = group
            self.executor.register_group_override(group.members, self._group_run(group))

    def _group_run(self, group: 'MXFusedGroup'):
        run, names = self._runs[group.members[0]], group.members

        def fn(ops, inputs, need_float):
            residual = None
            if group.residual is not None:
                residual = next(x for x, v in zip(inputs[1], ops[1].inputs) if v.name == group.residual)
                if isinstance(residual, MXTensor): raise RuntimeError(f'{names[0]}: the residual {group.residual} arrived packed, not as float32')
            want_float = group.out_format is None or group.output in need_float
            tail = {}
            if residual is not None or group.relu or group.out_format is not None:
                tail = dict(residual=residual, relu=group.relu, out_format=group.out_format, out_float=want_float)
            out = run(ops[0], inputs[0], **tail)
            y, packed = (out if isinstance(out, tuple) else (None, out) if isinstance(out, MXTensor) else (out, None))
            inner = [v.name for m in ops for v in m.outputs]
            if y is not None: return {n: y for n in inner}, ({group.output: packed} if packed is not None else {})
            return {}, {n: packed for n in inner}
        return fn

    def remove(self) -> None:
        for name in getattr(self, 'groups', {}): self.executor.remove_group_override(name)
        for name in self.deployed: self.executor.remove_operation_override(name)
        self.deployed, self.skipped, self._operands, self._runs, self.groups = [], {}, {}, {}, {}


def deploy_graph_mx(graph, executor, delegators=None, use_kernels: bool = True, fuse: bool = False) -> MXDeployment:
    """Put the MX operations of a ``quantize_graph_mx`` graph on the hardware path: the weights are packed (``export_graph_mx``) and
    every eligible operation gets an operation override on ``executor`` that quantises its activation and runs the packed kernel --
    a Conv with ``group`` 1 ``mx_conv2d`` (the activation delegator's format, the bias, ``strides`` and ``pads``), a Gemm ``mx_linear``,
    a MatMul with a 2-D parameter on the right ``mx_linear`` on the weight's own bytes.  MXINT8 on either side, grouped convolutions,
    a MatMul of two activations and weights the export left out stay on the simulated path (``.skipped``).  ``delegators``: what
    ``quantize_graph_mx`` returned (default: the formats recorded in the configs).  ``use_kernels=False``: the torch arms, any device.
    ``fuse=True``: every deployed operation additionally runs together with its tail -- an optional
    residual ``Add``, then an optional ``Relu`` -- as ONE launch (``TorchExecutor.register_group_override``), and the tail's last
    tensor leaves that launch packed when every deployed consumer reads it as its activation in one format (Conv -> Conv, Gemm ->
    Gemm) and by the FLOOR rule, the one the fused epilogue packs by (a consumer with another ``MXScaleRule`` gets the float tensor and
    quantises it itself): the consumer then quantises nothing.  It is written as float32 only when something reads it as float.  ``.groups``
    records every group: members, residual, relu, ``out_format`` and, in ``notes``, why an Add was not fused or the output not
    packed.  A forward that hooks a member or asks for an intermediate runs that group's operations one by one, as ``fuse=False``."""
    return MXDeployment(graph, executor, delegators, use_kernels, fuse)
