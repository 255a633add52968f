"""Linear INT8 layers as an integer backend runs them: the per-tensor / per-channel INT8 graphs PPQ calibrates,
executed on integers instead of simulated in float32.  An ``Int8Tensor`` holds the codes ``LinearQuantize_ToInt`` makes of a tensor under
a PPQ ``TensorQuantizationConfig``; ``int8_matmul`` and ``int8_conv2d_packed`` multiply two of them on the int8 MFMA of gfx950 with the
int32 accumulator chained over all of K (``csrc/int8_gemm.hip``, ``csrc/int8_conv.hip``) and finish every output once:

    I = sum_k w[o, k] (x[m, k] - zx)       exact, int32
    v = float32(I) * (sx * sw[o])          one conversion (nearest even), one float32 multiply
    v = v + bias[o];  v = v + residual[m, o];  ReLU as v > 0 ? v : +0 (NaN kept)
    q = clamp(round(v / sy) + zy, qmin, qmax)   the bits of LinearQuantize_ToInt on v

``use_kernels=False`` states the same contract in torch ops on any device, with identical bits (``tests/int8_reference.py`` is the NumPy
oracle of both).  Codes are stored as int8: a config whose range lies in 0 .. 255 is stored re-centred, code - 128 and zero point - 128.

A weight may also be INT4 (section 9.23): an ``Int4Weight`` holds codes in -8 .. 7 two per byte, and every layer function takes it where
it takes a weight.  The layer then has the bits of the int8 layer on the same codes, from ONE launch of ``csrc/int4_gemm.hip`` /
``csrc/int4_conv.hip``, which read half the weight bytes and unpack a nibble on its way from LDS to the MFMA.

A depthwise convolution (groups == C, channel multiplier 1; section 9.24) has no reduction over channels for the MFMA: the sum over
``k`` is the sum over the taps of one channel, and ``int8_depthwise_conv2d_packed`` runs it on ``v_dot4c_i32_i8``
(``csrc/int8_dwconv.hip``) on an ``Int8DepthwiseWeight``, with the same tail and the bits of the dense layer on the block-diagonal weight.

Every other grouped convolution (1 < groups < C, or a channel multiplier; section 9.25) runs on the int8 MFMA again:
``int8_grouped_conv2d_packed`` on an ``Int8GroupedWeight`` (``csrc/int8_gconv.hip``), whose rows hold only the channel blocks their
slice of 32 output channels needs -- the bits of the dense layer on the block-diagonal weight at 1 / groups of its work.

A Gemm with at most 64 rows -- a classifier head, a transformer's Gemms at small batch -- is bound by reading its weight once, not by
the MFMA (section 9.26).  ``int8_matmul(..., skinny=True)`` / ``int8_linear(..., skinny=True)`` run it on a kernel of its own
(``csrc/int8_skinny.hip``): a workgroup per 16 columns, K split between its waves, fragments straight from global memory, for int8
and INT4 weights alike -- the same bits, since integer sums do not depend on their order.  The flag is opt-in.

Attention multiplies two ACTIVATIONS (section 9.27): ``int8_bmm`` is the batched ``Q . K^T`` / ``P . V`` of two ``Int8Tensor`` with a
zero point each and no precomputed sums (``csrc/int8_bmm.hip``): one launch for all batches, the row and column sums made in the
kernel from the fragments it holds, and a ``b`` packed along ``N`` transposed on its way to the MFMA.
"""
from typing import Optional

import torch

from .core import QuantizationProperty, rounding_value
from .ffi import BMM_MAX_KP, CUDA, DEPTHWISE_LDS_BYTES, INT8_BLOCK, SKINNY_MAX_M, depthwise_lds_bytes
from .mx import _pair, relu_positive_zero
from .round import ppq_tensor_round

__all__ = ['Int8Tensor', 'Int4Weight', 'int8_quantize', 'int8_dequantize', 'int4_quantize_weight', 'int4_pack', 'int4_unpack', 'int8_matmul', 'int8_bmm', 'int8_linear',
           'int8_conv2d_packed', 'int8_conv2d', 'Int8DepthwiseWeight', 'int8_depthwise_weight', 'int8_depthwise_conv2d_packed', 'int8_depthwise_conv2d',
           'Int8GroupedWeight', 'int8_grouped_weight', 'int8_grouped_conv2d_packed', 'int8_grouped_conv2d']

MAX_KP = 65536           # padded reduction lengths from here on are refused: |I| could leave int32


class Int8Tensor:
    """int8 codes of a tensor of ``shape`` under one linear grid.  ``values``: the codes with axis ``axis`` -- the reduction axis of
    the layer -- moved last and padded to a multiple of 32 (with the zero point; a weight's is 0).  ``scale``: float32, a scalar
    tensor or ``[shape[0]]`` (a weight quantised per output channel); ``zero_point``, ``qmin``, ``qmax``: ints in the stored int8
    domain; ``rounding``: the policy's number.  A weight also carries ``sums``: int32 ``[shape[0]]``, the sum of its codes per row."""
    __slots__ = ('values', 'shape', 'axis', 'scale', 'zero_point', 'qmin', 'qmax', 'rounding', 'sums')

    def __init__(self, values, shape, axis, scale, zero_point, qmin, qmax, rounding, sums=None):
        self.values, self.shape, self.axis = values, tuple(int(d) for d in shape), int(axis)
        self.scale, self.zero_point, self.qmin, self.qmax, self.rounding, self.sums = scale, int(zero_point), int(qmin), int(qmax), int(rounding), sums

    @ property
    def device(self): return self.values.device

    def dequantize(self) -> torch.Tensor:
        """``(code - zero_point) * scale`` in float32, in the tensor's own layout."""
        codes = self.values[..., :self.shape[self.axis]].movedim(-1, self.axis).to(torch.float32)
        scale = self.scale.reshape([-1] + [1] * (len(self.shape) - 1)) if self.scale.numel() > 1 else self.scale
        return (codes - float(self.zero_point)) * scale


class Int4Weight:
    """INT4 codes (-8 .. 7) of a symmetric weight of ``shape``, packed for the int4 kernels.  ``values``: uint8, the reduction axis
    ``axis`` moved last, padded with code 0 to a multiple of 32 codes and packed two per byte: of every 8 consecutive codes (group
    ``g``) byte ``4 g + j``, ``j`` = 0 .. 3, holds code ``8 g + j`` in bits 0 .. 3 and code ``8 g + 4 + j`` in bits 4 .. 7, two's
    complement -- so that one dword is a lane's MFMA fragment.  ``scale``, ``qmin``, ``qmax``, ``rounding``
    as in ``Int8Tensor``; ``sums``: int32 ``[shape[0]]``, the sums of the codes; ``zero_point`` is 0."""
    __slots__ = ('values', 'shape', 'axis', 'scale', 'qmin', 'qmax', 'rounding', 'sums')
    zero_point = 0

    def __init__(self, values, shape, axis, scale, qmin, qmax, rounding, sums):
        self.values, self.shape, self.axis = values, tuple(int(d) for d in shape), int(axis)
        self.scale, self.qmin, self.qmax, self.rounding, self.sums = scale, int(qmin), int(qmax), int(rounding), sums

    @ property
    def device(self): return self.values.device

    def dequantize(self) -> torch.Tensor:
        """``code * scale`` in float32, in the tensor's own layout."""
        return int4_unpack(self).dequantize()


class Int8DepthwiseWeight:
    """int8 codes of a symmetric depthwise weight of ``shape`` ``(C, 1, kh, kw)``, laid out for ``csrc/int8_dwconv.hip``: ``values``
    int8 ``[kh, kw, Cp]``, tap-major and channels-last, ``Cp = ceil32(C)``, the channels ``C .. Cp - 1`` code 0.  ``scale``: float32, a
    scalar tensor or ``[C]``; ``sums``: int32 ``[C]``, the sum of a channel's taps; ``qmin``, ``qmax``, ``rounding`` as in
    ``Int8Tensor``; ``zero_point`` is 0."""
    __slots__ = ('values', 'shape', 'scale', 'qmin', 'qmax', 'rounding', 'sums')
    zero_point = 0

    def __init__(self, values, shape, scale, qmin, qmax, rounding, sums):
        self.values, self.shape = values, tuple(int(d) for d in shape)
        self.scale, self.qmin, self.qmax, self.rounding, self.sums = scale, int(qmin), int(qmax), int(rounding), sums

    @ property
    def device(self): return self.values.device

    def dequantize(self) -> torch.Tensor:
        """``code * scale`` in float32 ``[C, 1, kh, kw]``."""
        codes = self.values[..., :self.shape[0]].permute(2, 0, 1).unsqueeze(1).to(torch.float32)
        return codes * (self.scale.reshape(-1, 1, 1, 1) if self.scale.numel() > 1 else self.scale)


class Int8GroupedWeight:
    """int8 codes of a symmetric grouped weight of ``shape`` ``(O, C_g, kh, kw)`` for ``groups`` groups, laid out for
    ``csrc/int8_gconv.hip``: ``values`` int8 ``[O, kh, kw, 32 nbs]``, block ``j`` of a tap of row ``o`` holding the codes of ``w[o]`` for
    the input channels ``32 (cb0[o // 32] + j) .. + 31`` -- the channels of the row's own group in their places, code 0 everywhere else.
    ``cb0``: int32 ``[ceil(O / 32)]``, the first channel block the slice of output channels ``32 s .. 32 s + 31`` reads; ``nbs``: the
    most channel blocks any slice reads.  ``scale``: float32, a scalar tensor or ``[O]``; ``sums``: int32 ``[O]``, the sum of a row's
    codes; ``qmin``, ``qmax``, ``rounding`` as in ``Int8Tensor``; ``zero_point`` is 0."""
    __slots__ = ('values', 'shape', 'groups', 'nbs', 'cb0', 'scale', 'qmin', 'qmax', 'rounding', 'sums')
    zero_point = 0

    def __init__(self, values, shape, groups, nbs, cb0, scale, qmin, qmax, rounding, sums):
        self.values, self.shape, self.groups, self.nbs, self.cb0 = values, tuple(int(d) for d in shape), int(groups), int(nbs), cb0
        self.scale, self.qmin, self.qmax, self.rounding, self.sums = scale, int(qmin), int(qmax), int(rounding), sums

    @ property
    def device(self): return self.values.device

    def codes(self) -> torch.Tensor:
        """The codes of the rows' own groups, int8 ``[O, kh, kw, C_g]``."""
        return self.values.gather(3, _grouped_places(self.shape, self.groups, self.cb0).expand(-1, *self.shape[2:], -1))

    def dequantize(self) -> torch.Tensor:
        """``code * scale`` in float32 ``[O, C_g, kh, kw]``."""
        return self.codes().permute(0, 3, 1, 2).to(torch.float32) * (self.scale.reshape(-1, 1, 1, 1) if self.scale.numel() > 1 else self.scale)


def _grouped_places(shape, groups: int, cb0: torch.Tensor) -> torch.Tensor:
    """Where the ``C_g`` codes of a tap of row ``o`` lie in its ``32 nbs`` stored ones: int64 ``[O, 1, 1, C_g]``, channel
    ``(o // O_g) C_g + i`` relative to the first channel of the row's slice, ``32 cb0[o // 32]``."""
    o, cg = shape[0], shape[1]
    rows = torch.arange(o, device=cb0.device)
    first = torch.div(rows, o // groups, rounding_mode='floor') * cg - INT8_BLOCK * cb0.to(torch.int64)[torch.div(rows, INT8_BLOCK, rounding_mode='floor')]
    return (first[:, None] + torch.arange(cg, device=cb0.device)).reshape(o, 1, 1, cg)


def _grid(what: str, config):
    """(scale, offset, recentre, stored zero point or None for a per-channel config, stored qmin, stored qmax, rounding, channel
    axis) of a linear INT8 config; refuses what int8 codes cannot hold."""
    policy = getattr(config, 'policy', None)
    if policy is not None and policy.has_property(QuantizationProperty.FLOATING): raise RuntimeError(f'{what}: a floating-point config has no int8 codes')
    scale, offset = config.scale, config.offset
    if not isinstance(scale, torch.Tensor) or not isinstance(offset, torch.Tensor): raise RuntimeError(f'{what}: the config has no scale / offset tensors: calibrate it first')
    qmin, qmax = int(config.quant_min), int(config.quant_max)
    if qmin > qmax: raise RuntimeError(f'{what}: quant_min {qmin} above quant_max {qmax}')
    if -128 <= qmin and qmax <= 127: recentre = 0
    elif 0 <= qmin and qmax <= 255: recentre = 128
    else: raise RuntimeError(f'{what}: the range {qmin} .. {qmax} fits neither -128 .. 127 nor 0 .. 255')
    scale, offset = scale.detach().to(torch.float32), offset.detach().to(torch.float32)
    if not bool((offset == offset.round()).all()): raise RuntimeError(f'{what}: the offset is not an integer: an int8 zero point cannot hold it')
    per_channel = policy is not None and policy.has_property(QuantizationProperty.PER_CHANNEL)
    zero_point = None
    if not per_channel:
        if scale.numel() != 1 or offset.numel() != 1: raise RuntimeError(f'{what}: a per-tensor config with {scale.numel()} scales')
        zero_point = int(offset.reshape(-1)[0]) - recentre
        if not -128 <= zero_point <= 127: raise RuntimeError(f'{what}: the offset {zero_point + recentre} lies outside the range it is stored in')
    return scale, offset, recentre, zero_point, qmin - recentre, qmax - recentre, rounding_value(config.rounding), (config.channel_axis if per_channel else None)


def _to_int_torch(v, scale, offset, qmin, qmax, rounding, nan_code=0):
    """``LinearQuantize_ToInt`` in torch ops: ``clamp(ppq_tensor_round(v / s) + o, qmin, qmax)`` in float32, truncated; NaN gives ``nan_code``."""
    t = torch.clamp(ppq_tensor_round(v / scale, rounding) + offset, qmin, qmax)
    return torch.where(t != t, torch.full_like(t, nan_code), t).to(torch.int32)


def _pad_last(values, fill: int):
    pad = -values.shape[-1] % INT8_BLOCK
    return torch.nn.functional.pad(values, (0, pad), value=fill) if pad else values


def int8_quantize(tensor: torch.Tensor, config, axis: int = -1, weight: bool = False, use_kernels: bool = True, what: str = 'int8_quantize') -> Int8Tensor:
    """The codes of float32 ``tensor`` under ``config`` -- scale, offset, quant_min / quant_max, rounding and, for a per-channel
    config, channel_axis of a PPQ ``TensorQuantizationConfig`` (anything with those attributes) -- as an ``Int8Tensor`` whose
    reduction axis is ``axis``.  ``use_kernels=True``: the codes are ``CUDA.LinearQuantize_ToInt``'s (the tensor must be on the GPU);
    ``False``: the same arithmetic in torch ops, identical bits.  The move of ``axis`` to the end, the padding and the re-centring
    are torch ops.  ``weight=True``: the B operand of a layer -- symmetric (offset 0), per tensor or per channel along axis 0, with
    ``sums``; an activation (``weight=False``) is per tensor and may have any zero point.
    Refused: a range that fits neither -128 .. 127 nor 0 .. 255, a fractional offset, a weight with a non-zero offset, a per-channel
    activation, a channel axis other than 0 -- under the name ``what``."""
    if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float32: raise RuntimeError(f'{what}: expected a float32 tensor')
    if tensor.dim() < 1 or tensor.numel() == 0: raise RuntimeError(f'{what}: empty tensor of shape {list(tensor.shape)}')
    axis = axis % tensor.dim()
    scale, offset, recentre, zero_point, qmin, qmax, rounding, channel_axis = _grid(what, config)
    scale, offset = scale.to(tensor.device), offset.to(tensor.device)
    if weight:
        if bool((offset != 0).any()): raise RuntimeError(f'{what}: a weight must be symmetric: its offset is not 0')
        if channel_axis is not None and (channel_axis % tensor.dim() != 0 or axis == 0 or scale.numel() != tensor.shape[0]):
            raise RuntimeError(f'{what}: a weight is quantised per tensor or along axis 0 with one scale per row, got axis {channel_axis} and {scale.numel()} scales')
        if recentre: raise RuntimeError(f'{what}: a weight must be symmetric: its range {qmin + recentre} .. {qmax + recentre} is an unsigned one')
        zero_point = 0
    elif channel_axis is not None: raise RuntimeError(f'{what}: an activation must be quantised per tensor')
    if use_kernels:
        codes = CUDA.LinearQuantize_ToInt(tensor, scale.reshape(-1), offset.reshape(-1), qmin + recentre, qmax + recentre, rounding, channel_axis,
                                          torch.uint8 if recentre else torch.int8)
        if recentre: codes = codes.view(torch.int8) ^ -128                                  # code - 128, on the byte
    else:
        shape = [-1] + [1] * (tensor.dim() - 1) if channel_axis is not None else [1] * tensor.dim()
        codes = (_to_int_torch(tensor, scale.reshape(shape), offset.reshape(shape), qmin + recentre, qmax + recentre, rounding) - recentre).to(torch.int8)
    values = _pad_last(codes.movedim(axis, -1), zero_point).contiguous()
    sums = values.sum(dim=tuple(range(1, values.dim())), dtype=torch.int32) if weight else None
    return Int8Tensor(values, tensor.shape, axis, scale.reshape(-1) if channel_axis is not None else scale.reshape(()), zero_point, qmin, qmax, rounding, sums)


def int8_dequantize(t: Int8Tensor) -> torch.Tensor:
    """The inverse of ``int8_quantize`` on the grid: ``(code - zero_point) * scale`` as float32 of ``t.shape``."""
    return t.dequantize()


def int4_pack(w: Int8Tensor) -> Int4Weight:
    """The weight ``w`` -- ``int8_quantize(..., weight=True)`` or codes that already exist -- as an ``Int4Weight``: torch ops, done
    once.  Refused: anything but a symmetric ``Int8Tensor``, a code outside -8 .. 7."""
    what = 'int4_pack'
    if not isinstance(w, Int8Tensor) or w.values.dtype != torch.int8: raise TypeError(f'{what}: expected an Int8Tensor of int8 codes, got {type(w)}')
    if w.zero_point != 0: raise RuntimeError(f'{what}: a weight must be symmetric: its zero point is {w.zero_point}')
    v = _pad_last(w.values, 0).to(torch.int32)
    if v.numel() and (int(v.min()) < -8 or int(v.max()) > 7): raise RuntimeError(f'{what}: the codes reach {int(v.min())} .. {int(v.max())}: outside -8 .. 7')
    v = v.reshape(list(v.shape[:-1]) + [-1, 2, 4]) & 15                                 # groups of 8 codes: the low and the high nibbles' four
    packed = (v[..., 0, :] | (v[..., 1, :] << 4)).to(torch.uint8).reshape(list(v.shape[:-3]) + [-1])
    sums = w.sums if w.sums is not None else w.values.sum(dim=tuple(range(1, w.values.dim())), dtype=torch.int32)
    return Int4Weight(packed.contiguous(), w.shape, w.axis, w.scale, max(w.qmin, -8), min(w.qmax, 7), w.rounding, sums)


def int4_unpack(w: Int4Weight) -> Int8Tensor:
    """The codes of ``w`` back as an ``Int8Tensor`` weight (one code per byte, padded to a multiple of 32)."""
    if not isinstance(w, Int4Weight) or w.values.dtype != torch.uint8: raise TypeError(f'int4_unpack: expected an Int4Weight of uint8 bytes, got {type(w)}')
    b = w.values.reshape(list(w.values.shape[:-1]) + [-1, 1, 4]).to(torch.int32)
    codes = ((torch.cat((b & 15, b >> 4), -2) ^ 8) - 8).to(torch.int8)                  # sign extension of a nibble
    return Int8Tensor(codes.reshape(list(w.values.shape[:-1]) + [-1]).contiguous(), w.shape, w.axis, w.scale, 0, w.qmin, w.qmax, w.rounding, w.sums)


def int4_quantize_weight(tensor: torch.Tensor, config, axis: int = 1, use_kernels: bool = True) -> Int4Weight:
    """The INT4 codes of the float32 weight ``tensor`` under ``config`` -- ``LinearQuantize_ToInt``'s, exactly as
    ``int8_quantize(..., weight=True)`` makes them --, packed: ``int4_pack`` of that.  Refused by name: a range outside -8 .. 7, a
    non-zero offset, and everything ``int8_quantize`` refuses of a weight."""
    what = 'int4_quantize_weight'
    qmin, qmax = int(getattr(config, 'quant_min', 0)), int(getattr(config, 'quant_max', 0))
    if not -8 <= qmin <= qmax <= 7: raise RuntimeError(f'{what}: the range {qmin} .. {qmax} does not lie in -8 .. 7')
    return int4_pack(int8_quantize(tensor, config, axis, weight=True, use_kernels=use_kernels, what=what))


def _check_operands(what, x, w, rank, bias):
    for name, t, kinds in (('x', x, Int8Tensor), ('w', w, (Int8Tensor, Int4Weight))):
        if not isinstance(t, kinds): raise TypeError(f'{what}: {name}: expected an Int8Tensor{" or an Int4Weight" if name == "w" else ""}, got {type(t)}')
        want = torch.uint8 if isinstance(t, Int4Weight) else torch.int8
        if t.values.dtype != want: raise RuntimeError(f'{what}: {name}: the codes are {t.values.dtype}, not {str(want)[6:]}')
    if len(w.shape) != rank or (rank == 4 and len(x.shape) != 4): raise RuntimeError(f'{what}: operands must be {rank}-d, got x {list(x.shape)}, w {list(w.shape)}')
    if x.axis != (len(x.shape) - 1 if rank == 2 else 1) or w.axis != 1:
        raise RuntimeError(f'{what}: x {list(x.shape)} / w {list(w.shape)} are packed along axes {x.axis} / {w.axis}, not along the reduction axis')
    if x.shape[x.axis] != w.shape[1]: raise RuntimeError(f'{what}: K mismatch: x reduces over {x.shape[x.axis]}, w over {w.shape[1]} (groups must be 1)')
    if x.device != w.device: raise RuntimeError(f'{what}: x is on {x.device}, w on {w.device}')
    if (w.sums is None and x.zero_point != 0) or w.zero_point != 0: raise RuntimeError(f'{what}: w is not a weight: quantise it with int8_quantize(..., weight=True)')
    if x.scale.numel() != 1: raise RuntimeError(f'{what}: x must be quantised per tensor')
    kp = w.values[0].numel() * (2 if isinstance(w, Int4Weight) else 1)
    if kp >= MAX_KP: raise RuntimeError(f'{what}: a padded reduction length of {kp}: {MAX_KP} and more could overflow int32')
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32: raise RuntimeError(f'{what}: bias must be a float32 tensor')
        if list(bias.shape) != [w.shape[0]]: raise RuntimeError(f'{what}: bias of shape {list(bias.shape)}, expected [{w.shape[0]}]')


def _check_tail(what, like, shape, residual, out_config, out_float):
    """The checks of ``residual`` / ``out_config`` / ``out_float``; returns (out_float, the output grid ``(sy, zy, qmin, qmax,
    rounding, q_nan)`` in the stored domain or None)."""
    if out_float is None: out_float = out_config is None
    if out_config is None and not out_float: raise RuntimeError(f'{what}: no output: out_config is None and out_float is False')
    if residual is not None:
        if not isinstance(residual, torch.Tensor) or residual.dtype != torch.float32: raise RuntimeError(f'{what}: residual must be a float32 tensor')
        if list(residual.shape) != list(shape): raise RuntimeError(f'{what}: residual of shape {list(residual.shape)}, expected {list(shape)}')
        if residual.device != like.device: raise RuntimeError(f'{what}: residual is on {residual.device}, the operands on {like.device}')
    if out_config is None: return bool(out_float), None
    scale, _, recentre, zero_point, qmin, qmax, rounding, channel_axis = _grid(what + ': out_config', out_config)
    if channel_axis is not None: raise RuntimeError(f'{what}: out_config must be per tensor')
    return bool(out_float), (float(scale.reshape(-1)[0]), zero_point, qmin, qmax, rounding, -recentre)


def _mul(x: Int8Tensor, w: Int8Tensor) -> torch.Tensor:
    """``sx * sw`` as float32 ``[O]``: one float32 multiply per channel, a per-tensor weight scale broadcast."""
    return (x.scale.reshape(1).to(w.device) * w.scale.reshape(-1).to(w.device)).expand(w.shape[0]).contiguous()


def _tail_torch(i, mul, bias, residual, relu, out_q):
    """The contract's steps 2 .. 6 on the exact integer sums ``i`` (columns last): the float32 result and the padded codes or None."""
    v = i.to(torch.float32) * mul
    if bias is not None: v = v + bias
    if residual is not None: v = v + residual
    if relu: v = relu_positive_zero(v)
    if out_q is None: return v, None
    sy, zy, qmin, qmax, rounding, q_nan = out_q
    sy = torch.tensor(sy, dtype=torch.float32, device=v.device)                         # a tensor: a Python scalar may be divided by as a reciprocal
    return v, _pad_last(_to_int_torch(v, sy, float(zy), qmin, qmax, rounding, q_nan).to(torch.int8), zy)


def _result(y, q, shape, axis, out_q, out_float, like):
    if q is None: return y
    sy, zy, qmin, qmax, rounding, _ = out_q
    scale = torch.full((), sy, dtype=torch.float32, device=like.device)                 # a fill, not a copy from the host: no synchronisation
    packed = Int8Tensor(q, shape, axis, scale, zy, qmin, qmax, rounding)
    return (y, packed) if out_float else packed


def int8_matmul(a: Int8Tensor, b, bias: torch.Tensor = None, residual: torch.Tensor = None, relu: bool = False, out_config=None,
                out_float: Optional[bool] = None, use_kernels: bool = True, skinny: bool = False):
    """``a . b^T`` as a linear INT8 layer (the contract at the top of this module): ``a`` an activation ``[..., K]`` packed along its
    last axis, ``b`` a weight ``[N, K]`` (``int8_quantize(..., axis=1, weight=True)``, or an ``Int4Weight``: ``CUDA.Int4Matmul`` then,
    the same bits from half the weight bytes), ``bias`` float32 ``[N]``, ``residual`` float32
    ``[..., N]``.  Returns the float32 ``[..., N]``; with ``out_config`` (a per-tensor config: the next layer's activation) the result
    as an ``Int8Tensor`` packed along its last axis -- the bits of ``int8_quantize`` on the float32 result --, and with
    ``out_float=True`` both, ``(tensor, Int8Tensor)``.  ONE launch (``CUDA.Int8Matmul``); ``use_kernels=False``: torch ops, any device.
    ``skinny=True``: the launch is ``CUDA.Int8MatmulSkinny`` / ``Int4MatmulSkinny``, the kernel for a layer bound by reading its weight
    (section 9.26) -- the same bits; the flattened ``M = prod(a.shape[:-1])`` must be 1 .. 64, under either arm."""
    what = 'int8_matmul'
    _check_operands(what, a, b, 2, bias)
    shape = list(a.shape[:-1]) + [b.shape[0]]
    if skinny:
        m = a.values[..., 0].numel()
        if not 1 <= m <= SKINNY_MAX_M: raise RuntimeError(f'{what}: skinny=True takes M = 1 .. {SKINNY_MAX_M} rows, got M = {m}')
    out_float, out_q = _check_tail(what, a, shape, residual, out_config, out_float)
    av, mul = a.values.reshape(-1, a.values.shape[-1]), _mul(a, b)
    res = residual.reshape(-1, shape[-1]) if residual is not None else None
    int4 = isinstance(b, Int4Weight)
    if use_kernels:
        if skinny: gemm = CUDA.Int4MatmulSkinny if int4 else CUDA.Int8MatmulSkinny
        else: gemm = CUDA.Int4Matmul if int4 else CUDA.Int8Matmul
        y, q = gemm(av, b.values, b.sums if a.zero_point else None, a.zero_point, mul, bias, res, relu, out_float, out_q)
    else:
        i = (av.to(torch.float64) - a.zero_point) @ (int4_unpack(b) if int4 else b).values.to(torch.float64).t()       # every partial sum is an integer below 2^31: exact
        y, q = _tail_torch(i.to(torch.int64), mul, bias, res, relu, out_q)
    y = y.reshape(shape) if y is not None and out_float else None
    return _result(y, q.reshape(shape[:-1] + [-1]) if q is not None else None, shape, len(shape) - 1, out_q, out_float, a)


def int8_bmm(a: Int8Tensor, b: Int8Tensor, transpose_b: bool = False, residual: torch.Tensor = None, relu: bool = False, out_config=None,
             out_float: Optional[bool] = None, use_kernels: bool = True):
    """The batched matmul of TWO activations, attention's ``Q . K^T`` and ``P . V`` (section 9.27): ``a`` ``[*batch, M, K]`` and ``b``
    ``[*batch, N, K]`` (``transpose_b=True``: ``a @ b^T``) or ``[*batch, K, N]`` (``a @ b``), each an ``Int8Tensor`` packed along its
    LAST axis -- so with ``transpose_b=False`` ``b`` is packed along ``N``, as the Gemm that made it left it, and the kernel transposes
    it on its way to the MFMA.  Both are per-tensor activations with any zero point and no ``sums``; the batch shapes are equal (no
    broadcasting) and ``values`` contiguous.  Per batch

        I = sum_k (a[m, k] - za) (b[k, n] - zb)     exact, int32
        v = float32(I) * (sa * sb)                  sa * sb one float32 product

    then ``residual`` (float32 ``[*batch, M, N]``: an additive mask), ``relu``, ``out_config`` and ``out_float`` as in ``int8_matmul``;
    there is no bias.  Returns the float32 ``[*batch, M, N]``, the ``Int8Tensor`` packed along its last axis, or both.  ONE launch
    for all batches (``CUDA.Int8Bmm``); ``use_kernels=False``: torch ops on any device, identical bits.  A padded reduction length
    above 32768 is refused: ``32768 * 255 * 255 < 2^31``."""
    what = 'int8_bmm'
    for name, t in (('a', a), ('b', b)):
        if not isinstance(t, Int8Tensor): raise TypeError(f'{what}: {name}: expected an Int8Tensor, got {type(t)}')
        if t.values.dtype != torch.int8: raise RuntimeError(f'{what}: {name}: the codes are {t.values.dtype}, not int8')
        if t.scale.numel() != 1: raise RuntimeError(f'{what}: {name} must be quantised per tensor')
        if len(t.shape) < 2 or t.axis != len(t.shape) - 1:
            raise RuntimeError(f'{what}: {name} {list(t.shape)} must be at least 2-d and packed along its last axis, not along axis {t.axis}')
        if list(t.values.shape) != list(t.shape[:-1]) + [t.shape[-1] + -t.shape[-1] % INT8_BLOCK] or not t.values.is_contiguous() or t.values.numel() == 0:
            raise RuntimeError(f'{what}: {name}: values of shape {list(t.values.shape)} are not the contiguous, padded codes of a non-empty {list(t.shape)}')
    if a.shape[:-2] != b.shape[:-2]: raise RuntimeError(f'{what}: batch mismatch: a {list(a.shape)}, b {list(b.shape)} (no broadcasting)')
    (kb, n), k = (b.shape[-1], b.shape[-2]) if transpose_b else (b.shape[-2], b.shape[-1]), a.shape[-1]
    if k != kb: raise RuntimeError(f'{what}: K mismatch: a reduces over {k}, b over {kb} (transpose_b={bool(transpose_b)})')
    if a.device != b.device: raise RuntimeError(f'{what}: a is on {a.device}, b on {b.device}')
    m, kp = a.shape[-2], a.values.shape[-1]
    if kp > BMM_MAX_KP: raise RuntimeError(f'{what}: a padded reduction length of {kp}: more than {BMM_MAX_KP} could overflow int32')
    shape = list(a.shape[:-1]) + [n]
    out_float, out_q = _check_tail(what, a, shape, residual, out_config, out_float)
    av, bv = a.values.reshape(-1, m, kp), b.values.reshape([-1] + list(b.values.shape[-2:]))
    mul = a.scale.reshape(1) * b.scale.reshape(1)                                       # one float32 multiply, on the device
    res = residual.reshape(-1, m, n) if residual is not None else None
    if use_kernels:
        y, q = CUDA.Int8Bmm(av, bv, transpose_b, a.zero_point, b.zero_point, mul, n, res, relu, out_float, out_q)
    else:
        bf = bv.to(torch.float64) - b.zero_point                                        # the padding of both is (za, zb): it adds 0 . 0
        bf = bf.transpose(1, 2) if transpose_b else bf[..., :n]
        i = (av[..., :bf.shape[1]].to(torch.float64) - a.zero_point) @ bf               # every partial sum is an integer below 2^31: exact
        y, q = _tail_torch(i.to(torch.int64), mul, None, res, relu, out_q)
    y = y.reshape(shape) if y is not None and out_float else None
    return _result(y, q.reshape(shape[:-1] + [-1]) if q is not None else None, shape, len(shape) - 1, out_q, out_float, a)


def int8_linear(x: torch.Tensor, weight, x_config, bias: torch.Tensor = None, residual: torch.Tensor = None, relu: bool = False,
                out_config=None, out_float: Optional[bool] = None, use_kernels: bool = True, skinny: bool = False):
    """A Gemm on an INT8 (or ``Int4Weight``) weight as it runs in deployment: ``int8_quantize(x, x_config, -1)``, then ``int8_matmul``: two launches.
    ``skinny`` is ``int8_matmul``'s: the kernel for at most 64 rows."""
    return int8_matmul(int8_quantize(x, x_config, -1, use_kernels=use_kernels), weight, bias, residual, relu, out_config, out_float, use_kernels, skinny)


def int8_conv2d_packed(x: Int8Tensor, w, bias: torch.Tensor = None, stride=1, padding=0, dilation=1, residual: torch.Tensor = None,
                       relu: bool = False, out_config=None, out_float: Optional[bool] = None, use_kernels: bool = True):
    """``conv2d(x, w)`` as a linear INT8 layer: ``x`` an activation ``[N, C, H, W]`` and ``w`` a weight ``[O, C, kh, kw]``, both packed
    along axis 1 (``w`` may be an ``Int4Weight``: ``CUDA.Int4Conv2d`` then); ``stride``, ``padding`` (symmetric) and ``dilation`` are ints or (h, w) pairs, groups is 1.  A tap in the padding is a
    real 0, which is the code ``x.zero_point``.  The float32 result is ``[N, O, OH, OW]`` (channels-last strides from the kernel);
    ``residual`` (float32, that shape; channels-last is read in place), ``relu``, ``out_config`` and ``out_float`` as in ``int8_matmul``
    -- the ``Int8Tensor`` is packed along axis 1, what this function takes as ``x``.  ONE launch (``CUDA.Int8Conv2d``), an implicit
    GEMM; ``use_kernels=False``: torch ops on any device, identical bits."""
    what = 'int8_conv2d'
    _check_operands(what, x, w, 4, bias)
    stride, padding, dilation = _pair(stride, 'stride', 1, what), _pair(padding, 'padding', 0, what), _pair(dilation, 'dilation', 1, what)
    out = tuple((x.shape[2 + i] + 2 * padding[i] - dilation[i] * (w.shape[2 + i] - 1) - 1) // stride[i] + 1 for i in range(2))
    if min(out) < 1:
        raise RuntimeError(f'{what}: a {w.shape[2]} x {w.shape[3]} kernel with dilation {dilation} does not fit an input of '
                           f'{x.shape[2]} x {x.shape[3]} padded by {padding}')
    shape = [x.shape[0], w.shape[0], out[0], out[1]]
    out_float, out_q = _check_tail(what, x, shape, residual, out_config, out_float)
    mul = _mul(x, w)
    int4 = isinstance(w, Int4Weight)
    if use_kernels:
        y, q = (CUDA.Int4Conv2d if int4 else CUDA.Int8Conv2d)(x.values, w.values, w.sums if x.zero_point else None, x.zero_point, mul, x.shape[1], bias, stride, padding, dilation,
                                                              residual, relu, out_float, out_q)
    else:
        xf = torch.nn.functional.pad(x.values.permute(0, 3, 1, 2).to(torch.float64), (padding[1],) * 2 + (padding[0],) * 2, value=x.zero_point)
        i = torch.nn.functional.conv2d(xf - x.zero_point, (int4_unpack(w) if int4 else w).values.permute(0, 3, 1, 2).to(torch.float64), None, stride, 0, dilation)      # exact: integers below 2^31
        y, q = _tail_torch(i.permute(0, 2, 3, 1).to(torch.int64), mul, bias, residual.permute(0, 2, 3, 1) if residual is not None else None, relu, out_q)
        y = y.permute(0, 3, 1, 2)
    return _result(y if out_float else None, q, shape, 1, out_q, out_float, x)


def int8_depthwise_weight(tensor: torch.Tensor, config, use_kernels: bool = True) -> Int8DepthwiseWeight:
    """The codes of the float32 depthwise weight ``tensor`` ``[C, 1, kh, kw]`` under ``config`` -- ``int8_quantize(..., weight=True)``'s,
    per tensor or per channel along axis 0, with its refusals under this name --, re-laid as an ``Int8DepthwiseWeight`` (torch ops, done
    once).  Refused too: a weight whose axis 1 is not 1 (a channel multiplier, or a grouped convolution that is not depthwise)."""
    what = 'int8_depthwise_weight'
    if not isinstance(tensor, torch.Tensor) or tensor.dim() != 4 or tensor.shape[1] != 1:
        raise RuntimeError(f'{what}: expected a [C, 1, kh, kw] weight (groups == C, channel multiplier 1), got shape {list(getattr(tensor, "shape", []))}')
    t = int8_quantize(tensor, config, 1, weight=True, use_kernels=use_kernels, what=what)             # [C, kh, kw, 32]: code, then 31 zeros
    values = _pad_last(t.values[..., 0].permute(1, 2, 0), 0).contiguous()
    return Int8DepthwiseWeight(values, tensor.shape, t.scale, t.qmin, t.qmax, t.rounding, t.sums)


def int8_depthwise_conv2d_packed(x: Int8Tensor, w: Int8DepthwiseWeight, bias: torch.Tensor = None, stride=1, padding=0, dilation=1,
                                 residual: torch.Tensor = None, relu: bool = False, out_config=None, out_float: Optional[bool] = None,
                                 use_kernels: bool = True):
    """``conv2d(x, w, groups=C)`` as a linear INT8 layer: ``x`` an activation ``[N, C, H, W]`` packed along axis 1, ``w`` an
    ``Int8DepthwiseWeight`` ``[C, 1, kh, kw]``.  Everything else -- the geometry, the padding's code, ``bias`` ``[C]``, ``residual``,
    ``relu``, ``out_config``, ``out_float`` and what is returned -- is ``int8_conv2d_packed``'s: the ``Int8Tensor`` is packed along axis
    1, so depthwise and dense layers chain.  ONE launch (``CUDA.Int8DepthwiseConv2d``, on ``v_dot4c_i32_i8``); ``use_kernels=False``:
    torch ops on any device, identical bits.  Refused under either arm: a geometry whose input patch and weights exceed the 64 KiB of
    LDS the kernel stages them in (every window with ``(k - 1) * dilation <= 6`` per axis fits at stride 1 and 2)."""
    what = 'int8_depthwise_conv2d'
    if not isinstance(x, Int8Tensor): raise TypeError(f'{what}: x: expected an Int8Tensor, got {type(x)}')
    if not isinstance(w, Int8DepthwiseWeight): raise TypeError(f'{what}: w: expected an Int8DepthwiseWeight, got {type(w)}')
    for name, t in (('x', x), ('w', w)):
        if t.values.dtype != torch.int8: raise RuntimeError(f'{what}: {name}: the codes are {t.values.dtype}, not int8')
    if len(x.shape) != 4 or x.axis != 1: raise RuntimeError(f'{what}: x {list(x.shape)} must be 4-d and packed along axis 1, not {x.axis}')
    if x.shape[1] != w.shape[0]: raise RuntimeError(f'{what}: channel mismatch: x has {x.shape[1]} channels, w {w.shape[0]}')
    if x.device != w.device: raise RuntimeError(f'{what}: x is on {x.device}, w on {w.device}')
    if x.scale.numel() != 1: raise RuntimeError(f'{what}: x must be quantised per tensor')
    c, kh, kw = w.shape[0], w.shape[2], w.shape[3]
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32: raise RuntimeError(f'{what}: bias must be a float32 tensor')
        if list(bias.shape) != [c]: raise RuntimeError(f'{what}: bias of shape {list(bias.shape)}, expected [{c}]')
    stride, padding, dilation = _pair(stride, 'stride', 1, what), _pair(padding, 'padding', 0, what), _pair(dilation, 'dilation', 1, what)
    out = tuple((x.shape[2 + i] + 2 * padding[i] - dilation[i] * (w.shape[2 + i] - 1) - 1) // stride[i] + 1 for i in range(2))
    if min(out) < 1:
        raise RuntimeError(f'{what}: a {kh} x {kw} kernel with dilation {dilation} does not fit an input of {x.shape[2]} x {x.shape[3]} padded by {padding}')
    need = depthwise_lds_bytes(kh, kw, stride, dilation)
    if need > DEPTHWISE_LDS_BYTES:
        raise RuntimeError(f'{what}: a {kh} x {kw} window at stride {stride} and dilation {dilation} stages {need} bytes of LDS: a workgroup has {DEPTHWISE_LDS_BYTES}')
    shape = [x.shape[0], c, out[0], out[1]]
    out_float, out_q = _check_tail(what, x, shape, residual, out_config, out_float)
    mul = _mul(x, w)
    if use_kernels:
        y, q = CUDA.Int8DepthwiseConv2d(x.values, w.values, w.sums if x.zero_point else None, x.zero_point, mul, c, bias, stride, padding, dilation,
                                        residual, relu, out_float, out_q)
    else:
        xf = torch.nn.functional.pad(x.values[..., :c].permute(0, 3, 1, 2).to(torch.float64), (padding[1],) * 2 + (padding[0],) * 2, value=x.zero_point)
        wf = w.values[..., :c].permute(2, 0, 1).unsqueeze(1).to(torch.float64)
        i = torch.nn.functional.conv2d(xf - x.zero_point, wf, None, stride, 0, dilation, groups=c)          # exact: integers below 2^31
        y, q = _tail_torch(i.permute(0, 2, 3, 1).to(torch.int64), mul, bias, residual.permute(0, 2, 3, 1) if residual is not None else None, relu, out_q)
        y = y.permute(0, 3, 1, 2)
    return _result(y if out_float else None, q, shape, 1, out_q, out_float, x)


def int8_depthwise_conv2d(x: torch.Tensor, weight: Int8DepthwiseWeight, x_config, bias: torch.Tensor = None, stride=1, padding=0, dilation=1,
                          residual: torch.Tensor = None, relu: bool = False, out_config=None, out_float: Optional[bool] = None, use_kernels: bool = True):
    """A depthwise convolution on an INT8 weight as it runs in deployment: ``int8_quantize(x, x_config, 1)`` -- ``x`` ``[N, C, H, W]`` --,
    then ``int8_depthwise_conv2d_packed``: two launches."""
    if isinstance(x, torch.Tensor) and x.dim() != 4: raise RuntimeError(f'int8_depthwise_conv2d: x must be 4-d [N, C, H, W], got shape {list(x.shape)}')
    return int8_depthwise_conv2d_packed(int8_quantize(x, x_config, 1, use_kernels=use_kernels), weight, bias, stride, padding, dilation, residual, relu,
                                        out_config, out_float, use_kernels)


def int8_grouped_weight(tensor: torch.Tensor, config, groups: int, use_kernels: bool = True) -> Int8GroupedWeight:
    """The codes of the float32 grouped weight ``tensor`` ``[O, C_g, kh, kw]`` of a convolution with ``groups`` groups under ``config`` --
    ``int8_quantize(..., weight=True)``'s, per tensor or per output channel, with its refusals under this name --, re-laid as an
    ``Int8GroupedWeight`` (torch ops, done once).  ``groups == 1`` and a depthwise weight are laid out like any other, though
    ``int8_conv2d_packed`` and ``int8_depthwise_conv2d_packed`` are the fast paths for them.  Refused too: an ``Int4Weight`` (INT4 grouped
    weights are not supported), ``groups`` that do not divide ``O``."""
    what = 'int8_grouped_weight'
    if isinstance(tensor, Int4Weight): raise TypeError(f'{what}: INT4 grouped weights are not supported: got an Int4Weight')
    if not isinstance(tensor, torch.Tensor) or tensor.dim() != 4: raise RuntimeError(f'{what}: expected a [O, C_g, kh, kw] weight, got shape {list(getattr(tensor, "shape", []))}')
    groups, (o, cg) = int(groups), tensor.shape[:2]
    if groups < 1 or o % groups: raise RuntimeError(f'{what}: {groups} groups do not divide the {o} output channels')
    t = int8_quantize(tensor, config, 1, weight=True, use_kernels=use_kernels, what=what)             # [O, kh, kw, ceil32(C_g)]
    # slice s (outputs 32 s .. 32 s + 31) reads the channels of its first to its last group, rounded outwards to blocks of 32
    og, starts = o // groups, range(0, o, INT8_BLOCK)
    first = [s // og * cg // INT8_BLOCK for s in starts]
    last = [((min(s + INT8_BLOCK, o) - 1) // og + 1) * cg - 1 for s in starts]
    nbs = max(b // INT8_BLOCK - a + 1 for a, b in zip(first, last))
    cb0 = torch.tensor(first, dtype=torch.int32, device=tensor.device)
    values = torch.zeros(list(t.values.shape[:3]) + [INT8_BLOCK * nbs], dtype=torch.int8, device=tensor.device)
    values.scatter_(3, _grouped_places(tensor.shape, groups, cb0).expand(-1, *tensor.shape[2:], -1), t.values[..., :cg])
    return Int8GroupedWeight(values, tensor.shape, groups, nbs, cb0, t.scale, t.qmin, t.qmax, t.rounding, t.sums)


def int8_grouped_conv2d_packed(x: Int8Tensor, w: Int8GroupedWeight, bias: torch.Tensor = None, stride=1, padding=0, dilation=1,
                               residual: torch.Tensor = None, relu: bool = False, out_config=None, out_float: Optional[bool] = None,
                               use_kernels: bool = True):
    """``conv2d(x, w, groups=w.groups)`` as a linear INT8 layer: ``x`` an activation ``[N, C, H, W]`` packed along axis 1, ``w`` an
    ``Int8GroupedWeight`` ``[O, C / groups, kh, kw]``.  Everything else -- the geometry, the padding's code, ``bias`` ``[O]``,
    ``residual``, ``relu``, ``out_config``, ``out_float`` and what is returned -- is ``int8_conv2d_packed``'s: the ``Int8Tensor`` is
    packed along axis 1, so dense, depthwise and grouped layers chain.  ONE launch (``CUDA.Int8GroupedConv2d``, on the int8 MFMA);
    ``use_kernels=False``: torch ops on any device, identical bits."""
    what = 'int8_grouped_conv2d'
    if not isinstance(x, Int8Tensor): raise TypeError(f'{what}: x: expected an Int8Tensor, got {type(x)}')
    if isinstance(w, Int4Weight): raise TypeError(f'{what}: w: INT4 grouped weights are not supported: got an Int4Weight')
    if not isinstance(w, Int8GroupedWeight): raise TypeError(f'{what}: w: expected an Int8GroupedWeight, got {type(w)}')
    for name, t in (('x', x), ('w', w)):
        if t.values.dtype != torch.int8: raise RuntimeError(f'{what}: {name}: the codes are {t.values.dtype}, not int8')
    if len(x.shape) != 4 or x.axis != 1: raise RuntimeError(f'{what}: x {list(x.shape)} must be 4-d and packed along axis 1, not {x.axis}')
    o, cg, kh, kw = w.shape
    c = cg * w.groups
    if x.shape[1] != c: raise RuntimeError(f'{what}: channel mismatch: x has {x.shape[1]} channels, w {cg} for each of {w.groups} groups')
    if x.device != w.device: raise RuntimeError(f'{what}: x is on {x.device}, w on {w.device}')
    if x.scale.numel() != 1: raise RuntimeError(f'{what}: x must be quantised per tensor')
    kp = w.values[0].numel()
    if kp >= MAX_KP: raise RuntimeError(f'{what}: a padded reduction length of {kp}: {MAX_KP} and more could overflow int32')
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32: raise RuntimeError(f'{what}: bias must be a float32 tensor')
        if list(bias.shape) != [o]: raise RuntimeError(f'{what}: bias of shape {list(bias.shape)}, expected [{o}]')
    stride, padding, dilation = _pair(stride, 'stride', 1, what), _pair(padding, 'padding', 0, what), _pair(dilation, 'dilation', 1, what)
    out = tuple((x.shape[2 + i] + 2 * padding[i] - dilation[i] * (w.shape[2 + i] - 1) - 1) // stride[i] + 1 for i in range(2))
    if min(out) < 1:
        raise RuntimeError(f'{what}: a {kh} x {kw} kernel with dilation {dilation} does not fit an input of {x.shape[2]} x {x.shape[3]} padded by {padding}')
    shape = [x.shape[0], o, out[0], out[1]]
    out_float, out_q = _check_tail(what, x, shape, residual, out_config, out_float)
    mul = _mul(x, w)
    if use_kernels:
        y, q = CUDA.Int8GroupedConv2d(x.values, w.values, w.sums if x.zero_point else None, x.zero_point, mul, c, w.groups, w.nbs, w.cb0, bias, stride, padding,
                                      dilation, residual, relu, out_float, out_q)
    else:
        xf = torch.nn.functional.pad(x.values[..., :c].permute(0, 3, 1, 2).to(torch.float64), (padding[1],) * 2 + (padding[0],) * 2, value=x.zero_point)
        i = torch.nn.functional.conv2d(xf - x.zero_point, w.codes().permute(0, 3, 1, 2).to(torch.float64), None, stride, 0, dilation, groups=w.groups)  # exact: integers below 2^31
        y, q = _tail_torch(i.permute(0, 2, 3, 1).to(torch.int64), mul, bias, residual.permute(0, 2, 3, 1) if residual is not None else None, relu, out_q)
        y = y.permute(0, 3, 1, 2)
    return _result(y if out_float else None, q, shape, 1, out_q, out_float, x)


def int8_grouped_conv2d(x: torch.Tensor, weight: Int8GroupedWeight, x_config, bias: torch.Tensor = None, stride=1, padding=0, dilation=1,
                        residual: torch.Tensor = None, relu: bool = False, out_config=None, out_float: Optional[bool] = None, use_kernels: bool = True):
    """A grouped convolution on an INT8 weight as it runs in deployment: ``int8_quantize(x, x_config, 1)`` -- ``x`` ``[N, C, H, W]`` --,
    then ``int8_grouped_conv2d_packed``: two launches."""
    if isinstance(x, torch.Tensor) and x.dim() != 4: raise RuntimeError(f'int8_grouped_conv2d: x must be 4-d [N, C, H, W], got shape {list(x.shape)}')
    return int8_grouped_conv2d_packed(int8_quantize(x, x_config, 1, use_kernels=use_kernels), weight, bias, stride, padding, dilation, residual, relu,
                                      out_config, out_float, use_kernels)


def int8_conv2d(x: torch.Tensor, weight, x_config, bias: torch.Tensor = None, stride=1, padding=0, dilation=1, groups: int = 1,
                residual: torch.Tensor = None, relu: bool = False, out_config=None, out_float: Optional[bool] = None, use_kernels: bool = True):
    """A convolution on an INT8 (or ``Int4Weight``) weight as it runs in deployment: ``int8_quantize(x, x_config, 1)`` -- ``x`` ``[N, C, H, W]`` --, then
    ``int8_conv2d_packed``: two launches.  With an ``Int8DepthwiseWeight`` and ``groups == C`` it is ``int8_depthwise_conv2d``, with an
    ``Int8GroupedWeight`` and ``groups == weight.groups`` ``int8_grouped_conv2d``; groups other than 1 with any other weight are refused."""
    if isinstance(weight, Int8GroupedWeight):
        if groups != weight.groups: raise RuntimeError(f'int8_conv2d: a grouped weight of {weight.groups} groups needs groups == {weight.groups}, got {groups}')
        return int8_grouped_conv2d(x, weight, x_config, bias, stride, padding, dilation, residual, relu, out_config, out_float, use_kernels)
    if isinstance(weight, Int8DepthwiseWeight):
        if groups != weight.shape[0]: raise RuntimeError(f'int8_conv2d: a depthwise weight of {weight.shape[0]} channels needs groups == {weight.shape[0]}, got {groups}')
        return int8_depthwise_conv2d(x, weight, x_config, bias, stride, padding, dilation, residual, relu, out_config, out_float, use_kernels)
    if groups != 1: raise RuntimeError(f'int8_conv2d: groups must be 1, got {groups}')
    if isinstance(x, torch.Tensor) and x.dim() != 4: raise RuntimeError(f'int8_conv2d: x must be 4-d [N, C, H, W], got shape {list(x.shape)}')
    return int8_conv2d_packed(int8_quantize(x, x_config, 1, use_kernels=use_kernels), weight, bias, stride, padding, dilation, residual, relu,
                              out_config, out_float, use_kernels)
