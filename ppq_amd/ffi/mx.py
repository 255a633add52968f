"""OCP Microscaling: fake quant, round tuning on the MX grid, the packed export and the operand checks of the MX MFMA bindings
(include/ppq_hip.h ppqhip_mx_fq[_multi], ppqhip_mx_round_*_multi, ppqhip_mx_pack / ppqhip_mx_unpack and their _multi forms;
DESIGN.md sections 9.13 - 9.18)."""
import math
from typing import List

import torch

from .._lib import lib
from ._base import _KERNEL_FAILURE, JobTable, _check, _f32, _ptr, _same_length
from .abi import MX_JOB, MX_PACK_JOB, MX_ROUND_FWD_JOB, MX_ROUND_SPLIT_JOB, MX_UNPACK_JOB
from .plans import _carve

MX_BLOCK = 32
MX_FORMATS = {'MXFP8_E4M3': 0, 'MXFP8_E5M2': 1, 'MXFP6_E3M2': 2, 'MXFP6_E2M3': 3, 'MXFP4_E2M1': 4, 'MXINT8': 5}      # PPQHIP_MX*


def mx_format_id(format) -> int:
    """The library's id of an MX format given as ``ppq_amd.mx.MXFormat``, its name or the id itself."""
    key = getattr(format, 'name', format)
    if isinstance(key, str) and key in MX_FORMATS: return MX_FORMATS[key]
    if isinstance(key, int) and not isinstance(key, bool) and key in MX_FORMATS.values(): return key
    raise ValueError(f'unknown MX format {format!r}: expected one of {", ".join(MX_FORMATS)}')


MX_SCALE_RULES = {'FLOOR': 0, 'CEIL': 1, 'EVEN': 2, 'MSE': 3}      # PPQHIP_MX_FLOOR .. PPQHIP_MX_MSE
MX_RULE_SHIFT = 8                                                   # PPQHIP_MX_RULE_SHIFT


def mx_rule_id(rule) -> int:
    """The library's id of an MX scale rule given as ``ppq_amd.mx.MXScaleRule``, its name or the id itself; None is FLOOR."""
    if rule is None: return MX_SCALE_RULES['FLOOR']
    key = getattr(rule, 'name', rule)
    if isinstance(key, str) and key in MX_SCALE_RULES: return MX_SCALE_RULES[key]
    if isinstance(key, int) and not isinstance(key, bool) and key in MX_SCALE_RULES.values(): return key
    raise ValueError(f'unknown MX scale rule {rule!r}: expected one of {", ".join(MX_SCALE_RULES)}')


def mx_format_arg(format, scale_rule=None) -> int:
    """The ``format`` argument of the entry points that make scales: ``format | rule << 8`` (FLOOR: the format's id as it is)."""
    return mx_format_id(format) | (mx_rule_id(scale_rule) << MX_RULE_SHIFT)


def _mx_item(item):
    """``(value, format, axis)`` or ``(value, format, axis, scale_rule)`` of a plan as (value, format, axis, rule id)."""
    if len(item) not in (3, 4): raise ValueError(f'an MX plan item is (value, format, axis[, scale_rule]), got {len(item)} entries')
    return item[0], item[1], item[2], mx_rule_id(item[3] if len(item) == 4 else None)


def _mx_axis(ndim: int, axis: int) -> int:
    if not isinstance(axis, int) or not -ndim <= axis < ndim:
        raise RuntimeError(_KERNEL_FAILURE + f'axis {axis} out of range for a {ndim}-d tensor')
    return axis % ndim


def _mx_channels_last(t: torch.Tensor, axis: int) -> bool:
    """A dense 4-D channels-last tensor quantised along its channels: the blocks are contiguous in storage as they are."""
    return t.dim() == 4 and axis == 1 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def _mx_geometry(t: torch.Tensor, axis: int):
    """(outer, axis_len, inner) of the storage of ``t`` (contiguous, or channels-last with axis 1) and the shape of its scale codes."""
    shape = list(t.shape)
    codes = shape[:axis] + [(shape[axis] + MX_BLOCK - 1) // MX_BLOCK] + shape[axis + 1:]
    if _mx_channels_last(t, axis): return t.numel() // shape[1], shape[1], 1, codes
    inner = 1
    for d in shape[axis + 1:]: inner *= int(d)
    return t.numel() // (shape[axis] * inner), shape[axis], inner, codes


def _mx_dense(t: torch.Tensor, axis: int) -> torch.Tensor:
    return t if t.is_contiguous() or _mx_channels_last(t, axis) else t.contiguous()


def _mx_codes_like(v: torch.Tensor, axis: int, shape) -> torch.Tensor:
    fmt = torch.channels_last if _mx_channels_last(v, axis) else torch.contiguous_format
    return torch.empty(shape, dtype=torch.uint8, device=v.device, memory_format=fmt)


class MXQuantizePlan:
    """MX fake-quant of MANY tensors with ONE launch per call (``ppqhip_mx_fq_multi``): the MX weights of a graph.  Built once from
    ``(value, format, axis)`` items; ``run()`` re-quantises all of them into one resident arena and returns views shaped like the
    inputs -- bits identical to ``CUDA.MXQuantize`` per item.  The job table travels in the kernel arguments and holds POINTERS to
    the callers' tensors: in-place updates are seen by later runs, a REPLACED tensor needs a new plan.  A value that is not dense
    (contiguous, or 4-D channels-last along axis 1) would need a private copy that later updates never reach: refused
    (``accepts()``).  ``with_codes``: also keep every item's E8M0 scale codes (``codes``).  An item may carry a fourth entry, its
    scale rule (``ppq_amd.mx.MXScaleRule``; default FLOOR): one launch serves any mix of rules and formats."""
    @ staticmethod
    def accepts(value, axis) -> bool:
        return value.dim() > 0 and -value.dim() <= axis < value.dim() and _mx_dense(value, axis % value.dim()) is value

    def __init__(self, items, with_codes: bool = False):
        table, items = _mx_plan_table('MXQuantizePlan', MX_JOB, items)
        self._arena, pieces = _carve([it[0].numel() for it in items], torch.float32, table.dev)
        self._jobs, self._outs, self.codes = table, [], []
        for k, (v, format, axis, rule) in enumerate(items):
            outer, length, inner, codes_shape = _mx_geometry(v, axis)
            out = pieces[k].as_strided(v.shape, v.stride())          # same memory format as the input
            codes = _mx_codes_like(v, axis, codes_shape) if with_codes else None
            self._outs.append(out); self.codes.append(codes)
            table.jobs[k] = (v.data_ptr(), out.data_ptr(), _ptr(codes), outer, length, inner, mx_format_arg(format, rule), 0)
        self.bytes = 8 * sum(it[0].numel() for it in items)

    def run(self) -> List[torch.Tensor]:
        self._jobs.launch(lib.ppqhip_mx_fq_multi)
        return self._outs


def _mx_plan_table(plan: str, dtype, items):
    """The first loop of the MX plans: the table that keeps the values -- float32, on one device, dense in storage order -- and the
    items as (value, format, axis >= 0, rule id)."""
    if not items: raise ValueError(f'{plan} needs at least one item')
    items = [_mx_item(item) for item in items]
    table = JobTable(dtype, plan, len(items))
    for k, (value, format, axis, rule) in enumerate(items):
        table.tensor(value, 'Value', k, contiguous=False)
        axis = _mx_axis(value.dim(), axis)
        if not MXQuantizePlan.accepts(value, axis):
            raise RuntimeError(_KERNEL_FAILURE + f'{plan}: value must be dense in storage order (a private copy would go stale); see accepts()')
        items[k] = (value, format, axis, rule)
    return table, items


# ---- round tuning on the MX grid (include/ppq_hip.h ppqhip_mx_round_split_multi / ppqhip_mx_round_fwd_multi) ----
def mx_round_split_multi(items) -> List[tuple]:
    """The split of MX round tuning for every item in ONE launch (``ppqhip_mx_round_split_multi``).  items[k] = ``(w, format, axis)`` or
    ``(w, format, axis, scale_rule)``: ``w`` a float32 CUDA tensor (a non-contiguous one is copied).  Returns
    ``[(floored, rounding, scale_codes)]``: two contiguous float32 tensors shaped like ``w`` and the uint8 E8M0 codes (the axis replaced
    by ceil(len / 32))."""
    if not items: return []
    items = [_mx_item(item) for item in items]
    table, results = JobTable(MX_ROUND_SPLIT_JOB, 'MXRoundSplit', len(items)), []
    for k, (w, format, axis, rule) in enumerate(items):
        table.tensor(w, 'Value', k, contiguous=False)
        axis = _mx_axis(w.dim(), axis)
        v = w.detach().contiguous()
        outer, length, inner, codes_shape = _mx_geometry(v, axis)
        floored, rounding = torch.empty_like(v), torch.empty_like(v)
        codes = torch.empty(codes_shape, dtype=torch.uint8, device=table.dev)
        table.keep.append(v); results.append((floored, rounding, codes))
        table.jobs[k] = (v.data_ptr(), floored.data_ptr(), rounding.data_ptr(), codes.data_ptr(), outer, length, inner, mx_format_arg(format, rule), 0)
    table.launch(lib.ppqhip_mx_round_split_multi)
    return results


def mx_round_forward_jobs(items, outs) -> JobTable:
    """The job table of ``mx_round_forward_multi``: it holds POINTERS, so a caller whose tensors stay where they are (a group
    that is launched every step) builds it once."""
    _same_length('MXRoundForward', len(items), outs)
    table = JobTable(MX_ROUND_FWD_JOB, 'MXRoundForward', len(items), lib.ppqhip_mx_round_fwd_multi)
    for k, (floored, rounding, codes, format, axis) in enumerate(items):
        table.tensor(floored, 'Value', k); table.tensor(rounding, 'Rounding', k, like=floored); table.tensor(outs[k], 'Out', k, like=floored)
        axis = _mx_axis(floored.dim(), axis)
        outer, length, inner, codes_shape = _mx_geometry(floored, axis)
        _check(codes, torch.uint8, 'Scale codes(Expect to be UINT8)')
        if list(codes.shape) != codes_shape or not codes.is_contiguous() or codes.device != table.dev:
            table.refuse(k, f'scale_codes must be a contiguous uint8 tensor of shape {codes_shape} on the weight\'s device')
        table.keep.append(codes)
        table.jobs[k] = (floored.data_ptr(), rounding.data_ptr(), codes.data_ptr(), outs[k].data_ptr(), outer, length, inner, mx_format_id(format), 0)
    return table


def mx_round_forward_multi(items, outs=None, jobs=None) -> List[torch.Tensor]:
    """The forward of MX round tuning for every item in ONE launch (``ppqhip_mx_round_fwd_multi``).  items[k] =
    ``(floored, rounding, scale_codes, format, axis)``: contiguous float32 CUDA tensors of one shape and the uint8 codes of the split;
    ``outs`` (optional, caller-owned) receive the weights; ``jobs``: the table ``mx_round_forward_jobs`` built from the same items and
    outs.  The job table travels in the kernel arguments: capturable.  The backward is the identity: nothing else to launch."""
    if not items: return []
    if outs is None: outs = [torch.empty_like(it[0]) for it in items]
    if jobs is None: jobs = mx_round_forward_jobs(items, outs)
    jobs.run()
    return outs


# ---- packed MX export (include/ppq_hip.h ppqhip_mx_pack / ppqhip_mx_unpack and their _multi forms) ----
MX_BLOCK_BYTES = {'MXFP8_E4M3': 32, 'MXFP8_E5M2': 32, 'MXFP6_E3M2': 24, 'MXFP6_E2M3': 24, 'MXFP4_E2M1': 16, 'MXINT8': 32}
_MX_BLOCK_BYTES_BY_ID = {MX_FORMATS[k]: v for k, v in MX_BLOCK_BYTES.items()}


def mx_block_bytes(format) -> int:
    """Bytes of one packed block of 32 elements: 32 (MXFP8, MXINT8), 24 (MXFP6), 16 (MXFP4)."""
    return _MX_BLOCK_BYTES_BY_ID[mx_format_id(format)]


def mx_packed_shapes(shape, axis: int, format):
    """(shape of ``elements``, shape of ``scales``) of a tensor of ``shape`` packed along ``axis`` (not negative): the shape without
    the axis, plus [nb * B] resp. [nb] -- the block axis is last."""
    shape = [int(d) for d in shape]
    nb = (shape[axis] + MX_BLOCK - 1) // MX_BLOCK
    lead = shape[:axis] + shape[axis + 1:]
    return lead + [nb * mx_block_bytes(format)], lead + [nb]


def _mx_operand_args(rank, size, operands, shapes, bias):
    """The operand checks of the MX MFMA bindings at rank 2 (matmul) or 4 (conv).  ``operands``: (name, elements, scales, format id)
    each; ``shapes()``: their logical shapes, packed along axis 1, whose length ``size`` names (``'k'``) -- asked for once dtype,
    rank and device are known.  The bias has one entry per row of the last operand.  Returns the tensors as the kernel takes them,
    [elements, scales] of each operand in turn, the bias and the shapes."""
    dev = operands[0][1].device
    for op, e, s, _ in operands:
        for kind, t in (('elements', e), ('scales', s)):
            if isinstance(t, torch.Tensor) and t.dtype is torch.uint8 and t.is_cuda and t.dim() == rank and t.device == dev and t.numel(): continue
            _check(t, torch.uint8, f'{op} {kind}(Expect to be UINT8)')                   # not the common case: name what is wrong
            if t.dim() != rank: raise RuntimeError(_KERNEL_FAILURE + f'{op} {kind} must be {rank}-d, got {list(t.shape)}')
            if t.device != dev: raise RuntimeError(_KERNEL_FAILURE + f'{op} {kind} is on another device')
    shapes, out = shapes(), []
    for (name, e, s, fmt), shape in zip(operands, shapes):
        eshape, sshape = mx_packed_shapes(shape, 1, fmt)
        if list(e.shape) != eshape or list(s.shape) != sshape:
            raise RuntimeError(_KERNEL_FAILURE + f'{name}: elements / scales of shape {list(e.shape)} / {list(s.shape)}, expected {eshape} / {sshape} for {size} = {shape[1]}')
        e = e.contiguous()
        out += [e.clone() if e.data_ptr() % 16 else e, s.contiguous()]                   # the kernel's 16-byte loads; the allocator aligns
    if bias is not None:
        n = shapes[-1][0]
        _f32(bias, 'Bias')
        if list(bias.shape) != [n]: raise RuntimeError(_KERNEL_FAILURE + f'bias of shape {list(bias.shape)}, expected [{n}]')
        if bias.device != dev: raise RuntimeError(_KERNEL_FAILURE + 'bias is on another device')
        bias = bias.contiguous()
    return out, bias, shapes


def _mx_matmul_args(a_elements, a_scales, a_format, b_elements, b_scales, b_format, k, bias):
    """The checks of ``CUDA.MXMatmul`` / ``MXMatmulFused``; returns the tensors as the kernel takes them, the format ids, k, M and N."""
    fa, fb = mx_format_id(a_format), mx_format_id(b_format)
    k = int(k)
    if k <= 0: raise RuntimeError(_KERNEL_FAILURE + f'k must be positive, got {k}')
    (a_elements, a_scales, b_elements, b_scales), bias, ((m, _), (n, _)) = _mx_operand_args(
        2, 'k', (('A', a_elements, a_scales, fa), ('B', b_elements, b_scales, fb)),
        lambda: ([a_elements.shape[0], k], [b_elements.shape[0], k]), bias)
    return a_elements, a_scales, fa, b_elements, b_scales, fb, k, bias, m, n


def _mx_conv_args(x_elements, x_scales, x_format, w_elements, w_scales, w_format, c, bias, stride, padding, dilation):
    """The checks of ``CUDA.MXConv2d`` / ``MXConv2dFused``; returns the tensors as the kernel takes them, the format ids and
    ``geo = (n, c, h, w, o, kh, kw, sh, sw, ph, pw, dh, dw, oh, ow)``: the entry point's sizes, then the output's."""
    fx, fw = mx_format_id(x_format), mx_format_id(w_format)
    c = int(c)
    if c <= 0: raise RuntimeError(_KERNEL_FAILURE + f'c must be positive, got {c}')
    (x_elements, x_scales, w_elements, w_scales), bias, ((n, _, h, w), (o, _, kh, kw)) = _mx_operand_args(
        4, 'c', (('x', x_elements, x_scales, fx), ('w', w_elements, w_scales, fw)),
        lambda: [[v[0], c, v[1], v[2]] for v in (x_scales.shape, w_scales.shape)], bias)
    (sh, sw), (ph, pw), (dh, dw) = ([int(v) for v in pair] for pair in (stride, padding, dilation))
    if min(sh, sw, dh, dw) < 1 or min(ph, pw) < 0:
        raise RuntimeError(_KERNEL_FAILURE + f'stride {(sh, sw)} and dilation {(dh, dw)} must be at least 1, padding {(ph, pw)} at least 0')
    oh, ow = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if oh < 1 or ow < 1:
        raise RuntimeError(_KERNEL_FAILURE + f'a {kh} x {kw} kernel with dilation {(dh, dw)} does not fit an input of {h} x {w} padded by {(ph, pw)}')
    return x_elements, x_scales, fx, w_elements, w_scales, fw, bias, (n, c, h, w, o, kh, kw, sh, sw, ph, pw, dh, dw, oh, ow)


def _mx_fused_args(out_format, out_float, residual, shape, device):
    """The checks the fused bindings add: returns the id of ``out_format`` (a float format; without one nothing is packed and the id
    is a placeholder) and the residual, float32 of ``shape`` on ``device``."""
    fo = mx_format_id(out_format) if out_format is not None else MX_FORMATS['MXFP8_E4M3']
    if fo == MX_FORMATS['MXINT8']: raise RuntimeError(_KERNEL_FAILURE + 'out_format MXINT8 is not a format the fused epilogue packs')
    if out_format is None and not out_float: raise RuntimeError(_KERNEL_FAILURE + 'no output: out_format is None and out_float is False')
    if residual is not None:
        _f32(residual, 'Residual')
        if list(residual.shape) != list(shape): raise RuntimeError(_KERNEL_FAILURE + f'residual of shape {list(residual.shape)}, expected {list(shape)}')
        if residual.device != device: raise RuntimeError(_KERNEL_FAILURE + 'residual is on another device')
        if len(shape) == 2: residual = residual.contiguous()
    return fo, residual


def _mx_fused_outputs(shape, fo, out_format, out_float, device):
    """The outputs of a fused binding for a result of ``shape`` packed along axis 1: the float32 tensor with that axis last, or
    None, and the packed pair, or None, None."""
    out = torch.empty(shape[:1] + shape[2:] + shape[1:2], dtype=torch.float32, device=device) if out_float else None
    if out_format is None: return out, None, None
    eshape, sshape = mx_packed_shapes(shape, 1, fo)
    return out, torch.empty(eshape, dtype=torch.uint8, device=device), torch.empty(sshape, dtype=torch.uint8, device=device)


class MXPackPlan:
    """The sibling of ``MXQuantizePlan`` for the packed export: MANY tensors packed with ONE launch per call
    (``ppqhip_mx_pack_multi``).  Built once from ``(value, format, axis)`` items; ``run()`` packs all of them into one resident
    uint8 arena (every ``elements`` and every ``scales`` starts 16-B aligned) and returns ``[(elements, scales)]`` -- bytes identical
    to ``CUDA.MXPack`` per item.  The table holds POINTERS to the callers' tensors: in-place updates are seen by later runs; a value
    that is not dense in storage order is refused (``MXQuantizePlan.accepts``).  An item may carry its scale rule as a fourth entry."""
    accepts = staticmethod(MXQuantizePlan.accepts)

    def __init__(self, items):
        table, items = _mx_plan_table('MXPackPlan', MX_PACK_JOB, items)
        shapes = [mx_packed_shapes(v.shape, axis, format) for v, format, axis, _ in items]
        self._arena, pieces = _carve([math.prod(shape) for pair in shapes for shape in pair], torch.uint8, table.dev)
        self._jobs, self._outs = table, []
        for k, ((v, format, axis, rule), (eshape, sshape)) in enumerate(zip(items, shapes)):
            outer, length, inner, _ = _mx_geometry(v, axis)
            elements, scales = pieces[2 * k].view(eshape), pieces[2 * k + 1].view(sshape)
            self._outs.append((elements, scales))
            table.jobs[k] = (v.data_ptr(), elements.data_ptr(), scales.data_ptr(), outer, length, inner, mx_format_arg(format, rule), 0)
        self.bytes = sum(4 * it[0].numel() + e.numel() + s.numel() for it, (e, s) in zip(items, self._outs))

    def run(self):
        self._jobs.launch(lib.ppqhip_mx_pack_multi)
        return self._outs


def mx_unpack_multi(items) -> None:
    """``ppqhip_mx_unpack_multi``: every ``(elements, scales, y, format, axis)`` item in ONE call (one launch per 40 live jobs).
    ``y`` is the float32 tensor the packed pair unpacks INTO, dense in storage order (``MXQuantizePlan.accepts``); nothing is
    copied, the library checks pointers, sizes and overlaps."""
    table = JobTable(MX_UNPACK_JOB, 'mx_unpack_multi', len(items))
    for k, (elements, scales, y, format, axis) in enumerate(items):
        if y.numel() == 0:                                                                # an empty job: sizes 0, nothing launched for it
            table.jobs[k]['format'] = mx_format_id(format)
            continue
        for name, t, dtype in (('Elements', elements, torch.uint8), ('Scales', scales, torch.uint8), ('Out', y, torch.float32)):
            table.tensor(t, name, k, dtype, contiguous=False)
        axis = _mx_axis(y.dim(), axis)
        if not MXQuantizePlan.accepts(y, axis): table.refuse(k, 'Out must be dense in storage order')
        outer, length, inner, _ = _mx_geometry(y, axis)
        table.jobs[k] = (elements.data_ptr(), scales.data_ptr(), y.data_ptr(), outer, length, inner, mx_format_id(format), 0)
    table.launch(lib.ppqhip_mx_unpack_multi)
