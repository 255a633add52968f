"""The bindings of the linear INT8 kernels (``csrc/int8_gemm.hip``, ``csrc/int8_conv.hip``) and of their forms
with a packed INT4 weight (``csrc/int4_gemm.hip``, ``csrc/int4_conv.hip``; section 9.23): ``CUDA.Int8Matmul`` / ``Int8Conv2d`` /
``Int4Matmul`` / ``Int4Conv2d`` forward here, ``Int8DepthwiseConv2d`` to the depthwise kernel (``csrc/int8_dwconv.hip``; section
9.24) and ``Int8GroupedConv2d`` to the grouped one (``csrc/int8_gconv.hip``; section 9.25), ``Int8Bmm`` to the batched matmul of two activations
(``csrc/int8_bmm.hip``; section 9.27).  Operands are int8 codes with the reduction
axis last and padded to a multiple of 32; an INT4 weight is uint8, two codes per byte, half as many bytes along that axis; a depthwise
weight is ``[kh, kw, Cp]``, a grouped one ``[O, kh, kw, 32 nbs]``."""
import torch

from .._lib import lib
from ._base import _KERNEL_FAILURE, _DeviceOf, _check, _f32, _ptr, _raise, _stream

INT8_BLOCK = 32          # the K of one v_mfma_i32_16x16x32_i8: rows are padded to it
DEPTHWISE_LDS_BYTES = 65536      # what a workgroup of the depthwise kernel may stage


def _refuse(what: str): raise RuntimeError(_KERNEL_FAILURE + what)


def _int8_operands(rank, names, operands, int4=False, same_k=True):
    """int8 -- with ``int4`` the second one uint8, two codes per byte --, on one GPU, ``rank``-d (a pair: one rank each), contiguous,
    the last axis a multiple of 32 codes and (``same_k``) the same for both; a tensor whose data does not start on a 16-byte boundary
    is copied (the allocator aligns)."""
    dev, out = operands[0].device if isinstance(operands[0], torch.Tensor) else None, []
    for name, t, per_byte, rank in zip(names, operands, (1, 2 if int4 else 1), rank if isinstance(rank, tuple) else (rank, rank)):
        if per_byte == 2: _check(t, torch.uint8, f'{name}(Expect to be UINT8: packed INT4)')
        else: _check(t, torch.int8, f'{name}(Expect to be INT8)')
        if t.dim() != rank: _refuse(f'{name} must be {rank}-d, got {list(t.shape)}')
        if t.device != dev: _refuse(f'{name} is on another device')
        if not t.is_contiguous(): _refuse(f'{name} must be contiguous')
        if t.shape[-1] * per_byte % INT8_BLOCK: _refuse(f'{name}: the last axis ({t.shape[-1] * per_byte} codes) must be padded to a multiple of {INT8_BLOCK}')
        out.append(t.clone() if t.data_ptr() % 16 else t)
    if same_k and out[0].shape[-1] != out[1].shape[-1] * (2 if int4 else 1):
        _refuse(f'{names[0]} and {names[1]} differ in their last axis: {out[0].shape[-1]} and {out[1].shape[-1] * (2 if int4 else 1)}' + (' codes' if int4 else ''))
    return out


def _int8_tail(n, shape, dev, sums, zx, mul, bias, residual, out_float, out_q, mul_len=None, need_sums=True):
    """The checks of everything but the operands; ``shape`` is the result's with the columns last.  Returns the tensors as the kernel
    takes them, the outputs and the seven scalars of the output grid.  ``mul`` is ``[n]`` unless ``mul_len`` says otherwise;
    ``need_sums=False``: the kernel makes the sums a zero point needs itself."""
    zx = int(zx)
    if not -128 <= zx <= 127: _refuse(f'zx {zx} is not an int8 zero point')
    for name, t in (('mul', mul), ('bias', bias)):
        if t is None and name == 'bias': continue
        _f32(t, name)
        want = n if mul_len is None or name == 'bias' else mul_len
        if list(t.shape) != [want]: _refuse(f'{name} of shape {list(t.shape)}, expected [{want}]')
        if t.device != dev: _refuse(f'{name} is on another device')
    if sums is not None:
        _check(sums, torch.int32, 'sums(Expect to be INT32)')
        if list(sums.shape) != [n] or sums.device != dev: _refuse(f'sums of shape {list(sums.shape)} on {sums.device}, expected [{n}] on {dev}')
        sums = sums.contiguous()
    elif zx != 0 and need_sums: _refuse('sums is required with a zero point other than 0')
    if residual is not None:
        _f32(residual, 'Residual')
        if list(residual.shape) != list(shape): _refuse(f'residual of shape {list(residual.shape)}, expected {list(shape)}')
        if residual.device != dev: _refuse('residual is on another device')
        residual = residual.contiguous()
    if out_q is None and not out_float: _refuse('no output: out_q is None and out_float is False')
    c = torch.empty(shape, dtype=torch.float32, device=dev) if out_float else None
    q, grid = None, (1.0, 0, -128, 127, 0, 0)
    if out_q is not None:
        sy, zy, qmin, qmax, rounding, q_nan = out_q
        grid = (float(sy), int(zy), int(qmin), int(qmax), int(rounding), int(q_nan))
        q = torch.empty(list(shape[:-1]) + [(n + INT8_BLOCK - 1) // INT8_BLOCK * INT8_BLOCK], dtype=torch.int8, device=dev)
    return sums, zx, mul.contiguous(), (bias.contiguous() if bias is not None else None), residual, c, q, grid


SKINNY_MAX_M = 64        # the rows the skinny GEMM takes (csrc/int8_skinny.hpp)


def int8_matmul(a, b, b_sums, zx: int, mul, bias=None, residual=None, relu: bool = False, out_float: bool = True, out_q=None, int4: bool = False,
                skinny: bool = False):
    """``ppqhip_int8_gemm``: ``a [M, Kp]`` and ``b [N, Kp]`` int8 codes, ``b_sums [N]`` int32 (None with ``zx == 0``), ``mul [N]``
    float32.  ``out_q``: None or ``(sy, zy, qmin, qmax, rounding, q_nan)`` in the stored int8 domain.  Returns ``(c, q)``: float32
    ``[M, N]`` (None with ``out_float=False``) and int8 ``[M, ceil32(N)]`` (None without ``out_q``).
    ``int4``: ``ppqhip_int4_gemm``, ``b [N, Kp / 2]`` uint8, the packed INT4 codes.  ``skinny``: ``ppqhip_int8_gemm_skinny`` /
    ``ppqhip_int4_gemm_skinny``, the kernel for ``M <= 64`` (section 9.26): the same bits; more rows are refused."""
    a, b = _int8_operands(2, ('A', 'B'), (a, b), int4)
    m, n = a.shape[0], b.shape[0]
    if skinny and m > SKINNY_MAX_M: _refuse(f'M = {m}: the skinny kernel takes at most {SKINNY_MAX_M} rows')
    sums, zx, mul, bias, residual, c, q, grid = _int8_tail(n, [m, n], a.device, b_sums, zx, mul, bias, residual, out_float, out_q)
    if skinny: gemm = lib.ppqhip_int4_gemm_skinny if int4 else lib.ppqhip_int8_gemm_skinny
    else: gemm = lib.ppqhip_int4_gemm if int4 else lib.ppqhip_int8_gemm
    with _DeviceOf(a):
        _raise(gemm(a.data_ptr(), b.data_ptr(), _ptr(sums), zx, mul.data_ptr(), _ptr(bias), _ptr(residual), 1 if relu else 0, _ptr(c), _ptr(q), *grid,
                    m, n, a.shape[1], _stream()))
    return c, q


BMM_MAX_KP = 32768       # the longest padded reduction of int8_bmm: 32768 * 255 * 255 < 2^31 (csrc/int8_bmm.hpp)


def int8_bmm(a, b, transpose_b: bool, za: int, zb: int, mul, n: int = None, residual=None, relu: bool = False, out_float: bool = True, out_q=None):
    """``ppqhip_int8_bmm``: ``a [B, M, Kp]`` int8 codes with zero point ``za``; ``b`` with zero point ``zb`` is ``[B, N, Kp]``
    (``transpose_b``: ``a . b^T``) or ``[B, K, Np]`` with ``n`` of its ``Np`` columns live (``a . b``: K is the rows ``b`` has, not
    padded); ``mul`` ONE float32 on the device, ``sa * sb``.  Neither operand has sums: the kernel makes them.  ``out_q`` as in
    ``int8_matmul``.  Returns ``(c, q)``: float32 ``[B, M, N]`` (None with ``out_float=False``) and int8 ``[B, M, ceil32(N)]`` (None
    without ``out_q``).  ONE launch for all batches."""
    a, b = _int8_operands(3, ('A', 'B'), (a, b), same_k=bool(transpose_b))
    batch, m, kp = a.shape
    if b.shape[0] != batch: _refuse(f'A and B differ in their batch: {batch} and {b.shape[0]}')
    if transpose_b: k, n = kp, b.shape[1]
    else:
        k, n = b.shape[1], int(b.shape[2] if n is None else n)
        if not kp - INT8_BLOCK < k <= kp: _refuse(f'B has {k} rows, which do not pad to the {kp} codes of a row of A')
        if not b.shape[2] - INT8_BLOCK < n <= b.shape[2]: _refuse(f'n = {n} does not pad to the {b.shape[2]} stored columns of B')
    if kp > BMM_MAX_KP: _refuse(f'a padded reduction length of {kp}: more than {BMM_MAX_KP} could overflow int32')
    zb = int(zb)
    if not -128 <= zb <= 127: _refuse(f'zb {zb} is not an int8 zero point')
    _, za, mul, _, residual, c, q, grid = _int8_tail(n, [batch, m, n], a.device, None, za, mul, None, residual, out_float, out_q, mul_len=1, need_sums=False)
    with _DeviceOf(a):
        _raise(lib.ppqhip_int8_bmm(a.data_ptr(), b.data_ptr(), 1 if transpose_b else 0, za, zb, mul.data_ptr(), _ptr(residual), 1 if relu else 0, _ptr(c), _ptr(q),
                                   *grid, batch, m, n, k, _stream()))
    return c, q


def int8_conv2d(x, w, w_sums, zx: int, mul, c: int, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), residual=None,
                relu: bool = False, out_float: bool = True, out_q=None, int4: bool = False):
    """``ppqhip_int8_conv2d``: ``x [N, H, W, Cp]`` and ``w [O, kh, kw, Cp]`` int8 codes of a convolution with ``c`` channels.
    ``residual`` is ``[N, O, OH, OW]``; a tensor that is not channels-last is copied into that layout.  Returns ``(y, q)``: float32
    ``[N, O, OH, OW]`` with channels-last strides and int8 ``[N, OH, OW, ceil32(O)]``.
    ``int4``: ``ppqhip_int4_conv2d``, ``w [O, kh, kw, Cp / 2]`` uint8, the packed INT4 codes."""
    x, w = _int8_operands(4, ('x', 'w'), (x, w), int4)
    c = int(c)
    if not 0 < c <= x.shape[-1] or x.shape[-1] - c >= INT8_BLOCK: _refuse(f'c = {c} does not pad to the {x.shape[-1]} stored channels')
    (n, h, wd, _), (o, kh, kw, _) = x.shape, w.shape
    (sh, sw), (ph, pw), (dh, dw) = ([int(v) for v in pair] for pair in (stride, padding, dilation))
    if min(sh, sw, dh, dw) < 1 or min(ph, pw) < 0: _refuse(f'stride {(sh, sw)} and dilation {(dh, dw)} must be at least 1, padding {(ph, pw)} at least 0')
    oh, ow = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (wd + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if oh < 1 or ow < 1: _refuse(f'a {kh} x {kw} kernel with dilation {(dh, dw)} does not fit an input of {h} x {wd} padded by {(ph, pw)}')
    if residual is not None and isinstance(residual, torch.Tensor) and residual.dim() == 4: residual = residual.permute(0, 2, 3, 1)
    sums, zx, mul, bias, residual, y, q, grid = _int8_tail(o, [n, oh, ow, o], x.device, w_sums, zx, mul, bias, residual, out_float, out_q)
    conv = lib.ppqhip_int4_conv2d if int4 else lib.ppqhip_int8_conv2d
    with _DeviceOf(x):
        _raise(conv(x.data_ptr(), w.data_ptr(), _ptr(sums), zx, mul.data_ptr(), _ptr(bias), _ptr(residual), 1 if relu else 0, _ptr(y), _ptr(q), *grid,
                    n, c, h, wd, o, kh, kw, sh, sw, ph, pw, dh, dw, _stream()))
    return (y.permute(0, 3, 1, 2) if y is not None else None), q


def depthwise_lds_bytes(kh: int, kw: int, stride, dilation) -> int:
    """What a workgroup of ``csrc/int8_dwconv.hip`` stages for one 8 x 8 tile: the input patch, ``7 stride + (k - 1) dilation + 1``
    pixels per axis at 32 bytes (48 where the horizontal stride is 2 mod 4: DESIGN.md section 9.24), and ``128 kh kw`` bytes of
    expanded weights."""
    (sh, sw), (dh, dw) = stride, dilation
    return (7 * sh + (kh - 1) * dh + 1) * (7 * sw + (kw - 1) * dw + 1) * (48 if sw % 4 == 2 else 32) + 128 * kh * kw


def int8_depthwise_conv2d(x, w, w_sums, zx: int, mul, c: int, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), residual=None,
                          relu: bool = False, out_float: bool = True, out_q=None):
    """``ppqhip_int8_dwconv2d``: ``x [N, H, W, Cp]`` and ``w [kh, kw, Cp]`` int8 codes of a depthwise convolution (groups == ``c``,
    channel multiplier 1), ``w_sums`` / ``mul`` / ``bias`` ``[c]``.  ``residual`` is ``[N, c, OH, OW]``; a tensor that is not
    channels-last is copied into that layout.  Returns ``(y, q)``: float32 ``[N, c, OH, OW]`` with channels-last strides and int8
    ``[N, OH, OW, Cp]``.  Refused like ``int8_conv2d``, and a geometry that stages more than 64 KiB of LDS."""
    x, w = _int8_operands((4, 3), ('x', 'w'), (x, w))
    c = int(c)
    if not 0 < c <= x.shape[-1] or x.shape[-1] - c >= INT8_BLOCK: _refuse(f'c = {c} does not pad to the {x.shape[-1]} stored channels')
    (n, h, wd, _), (kh, kw, _) = x.shape, w.shape
    (sh, sw), (ph, pw), (dh, dw) = ([int(v) for v in pair] for pair in (stride, padding, dilation))
    if min(sh, sw, dh, dw) < 1 or min(ph, pw) < 0: _refuse(f'stride {(sh, sw)} and dilation {(dh, dw)} must be at least 1, padding {(ph, pw)} at least 0')
    oh, ow = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (wd + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if oh < 1 or ow < 1: _refuse(f'a {kh} x {kw} kernel with dilation {(dh, dw)} does not fit an input of {h} x {wd} padded by {(ph, pw)}')
    need = depthwise_lds_bytes(kh, kw, (sh, sw), (dh, dw))
    if need > DEPTHWISE_LDS_BYTES:
        _refuse(f'a {kh} x {kw} window at stride {(sh, sw)} and dilation {(dh, dw)} stages {need} bytes of LDS: a workgroup has {DEPTHWISE_LDS_BYTES}')
    if residual is not None and isinstance(residual, torch.Tensor) and residual.dim() == 4: residual = residual.permute(0, 2, 3, 1)
    sums, zx, mul, bias, residual, y, q, grid = _int8_tail(c, [n, oh, ow, c], x.device, w_sums, zx, mul, bias, residual, out_float, out_q)
    with _DeviceOf(x):
        _raise(lib.ppqhip_int8_dwconv2d(x.data_ptr(), w.data_ptr(), _ptr(sums), zx, mul.data_ptr(), _ptr(bias), _ptr(residual), 1 if relu else 0, _ptr(y),
                                        _ptr(q), *grid, n, c, h, wd, kh, kw, sh, sw, ph, pw, dh, dw, _stream()))
    return (y.permute(0, 3, 1, 2) if y is not None else None), q


def int8_grouped_conv2d(x, w, w_sums, zx: int, mul, c: int, groups: int, nbs: int, cb0, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1),
                        residual=None, relu: bool = False, out_float: bool = True, out_q=None):
    """``ppqhip_int8_gconv2d``: ``x [N, H, W, Cp]`` int8 codes of ``c`` channels and ``w [O, kh, kw, 32 nbs]`` the grouped weight as
    ``int8_grouped_weight`` lays it out for ``groups`` groups -- block ``j`` of a tap of row ``o`` is channel block ``cb0[o // 32] + j``,
    zero outside the row's own group --, ``cb0`` int32 ``[ceil(O / 32)]``, ``w_sums`` / ``mul`` / ``bias`` ``[O]``.  ``residual`` is
    ``[N, O, OH, OW]``; a tensor that is not channels-last is copied into that layout.  Returns ``(y, q)``: float32 ``[N, O, OH, OW]``
    with channels-last strides and int8 ``[N, OH, OW, ceil32(O)]``.  Refused like ``int8_conv2d``, and groups that do not divide ``c``
    and ``O``."""
    x, w = _int8_operands(4, ('x', 'w'), (x, w), same_k=False)
    c, groups, nbs = int(c), int(groups), int(nbs)
    if not 0 < c <= x.shape[-1] or x.shape[-1] - c >= INT8_BLOCK: _refuse(f'c = {c} does not pad to the {x.shape[-1]} stored channels')
    (n, h, wd, _), (o, kh, kw, wk) = x.shape, w.shape
    if groups < 1 or c % groups or o % groups: _refuse(f'c = {c} and o = {o} must both be multiples of groups = {groups}')
    if nbs < 1 or wk != nbs * INT8_BLOCK: _refuse(f'w stores {wk} codes per tap, expected {INT8_BLOCK} * nbs = {nbs * INT8_BLOCK}')
    slices = (o + INT8_BLOCK - 1) // INT8_BLOCK
    _check(cb0, torch.int32, 'cb0(Expect to be INT32)')
    if list(cb0.shape) != [slices] or cb0.device != x.device: _refuse(f'cb0 of shape {list(cb0.shape)} on {cb0.device}, expected [{slices}] on {x.device}')
    (sh, sw), (ph, pw), (dh, dw) = ([int(v) for v in pair] for pair in (stride, padding, dilation))
    if min(sh, sw, dh, dw) < 1 or min(ph, pw) < 0: _refuse(f'stride {(sh, sw)} and dilation {(dh, dw)} must be at least 1, padding {(ph, pw)} at least 0')
    oh, ow = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (wd + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if oh < 1 or ow < 1: _refuse(f'a {kh} x {kw} kernel with dilation {(dh, dw)} does not fit an input of {h} x {wd} padded by {(ph, pw)}')
    if residual is not None and isinstance(residual, torch.Tensor) and residual.dim() == 4: residual = residual.permute(0, 2, 3, 1)
    sums, zx, mul, bias, residual, y, q, grid = _int8_tail(o, [n, oh, ow, o], x.device, w_sums, zx, mul, bias, residual, out_float, out_q)
    cb0 = cb0.contiguous()
    with _DeviceOf(x):
        _raise(lib.ppqhip_int8_gconv2d(x.data_ptr(), w.data_ptr(), _ptr(sums), zx, mul.data_ptr(), _ptr(bias), _ptr(residual), 1 if relu else 0, _ptr(y),
                                       _ptr(q), *grid, n, c, h, wd, o, kh, kw, sh, sw, ph, pw, dh, dw, groups, nbs, cb0.data_ptr(), _stream()))
    return (y.permute(0, 3, 1, 2) if y is not None else None), q
