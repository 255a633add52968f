"""The packed MX export on the GPU: the HIP kernels (ppq_amd/csrc/mx_pack.hip) against the oracle (tests/mx_pack_reference.py).
The contract is exact, so every comparison is ``==`` on bytes, or on the uint32 view of the values."""
import functools

import numpy as np
import pytest
import torch

import mx_pack_reference as P
import mx_reference as R
from ppq_amd import CUDA, MXFormat, MXTensor, _lib, export_graph_mx, ffi, harness, mx_dequantize, mx_fake_quant, mx_quantize, quantize_graph_mx

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORMATS = R.FORMATS
SENTINEL = 0xA5


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hip_pack(x, fmt: str, axis: int = -1):
    """CUDA.MXPack of a NumPy array or a CUDA tensor -> (elements, scales) as NumPy arrays."""
    e, s = CUDA.MXPack(dev(x) if isinstance(x, np.ndarray) else x, MXFormat[fmt], axis)
    assert e.is_contiguous() and s.is_contiguous() and e.dtype == torch.uint8 and s.dtype == torch.uint8
    return e.cpu().numpy(), s.cpu().numpy()


def hip_unpack(e: np.ndarray, s: np.ndarray, fmt: str, shape, axis: int = -1) -> np.ndarray:
    y = CUDA.MXUnpack(dev(e), dev(s), MXFormat[fmt], shape, axis)
    assert y.is_contiguous() and tuple(y.shape) == tuple(shape)
    return y.cpu().numpy()


def assert_same(got, want, what):
    (e, s), (re_, rs) = got, want
    assert e.shape == re_.shape and s.shape == rs.shape, (what, e.shape, re_.shape, s.shape, rs.shape)
    assert np.array_equal(s, rs), f'{what}: scales differ'
    bad = np.flatnonzero(e.ravel() != re_.ravel())
    assert bad.size == 0, f'{what}: {bad.size} element bytes differ, first at {bad[:4]}: {e.ravel()[bad[:4]]} != {re_.ravel()[bad[:4]]}'


def assert_bits(got: np.ndarray, want: np.ndarray, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
    assert bad.size == 0, f'{what}: {bad.size} values differ, first at {bad[:4]}: {got.ravel()[bad[:4]]} != {want.ravel()[bad[:4]]}'


@functools.lru_cache(maxsize=None)
def layout_case(k: int, fmt: str):
    """(input, axis, the oracle's packed tensor, the oracle's unpacking of it)."""
    shape, axis = (R.LAYOUTS + [(R.CHANNELS_LAST_SHAPE, 1)])[k]
    x = R.layout_input(shape, seed=k)
    packed = P.pack(x, fmt, axis)
    return x, axis, packed, P.unpack(*packed, fmt, shape, axis)


@functools.lru_cache(maxsize=None)
def block_case(kind: str, fmt: str):
    x = R.special_blocks(fmt) if kind == 'special' else R.exhaustive_blocks(fmt)
    packed = P.pack(x, fmt)
    return x, packed, P.unpack(*packed, fmt, x.shape)


# ------------------------------------------------------------------------------------------------------- kernels against the oracle
@pytest.mark.parametrize('fmt', FORMATS)
def test_layouts(fmt):
    for k, (shape, axis) in enumerate(R.LAYOUTS):
        x, axis, packed, values = layout_case(k, fmt)
        assert_same(hip_pack(x, fmt, axis), packed, f'{fmt} {shape} axis {axis}')
        assert_bits(hip_unpack(*packed, fmt, shape, axis), values, f'{fmt} {shape} axis {axis} unpack')
        if axis == -1: assert_same(hip_pack(x, fmt, len(shape) - 1), packed, f'{fmt} {shape} positive axis')
    sliced = dev(layout_case(1, fmt)[0])[:, 4:36]                                        # not dense: copied
    assert_same(hip_pack(sliced, fmt), P.pack(sliced.cpu().numpy(), fmt), f'{fmt} non-contiguous slice')


@pytest.mark.parametrize('fmt', FORMATS)
def test_channels_last_takes_the_contiguous_path(fmt):
    x, axis, packed, values = layout_case(len(R.LAYOUTS), fmt)
    nchw = dev(x)
    nhwc = nchw.contiguous(memory_format=torch.channels_last)
    assert ffi._mx_dense(nhwc, 1) is nhwc and ffi._mx_geometry(nhwc, 1)[:3] == (32, 64, 1)       # no copy; blocks are rows
    assert ffi._mx_geometry(nchw, 1)[:3] == (2, 64, 16)
    assert_same(hip_pack(nchw, fmt, 1), packed, fmt + ' NCHW')
    assert_same(hip_pack(nhwc, fmt, 1), packed, fmt + ' channels-last')
    assert list(packed[0].shape) == [2, 4, 4, 2 * P.BLOCK_BYTES[fmt]] and list(packed[1].shape) == [2, 4, 4, 2]
    assert_bits(hip_unpack(*packed, fmt, x.shape, 1), values, fmt + ' unpack')


@pytest.mark.parametrize('fmt', FORMATS)
def test_exhaustive_cast(fmt):
    """Every float32 pattern whose exponent is at most emax (high half-word x three low half-words), in blocks with X = 1."""
    x, packed, values = block_case('exhaustive', fmt)
    assert (packed[1] == 127).all() and x.size > 90000
    assert_same(hip_pack(x, fmt), packed, fmt)
    assert_bits(hip_unpack(*packed, fmt, x.shape), values, fmt + ' unpack')
    assert P.same_but_nan(values, R.quantize(x, fmt)[0], np.zeros(x.shape, bool), fmt)                  # the oracle's own parity


@pytest.mark.parametrize('fmt', FORMATS)
def test_special_blocks(fmt):
    x, packed, values = block_case('special', fmt)
    assert_same(hip_pack(x, fmt), packed, fmt + ' rows')
    assert_same(hip_pack(np.ascontiguousarray(x.T), fmt, 0), packed, fmt + ' strided')    # the packed form is the same: the axis is last
    assert_bits(hip_unpack(*packed, fmt, x.shape), values, fmt + ' unpack rows')
    assert_bits(hip_unpack(*packed, fmt, x.T.shape, 0), np.ascontiguousarray(values.T), fmt + ' unpack strided')
    odd = np.ascontiguousarray(x[:, :31])                                                # the one-element-per-lane rows
    want = P.pack(odd, fmt)
    assert_same(hip_pack(odd, fmt), want, fmt + ' scalar rows')
    assert_bits(hip_unpack(*want, fmt, odd.shape), P.unpack(*want, fmt, odd.shape), fmt + ' unpack scalar rows')


@pytest.mark.parametrize('fmt', FORMATS)
def test_foreign_codes(fmt):
    """Every code of the format under scale 127 and under scale 0xFF, through the three bodies of the unpack kernel."""
    e, s = P.foreign_codes(fmt)
    n = s.shape[-1] * 32
    want = P.unpack(e, s, fmt, (2, n))
    assert_bits(hip_unpack(e, s, fmt, (2, n)), want, fmt + ' rows')
    assert_bits(hip_unpack(e, s, fmt, (n, 2), 0), np.ascontiguousarray(want.T), fmt + ' strided')
    assert_bits(hip_unpack(e, s, fmt, (2, n - 1)), np.ascontiguousarray(want[:, :n - 1]), fmt + ' scalar rows')


@pytest.mark.parametrize('fmt', ['MXFP4_E2M1', 'MXFP6_E3M2', 'MXFP8_E4M3'])            # one format per store width of rows4
def test_rows_above_the_two_float4_threshold(fmt):
    """[2048, 2084]: more than 4 M elements, where a rows4 lane of the single-tensor launch owns two float4; a tail of 4 in every row."""
    shape = (2048, 2084)
    assert shape[0] * shape[1] > 4 << 20 and shape[1] % 32 == 4
    x = R.layout_input(shape, seed=21)
    packed = P.pack(x, fmt)
    assert_same(hip_pack(x, fmt), packed, fmt)
    assert_bits(hip_unpack(*packed, fmt, shape), P.unpack(*packed, fmt, shape), fmt + ' unpack')


# ------------------------------------------------------------------------------------------------------------- parity on the device
@pytest.mark.parametrize('fmt', FORMATS)
def test_parity_with_fake_quant_and_the_torch_arm(fmt):
    x = dev(R.gaussian_blocks())
    t = mx_quantize(x, fmt)
    arm = mx_quantize(x, fmt, use_kernels=False)
    assert torch.equal(t.elements, arm.elements) and torch.equal(t.scales, arm.scales)
    y, fq = mx_dequantize(t), mx_fake_quant(x, fmt)
    assert torch.equal(y.view(torch.int32), mx_dequantize(t, use_kernels=False).view(torch.int32))
    none = np.zeros(x.shape, bool)
    assert P.same_but_nan(y.cpu().numpy(), fq.cpu().numpy(), none, fmt)
    s = dev(R.special_blocks(fmt))                                                       # with NaN, Inf and signed zeros
    for v, axis in ((s, -1), (s.T.contiguous(), 0)):
        t = mx_quantize(v, fmt, axis)
        arm = mx_quantize(v, fmt, axis, use_kernels=False)
        assert torch.equal(t.elements, arm.elements) and torch.equal(t.scales, arm.scales)
        y = mx_dequantize(t)
        assert torch.equal(y.view(torch.int32), mx_dequantize(arm, use_kernels=False).view(torch.int32))
        assert P.same_but_nan(y.cpu().numpy(), mx_fake_quant(v, fmt, axis).cpu().numpy(), P.nan_mask(v.cpu().numpy(), fmt, axis), fmt)


# ------------------------------------------------------------------------------------------------------------- neighbours untouched
@pytest.mark.parametrize('fmt', ['MXFP4_E2M1', 'MXFP6_E2M3', 'MXFP8_E4M3'])
@pytest.mark.parametrize('k', [2, 4, 5])            # rows with a tail of 8; a one-element tail on unaligned rows; strided with a short tail
@pytest.mark.parametrize('shift', [0, 3])           # outputs 16-B aligned, and not even 4-B aligned (the byte-store bodies)
def test_neighbours_untouched(fmt, k, shift):
    """elements, scales and the unpacked output carved out of larger buffers full of a sentinel: every byte outside keeps it."""
    x, axis, (e, s), values = layout_case(k, fmt)
    t = dev(x)
    outer, length, inner, _ = ffi._mx_geometry(t, axis % t.dim())
    at_e, at_s = 64 + shift, 64 + shift + (e.size + 63) // 64 * 64 + 64
    buf = torch.full((at_s + s.size + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    assert base % 16 == 0
    assert _lib.lib.ppqhip_mx_pack(t.data_ptr(), base + at_e, base + at_s, outer, length, inner, MXFormat[fmt].value, None) == 0, _lib.last_error()
    got = buf.cpu().numpy()
    assert np.array_equal(got[at_e: at_e + e.size], e.ravel()) and np.array_equal(got[at_s: at_s + s.size], s.ravel())
    keep = np.ones(got.size, bool)
    keep[at_e: at_e + e.size] = False; keep[at_s: at_s + s.size] = False
    assert (got[keep] == SENTINEL).all()

    out = torch.full((4 * (x.size + 32),), SENTINEL, dtype=torch.uint8, device=DEV)
    at_y = 16 + (1 if shift else 0)                                                      # 16-B aligned, or only 4-B aligned
    assert _lib.lib.ppqhip_mx_unpack(base + at_e, base + at_s, out.data_ptr() + 4 * at_y, outer, length, inner, MXFormat[fmt].value, None) == 0, _lib.last_error()
    got_y = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_y[at_y: at_y + x.size], R.bits(values).ravel())
    assert (np.delete(got_y, np.s_[at_y: at_y + x.size]) == SENTINEL * 0x01010101).all()
    assert np.array_equal(buf.cpu().numpy(), got)                                        # unpack writes nothing into its inputs


# ---------------------------------------------------------------------------------------------------------------------------- multi
def test_multi_tensor_plan():
    """45 small tensors of mixed formats and paths in one call (more than 40: the table is chunked) equal the 45 single calls."""
    shapes = [((1, 32), -1), ((2, 33), -1), ((4, 35, 3, 3), 1)]
    items = []
    for k in range(45):
        shape, axis = shapes[k % 3]
        items.append((dev(R.layout_input(shape, seed=100 + k)), MXFormat[FORMATS[(k // 3) % 6]], axis))
    assert len({(tuple(t.shape), f) for t, f, _ in items}) == 18                         # every format on every path
    plan = ffi.MXPackPlan(items)
    outs = plan.run()
    assert len(outs) == 45
    for k, ((t, fmt, axis), (e, s)) in enumerate(zip(items, outs)):
        assert e.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
        we, ws = CUDA.MXPack(t, fmt, axis)
        assert e.shape == we.shape and s.shape == ws.shape and torch.equal(e, we) and torch.equal(s, ws), f'plan item {k} {fmt.name}'
        assert_same((e.cpu().numpy(), s.cpu().numpy()), P.pack(t.cpu().numpy(), fmt.name, axis), f'plan item {k} {fmt.name}')
    before = [(e.clone(), s.clone()) for e, s in outs]
    with torch.no_grad(): items[43][0].mul_(3.0)                                         # the table holds pointers: in-place updates are seen
    outs = plan.run()
    we, ws = CUDA.MXPack(*items[43])
    assert torch.equal(outs[43][0], we) and torch.equal(outs[43][1], ws) and not torch.equal(outs[43][0], before[43][0])
    for k in range(43): assert torch.equal(outs[k][0], before[k][0]) and torch.equal(outs[k][1], before[k][1])
    with pytest.raises(RuntimeError, match='dense'): ffi.MXPackPlan([(items[1][0][:, ::2], 'MXINT8', -1)])
    with pytest.raises(ValueError, match='at least one'): ffi.MXPackPlan([])


# ------------------------------------------------------------------------------------------------------------------- unpack, multi
class _Arena:
    """A device buffer full of SENTINEL that tensors are carved out of; ``untouched()``: every byte outside them still holds it."""
    def __init__(self, nbytes: int):
        self.buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.at, self.spans = 64, []
        assert self.buf.data_ptr() % 16 == 0

    def take(self, nbytes: int, shift: int = 0) -> torch.Tensor:
        """``nbytes`` bytes, ``shift`` bytes behind a 16-B boundary, at least 16 sentinel bytes away from their neighbours."""
        lo = (self.at + 15) // 16 * 16 + shift
        self.at = lo + nbytes + 16
        assert self.at + 64 <= self.buf.numel()
        self.spans.append((lo, lo + nbytes))
        return self.buf[lo: lo + nbytes]

    def floats(self, shape, shift: int = 0, channels_last: bool = False) -> torch.Tensor:
        t = self.take(4 * int(np.prod(shape)), shift).view(torch.float32)
        if not channels_last: return t.view(tuple(shape))
        n, c, h, w = shape
        return t.as_strided(tuple(shape), (c * h * w, 1, w * c, c))

    def untouched(self) -> bool:
        keep = np.ones(self.buf.numel(), bool)
        for lo, hi in self.spans: keep[lo:hi] = False
        return bool((self.buf.cpu().numpy()[keep] == SENTINEL).all())


def _unpack_alone(e: torch.Tensor, s: torch.Tensor, fmt: str, shape, axis: int, channels_last: bool = False) -> np.ndarray:
    """The single-job entry point on the same bytes, into a tensor of the same memory format."""
    y = torch.empty(tuple(shape), dtype=torch.float32, device=DEV, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    outer, length, inner, _ = ffi._mx_geometry(y, axis % len(shape))
    assert _lib.lib.ppqhip_mx_unpack(e.data_ptr(), s.data_ptr(), y.data_ptr(), outer, length, inner, MXFormat[fmt].value, None) == 0, _lib.last_error()
    return y.cpu().numpy()


def _unpack_table(picks, ins: _Arena, outs: _Arena):
    """picks[k] = (x or (elements, scales, shape), fmt, axis, shift of `elements`, shift of y, channels-last y) -> the items of one ``ffi.mx_unpack_multi`` call
    on the ORACLE's packed bytes, and per item (fmt, shape, axis, elements, scales, y, channels_last, the oracle's values)."""
    items, book = [], []
    for x, fmt, axis, shift_e, shift_y, cl in picks:
        if isinstance(x, tuple): pe, ps, shape = x                                       # bytes no pack produces
        else: shape = x.shape
        if int(np.prod(shape)) == 0:
            e = s = torch.empty(0, dtype=torch.uint8, device=DEV)
            y, want = torch.empty(shape, dtype=torch.float32, device=DEV), np.zeros(shape, np.float32)
        else:
            if not isinstance(x, tuple): pe, ps = P.pack(x, fmt, axis)
            e, s = ins.take(pe.size, shift_e), ins.take(ps.size)
            e.copy_(torch.from_numpy(pe.ravel())); s.copy_(torch.from_numpy(ps.ravel()))
            y, want = outs.floats(shape, shift_y, cl), P.unpack(pe, ps, fmt, shape, axis)
        items.append((e, s, y, MXFormat[fmt], axis))
        book.append((fmt, tuple(shape), axis, e, s, y, cl, want))
    return items, book


def test_unpack_multi_on_a_mixed_table():
    """ppqhip_mx_unpack_multi (mx_unpack_kernel<kMxMaxJobs, 1>) on a table of every body and every format, with an empty job in
    the middle: rows4, rows1 (a 33-element row; a float side 4 bytes off), strided, the strided body with `elements` not 16-B
    aligned (byte loads), a channels-last output, special blocks (NaN, Inf, signed zeros; NaN blocks under scale 0xFF) and every
    E5M2 code under scales 127 and 0xFF.  Every
    output equals the oracle's unpacking of the same bytes and the single-job entry point, on bits, NaN patterns included; no
    byte outside the outputs changes, and the inputs are not written."""
    foreign = P.foreign_codes('MXFP8_E5M2')
    picks = [(R.layout_input((3, 64), 31), 'MXFP8_E4M3', -1, 0, 0, False),                              # rows4
             (R.layout_input((2, 33), 32), 'MXFP6_E3M2', -1, 0, 0, False),                              # rows1
             (R.layout_input((4, 35, 3, 3), 33), 'MXFP4_E2M1', 1, 0, 0, False),                         # strided
             (np.zeros((0, 32), np.float32), 'MXINT8', -1, 0, 0, False),                                # empty
             (R.layout_input(R.CHANNELS_LAST_SHAPE, 34), 'MXINT8', 1, 0, 0, True),                      # channels-last: rows4 of [N H W, C]
             (R.layout_input((70, 9), 35), 'MXFP6_E2M3', 0, 4, 0, False),                               # strided, byte loads
             (R.special_blocks('MXFP8_E5M2'), 'MXFP8_E5M2', -1, 0, 0, False),
             (R.special_blocks('MXFP4_E2M1'), 'MXFP4_E2M1', -1, 0, 0, False),
             (R.layout_input((3, 64), 36), 'MXFP6_E3M2', -1, 0, 4, False),                              # rows1: y is not 16-B aligned
             (np.ascontiguousarray(R.special_blocks('MXFP6_E2M3').T), 'MXFP6_E2M3', 0, 0, 0, False),    # strided NaN blocks
             (foreign + ((2, 32 * foreign[1].shape[-1]),), 'MXFP8_E5M2', -1, 0, 0, False)]              # every code: Inf, NaN, scale 0xFF
    assert {p[1] for p in picks} == set(FORMATS)
    ins, outs = _Arena(1 << 18), _Arena(1 << 19)
    items, book = _unpack_table(picks, ins, outs)
    assert items[5][0].data_ptr() % 16 == 4 and items[8][2].data_ptr() % 16 == 4 and items[0][2].data_ptr() % 16 == 0
    assert not items[4][2].is_contiguous() and ffi._mx_geometry(items[4][2], 1)[:3] == (32, 64, 1)
    before = ins.buf.clone()
    ffi.mx_unpack_multi(items)
    torch.cuda.synchronize()
    nan_blocks = 0
    for k, (fmt, shape, axis, e, s, y, cl, want) in enumerate(book):
        if not len(want.ravel()): continue
        assert_bits(y.cpu().numpy(), want, f'job {k} {fmt} {shape}')
        assert_bits(_unpack_alone(e, s, fmt, shape, axis, cl), want, f'job {k} {fmt} {shape} alone')
        nan_blocks += int((s.cpu().numpy() == 0xff).sum())
    assert nan_blocks > 0 and np.isnan(book[6][7]).any() and np.isinf(book[10][7]).any()
    assert outs.untouched() and torch.equal(ins.buf, before)


@pytest.mark.parametrize('jobs', [41, 43])
def test_unpack_multi_of_more_jobs_than_one_launch_carries(jobs):
    """kMxMaxJobs = 40: job 41 rides in a second launch with a table of its own (43: a table of three jobs on three paths,
    first_block restarted).  Small tensors of every format on the three paths."""
    shapes = [((1, 32), -1), ((2, 33), -1), ((4, 35, 3, 3), 1)]
    picks = [(R.layout_input(shapes[k % 3][0], 200 + k), FORMATS[(k // 3) % 6], shapes[k % 3][1], 0, 0, False) for k in range(jobs)]
    assert len({(p[0].shape, p[1]) for p in picks}) == 18 and picks[40][1] != picks[0][1]
    ins, outs = _Arena(1 << 18), _Arena(1 << 19)
    items, book = _unpack_table(picks, ins, outs)
    ffi.mx_unpack_multi(items)
    torch.cuda.synchronize()
    for k, (fmt, shape, axis, e, s, y, cl, want) in enumerate(book): assert_bits(y.cpu().numpy(), want, f'job {k} {fmt} {shape}')
    assert outs.untouched()


def test_pack_plan_then_unpack_multi_is_fake_quant():
    """MXPackPlan(...).run() followed by ONE mx_unpack_multi call: every tensor is mx_fake_quant of its input, except at the NaN
    positions (same_but_nan)."""
    xs = [(R.layout_input((3, 64), 41), 'MXFP8_E4M3', -1), (R.layout_input((2, 33), 42), 'MXINT8', -1),
          (R.layout_input((4, 35, 3, 3), 43), 'MXFP6_E3M2', 1), (R.layout_input((70, 9), 44), 'MXFP4_E2M1', 0)]
    xs += [(R.special_blocks(fmt), fmt, -1) for fmt in FORMATS]
    xs += [(R.gaussian_blocks(), 'MXFP6_E2M3', -1), (R.gaussian_blocks(), 'MXFP8_E5M2', -1)]
    assert {fmt for _, fmt, _ in xs} == set(FORMATS)
    tensors = [dev(x) for x, _, _ in xs]
    packed = ffi.MXPackPlan([(t, MXFormat[fmt], axis) for t, (_, fmt, axis) in zip(tensors, xs)]).run()
    outs = _Arena(4 * sum(x.size for x, _, _ in xs) + 64 * len(xs) + 256)
    ys = [outs.floats(x.shape) for x, _, _ in xs]
    ffi.mx_unpack_multi([(e, s, y, MXFormat[fmt], axis) for (e, s), y, (_, fmt, axis) in zip(packed, ys, xs)])
    torch.cuda.synchronize()
    nans = 0
    for (x, fmt, axis), t, y in zip(xs, tensors, ys):
        mask = P.nan_mask(x, fmt, axis)
        nans += int(mask.sum())
        assert P.same_but_nan(y.cpu().numpy(), mx_fake_quant(t, fmt, axis).cpu().numpy(), mask, fmt), (fmt, x.shape)
    assert nans > 0 and outs.untouched()


# ---------------------------------------------------------------------------------------------------------------------------- graph
def _launches(fn):
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    try: result = fn()
    finally:
        torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 40)()
    n = _lib.lib.ppqhip_prof_collect(arr, 40)
    return result, {arr[i].name.decode(): arr[i].launches for i in range(n)}


@pytest.mark.parametrize('kind', ['mlp', 'cnn'])
def test_export_graph(kind):
    graph = harness.transformer_mlp_graph(seed=0) if kind == 'mlp' else harness.small_cnn_graph(seed=0)
    ex = harness.TorchExecutor(graph, DEV)
    delegators = quantize_graph_mx(graph, ex, 'MXFP4_E2M1', 'MXFP8_E4M3')
    weights = {}
    for op in graph.operations.values():
        for v, c in zip(op.inputs, op.config.input_quantization_config):
            if v.is_parameter and c in delegators: weights[v.name] = (v, delegators[c])
    assert len(weights) == (2 if kind == 'mlp' else 3)
    exported, launches = _launches(lambda: export_graph_mx(graph, delegators))
    assert launches.get('mx_pack', 0) == 1 and launches.get('mx_fq', 0) == 0, launches   # all weights, one launch
    assert set(exported) == set(weights)
    total = 0
    for name, (v, d) in weights.items():
        t = exported[name]
        assert isinstance(t, MXTensor) and t.format is MXFormat.MXFP4_E2M1 and t.shape == tuple(v.value.shape) and t.axis == d.axis % v.value.dim()
        assert torch.equal(mx_dequantize(t).view(torch.int32), d(v.value, None).view(torch.int32)), name
        total += (v.value.numel() // v.value.shape[t.axis]) * ((v.value.shape[t.axis] + 31) // 32) * (16 + 1)
    assert sum(t.nbytes for t in exported.values()) == total
    for other in (export_graph_mx(graph), export_graph_mx(graph, delegators, use_kernels=False)):        # formats from the configs; torch arm
        assert set(other) == set(exported)
        for name, t in other.items():
            assert (t.format, t.shape, t.axis) == (exported[name].format, exported[name].shape, exported[name].axis)
            assert torch.equal(t.elements, exported[name].elements) and torch.equal(t.scales, exported[name].scales)


# ------------------------------------------------------------------------------------------------------------------------- 2^30 + 64
def test_offsets_past_4_gib():
    """2^30 + 64 elements in MXFP4: the byte offsets of the last input rows do not fit 32 bits (the addressing is mx.hip's size_t
    arithmetic, so one rows case is enough).  Only the ends are compared."""
    shape = ((1 << 24) + 1, 64)
    x = torch.zeros(shape, device=DEV)
    head, tail = R.layout_input((3, 64), 1), R.layout_input((3, 64), 2)
    x[:3], x[-3:] = dev(head), dev(tail)
    e, s = CUDA.MXPack(x, 'MXFP4_E2M1', -1)
    del x
    assert list(e.shape) == [shape[0], 32] and list(s.shape) == [shape[0], 2]
    for part_e, part_s, want in ((e[:3], s[:3], head), (e[-3:], s[-3:], tail)):
        assert_same((part_e.cpu().numpy(), part_s.cpu().numpy()), P.pack(want, 'MXFP4_E2M1'), 'ends')
    assert not e[3:-3].any() and not s[3:-3].any()                                       # zero blocks: scale code 0, +0 elements
