"""The integer export kernels of linear.hip (to_int8_vec_kernel, to_int_kernel behind ppqhip_to_int_t / ppqhip_to_int_c) on every
launch path of to_int_impl, for the six rounding policies and the three containers: every output equals the plain numpy
reference of tests/to_int_reference.py, integer for integer -- nothing here has a tolerance.  The case tables, their seeded data
(ties and values 1 and 2 ulp off them on both sides of 0 and of both clip edges; NaN, +-inf, denormals, +-FLT_MAX; scales 0,
negative, inf and NaN; values beyond +-2^31) and the reference live there; tests/test_host_to_int.py pins the reference to the
oracle and shows which launch each case takes.  Nothing here branches on that path: the integers must hold wherever a case lands."""
import time

import numpy as np
import pytest
import torch

import to_int_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TORCH_DTYPE = {'int8': torch.int8, 'uint8': torch.uint8, 'int32': torch.int32}


@pytest.fixture(scope='module')
def CUDA():
    from ppq_amd import CUDA as C
    yield C
    _views.clear()                                                          # hand the tensors back when the module is done


# ---- helpers -------------------------------------------------------------------------------------------------------------------
_views = {}


def _dev(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _view(host: np.ndarray, off: int) -> torch.Tensor:
    """``host`` on the device as a view ``off`` floats into a larger (16-B aligned) buffer: off 1 .. 3 is a REAL misaligned view."""
    n = host.size
    buf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
    x = buf[off:off + n].view(*host.shape)
    x.copy_(torch.from_numpy(host))
    assert buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4 * off and x.is_contiguous()
    return x


def _shared_view(key, make, off):
    """A device view built once per module and never written to."""
    if (key, off) not in _views: _views[(key, off)] = _view(make(), off)
    return _views[(key, off)]


def _assert_equal(got, want: np.ndarray, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, want.dtype, g.shape, want.shape)
    if not np.array_equal(g, want):
        bad = np.flatnonzero(g.reshape(-1) != want.reshape(-1))
        i = int(bad[0])
        raise AssertionError(f'{what}: {bad.size} of {g.size} integers differ; first at flat index {i}: {g.reshape(-1)[i]} against '
                             f'{want.reshape(-1)[i]}; the last at {int(bad[-1])}')


# ---- 1. every case of the table through the Python entry point ------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_every_case_equals_the_reference(CUDA, case):
    x_host, s, o = R.case_inputs(case)
    x = _view(x_host, case.x_off)
    sd, od = _dev(s), _dev(o)
    for r in R.POLICIES:
        got = CUDA.LinearQuantize_ToInt(x, sd, od, case.qmin, case.qmax, r, case.axis, TORCH_DTYPE[case.dtype])
        assert got.shape == x.shape and got.is_contiguous()
        _assert_equal(got, R.reference(x_host, s, o, case.qmin, case.qmax, r, case.axis, case.dtype), (case.name, r))
    assert np.array_equal(x.cpu().numpy().view(np.uint32), x_host.view(np.uint32))      # the input is only read


# ---- 2. the raw entry points: the output pointer at every byte offset, guard bytes around it ------------------------------------
GUARD = 64
RAW_GROUPS = [(dt, off) for dt in R.DTYPES for off in R.RAW_OUT_OFFSETS[dt]]


def _raw(lib, x, s, o, out_ptr, run, qmin, qmax, rounding):
    n = x.numel()
    code = R.OUT_CODE[run.dtype]
    if run.axis is None:
        return lib.ppqhip_to_int_t(x.data_ptr(), s.data_ptr(), o.data_ptr(), out_ptr, n, qmin, qmax, rounding, code, None)
    C, epc = R.geometry(run.shape, run.axis)
    return lib.ppqhip_to_int_c(x.data_ptr(), s.data_ptr(), o.data_ptr(), out_ptr, n, C, epc, qmin, qmax, rounding, code, None)


@pytest.mark.parametrize('dtype,out_off', RAW_GROUPS, ids=lambda v: str(v))
def test_raw_calls_write_the_payload_and_nothing_else(dtype, out_off):
    """ppqhip_to_int_t on every per-tensor edge size and ppqhip_to_int_c on the float4-friendly shapes, writing ``out_off`` bytes
    past a 16-B aligned address inside a sentinel-filled byte buffer: the payload is the reference, the 64 bytes in front of it and
    the 64 behind it keep the sentinel.  Offset 0 takes the dword / 16-B stores, the others the element stores; the Python wrapper
    allocates its own output and can reach the first only.  Two sentinels, so that no payload byte can pass by coincidence."""
    from ppq_amd import _lib
    elem = R.ELEM_BYTES[dtype]
    runs = [r for r in R.RAW_RUNS if r.dtype == dtype and r.out_off == out_off]
    assert len(runs) == len(R.RAW_T_SIZES[dtype]) + len(R.VEC_C_SHAPES)
    for k, run in enumerate(runs):
        qmin, qmax = R.CLIPS[dtype][k % 2]
        rounding = R.POLICIES[k % len(R.POLICIES)]
        case = R.Case('raw_' + 'x'.join(map(str, run.shape)), run.shape, run.axis, dtype, 0, qmin, qmax)
        x_host, s, o = R.case_inputs(case)
        x, sd, od = _view(x_host, 0), _dev(s), _dev(o)
        want = R.reference(x_host, s, o, qmin, qmax, rounding, run.axis, dtype).reshape(-1).view(np.uint8)
        nbytes = x_host.size * elem
        assert want.size == nbytes
        for sentinel in (0xA5, 0x5A):
            buf = torch.full((GUARD + 16 + nbytes + GUARD,), sentinel, dtype=torch.uint8, device=DEV)
            assert buf.data_ptr() % 16 == 0
            first = GUARD + out_off
            st = _raw(_lib.lib, x, sd, od, buf.data_ptr() + first, run, qmin, qmax, rounding)
            assert st == 0, _lib.last_error()
            torch.cuda.synchronize()
            raw = buf.cpu().numpy()
            _assert_equal(raw[first:first + nbytes], want, (run, rounding, sentinel))
            assert (raw[:first] == sentinel).all(), (run, 'bytes in front of the output were written')
            assert (raw[first + nbytes:] == sentinel).all(), (run, 'bytes behind the output were written')


# ---- 3. the value classes ------------------------------------------------------------------------------------------------------
ALL_SCALES = np.array(R.SCALES + R.DEGENERATE_SCALES, np.float32)


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('rounding', R.POLICIES)
def test_value_classes_per_tensor(CUDA, rounding, dtype):
    """The value-class vector (2.8 * 10^5 elements and a rest of three) with each of the six scales and with the scales 0, negative,
    inf and NaN, on both clip ranges of the container, fractional and integral offsets: once as an aligned view (the coalesced kernel
    for 1-byte outputs, the float4 body of the general kernel for int32) and once one float further (the element body)."""
    host = R.value_vector()
    views = [_shared_view('vector', R.value_vector, off) for off in (0, 1)]
    tails = R.special_tails()
    for qmin, qmax in R.CLIPS[dtype]:
        offs = R.channel_rules(len(ALL_SCALES), qmin, qmax)
        for c in range(len(ALL_SCALES)):
            s, o = ALL_SCALES[c:c + 1], offs[c:c + 1]
            want = R.reference(host, s, o, qmin, qmax, rounding, None, dtype)
            for x in views:
                got = CUDA.LinearQuantize_ToInt(x, _dev(s), _dev(o), qmin, qmax, rounding, None, TORCH_DTYPE[dtype])
                _assert_equal(got, want, (float(s[0]), float(o[0]), qmin, x.data_ptr() % 16))
        # every special in the partial last float4 (scale 1)
        for t in tails:
            want = R.reference(t, ALL_SCALES[:1], offs[:1], qmin, qmax, rounding, None, dtype)
            for off in (0, 1):
                got = CUDA.LinearQuantize_ToInt(_view(t, off), _dev(ALL_SCALES[:1]), _dev(offs[:1]), qmin, qmax, rounding, None, TORCH_DTYPE[dtype])
                _assert_equal(got, want, ('tail', t[4:].tolist(), qmin, off))
    if rounding == 6 and dtype == 'int8':       # ROUND_UP of a positive denormal at scale 1 is 1 + o: a flushed denormal would give o
        x = _view(np.array([R.DENORM_MIN, -R.DENORM_MIN, R.FLT_MIN, 0.0, R.DENORM_MIN], np.float32), 0)
        got = CUDA.LinearQuantize_ToInt(x, _dev(np.ones(1, np.float32)), _dev(np.full(1, 7, np.float32)), -128, 127, 6, None, torch.int8)
        assert got.cpu().tolist() == [8, 7, 8, 7, 8]


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('rounding', R.POLICIES)
def test_value_classes_per_channel(CUDA, rounding, dtype):
    """[4, 10, epc] over axis 1: six channels with the six scales, one each with scale 0, a negative scale, inf and NaN; offsets
    +-0.5, +-0.37 and integral ones; both clip ranges of the container -- for uint8 that is [16, 235] too, which does not contain
    the 0 that NaN becomes.  Aligned (coalesced kernel / float4 body) and one float further (element body)."""
    make = lambda: R.value_classes(R.SCALES + R.DEGENERATE_SCALES)
    host = make()
    for qmin, qmax in R.CLIPS[dtype]:
        offs = R.channel_rules(len(ALL_SCALES), qmin, qmax)
        want = R.reference(host, ALL_SCALES, offs, qmin, qmax, rounding, 1, dtype)
        for off in (0, 1):
            x = _shared_view('classes', make, off)
            got = CUDA.LinearQuantize_ToInt(x, _dev(ALL_SCALES), _dev(offs), qmin, qmax, rounding, 1, TORCH_DTYPE[dtype])
            _assert_equal(got, want, (qmin, qmax, off))


# ---- 4. export agrees with simulation -------------------------------------------------------------------------------------------
RANGES = {'int8': ('int8', -128, 127), 'uint8': ('uint8', 0, 255), 'int4': ('int8', -8, 7)}


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize('layout', ['per_tensor', 'per_channel'])
@pytest.mark.parametrize('name', list(RANGES))
@pytest.mark.parametrize('rounding', [0, 6], ids=['half_even', 'up'])
def test_export_agrees_with_simulation(CUDA, rounding, name, layout):
    """(to_int(x).float() - o) * s == LinearQuantize_T / _C (x), bit for bit, for integral offsets and positive normal scales: the
    integers a user persists are the ones the simulation computed with.  On the value classes, +-inf, denormals and +-FLT_MAX
    included.  Two exclusions, both because the RULES differ there, not the kernels:
      * NaN inputs are left out of the data: to_int maps NaN to the integer 0, the fake-quant integer for NaN is clamp(0 + o),
        and those differ whenever o != 0;
      * the policies 1-4: ppq_tensor_round evaluates them in float32 (floorf(v + 0.5f) of nextafter(0.5f, 0) is 1), the
        fake-quant kernels' _round2int adds .5 in double (0).  ROUND_HALF_EVEN and ROUND_UP have one form only."""
    dtype, qmin, qmax = RANGES[name]
    mid = (qmin + qmax) // 2
    scales = np.array(R.SCALES, np.float32)
    offs = np.array([mid, mid + 3, mid - 5, qmin, qmax, mid + 17], np.float32)
    assert (offs == np.round(offs)).all() and (scales > 0).all() and (scales >= R.FLT_MIN).all()
    for off in (0, 1):
        if layout == 'per_tensor':
            x = _shared_view('vector_no_nan', lambda: R.value_vector(with_nan=False), off)
            assert not torch.isnan(x).any()
            for c in range(len(scales)):
                s, o = _dev(scales[c:c + 1]), _dev(offs[c:c + 1])
                q = CUDA.LinearQuantize_ToInt(x, s, o, qmin, qmax, rounding, None, TORCH_DTYPE[dtype])
                sim = CUDA.LinearQuantize_T(x, s, o, qmin, qmax, rounding)
                _assert_equal(_bits((q.float() - o) * s), _bits(sim), (name, float(scales[c]), float(offs[c]), off))
        else:
            x = _shared_view('classes_no_nan', lambda: R.value_classes(R.SCALES, with_nan=False), off)
            assert not torch.isnan(x).any()
            s, o = _dev(scales), _dev(offs)
            q = CUDA.LinearQuantize_ToInt(x, s, o, qmin, qmax, rounding, 1, TORCH_DTYPE[dtype])
            sim = CUDA.LinearQuantize_C(x, s, o, 1, qmin, qmax, rounding)
            _assert_equal(_bits((q.float() - o.view(1, -1, 1)) * s.view(1, -1, 1)), _bits(sim), (name, off))


# ---- 5. the nontemporal instantiations ------------------------------------------------------------------------------------------
def _device_reference(x, scale, offset, qmin, qmax, rounding, axis, dtype, chunk=8 << 20):
    """``R.reference`` restated in torch and evaluated on the device, at most ``chunk`` elements at a time: the double quotient
    rounded to float32, the float32 rounding formulas, the raw offset, the clamp, NaN -> 0, ``.to(torch.int32)`` (after the clamp
    to a 1-byte range every value is inside the int32 range), the low byte."""
    assert dtype in ('int8', 'uint8') and -2 ** 31 < qmin <= qmax < 2 ** 31
    flat = x.reshape(-1)
    n = flat.numel()
    C, epc = (1, n) if axis is None else R.geometry(x.shape, axis)
    out = torch.empty(n, dtype=torch.int32, device=x.device)
    lo, hi = torch.tensor(float(qmin), device=x.device), torch.tensor(float(qmax), device=x.device)
    one = torch.ones((), device=x.device)
    for b in range(0, n, chunk):
        e = min(b + chunk, n)
        v = flat[b:e]
        if axis is None: s, o = scale[0], offset[0]
        else:
            ch = (torch.arange(b, e, device=x.device) // epc) % C
            s, o = scale[ch], offset[ch]
        q = (v.double() / s.double()).float()
        sgn = torch.where(q > 0, one, torch.where(q < 0, -one, q))
        if rounding == 0: r = torch.round(q)
        elif rounding == 6: r = torch.ceil(q)
        elif rounding == 3: r = sgn * torch.ceil(q.abs() - 0.5)
        elif rounding == 4: r = sgn * torch.floor(q.abs() + 0.5)
        elif rounding == 2: r = torch.ceil(q - 0.5)
        else: r = torch.floor(q + 0.5)
        t = r + o
        assert t.dtype == torch.float32
        t = torch.where(t < lo, lo, t)
        t = torch.where(t > hi, hi, t)
        t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
        out[b:e] = t.to(torch.int32)
    low = (out & 0xFF).to(torch.uint8)
    return (low if dtype == 'uint8' else low.view(torch.int8)).view(x.shape)


def test_streaming_variants_on_48_mi_elements(CUDA):
    """to_int8_vec_kernel<.., NT = true>, the four instantiations that need kStreamElems = 48 Mi elements: per tensor
    n = 48 Mi + 7 (a rest of three re-enters the dispatcher), per channel (2, 3, 8 Mi + 4) over axis 1, for int8 and uint8, one
    rounding policy each.  ONE input buffer, generated on the device; the reference is ``_device_reference``, which is first
    shown to equal the numpy reference on the value classes for every policy.  The only test of this file above a few MB."""
    # the device restatement against the numpy reference
    vec_host, cls_host = R.value_vector(), R.value_classes(R.SCALES + R.DEGENERATE_SCALES)
    vec, cls = _shared_view('vector', R.value_vector, 0), _shared_view('classes', lambda: cls_host, 0)
    for dtype in ('int8', 'uint8'):
        for qmin, qmax in R.CLIPS[dtype]:
            offs = R.channel_rules(len(ALL_SCALES), qmin, qmax)
            for r in R.POLICIES:
                for c in (0, 1, 5, 6, 7, 9):
                    got = _device_reference(vec, _dev(ALL_SCALES[c:c + 1]), _dev(offs[c:c + 1]), qmin, qmax, r, None, dtype, chunk=100_003)
                    _assert_equal(got, R.reference(vec_host, ALL_SCALES[c:c + 1], offs[c:c + 1], qmin, qmax, r, None, dtype), ('restated', r, c))
                got = _device_reference(cls, _dev(ALL_SCALES), _dev(offs), qmin, qmax, r, 1, dtype, chunk=100_003)
                _assert_equal(got, R.reference(cls_host, ALL_SCALES, offs, qmin, qmax, r, 1, dtype), ('restated per channel', r))
    torch.cuda.synchronize()
    # the kernels
    t0 = time.perf_counter()
    n_c = int(np.prod(R.STREAM_C_SHAPE, dtype=np.int64))
    n_buf = max(R.STREAM_T_N, n_c)
    assert min(R.STREAM_T_N, n_c) >= R.K_STREAM_ELEMS
    g = torch.Generator(device=DEV).manual_seed(48)
    buf = torch.randn(n_buf + 8, dtype=torch.float32, device=DEV, generator=g)
    buf *= 30.0
    buf[::7] = torch.round(buf[::7]) + 0.5                                  # ties at scale 1
    buf[::11] = torch.round(buf[::11]) * 0.5 + 0.25                         # ties at scale 0.5
    policy = iter((0, 1, 4, 6))
    for dtype, shape, axis in R.STREAM_RUNS:
        n = int(np.prod(shape, dtype=np.int64))
        x = buf[:n].view(*shape)
        assert x.data_ptr() % 16 == 0 and x.is_contiguous()
        qmin, qmax = R.CLIPS[dtype][0]
        mid = (qmin + qmax + 1) // 2
        if axis is None: s, o = torch.tensor([0.5], device=DEV), torch.tensor([mid + 3.25], device=DEV)
        else: s, o = torch.tensor([1.0, 0.5, 0.731], device=DEV), torch.tensor([mid + 0.37, mid - 0.5, mid + 17.0], device=DEV)
        r = next(policy)
        got = CUDA.LinearQuantize_ToInt(x, s, o, qmin, qmax, r, axis, TORCH_DTYPE[dtype])
        want = _device_reference(x, s, o, qmin, qmax, r, axis, dtype)
        assert got.dtype == want.dtype and got.shape == want.shape
        differ = int((got != want).sum())
        assert differ == 0, (dtype, shape, r, differ, int((got != want).reshape(-1).nonzero()[0]))
        edges = [int((want == qmin).sum()), int((want == qmax).sum())]
        assert min(edges) > 1000 and max(edges) < n // 4, edges             # both clip edges, and mostly inside
        del got, want
    torch.cuda.synchronize()
    print(f'streaming variants: {time.perf_counter() - t0:.2f} s for the four 48 Mi element runs and their references')


# ---- 6. the wrapper's contract --------------------------------------------------------------------------------------------------
def test_wrapper_contract(CUDA):
    rng = np.random.default_rng(6)
    host = (rng.integers(-300, 300, (8, 12)).astype(np.float32) * np.float32(0.5))
    s12, o12 = rng.uniform(0.2, 1.0, 12).astype(np.float32), (rng.integers(-5, 5, 12) + 0.37).astype(np.float32)
    s8, o8 = s12[:8].copy(), o12[:8].copy()
    x = _view(host, 0)
    before = x.clone()
    # a transposed view gives what .contiguous() gives, in a contiguous output of the view's shape
    xt = x.t()
    assert not xt.is_contiguous() and xt.shape == (12, 8)
    for axis, s, o in ((None, s12[:1], o12[:1]), (0, s12, o12), (1, s8, o8)):
        got = CUDA.LinearQuantize_ToInt(xt, _dev(s), _dev(o), -128, 127, 0, axis, torch.int8)
        assert got.shape == xt.shape and got.is_contiguous()
        _assert_equal(got, R.reference(np.ascontiguousarray(host.T), s, o, -128, 127, 0, axis, 'int8'), ('transposed', axis))
    # a negative channel axis
    for axis, s, o in ((-1, s12, o12), (-2, s8, o8)):
        got = CUDA.LinearQuantize_ToInt(x, _dev(s), _dev(o), 0, 255, 1, axis, torch.uint8)
        _assert_equal(got, R.reference(host, s, o, 0, 255, 1, axis % 2, 'uint8'), ('negative axis', axis))
        assert torch.equal(got, CUDA.LinearQuantize_ToInt(x, _dev(s), _dev(o), 0, 255, 1, axis % 2, torch.uint8))
    # more scales than channels: the first C count; fewer: refused
    got = CUDA.LinearQuantize_ToInt(x, _dev(s12), _dev(o12), -32768, 32767, 3, 0, torch.int32)
    _assert_equal(got, R.reference(host, s8, o8, -32768, 32767, 3, 0, 'int32'), 'longer scale')
    with pytest.raises(RuntimeError): CUDA.LinearQuantize_ToInt(x, _dev(s8), _dev(o12), -128, 127, 0, 1, torch.int8)
    with pytest.raises(RuntimeError): CUDA.LinearQuantize_ToInt(x, _dev(s12), _dev(o8), -128, 127, 0, 1, torch.int8)
    # containers and policies that do not exist
    with pytest.raises(RuntimeError): CUDA.LinearQuantize_ToInt(x, _dev(s12[:1]), _dev(o12[:1]), -128, 127, 0, None, torch.int16)
    for r in (5, 7, -1):
        with pytest.raises(RuntimeError): CUDA.LinearQuantize_ToInt(x, _dev(s12[:1]), _dev(o12[:1]), -128, 127, r, None, torch.int8)
        with pytest.raises(RuntimeError): CUDA.LinearQuantize_ToInt(x, _dev(s12), _dev(o12), -128, 127, r, 1, torch.int8)
    # the library still works after the refusals, and the input was never written
    got = CUDA.LinearQuantize_ToInt(x, _dev(s12), _dev(o12), -128, 127, 6, 1, torch.int8)
    _assert_equal(got, R.reference(host, s12, o12, -128, 127, 6, 1, 'int8'), 'after the refusals')
    assert torch.equal(x.view(torch.int32), before.view(torch.int32))
