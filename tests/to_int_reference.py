"""Plain numpy reference of the integer export kernels (linear.hip: ppqhip_to_int_t, ppqhip_to_int_c), a mirror of the launch
decisions of to_int_impl, the table of cases the tests run and the seeded data of those cases.  Independent of oracle/ and of
the kernels: tests/test_host_to_int.py pins it to the oracle and to the reference's recorded outputs, tests/test_gpu_to_int.py
compares the kernels with it, integer for integer.

The operation (PPQLinearQuant_toInt, ppq/quantization/qfunction/linear.py:218-238), element by element in float32:
    t = ppq_tensor_round(x / s) + o          the IEEE quotient, the float32 formulas of utils/round.py:27-41, the RAW offset
    t = clamp(t, float32(qmin), float32(qmax))                                  NaN passes through
    q = int32(t)                             truncated towards zero, NaN -> 0, saturated to [-2^31, 2^31 - 1]
and a 1-byte container keeps the low byte of q.  The reference leaves the cast of an out-of-range float undefined (its CUDA
device saturates, x86 gives INT_MIN); the saturating form is what the kernel's v_cvt_i32_f32 does and what this project means.
"""
import zlib
from collections import namedtuple

import numpy as np

F32 = np.float32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
POLICIES = (0, 1, 2, 3, 4, 6)                   # every policy ppq_tensor_round implements; 5 (ROUND_TO_NEAR_INT) and 7 raise
DTYPES = ('int8', 'uint8', 'int32')
NP_DTYPE = {'int8': np.int8, 'uint8': np.uint8, 'int32': np.int32}
OUT_CODE = {'int8': 0, 'uint8': 1, 'int32': 2}  # out_dtype of the C entry points
ELEM_BYTES = {'int8': 1, 'uint8': 1, 'int32': 4}


# ------------------------------------------------------------------------------------------------------------- the reference
def quotient32(x: np.ndarray, s: np.ndarray) -> np.ndarray:
    """The correctly rounded float32 quotient (53 >= 2 * 24 + 2: the double quotient rounds to it)."""
    with np.errstate(all='ignore'):
        return (x.astype(np.float64) / s.astype(np.float64)).astype(F32)


def _sign(v: np.ndarray) -> np.ndarray:
    """torch.sign as the formulas below need it: 0 -> 0 (its sign kept), NaN -> NaN."""
    return np.where(v > 0, F32(1), np.where(v < 0, F32(-1), v)).astype(F32)


def tensor_round(v: np.ndarray, rounding: int) -> np.ndarray:
    """ppq_tensor_round, utils/round.py:27-41: one float32 formula per policy (every sum below is ONE float32 addition)."""
    assert v.dtype == F32
    half = F32(0.5)
    with np.errstate(all='ignore'):
        if rounding == 0: r = np.rint(v)                                        # ROUND_HALF_EVEN: torch.round
        elif rounding == 6: r = np.ceil(v)                                      # ROUND_UP
        elif rounding == 3: r = _sign(v) * np.ceil(np.abs(v) - half)            # ROUND_HALF_TOWARDS_ZERO
        elif rounding == 4: r = _sign(v) * np.floor(np.abs(v) + half)           # ROUND_HALF_FAR_FORM_ZERO
        elif rounding == 2: r = np.ceil(v - half)                               # ROUND_HALF_DOWN
        elif rounding == 1: r = np.floor(v + half)                              # ROUND_HALF_UP
        else: raise ValueError(f'rounding policy {rounding} has no tensor form')
    assert r.dtype == F32
    return r


def sat_i32(t: np.ndarray) -> np.ndarray:
    """float32 -> int32 as int64: truncated towards zero, NaN -> 0, saturated."""
    d = np.trunc(t.astype(np.float64))
    out = np.zeros(d.shape, np.int64)
    fin = np.isfinite(d) & (d > -2.0 ** 31) & (d < 2.0 ** 31)
    out[fin] = d[fin].astype(np.int64)
    out[d >= 2.0 ** 31] = INT_MAX
    out[d <= -2.0 ** 31] = INT_MIN
    return out


def narrow(q: np.ndarray, dtype: str) -> np.ndarray:
    """int32 values (held as int64) -> the container: int32 as is, 1-byte containers keep the low byte."""
    assert q.min() >= INT_MIN and q.max() <= INT_MAX
    if dtype == 'int32': return q.astype(np.int32)
    low = (q & 0xFF).astype(np.uint8)
    return low if dtype == 'uint8' else low.view(np.int8)


def geometry(shape, axis):
    """(C, elem_per_channel) of a contiguous tensor; ``axis`` may be negative."""
    shape = [int(d) for d in shape]
    axis = axis % len(shape)
    return shape[axis], int(np.prod(shape[axis + 1:], dtype=np.int64))


def reference(x, scale, offset, qmin: int, qmax: int, rounding: int, axis, dtype: str) -> np.ndarray:
    """What ppqhip_to_int_t (``axis`` None) / ppqhip_to_int_c write for a contiguous ``x``; of ``scale`` / ``offset`` the first C
    elements (per tensor: the first one) count."""
    x = np.ascontiguousarray(x, dtype=F32)
    s, o = np.asarray(scale, F32).reshape(-1), np.asarray(offset, F32).reshape(-1)
    if axis is None:
        s, o = s[:1], o[:1]
    else:
        C, _ = geometry(x.shape, axis)
        bshape = [1] * x.ndim
        bshape[axis % x.ndim] = C
        s, o = s[:C].reshape(bshape), o[:C].reshape(bshape)
    with np.errstate(all='ignore'):
        t = tensor_round(quotient32(x, np.broadcast_to(s, x.shape)), rounding) + o
        assert t.dtype == F32
        lo, hi = F32(qmin), F32(qmax)
        t = np.where(t < lo, lo, t)                                             # torch.clamp: NaN fails both compares and stays
        t = np.where(t > hi, hi, t)
    return narrow(sat_i32(t), dtype)


# ------------------------------------------------------------------------------------------ the launch decisions of to_int_impl
K_BLOCK = 256                       # common.hpp:26        constexpr int kBlock = 256
K_SLOTS = 4                         # linear.hip:128       constexpr int U = 4 (float4 per lane of to_int8_vec_kernel)
K_STREAM_ELEMS = 48 << 20           # fq_walk.hpp:64       constexpr int64_t kStreamElems = 48ll << 20
VEC_TILE = K_BLOCK * K_SLOTS        # float4 per workgroup of to_int8_vec_kernel (linear.hip:129, 487)
GENERAL_TILE = K_BLOCK * 4          # elements per workgroup of to_int_kernel (linear.hip:91, 481)

Vec = namedtuple('Vec', 'kernel out channel nt has_tail')
General = namedtuple('General', 'kernel out channel vec_ok')


def path_of(n, x_off_floats, out_off_bytes, dtype, axis, shape):
    """The FIRST launch of to_int_impl (linear.hip:468-513) for ``n`` elements of ``shape`` read ``x_off_floats`` floats and
    written ``out_off_bytes`` bytes past a 16-B aligned address:
      * 479  vec_ok = x 16-B aligned, out aligned to four outputs (4 B or 16 B), per channel: elem_per_channel % 4 == 0;
      * 485  1-byte outputs with vec_ok and n >= 4 take to_int8_vec_kernel<OUT, CHANNEL, NT> on n / 4 float4,
      * 489  nontemporal from kStreamElems elements,
      * 500-503  and a per-tensor rest of 1-3 elements re-enters to_int_impl (``has_tail``; see ``launches``);
      * 506-510  everything else takes to_int_kernel<OUT, CHANNEL> with the vec_ok flag.
    Only the coverage assertions of tests/test_host_to_int.py read this: no GPU test branches on it."""
    channel = axis is not None
    elem = ELEM_BYTES[dtype]
    assert n == int(np.prod(shape, dtype=np.int64)) and n > 0
    epc = geometry(shape, axis)[1] if channel else n
    vec_ok = x_off_floats % 4 == 0 and out_off_bytes % (4 * elem) == 0 and (not channel or epc % 4 == 0)
    if elem == 1 and vec_ok and n >= 4:
        return Vec('vec', dtype, channel, n >= K_STREAM_ELEMS, n % 4 != 0)
    return General('general', dtype, channel, int(vec_ok))


def launches(n, x_off_floats, out_off_bytes, dtype, axis, shape):
    """Every launch as (path, elements): the first one and, for a ragged per-tensor vec launch, the general kernel on the rest
    (x + done and out + done keep their alignment: done is a multiple of 4)."""
    p = path_of(n, x_off_floats, out_off_bytes, dtype, axis, shape)
    if p.kernel == 'vec' and p.has_tail:
        assert not p.channel                                                    # n % (C * epc) == 0 and epc % 4 == 0: no rest
        return [(p, n - n % 4), (path_of(n % 4, x_off_floats, out_off_bytes, dtype, None, (n % 4,)), n % 4)]
    return [(p, n)]


def general_branches(path, n):
    """Which bodies of to_int_kernel (linear.hip:98-115) some lane of a launch over ``n`` elements runs."""
    assert path.kernel == 'general'
    out = set()
    if path.vec_ok and n >= 4: out.add('float4')
    if not path.vec_ok or n % 4: out.add('scalar')
    return out


# ------------------------------------------------------------------------------------------------------------- the case table
# x_off: floats into a 16-B aligned device buffer (1 .. 3: a misaligned view).  The output of these cases is allocated by the
# Python wrapper (always aligned); RAW_RUNS below move the output pointer.
Case = namedtuple('Case', 'name shape axis dtype x_off qmin qmax')

CLIPS = {'int8': ((-128, 127), (-8, 7)), 'uint8': ((0, 255), (16, 235)), 'int32': ((INT_MIN, INT_MAX), (-32768, 32767))}
VEC_NVEC = (1, 255, 256, 257, 1023, 1024, 1025, 3598)          # float4: the slot (256) and workgroup (1024) edges, 4 workgroups
VEC_TAIL = (0, 1, 2, 3)
VEC_T_SIZES = tuple(4 * v + t for v in VEC_NVEC for t in VEC_TAIL)
SHORT_SIZES = (1, 2, 3)
I32_T_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 2051)
# per channel with elem_per_channel % 4 == 0: epc 4 (one channel per float4, C no power of two, wraps over outer); epc 8;
# 257 float4 per channel (channels change inside and across the 256-float4 slots, 4 workgroups); C == 1; outer == 1
VEC_C_SHAPES = (((3, 5, 4), 1), ((2, 3, 8), 1), ((2, 7, 1028), 1), ((6, 1, 16), 1), ((16, 8), 0))
# elem_per_channel 1 (the last axis), 2, 3, 5, 27: a float4 would straddle channels
GEOMETRY_SHAPES = (((6, 40), 1), ((4, 5, 2), 1), ((3, 4, 3), 1), ((6, 37, 5), 1), ((2, 6, 3, 9), 1))
POINTER_T_SIZE = 4 * 1025 + 3
POINTER_C_SHAPE = ((2, 7, 1028), 1)


def _cases():
    out, k = [], 0

    def add(name, shape, axis, dtype, x_off=0):
        nonlocal k
        qmin, qmax = CLIPS[dtype][k % 2]
        k += 1
        out.append(Case(name, tuple(shape), axis, dtype, x_off, qmin, qmax))

    def sname(shape): return 'x'.join(str(d) for d in shape)

    for dt in ('int8', 'uint8'):
        for n in VEC_T_SIZES: add(f't_{dt}_n{n}', (n,), None, dt)
        for n in SHORT_SIZES: add(f't_{dt}_n{n}', (n,), None, dt)
    for n in I32_T_SIZES: add(f't_int32_n{n}', (n,), None, 'int32')
    for dt in DTYPES:
        for shape, axis in VEC_C_SHAPES: add(f'c_{dt}_{sname(shape)}_axis{axis}', shape, axis, dt)
        for shape, axis in GEOMETRY_SHAPES: add(f'c_{dt}_{sname(shape)}_axis{axis}', shape, axis, dt)
        for off in (1, 2, 3):
            add(f't_{dt}_n{POINTER_T_SIZE}_xoff{off}', (POINTER_T_SIZE,), None, dt, off)
            add(f'c_{dt}_{sname(POINTER_C_SHAPE[0])}_axis{POINTER_C_SHAPE[1]}_xoff{off}', POINTER_C_SHAPE[0], POINTER_C_SHAPE[1], dt, off)
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# the raw entry points with the OUTPUT pointer moved: (entry, dtype, out offset in bytes, shape, axis)
RAW_OUT_OFFSETS = {'int8': (0, 1, 2, 3), 'uint8': (0, 1, 2, 3), 'int32': (0, 4, 8, 12)}
RAW_T_SIZES = {'int8': VEC_T_SIZES + SHORT_SIZES, 'uint8': VEC_T_SIZES + SHORT_SIZES, 'int32': I32_T_SIZES}
RawRun = namedtuple('RawRun', 'dtype out_off shape axis')
RAW_RUNS = ([RawRun(dt, off, (n,), None) for dt in DTYPES for off in RAW_OUT_OFFSETS[dt] for n in RAW_T_SIZES[dt]]
            + [RawRun(dt, off, shape, axis) for dt in DTYPES for off in RAW_OUT_OFFSETS[dt] for shape, axis in VEC_C_SHAPES])

# the nontemporal instantiations: the only shapes above a few MB (tests/test_gpu_to_int.py: one test, one shared buffer)
STREAM_T_N = (48 << 20) + 7                                    # per tensor: NT and a rest of 3
STREAM_C_SHAPE, STREAM_C_AXIS = (2, 3, (8 << 20) + 4), 1       # per channel: 50,331,672 elements, elem_per_channel % 4 == 0
STREAM_RUNS = [(dt, (STREAM_T_N,), None) for dt in ('int8', 'uint8')] + [(dt, STREAM_C_SHAPE, STREAM_C_AXIS) for dt in ('int8', 'uint8')]

# The ONE branch of the two kernels that no call can reach: the float4 body of to_int_kernel with a 1-byte OUT (linear.hip:104-105).
# It needs vec_ok == 1 and n >= 4, and exactly those 1-byte calls take to_int8_vec_kernel instead (linear.hip:485); a per-tensor
# rest is shorter than 4.  The kernel code stays as it is; tests/test_host_to_int.py shows the branch is out of reach for every
# size, alignment and geometry, and that everything else is reached.
UNREACHABLE = [('general', '1-byte', 'float4')]


def all_launches():
    """(path, elements) of every launch of every run of the three tables."""
    out = []
    for c in CASES:
        n = int(np.prod(c.shape))
        out += launches(n, c.x_off, 0, c.dtype, c.axis, c.shape)
    for r in RAW_RUNS:
        out += launches(int(np.prod(r.shape)), 0, r.out_off, r.dtype, r.axis, r.shape)
    for dt, shape, axis in STREAM_RUNS:
        out += launches(int(np.prod(shape, dtype=np.int64)), 0, 0, dt, axis, shape)
    return out


# --------------------------------------------------------------------------------------------------------- the data generator
FRACTIONS = (0.0, 0.5, -0.5, 0.37, -0.37, 0.25)


def ulp_shift(v: np.ndarray, k: int) -> np.ndarray:
    """``v`` moved |k| float32 steps towards +inf (k > 0) or -inf (k < 0); 0 steps into the denormals."""
    v = np.asarray(v, F32).copy()
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf))
    return v


def channel_index(shape, axis) -> np.ndarray:
    """The channel of every element of a contiguous tensor of ``shape`` (all 0 for ``axis`` None)."""
    if axis is None: return np.zeros(shape, np.int64)
    idx = [1] * len(shape)
    idx[axis % len(shape)] = shape[axis]
    return np.broadcast_to(np.arange(shape[axis]).reshape(idx), shape)


def offsets_for(C: int, qmin: int, qmax: int, seed: int) -> np.ndarray:
    """Integral offsets inside the clip range (about its middle) plus the fractions of FRACTIONS, rotating over the channels."""
    rng = np.random.default_rng(seed)
    mid = (max(qmin, -40000) + min(qmax, 40000)) // 2
    o = mid + rng.integers(-20, 21, C) + np.array([FRACTIONS[(c + seed) % len(FRACTIONS)] for c in range(C)])
    return o.astype(F32)


def case_inputs(case: Case):
    """Seeded (x, scale, offset) of a case: x = s_c * (k / 2) for integers k that straddle both clip edges, two thirds of them
    moved 1 or 2 ulp off the tie; scale 1.0 on channel 0, 0.731 on channel 2, random in [0.1, 1) elsewhere; int32 cases carry
    values beyond +-2^31 as well."""
    seed = zlib.crc32(case.name.encode())
    rng = np.random.default_rng(seed)
    C = 1 if case.axis is None else case.shape[case.axis]
    scale = rng.uniform(0.1, 1.0, C).astype(F32)
    scale[0] = 1.0
    if C > 2: scale[2] = 0.731
    offset = offsets_for(C, case.qmin, case.qmax, seed % 997)
    width = min(case.qmax - case.qmin, 65536)
    k = rng.integers(-width - 80, width + 81, case.shape)
    x = (k.astype(F32) * F32(0.5)) * scale[channel_index(case.shape, case.axis)]
    assert x.dtype == F32
    step = rng.integers(-2, 3, case.shape)
    for d in (-2, -1, 1, 2):
        x = np.where((step == d) & (x != 0), ulp_shift(x, d), x)
    if case.dtype == 'int32':
        flat = x.reshape(-1)
        flat[::5] *= F32(1000.0)
        flat[::13] *= F32(1e8)
    return np.ascontiguousarray(x, dtype=F32), scale, offset


# --------------------------------------------------------------------------------------------------------- the value classes
SCALES = (1.0, 0.731, 0.1, 2.0 ** -3, 1e30, 1e-30)
DEGENERATE_SCALES = (0.0, -0.731, np.inf, np.nan)
HALF_BELOW = np.nextafter(F32(0.5), F32(0))                    # floorf(v + 0.5f) is 1, floor((double)v + .5) is 0
NAMED = np.array([HALF_BELOW, -HALF_BELOW, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5], F32)
DENORM_MIN, FLT_MIN, FLT_MAX = F32(1e-45), np.finfo(F32).tiny, np.finfo(F32).max
BELOW_2_31 = F32(2147483520.0)                                 # the largest float below 2^31
_MAGNITUDES = np.array([DENORM_MIN, FLT_MIN, FLT_MAX, np.inf, 1e12, 3e9, BELOW_2_31, 2.0 ** 31, 32767.5, 32768.5, 2.0 ** 24 + 2], F32)
SPECIALS = np.concatenate([np.array([0.0, -0.0], F32), _MAGNITUDES, -_MAGNITUDES, np.array([np.nan], F32)])
SPECIALS_NO_NAN = SPECIALS[:-1]
VALUE_OUTER = 4


def channel_values(s, with_nan=True) -> np.ndarray:
    """The values of one channel of scale ``s``: s * (k / 2) for k in -700 .. 700 at 0, +-1 and +-2 ulp (ties and near-ties of
    every policy on both sides of 0 and of both clip edges of the int8, uint8 and int4 ranges), the named values of
    ``NAMED`` (as they are and times s) and ``SPECIALS``; padded with 0.25 s to a multiple of 4.  A degenerate scale (0,
    negative, inf, NaN) gets the values of |s|, or of 1."""
    base = F32(abs(s)) if np.isfinite(s) and s != 0 else F32(1.0)
    ties = (np.arange(-700, 701).astype(F32) * F32(0.5)) * base
    parts = [ulp_shift(ties, d) for d in (0, 1, -1, 2, -2)] + [NAMED, NAMED * base, SPECIALS if with_nan else SPECIALS_NO_NAN]
    v = np.concatenate(parts).astype(F32)
    return np.concatenate([v, np.full((-v.size) % 4, F32(0.25) * base, F32)])


def value_classes(scales, with_nan=True) -> np.ndarray:
    """float32 [4, len(scales), epc], epc % 4 == 0: channel c holds ``channel_values(scales[c])`` as built and rotated by one,
    two and three, so every special meets every position of a float4.  2.8 * 10^5 elements for ten channels: 69 workgroups of
    the coalesced kernel."""
    rows = [channel_values(s, with_nan) for s in scales]
    assert len({r.size for r in rows}) == 1
    x = np.stack([np.stack([np.roll(r, k) for r in rows]) for k in range(VALUE_OUTER)])
    assert x.shape[0] == VALUE_OUTER and x.shape[2] % 4 == 0
    return np.ascontiguousarray(x, dtype=F32)


def value_vector(with_nan=True) -> np.ndarray:
    """The per-tensor form: all ten channels of ``value_classes`` flat, plus three specials as the rest behind the last float4."""
    body = value_classes(SCALES + DEGENERATE_SCALES, with_nan).reshape(-1)
    return np.concatenate([body, np.array([-np.inf, DENORM_MIN, np.nan if with_nan else FLT_MAX], F32)])


def special_tails(with_nan=True):
    """Short per-tensor vectors (one float4 and a rest of three) that put EVERY special into the partial last float4."""
    sp = SPECIALS if with_nan else SPECIALS_NO_NAN
    sp = np.concatenate([sp, sp[:(-sp.size) % 3]])
    return [np.concatenate([np.array([1.5, -2.5, 0.25, 100.0], F32), sp[i:i + 3]]) for i in range(0, sp.size, 3)]


def channel_rules(C: int, qmin: int, qmax: int):
    """Per-channel offsets of the value-class runs: the fractions +-0.5, +-0.37 and integral ones, around the middle of the clip
    range."""
    return offsets_for(C, qmin, qmax, 3)
