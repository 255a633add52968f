"""Host checks of tests/to_int_reference.py, which tests/test_gpu_to_int.py compares the integer export kernels with: the numpy
reference equals the oracle and the reference's recorded outputs; its named values are the integers written out here; the
constants of its launch mirror are the ones in the sources; the case tables reach every launch path of to_int_impl and
leave out exactly one branch that no call can reach."""
import os
import re
import sys

import numpy as np
import pytest

import to_int_reference as R
from oracle import ppq_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ppq_amd', 'csrc')


# ---------------------------------------------------------------------------------------------- reference against the oracle
def _golden_cases(golden_dir):
    if golden_dir not in sys.path: sys.path.insert(0, golden_dir)
    from to_int_cases import to_int_cases, to_int_inputs
    return to_int_cases(), to_int_inputs


def test_reference_equals_the_oracle_and_the_recorded_outputs_on_every_golden_case(golden_dir):
    cases, inputs = _golden_cases(golden_dir)
    z = np.load(os.path.join(golden_dir, 'to_int.npz'))
    assert len(cases) == len(z.files)
    for key, shape, axis, sym, bits, qmin, qmax, r in cases:
        x, s, o = (t.numpy() for t in inputs(key, shape, axis))
        dt = z[key].dtype.name
        got = R.reference(x, s, o, qmin, qmax, r, axis, dt)
        assert got.dtype == z[key].dtype and np.array_equal(got, z[key]), key
        assert np.array_equal(got, O.to_int(x, s, o, qmin, qmax, r, axis, z[key].dtype)), key


@pytest.mark.parametrize('dtype', R.DTYPES)
@pytest.mark.parametrize('rounding', R.POLICIES)
def test_reference_equals_the_oracle_on_the_value_classes(rounding, dtype):
    """Per tensor with every scale, the degenerate ones included, and per channel with all ten at once, on both clip ranges of
    the container -- the int32 clip [-2^31, 2^31 - 1] among them, where the oracle used to wrap."""
    vec = R.value_vector()
    x = R.value_classes(R.SCALES + R.DEGENERATE_SCALES)
    C = x.shape[1]
    scales = np.array(R.SCALES + R.DEGENERATE_SCALES, np.float32)
    for qmin, qmax in R.CLIPS[dtype]:
        offs = R.channel_rules(C, qmin, qmax)
        for c in range(C):
            got = R.reference(vec, scales[c:c + 1], offs[c:c + 1], qmin, qmax, rounding, None, dtype)
            assert np.array_equal(got, O.to_int(vec, scales[c:c + 1], offs[c:c + 1], qmin, qmax, rounding, None, R.NP_DTYPE[dtype])), (qmin, c)
        got = R.reference(x, scales, offs, qmin, qmax, rounding, 1, dtype)
        assert np.array_equal(got, O.to_int(x, scales, offs, qmin, qmax, rounding, 1, R.NP_DTYPE[dtype])), qmin
        for tail in R.special_tails():
            got = R.reference(tail, scales[:1], offs[:1], qmin, qmax, rounding, None, dtype)
            assert np.array_equal(got, O.to_int(tail, scales[:1], offs[:1], qmin, qmax, rounding, None, R.NP_DTYPE[dtype]))


def test_oracle_saturates_at_the_int32_clip():
    """float(2^31 - 1) is 2^31: the clamp leaves 2147483648.0f and the cast decides.  Saturating, as the kernel's
    v_cvt_i32_f32 and the reference's CUDA device do; the int64 detour of the earlier oracle wrapped these to -2^31."""
    x = np.array([1e12, 3e9, np.inf, -1e12, -3e9, -np.inf, 2147483520.0, -2147483520.0, np.nan], np.float32)
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    want = [R.INT_MAX] * 3 + [R.INT_MIN] * 3 + [2147483520, -2147483520, 0]
    assert O.to_int(x, one, zero, R.INT_MIN, R.INT_MAX, 0, None, np.int32).tolist() == want
    assert R.reference(x, one, zero, R.INT_MIN, R.INT_MAX, 0, None, 'int32').tolist() == want
    # a 1-byte container keeps the low byte of the saturated int32; NaN is 0 even where the clip range excludes 0
    assert R.reference(x, one, zero, 16, 235, 0, None, 'uint8').tolist() == [235] * 3 + [16] * 3 + [235, 16, 0]
    assert O.to_int(x, one, zero, 16, 235, 0, None, np.uint8).tolist() == [235] * 3 + [16] * 3 + [235, 16, 0]
    assert R.sat_i32(np.array([-0.0, 7.9, -3.9, 2.0 ** 31, -2.0 ** 31], np.float32)).tolist() == [0, 7, -3, R.INT_MAX, R.INT_MIN]
    assert R.narrow(np.array([255, 256, -1, -129, 128], np.int64), 'int8').tolist() == [-1, 0, -1, 127, -128]
    assert R.narrow(np.array([255, 256, -1, -129, 128], np.int64), 'uint8').tolist() == [255, 0, 255, 127, 128]


# ------------------------------------------------------------------------------------------------------------ the named values
NAMED_WANT = {0: [0, 0, 0, 0, 2, -2, 2, -2],
              1: [1, 0, 1, 0, 2, -1, 3, -2],
              2: [0, -1, 0, -1, 1, -2, 2, -3],
              3: [0, 0, 0, 0, 1, -1, 2, -2],
              4: [1, -1, 1, -1, 2, -2, 3, -3],
              6: [1, 0, 1, 0, 2, -1, 3, -2]}


@pytest.mark.parametrize('rounding', R.POLICIES)
def test_named_values_round_by_the_float32_formulas(rounding):
    """[v, -v, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5] with v = nextafter(0.5f, 0), scale 1, offset 0.  ROUND_HALF_UP of v is 1: the
    float32 sum v + 0.5f rounds to 1.0.  _round2int of the fake-quant kernels adds .5 in double and gets 0 -- the two rule sets
    are NOT interchangeable."""
    assert R.NAMED[0] == np.float32(0.5) - np.float32(2.0 ** -25) and R.NAMED[0] < 0.5
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    for dt in ('int8', 'int32'):
        assert R.reference(R.NAMED, one, zero, -128, 127, rounding, None, dt).tolist() == NAMED_WANT[rounding]
    assert O.to_int(R.NAMED, one, zero, -128, 127, rounding, None, np.int8).tolist() == NAMED_WANT[rounding]
    if rounding == 1:
        assert O.round2int(float(R.NAMED[0]), 1) == 0 and NAMED_WANT[1][0] == 1


def test_offset_is_raw_truncation_is_towards_zero_and_a_zero_scale_clamps():
    one = np.ones(1, np.float32)
    for r in R.POLICIES:
        # -5 + 0.25 = -4.75 -> -4, 5 + 0.25 = 5.25 -> 5; the rounded offset (0) would give [-5, 5]
        assert R.reference(np.array([-5, 5], np.float32), one, np.array([0.25], np.float32), -128, 127, r, None, 'int8').tolist() == [-4, 5]
        # 0 / 0 is NaN -> 0 (not clamped), 1 / 0 = inf -> 127, -1 / 0 = -inf -> -128
        got = R.reference(np.array([0, 1, -1], np.float32), np.zeros(1, np.float32), np.array([3], np.float32), -128, 127, r, None, 'int8')
        assert got.tolist() == [0, 127, -128]
    # ROUND_UP of a positive denormal is 1 (+ o): a flushed denormal would give o
    got = R.reference(np.array([R.DENORM_MIN, -R.DENORM_MIN], np.float32), one, np.array([7], np.float32), -128, 127, 6, None, 'int8')
    assert got.tolist() == [8, 7]


# ------------------------------------------------------------------------------------------------- constants of the sources
def _constant(path, pattern):
    with open(os.path.join(CSRC, path)) as f: m = re.findall(pattern, f.read())
    assert len(m) == 1, (path, pattern, m)
    return m[0]


def test_launch_constants_are_the_ones_in_the_sources():
    """A retune of kBlock or kStreamElems must fail here instead of silently moving the table's cases off their paths."""
    assert int(_constant('common.hpp', r'constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;')) == R.K_BLOCK
    a, b = _constant('fq_walk.hpp', r'constexpr\s+int64_t\s+kStreamElems\s*=\s*(\d+)ll\s*<<\s*(\d+)\s*;')
    assert int(a) << int(b) == R.K_STREAM_ELEMS
    vec_kernel = _constant('linear.hip', r'(?s)void to_int8_vec_kernel\(.*?\n}\n')
    assert re.findall(r'constexpr int U = (\d+);', vec_kernel) == [str(R.K_SLOTS)]
    assert R.VEC_TILE == 1024 and R.GENERAL_TILE == 1024


# ------------------------------------------------------------------------------------------------------------ table coverage
def _hit(pred):
    return [(p, n) for p, n in R.all_launches() if pred(p, n)]


ONE_BYTE = ('int8', 'uint8')


def test_tables_reach_every_instantiation_of_the_coalesced_kernel():
    got = {(p.out, p.channel, p.nt) for p, n in _hit(lambda p, n: p.kernel == 'vec')}
    assert got == {(o, ch, nt) for o in ONE_BYTE for ch in (False, True) for nt in (False, True)}
    # the nontemporal ones come from the stream runs alone: nothing else is that large
    small = [R.launches(int(np.prod(c.shape)), c.x_off, 0, c.dtype, c.axis, c.shape) for c in R.CASES]
    assert not any(p.kernel == 'vec' and p.nt for ls in small for p, n in ls)
    assert max(int(np.prod(c.shape)) for c in R.CASES) <= 16384 and max(int(np.prod(r.shape)) for r in R.RAW_RUNS) <= 16384
    t = R.path_of(R.STREAM_T_N, 0, 0, 'int8', None, (R.STREAM_T_N,))
    assert t == R.Vec('vec', 'int8', False, True, True) and R.STREAM_T_N % 4 == 3
    n = int(np.prod(R.STREAM_C_SHAPE, dtype=np.int64))
    assert n == 50_331_672 and n >= R.K_STREAM_ELEMS
    assert R.path_of(n, 0, 0, 'uint8', R.STREAM_C_AXIS, R.STREAM_C_SHAPE) == R.Vec('vec', 'uint8', True, True, False)


def test_table_sits_on_every_slot_and_workgroup_edge_of_the_coalesced_kernel():
    for dt in ONE_BYTE:
        for nvec in (1, R.K_BLOCK - 1, R.K_BLOCK, R.K_BLOCK + 1, R.VEC_TILE - 1, R.VEC_TILE, R.VEC_TILE + 1, 3598):
            for tail in (0, 1, 2, 3):
                c = R.CASE[f't_{dt}_n{4 * nvec + tail}']
                ls = R.launches(4 * nvec + tail, c.x_off, 0, dt, None, c.shape)
                assert ls[0] == (R.Vec('vec', dt, False, False, tail != 0), 4 * nvec)
                # the rest re-enters the dispatcher and takes the general kernel's scalar body
                assert ls[1:] == ([(R.General('general', dt, False, 1), tail)] if tail else [])
                if tail: assert R.general_branches(ls[1][0], tail) == {'scalar'}
    assert (3598 + R.VEC_TILE - 1) // R.VEC_TILE == 4                       # four workgroups, the last one partial in slot 2
    # per channel: one channel per float4; channels that change inside and across slots; C == 1; outer == 1
    for dt in ONE_BYTE:
        for shape, axis in R.VEC_C_SHAPES:
            n = int(np.prod(shape))
            assert R.path_of(n, 0, 0, dt, axis, shape) == R.Vec('vec', dt, True, False, False), shape
    epcs = [R.geometry(s, a) for s, a in R.VEC_C_SHAPES]
    assert (5, 4) in epcs and (1, 16) in epcs and (7, 1028) in epcs and 1028 // 4 == R.K_BLOCK + 1


def test_tables_reach_every_use_of_the_general_kernel():
    general = _hit(lambda p, n: p.kernel == 'general')
    reached = {(p.out, p.channel, p.vec_ok, b) for p, n in general for b in R.general_branches(p, n)}
    want = set()
    for ch in (False, True):
        want |= {('int32', ch, 1, 'float4'), ('int32', ch, 0, 'scalar')}
        want |= {(o, ch, 0, 'scalar') for o in ONE_BYTE}
    want |= {('int32', False, 1, 'scalar')} | {(o, False, 1, 'scalar') for o in ONE_BYTE}      # n % 4 elements at the end; n < 4
    assert reached == want, reached ^ want
    # ... and WHY vec_ok is 0, for all three containers per tensor and per channel: the input pointer, the output pointer, the geometry
    for dt in R.DTYPES:
        for off in (1, 2, 3):
            for name in (f't_{dt}_n{R.POINTER_T_SIZE}_xoff{off}', f'c_{dt}_2x7x1028_axis1_xoff{off}'):
                c = R.CASE[name]
                assert R.path_of(int(np.prod(c.shape)), off, 0, dt, c.axis, c.shape) == R.General('general', dt, c.axis is not None, 0), name
                assert R.path_of(int(np.prod(c.shape)), 0, 0, dt, c.axis, c.shape).kernel == ('general' if dt == 'int32' else 'vec')
        assert sorted(R.geometry(s, a)[1] for s, a in R.GEOMETRY_SHAPES) == [1, 2, 3, 5, 27]
        for shape, axis in R.GEOMETRY_SHAPES:
            assert R.path_of(int(np.prod(shape)), 0, 0, dt, axis, shape) == R.General('general', dt, True, 0), shape
        for off in R.RAW_OUT_OFFSETS[dt][1:]:
            raws = [r for r in R.RAW_RUNS if r.dtype == dt and r.out_off == off]
            assert {r.axis is not None for r in raws} == {False, True}
            for r in raws:
                assert R.path_of(int(np.prod(r.shape)), 0, off, dt, r.axis, r.shape) == R.General('general', dt, r.axis is not None, 0)
    # the short 1-byte tensors and the int32 edges
    for dt in ONE_BYTE:
        for n in (1, 2, 3):
            assert R.path_of(n, 0, 0, dt, None, (n,)) == R.General('general', dt, False, 1)
    assert sorted(int(np.prod(c.shape)) for c in R.CASES if c.dtype == 'int32' and c.axis is None and c.x_off == 0) == [1, 3, 4, 5, 1023, 1024, 1025, 2051]
    for shape, axis in R.VEC_C_SHAPES:
        assert R.path_of(int(np.prod(shape)), 0, 0, 'int32', axis, shape) == R.General('general', 'int32', True, 1)


def test_exactly_one_branch_is_out_of_reach():
    """The float4 body of to_int_kernel for a 1-byte output: every call that would run it takes to_int8_vec_kernel."""
    assert R.UNREACHABLE == [('general', '1-byte', 'float4')]
    assert not _hit(lambda p, n: p.kernel == 'general' and p.out in ONE_BYTE and 'float4' in R.general_branches(p, n))
    shapes = [((n,), None) for n in (1, 2, 3, 4, 5, 7, 8, 4096, 4099, R.K_STREAM_ELEMS)] + [(s, a) for s, a in R.VEC_C_SHAPES + R.GEOMETRY_SHAPES]
    for dt in ONE_BYTE:
        for shape, axis in shapes:
            n = int(np.prod(shape, dtype=np.int64))
            for x_off in range(4):
                for out_off in range(16):
                    for p, m in R.launches(n, x_off, out_off, dt, axis, shape):
                        assert p.kernel == 'vec' or 'float4' not in R.general_branches(p, m), (dt, shape, x_off, out_off)
    # for int32 the same body IS the aligned path
    assert 'float4' in R.general_branches(R.path_of(8, 0, 0, 'int32', None, (8,)), 8)


# --------------------------------------------------------------------------------------------------------------- non-vacuity
def test_case_data_are_seeded_and_sit_on_and_next_to_the_ties():
    c = R.CASE['c_int8_2x7x1028_axis1']
    (x, s, o), (x2, s2, o2) = R.case_inputs(c), R.case_inputs(c)
    assert np.array_equal(x.view(np.uint32), x2.view(np.uint32)) and np.array_equal(s, s2) and np.array_equal(o, o2)
    assert s[0] == 1.0 and s[2] == np.float32(0.731) and len(set(s.tolist())) == 7
    assert (o != np.round(o)).any() and (o == np.round(o)).any()
    q = R.quotient32(x, np.broadcast_to(s.reshape(1, 7, 1), x.shape))
    frac = np.abs(q - np.trunc(q))
    assert (frac == 0.5).mean() > 0.05 and ((frac != 0.5) & (np.abs(frac - 0.5) < 1e-4)).mean() > 0.1
    # the policies really differ on it, and both clip edges are hit
    outs = [R.reference(x, s, o, c.qmin, c.qmax, r, c.axis, c.dtype) for r in R.POLICIES]
    assert all(not np.array_equal(outs[i], outs[j]) for i in range(6) for j in range(i))
    assert (outs[0] == c.qmin).any() and (outs[0] == c.qmax).any() and ((outs[0] > c.qmin) & (outs[0] < c.qmax)).mean() > 0.3
    c = max((k for k in R.CASES if k.dtype == 'int32' and k.axis is None and k.qmax == R.INT_MAX), key=lambda k: k.shape[0])
    assert c.shape[0] >= 1023
    x, s, o = R.case_inputs(c)
    assert (np.abs(x) > 2.0 ** 31).any() and (c.qmin, c.qmax) == (R.INT_MIN, R.INT_MAX)
    out = R.reference(x, s, o, c.qmin, c.qmax, 0, None, 'int32')
    assert (out == R.INT_MAX).any() and (out == R.INT_MIN).any()
    # both clip ranges of every container appear in the table
    for dt in R.DTYPES:
        assert {(k.qmin, k.qmax) for k in R.CASES if k.dtype == dt} == set(R.CLIPS[dt])


def test_value_classes_carry_what_they_are_named_for():
    x = R.value_classes(R.SCALES + R.DEGENERATE_SCALES)
    assert x.shape[:2] == (4, 10) and x.shape[2] % 4 == 0 and 200_000 <= x.size <= 300_000
    assert x.size // (4 * R.VEC_TILE) >= 8                                   # several workgroups
    v = R.value_vector()
    assert v.size % 4 == 3 and np.isnan(v[-1]) and v[-3] == -np.inf
    for sp in R.SPECIALS:
        for lane in range(4):                                               # every special at every position of a float4
            at = np.flatnonzero(np.isnan(v) if np.isnan(sp) else (v == sp) & (np.signbit(v) == np.signbit(sp)))
            assert (at % 4 == lane).any(), (sp, lane)
        assert any((np.isnan(t[4:]).any() if np.isnan(sp) else ((t[4:] == sp) & (np.signbit(t[4:]) == np.signbit(sp))).any())
                   for t in R.special_tails()), sp
    assert all(t.size == 7 for t in R.special_tails())
    assert not np.isnan(R.value_vector(with_nan=False)).any() and not np.isnan(R.value_classes(R.SCALES, with_nan=False)).any()
    assert R.value_classes(R.SCALES, with_nan=False).shape[2] % 4 == 0
    # ties and near-ties at both clip edges of the three 1-byte ranges, for every scale
    for c, s in enumerate(R.SCALES):
        q = R.quotient32(x[0, c], np.full(x.shape[2], s, np.float32)).astype(np.float64)
        for edge in (-128, 127, 0, 255, -8, 7):
            for t in (edge - 0.5, edge + 0.5):
                near = q[np.abs(q - t) < 1e-3 * max(1.0, abs(t))]
                assert (near < t).any() and (near > t).any(), (s, t)
                if s in (1.0, 2.0 ** -3): assert (near == t).any(), (s, t)   # s * (k / 2) / s is exact for a power of two only
    offs = R.channel_rules(10, 0, 255)
    fr = {round(float(o - np.floor(o)), 2) for o in offs}
    assert {0.0, 0.5, 0.37, 0.63} <= fr
    # the clip range that excludes 0: NaN -> 0 lands outside it
    got = R.reference(x, np.array(R.SCALES + R.DEGENERATE_SCALES, np.float32), R.channel_rules(10, 16, 235), 16, 235, 0, 1, 'uint8')
    assert (got == 0).sum() >= np.isnan(x).sum() > 0 and ((got == 0) | ((got >= 16) & (got <= 235))).all()
