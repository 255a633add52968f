"""Host checks of tests/hist_c_reference.py, which tests/test_gpu_hist_channel.py compares the per-channel histogram kernels
with: the numpy reference equals the project's C oracle on every small case; the case table reaches every launch path of
hist_c_impl on a 256-CU device for every rule form and clip mode; the planted data carry what they are named for."""
import functools

import numpy as np
import pytest

import hist_c_reference as R
from oracle import ppq_oracle as O

HOST_CASES = [c for c in R.CASES if c.size in ('small', 'limit')]


@functools.lru_cache(maxsize=None)
def _planted(name):
    c = R.CASE[name]
    return R.planted(c.shape, c.axis)


def _bins_of(case):
    return R.BINS if case.size == 'small' else R.LIMIT_BINS


# ---------------------------------------------------------------------------------------------- reference against the oracle
@pytest.mark.parametrize('clip', [True, False], ids=['clip', 'clamp'])
@pytest.mark.parametrize('case', HOST_CASES, ids=lambda c: c.name)
def test_reference_equals_the_c_oracle(case, clip):
    p = _planted(case.name)
    C = case.shape[case.axis]
    xs = R.channel_slices(p.x, case.axis)
    for bins in _bins_of(case):
        hs, scales, mins, maxs = R.scales_of(p, bins)
        want = O.hist_sym_c(p.x, case.axis, float(hs), np.zeros((C, bins), np.int32), clip)
        assert np.array_equal(R.reference(p, 'shared', clip, bins), want), ('shared', bins)
        got_s, got_a = R.reference(p, 'scales', clip, bins), R.reference(p, 'ranges', clip, bins)
        for c in range(C):
            sl = np.ascontiguousarray(xs[c])
            want = O.hist_sym_t(sl, float(scales[c]), np.zeros(bins, np.int32), clip)
            assert np.array_equal(got_s[c], want), ('scales', bins, c)
            want = O.hist_asym_t(sl, float(mins[c]), float(maxs[c]), np.zeros(bins, np.int32), clip)
            assert np.array_equal(got_a[c], want), ('ranges', bins, c)


def test_reference_equals_the_c_oracle_on_special_values_and_degenerate_scales():
    """Every special value against every degenerate rule, element by element (one-element histograms)."""
    rng = np.random.default_rng(5)
    vals = np.concatenate([R.SPECIALS, -R.SPECIALS[5:], rng.standard_normal(64).astype(np.float32) * 3,
                           np.array([1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 1e-38], np.float32)])
    for clip in (True, False):
        for bins in (1, 50, 128, 16385):
            for hs in (0.0, np.inf, 1e-45, 3e38, 1.0 / 3.0, 2.0 ** -100):
                want = O.hist_sym_t(vals, float(hs), np.zeros(bins, np.int32), clip)
                assert np.array_equal(R.count(R.raw_bins(vals, hs), bins, clip, False), want), (clip, bins, hs)
            for lo, hi in ((0.0, 0.0), (1.5, 1.5), (-np.inf, np.inf), (0.0, np.inf), (-3e38, 3e38), (2.0, -2.0), (-1.0, 1.0)):
                want = O.hist_asym_t(vals, float(lo), float(hi), np.zeros(bins, np.int32), clip)
                got = R.count(R.raw_bins(vals, R.asym_scale(lo, hi, bins), np.float32(lo)), bins, clip, True)
                assert np.array_equal(got, want), (clip, bins, lo, hi)


def test_saturating_conversion():
    f = np.array([np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 2147483520.0, -2147483520.0, -0.0, 7.0, -3.0], np.float32)
    assert R.sat_i32(f).tolist() == [0, R.INT_MAX, R.INT_MIN, R.INT_MAX, R.INT_MIN, 2147483520, -2147483520, 0, 7, -3]


# ------------------------------------------------------------------------------------------------------------ table coverage
def _reached(pred, exact_runs=None):
    """The (form, clip) pairs of the table's runs whose launch path (256 CUs) satisfies ``pred``."""
    hit = set()
    for case, form, clip, bins in R.runs():
        if pred(R.expected_path(case.shape, case.axis, bins, aligned=case.offset % 4 == 0, num_cu=256)):
            hit.add((form, clip))
    return hit


EVERY = {(f, clip) for f in R.FORMS for clip in (True, False)}

PATHS = {
    'float4 rest only': lambda p: p.kernel == 'float4' and not p.tiles and p.rest,
    'float4 tiles + rest, one split': lambda p: p.kernel == 'float4' and p.tiles and p.rest and p.splits == 1,
    'float4 split boundary inside a row': lambda p: p.kernel == 'float4' and p.splits > 1 and p.inside_row,
    'float4 plain flush': lambda p: p.kernel == 'float4' and p.flush == 'rows_add',
    'float4 atomic flush': lambda p: p.kernel == 'float4' and p.flush == 'atomic',
    'float4 8 copies': lambda p: p.kernel == 'float4' and p.copies == 8,
    'float4 1 copy': lambda p: p.kernel == 'float4' and p.copies == 1,
    'scalar epc % 4, one split': lambda p: p.kernel == 'scalar' and p.entry == 'epc%4' and p.splits == 1,
    'scalar epc % 4, splits': lambda p: p.kernel == 'scalar' and p.entry == 'epc%4' and p.splits > 1 and p.inside_row,
    'scalar epc < 64, one split': lambda p: p.kernel == 'scalar' and p.entry == 'epc<64' and p.splits == 1,
    'scalar epc < 64, splits': lambda p: p.kernel == 'scalar' and p.entry == 'epc<64' and p.splits > 1,
    'scalar unaligned, one split': lambda p: p.kernel == 'scalar' and p.entry == 'unaligned' and p.splits == 1,
    'scalar unaligned, splits': lambda p: p.kernel == 'scalar' and p.entry == 'unaligned' and p.splits > 1,
    'scalar one partial trip': lambda p: p.kernel == 'scalar' and not p.tiles and p.rest,
    'global short rows': lambda p: p.kernel == 'global' and p.entry == 'short',
    'global bins > 16384': lambda p: p.kernel == 'global' and p.entry == 'bins',
}


@pytest.mark.parametrize('path', sorted(PATHS))
def test_table_reaches_every_path_with_every_rule_form_and_clip_mode(path):
    assert _reached(PATHS[path]) == EVERY, path


def test_table_reaches_the_largest_lds_histogram_and_the_nontemporal_loads():
    hit = set()
    for case, form, clip, bins in R.runs():
        p = R.expected_path(case.shape, case.axis, bins, aligned=case.offset % 4 == 0)
        if p.kernel == 'float4' and bins == 16384: hit.add((form, clip))
    assert hit == EVERY
    # the 48 Mi element case runs two of the six combinations only: it is the one case that costs seconds
    assert _reached(lambda p: p.kernel == 'float4' and p.nt) == {('shared', True), ('ranges', False)}
    nt = [c for c in R.CASES if int(np.prod(c.shape)) >= R.K_NT_ELEMS]
    assert [c.shape for c in nt] == [(3, 256, 65536)] and int(np.prod(nt[0].shape)) == 48 << 20


def test_table_paths_are_the_ones_the_cases_are_named_for():
    def path(name, bins=128):
        c = R.CASE[name]
        return R.expected_path(c.shape, c.axis, bins, aligned=c.offset % 4 == 0)
    p = path('f4_rest_one_wave');          assert (p.kernel, p.splits, p.tiles, p.rest, p.flush) == ('float4', 1, False, True, 'atomic')
    p = path('f4_tile_rest');              assert (p.kernel, p.splits, p.tiles, p.rest, p.flush) == ('float4', 1, True, True, 'atomic')
    p = path('f4_splits_inside_rows');     assert (p.kernel, p.splits, p.tiles, p.rest, p.inside_row) == ('float4', 3, True, True, True)
    p = path('f4_rows_add_c_eq_cu');       assert (p.kernel, p.splits, p.flush, p.nt) == ('float4', 1, 'rows_add', False)
    p = path('f4_rows_add_c_gt_cu');       assert (p.kernel, p.splits, p.flush, p.nt) == ('float4', 1, 'rows_add', False)
    p = path('f4_nontemporal');            assert (p.kernel, p.splits, p.flush, p.nt) == ('float4', 1, 'rows_add', True)
    p = path('scalar_epc_mod4');           assert (p.kernel, p.entry, p.splits, p.tiles, p.flush) == ('scalar', 'epc%4', 1, False, 'rows_add')
    p = path('scalar_epc_mod4_splits');    assert (p.kernel, p.entry, p.splits, p.inside_row, p.flush) == ('scalar', 'epc%4', 2, True, 'atomic')
    p = path('scalar_epc_lt64');           assert (p.kernel, p.entry, p.splits) == ('scalar', 'epc<64', 1)
    p = path('scalar_epc_lt64_splits');    assert (p.kernel, p.entry, p.splits) == ('scalar', 'epc<64', 2)
    p = path('scalar_unaligned_splits');   assert (p.kernel, p.entry, p.splits, p.inside_row) == ('scalar', 'unaligned', 3, True)
    p = path('scalar_unaligned');          assert (p.kernel, p.entry, p.splits) == ('scalar', 'unaligned', 1)
    p = path('scalar_last_axis');          assert (p.kernel, p.entry, p.splits) == ('scalar', 'epc%4', 1)
    for name in ('global_short', 'global_first_axis', 'global_last_axis'):
        assert path(name).kernel == 'global', name
    assert path('limit_bins', 16384)[:3] == ('float4', None, 2) and path('limit_bins', 16384).copies == 1
    assert path('limit_bins', 16385)[:2] == ('global', 'bins')
    # a partitioned device takes other paths for the same cases: fewer CUs, fewer splits
    assert R.expected_path((2, 5, 6160), 1, 128, num_cu=8).splits == 2 and R.expected_path((2, 5, 6160), 1, 128, num_cu=4).splits == 1


# ------------------------------------------------------------------------------------------------------------- non-vacuity
ROOMY = [c for c in HOST_CASES if int(np.prod(c.shape)) // c.shape[c.axis] >= 40]      # every role fits into a channel


@pytest.mark.parametrize('case', ROOMY, ids=lambda c: c.name)
def test_planted_data_carry_what_they_are_named_for(case):
    p = _planted(case.name)
    r = p.roles
    xs = R.channel_slices(p.x, case.axis)
    per = xs.shape[1]
    for bins in _bins_of(case):
        hs, scales, mins, maxs = R.scales_of(p, bins)
        # hot bins: ReLU channels under both rules, the saturated channel under clamp
        for c in r.relu:
            if c in (r.specials, r.saturated): continue
            assert R.count(R.raw_bins(xs[c], hs), bins, True, False).max() >= per // 4, ('relu shared', c, bins)
            if c != r.unbounded:
                assert R.count(R.raw_bins(xs[c], scales[c]), bins, True, False).max() >= per // 4, ('relu scales', c, bins)
            h = R.count(R.raw_bins(xs[c], R.asym_scale(mins[c], maxs[c], bins), mins[c]), bins, True, True)
            assert h.max() >= per // 4, ('relu ranges', c, bins)
            if c % 2 and bins >= 2048: assert 0 < int(h.argmax()) < bins - 1, ('interior hot bin', c, bins)
        c = r.saturated
        b = R.raw_bins(xs[c], R.asym_scale(mins[c], maxs[c], bins), mins[c])
        assert (b < 0).sum() >= per // 4 and (b > bins - 1).sum() >= per // 4, ('saturated ranges', bins)
        h = R.count(b, bins, False, True)
        assert h[0] >= per // 4 and h[-1] >= per // 4
        assert R.count(b, bins, True, True).sum() <= per - 2 * (per // 4)                      # under clip they vanish
        if c != r.unbounded:
            assert (R.raw_bins(xs[c], scales[c]) > bins - 1).sum() >= per // 2, ('saturated scales', bins)
        # the dead channel: degenerate rules, everything in bin 0
        c = r.dead
        assert scales[c] == 0 and mins[c] == 0 and maxs[c] == 0 and not xs[c].any()
        for clip in (True, False):
            assert R.count(R.raw_bins(xs[c], scales[c]), bins, clip, False)[0] == per
            assert R.count(R.raw_bins(xs[c], R.asym_scale(0, 0, bins), 0), bins, clip, True)[0] == per
        # the unbounded channel
        assert np.isinf(scales[r.unbounded]) and R.count(R.raw_bins(xs[r.unbounded], np.inf), bins, True, False)[0] == per
        # the specials: present, NaN counted in bin 0 by every rule
        c = r.specials
        nan = np.isnan(xs[c])
        assert nan.sum() >= 1 and np.isposinf(xs[c]).any() and np.isneginf(xs[c]).any()
        for h_, lo_ in ((hs, None), (scales[c], None), (R.asym_scale(mins[c], maxs[c], bins), mins[c])):
            assert (R.raw_bins(xs[c], h_, lo_)[nan] == 0).all()
            with_nan = R.count(R.raw_bins(xs[c], h_, lo_), bins, True, lo_ is not None)
            without = R.count(R.raw_bins(xs[c][~nan], h_, lo_), bins, True, lo_ is not None)
            assert with_nan[0] - without[0] == nan.sum() and np.array_equal(with_nan[1:], without[1:])
        if per >= 512:                                                      # every edge of every rule fits
            assert np.signbit(xs[c][xs[c] == 0]).any() and (xs[c] == np.float32(1e-45)).any() and (xs[c] == np.float32(3e38)).any()
            ha = R.asym_scale(mins[c], maxs[c], bins)
            for edge in (np.float32(bins // 2) * hs, -(np.float32(bins // 2) * scales[c]), mins[c] + np.float32(bins // 2) * ha):
                for v in (edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))):
                    assert (xs[c] == np.float32(v)).any(), ('edge', bins, v)


def test_planted_is_seeded_and_roles_do_not_collide():
    a, b = R.planted((2, 5, 6160), 1), R.planted((2, 5, 6160), 1)
    assert np.array_equal(a.x.view(np.uint32), b.x.view(np.uint32))
    for C in (3, 4, 5, 6, 7, 256, 600):
        r = R.roles(C)
        assert len({r.dead, r.specials, r.saturated}) == 3 and r.unbounded not in (r.dead, r.specials)
        assert r.relu == tuple(range(0, C, 3))
