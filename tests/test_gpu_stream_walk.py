"""The seams of the calibration statistics' shared walks (csrc/stream_walk.hpp): min/max, histogram and the quantile filters
at the sizes where a workgroup's share, the rows per trip (K), the register-tile form or the job changes.  Everything is exact
and compared with torch (min, max, sort) or the CPU oracle -- never with another entry point of the library.

The instantiations named in the docstrings are those a full MI355X (256 CUs) launches, read off the host dispatch of
reduce.hip / hist.hip / quantile_hot.hip; on a partitioned device other K are launched and the results are the same.
"""
import numpy as np
import pytest
import torch

from oracle import ppq_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
MM_ROW = 1024        # elements per row of minmax_small_kernel (256 lanes x float4)
H_ROW = 2048         # .. of hist_small_kernel and quantile_hot_filter_kernel (512 lanes x float4)
RESTS = (0, 1, 3)    # + ROW - 1: elements behind the last full row
BINS = 2048


@pytest.fixture(scope='module')
def CUDA():
    from ppq_amd import CUDA as C
    return C


@pytest.fixture(scope='module')
def base():
    """One read-only tensor every test slices: a smooth body with a heavy zero (the hot bin)."""
    g = torch.Generator(device=DEV).manual_seed(2051)
    x = torch.randn(2051 * H_ROW + H_ROW + 8, device=DEV, generator=g)
    x[::3] = torch.relu(x[::3])
    return x


def _spots(n, r, row):
    """an index in the first row, in the last full row and in the ragged rest (those that exist)"""
    s = [min(5, n - 1)]
    if r >= 2: s.append((r - 1) * row + row // 2)
    if n > r * row: s.append(n - 1)
    return s


def _planted(x, spots, turn, lo, hi):
    """a copy of x with lo at one spot and hi at the next one, rotated by `turn`"""
    y = x.clone()
    y[spots[turn % len(spots)]] = lo
    if len(spots) > 1: y[spots[(turn + 1) % len(spots)]] = hi
    return y


def _fold_slots(slots):
    return [slots[:, 0].min().item(), slots[:, 1].max().item()]


def _sort_want(x, q):
    """index rule of the reference (sort.cu:13-19) on a device sort"""
    n = x.numel()
    srt = torch.sort(x.flatten())[0]
    qf = np.float32(q)
    k_hi = min(max(int(np.rint(np.float32(n) * qf)), 0), n - 1)
    k_lo = min(max(int(np.rint(np.float32(n) * (np.float32(1) - qf))), 0), n - 1)
    return torch.stack([srt[k_hi], srt[k_lo]])


# ------------------------------------------------------------------------------------------------------------- row walk
@pytest.mark.parametrize('r', [0, 1, 3, 4095, 4096, 4101])
def test_minmax_row_walk_seams(CUDA, base, r):
    """MinMax_T_Slots on n = r * 1024 + d, d in {0, 1, 3, 1023}.  Up to 4 Mi elements the grid is ceil(rows / 2) <= 2048, so a share
    is at most two rows: minmax_small_kernel<2> is the only latency-bound form a full device launches (K = 4 and 8 need fewer CUs).
    r = 0: no full row, the rest alone; 1: one workgroup, a share of one row (half a trip); 3: shares of 2 and 1; 4095: 2048
    workgroups, the last share one row; 4096, d = 0: the limit itself, every share a whole trip.  Beyond it
    minmax_small_kernel<2, true, false>, grid rows / 8: r = 4096 (d > 0) shares of 8 rows = 4 trips, r = 4101 shares of 8 and 9 rows
    (an odd share: the last trip consumes one row of two).  (The streaming-load form <2, true, true> starts at 48 Mi elements:
    test_minmax_t_slots_mid_and_large_single_tensors.)  The extremes sit in the first row, the last full row and the rest in turn;
    two launches accumulate into the same slots."""
    for d in RESTS + (MM_ROW - 1,):
        n = r * MM_ROW + d
        if n == 0: continue
        x = base[:n]
        spots = _spots(n, r, MM_ROW)
        for turn in range(len(spots)):
            y = _planted(x, spots, turn, -77.5, 91.25)
            slots = torch.tensor([float('inf'), float('-inf')], device=DEV).repeat(CUDA.minmax_slots(), 1).contiguous()
            CUDA.MinMax_T_Slots(y, slots)
            assert _fold_slots(slots) == [y.min().item(), y.max().item()], (n, turn)
            z = x * 0.5
            CUDA.MinMax_T_Slots(z, slots)
            assert _fold_slots(slots) == [min(y.min().item(), z.min().item()), max(y.max().item(), z.max().item())], (n, turn, 'second launch')


@pytest.mark.parametrize('r', [0, 1, 3, 5, 1024, 1500, 2047, 2048, 2051])
def test_hist_row_walk_seams(CUDA, base, r):
    """Histogram_T_Rows (clipped), one-shot Histogram_T (clamped) and Histogram_Asymmetric_T (both) on n = r * 2048 + d, d in {0, 1, 3, 2047},
    against the oracle, outliers planted in the first row, the last full row and the rest.  hist_small_kernel<.., K> by r:
        own rows (grid ceil(rows / 2) <= 512)     r = 0 rest only; 1, 3, 1024: K = 2 (shares of 1 / 2 and 1 / 2 rows);
                                                  1500: K = 4, shares of 3 and 2; 2047: K = 4, shares of 4 and 3; 2048, d = 0: all 4
        one-shot (grid rows / 4 <= 112)           r = 1: K = 2; 3: K = 4 (3 rows); 5: K = 8 (5 rows); 1024: K = 8, shares of 9 and 10
                                                  rows = two trips; 1500 / 2047 / 2048: shares of 13-14 / 18-19 rows = two or three trips
        beyond 4 Mi elements (r = 2048 with d > 0, 2051)   <.., 2, true, false>, grid rows / 4 = 512, shares of 4 and 5 rows; own rows,
                                                  or eight partial rows and their reduce launch for the one-shot calls
    Each call runs twice: += semantics (and the partial rows must come back zeroed)."""
    hs = 3.5 / BINS
    lo, hi = -3.0, 3.25
    for d in RESTS + (H_ROW - 1,):
        n = r * H_ROW + d
        if n == 0: continue
        spots = _spots(n, r, H_ROW)
        y = _planted(base[:n], spots, r + d, -1.0e4, 2.0e4)
        if len(spots) > 2: y[spots[0]] = 3.4999                               # the last bin
        t = y.cpu().numpy()
        rows = torch.zeros(CUDA.hist_rows(), BINS, dtype=torch.int32, device=DEV)
        CUDA.Histogram_T_Rows(y, rows, hs, True); CUDA.Histogram_T_Rows(y, rows, hs, True)
        want = O.hist_sym_t(t, hs, np.zeros(BINS, np.int32), True)
        assert np.array_equal(rows.sum(dim=0, dtype=torch.int32).cpu().numpy(), 2 * want), ('rows', n)
        hist = torch.zeros(BINS, dtype=torch.int32, device=DEV)
        CUDA.Histogram_T(y, hist, hs, False); CUDA.Histogram_T(y, hist, hs, False)
        want = O.hist_sym_t(t, hs, np.zeros(BINS, np.int32), False)
        assert np.array_equal(hist.cpu().numpy(), 2 * want), ('one-shot', n)
        for clip in (True, False):
            hist = torch.zeros(BINS, dtype=torch.int32, device=DEV)
            CUDA.Histogram_Asymmetric_T(lo, hi, y, hist, clip); CUDA.Histogram_Asymmetric_T(lo, hi, y, hist, clip)
            want = O.hist_asym_t(t, lo, hi, np.zeros(BINS, np.int32), clip)
            assert np.array_equal(hist.cpu().numpy(), 2 * want), ('asym one-shot', n, clip)


@pytest.mark.parametrize('r', [128, 129, 1024, 1500, 2047, 2048, 2051])
def test_quantile_hot_filter_row_walk_seams(CUDA, base, r):
    """The hinted quantile of ONE tensor from its second call on (quantile_hot_filter_kernel; the first call on a hint takes the
    general sequence and leaves the thresholds) on n = r * 2048 + d, d in {0, 1, 3, 2047}, against a device sort.  The two-launch
    path starts at 2^18 elements (r = 128); grid ceil(rows / 2) <= 512: r = 128, 129, 1024: <2, false, false> (shares of 2 and 1
    rows); 1500, 2047, 2048 (d = 0): <4, false, false> (shares of 3 / 2, 4 / 3, 4 rows); K = 8 needs fewer CUs.  Beyond 4 Mi
    elements <2, true, false>, grid rows / 4: shares of 4 and 5 rows.  q = 0.9999 and q = 1 (the extremes themselves), which sit in
    the first row, the last full row and the rest in turn."""
    from ppq_amd.ffi import quantile_hint
    for d in RESTS + (H_ROW - 1,):
        n = r * H_ROW + d
        x = base[:n]
        spots = _spots(n, r, H_ROW)
        for q in (0.9999, 1.0):
            hint = quantile_hint(torch.device(DEV))
            assert torch.equal(CUDA.Quantile_Hinted(x, q, hint), _sort_want(x, q)), (n, q, 'first call')
            for turn in range(len(spots)):
                y = _planted(x, spots, turn, -77.5, 91.25)
                got, want = CUDA.Quantile_Hinted(y, q, hint), _sort_want(y, q)
                assert torch.equal(got, want), (n, q, turn, got.tolist(), want.tolist(), hint.cpu().tolist())
            if q == 0.9999: assert int(hint.cpu()[7]) >= 1, (n, hint.cpu().tolist())      # settled from the hint: the filter ran


# ------------------------------------------------------------------------------------------------------------ tile walk
def _job_mix(tile, extra=()):
    """289 = 3 x 96 + 1 jobs, so that min/max and the histograms launch four times and the LAST launch is one job of one tile:
    tiny jobs of 1 .. 9 elements (a tile each: a workgroup's share of two to four tiles crosses that many jobs), every tenth one
    a job of exactly one tile, one tile - 1 / + 1, two tiles + 1 or five tiles; odd jobs are views with an offset of one float."""
    special = [tile, tile - 1, tile + 1, 2 * tile + 1, 5 * tile] + list(extra)
    sizes = [special[(i // 10) % len(special)] if i % 10 == 4 else 1 + i % 9 for i in range(288)] + [7]
    return sizes


def _views(base, sizes):
    out, at = [], 0
    for i, n in enumerate(sizes):
        at = (at + 3) // 4 * 4                                               # 16-B aligned ..
        out.append(base[at + (i % 2): at + (i % 2) + n])                     # .. or one float behind
        at += n + 1
    return out


def test_tile_walk_job_mix_minmax_and_histograms(CUDA, base):
    """MinMax_T_Slots_Multi, Histogram_T_Rows_Multi and Histogram_Asymmetric_T_Rows_Multi over the job mix above (two rounds:
    accumulation), each job against torch min / max and the oracle.  Launches of 96, 96, 96 and 1 jobs: the job search, jobs that
    end inside a workgroup's share, full tiles next to the masked tail, and a grid of one workgroup."""
    S, R, bins = CUDA.minmax_slots(), CUDA.hist_rows(), 256
    xs = _views(base, _job_mix(2 * 256 * 4))                                 # min/max: tiles of 2048 elements
    slots = [torch.tensor([float('inf'), float('-inf')], device=DEV).repeat(S, 1).contiguous() for _ in xs]
    CUDA.MinMax_T_Slots_Multi(xs, slots)
    CUDA.MinMax_T_Slots_Multi([x * 2 for x in xs], slots)
    for i, (x, s) in enumerate(zip(xs, slots)):
        assert _fold_slots(s) == [min(x.min().item(), 2 * x.min().item()), max(x.max().item(), 2 * x.max().item())], ('minmax', i, x.numel())
    xs = _views(base, _job_mix(2 * 512 * 4))                                 # histograms: tiles of 4096 elements
    scales = [2.5 / bins] * len(xs)
    los, his = [-2.0 - 0.01 * (i % 7) for i in range(len(xs))], [2.75] * len(xs)
    for asym in (False, True):
        rows = [torch.zeros(R, bins, dtype=torch.int32, device=DEV) for _ in xs]
        for _ in range(2):
            if asym: CUDA.Histogram_Asymmetric_T_Rows_Multi(los, his, xs, rows)
            else: CUDA.Histogram_T_Rows_Multi(xs, rows, scales)
        for i, (x, rw) in enumerate(zip(xs, rows)):
            want = np.zeros(bins, np.int32)
            for _ in range(2):
                if asym: O.hist_asym_t(x.cpu().numpy(), los[i], his[i], want, True)
                else: O.hist_sym_t(x.cpu().numpy(), scales[i], want, True)
            assert np.array_equal(rw.sum(dim=0, dtype=torch.int32).cpu().numpy(), want), (asym, i, x.numel())


def test_tile_walk_job_mix_quantile_filter(CUDA, base):
    """Quantile_Multi over the job mix (tiles of 4096 elements) plus three jobs that lift the sequence over 2^18 elements -- below
    that the filter is not launched at all, so a quantile launch of a single tile does not exist.  Every job has a hint and the
    call runs twice: in the first the filter leaves the tiny jobs at once (nothing to filter by), streams the sampled ones; in the
    second most jobs run from their hints, the unaligned ones through the masked path.  Each job against a device sort."""
    from ppq_amd.ffi import quantile_hint
    xs = _views(base, _job_mix(4096, extra=(70_001, 300_000, 150_003)))
    assert sum(x.numel() for x in xs) >= 1 << 18
    hints = [quantile_hint(torch.device(DEV)) for _ in xs]
    for rnd in range(2):
        outs = CUDA.Quantile_Multi(xs, 0.999, None, hints)
        for i, (x, o) in enumerate(zip(xs, outs)):
            assert torch.equal(o, _sort_want(x, 0.999)), (rnd, i, x.numel(), o.tolist())
    assert sum(int(h.cpu()[7]) for h in hints) >= 1                          # some job of the second round was settled from its hint


@pytest.mark.parametrize('n', [300 * 4096 + 5, 600 * 4096 + 5, 12288 * 4096 + 5])
def test_unaligned_single_tensor_takes_the_one_job_tile_walk(CUDA, base, n):
    """A single tensor that is not 16-B aligned (a view one float behind) has no row walk: it is ONE job of the persistent kernels,
    every tile through the masked 4-B path.  hist.hip, launch_hist_one / persistent_grid: 301 tiles -> 301 / 2 = 150 > 128 ->
    301 / 4 = 75 workgroups, one-shot flush with device atomics (FLUSH_ATOMIC); 601 tiles -> 150 workgroups > 128: rows stored to
    scratch + the reduce launch (FLUSH_ROWS_STORE).  Own rows: FLUSH_ROWS_ADD in both.  Min/max: 601 / 1201 tiles of 2048 elements,
    grid tiles / 2.  The third size is 48 Mi + 5 elements: the streaming-load instantiations minmax_persistent_kernel<true> and
    hist_persistent_kernel<.., true, true> (grid 512, FLUSH_ROWS_STORE), which no multi-tensor test is large enough to launch; there
    an aligned view also takes hist_small_kernel<true, false, 2, true, true>, the one form of the row walk nothing else reaches.
    All four (asymmetric, clip) rules, so that every hist_persistent_kernel instantiation runs."""
    if n + 1 <= base.numel(): src = base
    else:
        src = torch.randn(n + 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(48))
        src[::3] = torch.relu(src[::3])
    x = src[1:n + 1]
    assert x.data_ptr() % 16 == 4
    slots = torch.tensor([float('inf'), float('-inf')], device=DEV).repeat(CUDA.minmax_slots(), 1).contiguous()
    CUDA.MinMax_T_Slots(x, slots)
    assert _fold_slots(slots) == [x.min().item(), x.max().item()]
    hs, lo, hi = 3.5 / BINS, -3.0, 3.25
    t = x.cpu().numpy()
    for asym in (False, True):
        for clip in (True, False):
            if asym: want = O.hist_asym_t(t, lo, hi, np.zeros(BINS, np.int32), clip)
            else: want = O.hist_sym_t(t, hs, np.zeros(BINS, np.int32), clip)
            hist = torch.zeros(BINS, dtype=torch.int32, device=DEV)
            for _ in range(2):
                if asym: CUDA.Histogram_Asymmetric_T(lo, hi, x, hist, clip)
                else: CUDA.Histogram_T(x, hist, hs, clip)
            assert np.array_equal(hist.cpu().numpy(), 2 * want), ('one-shot', asym, clip)
            if not asym and clip:
                rows = torch.zeros(CUDA.hist_rows(), BINS, dtype=torch.int32, device=DEV)
                CUDA.Histogram_T_Rows(x, rows, hs, True); CUDA.Histogram_T_Rows(x, rows, hs, True)
                assert np.array_equal(rows.sum(dim=0, dtype=torch.int32).cpu().numpy(), 2 * want), 'rows'
    if src is not base:
        y = src[:n]                                                           # 16-B aligned: the row walk with streaming loads
        hist = torch.zeros(BINS, dtype=torch.int32, device=DEV)
        CUDA.Histogram_Asymmetric_T(lo, hi, y, hist, False)
        assert np.array_equal(hist.cpu().numpy(), O.hist_asym_t(y.cpu().numpy(), lo, hi, np.zeros(BINS, np.int32), False)), 'aligned, asym clamped'
