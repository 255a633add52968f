"""Plain numpy reference of the per-channel calibration histograms (hist.hip: ppqhip_hist_sym_c, ppqhip_hist_sym_c_scales,
ppqhip_hist_asym_c_ranges), the table of cases the tests run, the data generator of those cases and a mirror of the launch
decisions of hist_c_impl.  Independent of oracle/ and of the kernels: tests/test_host_hist_channel.py pins it to the C oracle
on every small case, tests/test_gpu_hist_channel.py compares the kernels with it.

The operation, per channel slice (header of hist.hip): q = |x| / hs [symmetric; hs shared or scales[c]] or
(x - mins[c]) / hs with hs = float32(maxs[c] - mins[c]) / float32(bins) [asymmetric], all in float32 with the IEEE quotient;
b = floor(q) converted saturating to int32 (NaN -> 0, >= 2^31 -> INT_MAX, <= -2^31 -> INT_MIN); b > bins - 1 (asymmetric: or
b < 0) is dropped (clip) or clamped to the last (first) bin; counts are int64.
"""
from collections import namedtuple

import numpy as np

FORMS = ('shared', 'scales', 'ranges')          # Histogram_C | Histogram_C_Scales | Histogram_Asymmetric_C_Ranges
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ------------------------------------------------------------------------------------------------------------- the reference
def sat_i32(f: np.ndarray) -> np.ndarray:
    """float32 (already integral, +-inf or NaN) -> int32, saturating, NaN -> 0.  Returned as int64 so nothing can wrap."""
    d = f.astype(np.float64)
    out = np.zeros(d.shape, np.int64)
    fin = np.isfinite(d) & (d > -2.0 ** 31) & (d < 2.0 ** 31)
    out[fin] = d[fin].astype(np.int64)
    out[d >= 2.0 ** 31] = INT_MAX
    out[d <= -2.0 ** 31] = INT_MIN
    return out


def raw_bins(xc: np.ndarray, hs, lo=None) -> np.ndarray:
    """Bin index of every element of one channel slice BEFORE clipping / clamping; ``lo`` None: the symmetric rule."""
    xc = np.ascontiguousarray(xc, dtype=np.float32).reshape(-1)
    hs = np.float32(hs)
    with np.errstate(all='ignore'):
        a = np.abs(xc) if lo is None else xc - np.float32(lo)
        q = a / hs
        assert q.dtype == np.float32
        return sat_i32(np.floor(q))


def count(b: np.ndarray, bins: int, clip: bool, asym: bool) -> np.ndarray:
    """Raw indices -> int64[bins]."""
    if clip:
        keep = b <= bins - 1
        if asym: keep &= b >= 0
        b = b[keep]
    else:
        b = np.minimum(b, bins - 1)
        if asym: b = np.maximum(b, 0)
    assert b.size == 0 or (b.min() >= 0 and b.max() <= bins - 1)
    return np.bincount(b, minlength=bins).astype(np.int64)


def channel_slices(x: np.ndarray, axis: int) -> np.ndarray:
    """[C, elements of the channel] in the tensor's own order."""
    return np.moveaxis(x, axis, 0).reshape(x.shape[axis], -1)


def asym_scale(lo, hi, bins: int) -> np.float32:
    with np.errstate(all='ignore'):
        return np.float32(np.float32(hi) - np.float32(lo)) / np.float32(bins)


def rule_of(form: str, c: int, bins: int, hs=None, scales=None, mins=None, maxs=None):
    """(hs, lo) of channel c; lo is None for the symmetric forms."""
    if form == 'shared': return np.float32(hs), None
    if form == 'scales': return np.float32(scales[c]), None
    return asym_scale(mins[c], maxs[c], bins), np.float32(mins[c])


def hist_c(x: np.ndarray, axis: int, bins: int, clip: bool, form: str, hs=None, scales=None, mins=None, maxs=None) -> np.ndarray:
    """int64 [C, bins]: the per-channel histogram of ``x`` over ``axis``."""
    assert form in FORMS
    xs = channel_slices(np.asarray(x, dtype=np.float32), axis)
    out = np.zeros((xs.shape[0], bins), np.int64)
    for c in range(xs.shape[0]):
        h, lo = rule_of(form, c, bins, hs, scales, mins, maxs)
        out[c] = count(raw_bins(xs[c], h, lo), bins, clip, form == 'ranges')
    return out


# ---------------------------------------------------------------------------------------- the launch decisions of hist_c_impl
K_TILE_VEC = 512 * 2               # kHistBlock * kHistU float4 per tile
K_HIST_BLOCK = 512
K_MAX_LDS_BINS = 16384
K_SMALL_ELEMS = 4 << 20            # kHistSmallElems
K_NT_ELEMS = 48 << 20              # kHistNtElems

Path = namedtuple('Path', 'kernel entry splits tiles rest inside_row flush nt copies')


def even_split(total: int, groups: int, g: int):
    q, rem = divmod(total, groups)
    begin = g * q + min(g, rem)
    return begin, begin + q + (1 if g < rem else 0)


def expected_path(shape, axis, bins, aligned=True, num_cu=256) -> Path:
    """What hist_c_impl launches for a contiguous tensor of ``shape`` binned over ``axis`` on a device of ``num_cu`` CUs.

    Mirrors ppq_amd/csrc/hist.hip:
      * 689        float4 kernel when epc % 4 == 0, epc >= 64, x 16-B aligned, bins <= kMaxLdsBins (line 36);
      * 692-695    splits = 1 when C >= CUs, else ceil(CUs / C), at most the full tiles of a channel (at least 1);
      * 696, 425-430  copies = clamp(kLdsBudgetInts / bins, 1, kHistBlock / 64);
      * 699        plain read-modify-write flush when splits == 1 and n > kHistSmallElems (line 460), atomic otherwise;
      * 700        nontemporal loads from kHistNtElems (line 46);
      * 299-305, 316, 335  a split owns even_split (common.hpp:88-92) of the channel's float4 range: V / kTileVec full tiles and
                   a rest when V is no multiple of the tile;
      * 706-711    scalar kernel when n / C >= 256 (and bins fit LDS): the same splits against 8 trips of kHistBlock;
      * 395        its flush: plain when splits == 1, atomic otherwise;
      * 718-720    the global-atomic kernel for everything else.
    ``entry`` names why the float4 kernel was not taken ('epc%4', 'epc<64', 'unaligned', 'bins', or for the global kernel
    'short'); ``inside_row``: some split starts strictly inside a row.  Only the coverage assertions of
    tests/test_host_hist_channel.py read this: no GPU test branches on it."""
    shape = [int(s) for s in shape]
    n = int(np.prod(shape))
    C = shape[axis]
    epc = int(np.prod(shape[axis + 1:])) if axis + 1 < len(shape) else 1
    outer = n // (C * epc)
    copies = max(1, min(2048 // bins, K_HIST_BLOCK // 64))
    want_wgs = num_cu

    def splits_for(units_per_channel):
        s = 1 if C >= want_wgs else (want_wgs + C - 1) // C
        if s > units_per_channel: s = units_per_channel if units_per_channel > 0 else 1
        return s

    def walk(row_len, s, unit):
        tiles = rest = inside = False
        for g in range(s):
            v0, v1 = even_split(outer * row_len, s, g)
            V = v1 - v0
            tiles |= V // unit > 0
            rest |= V % unit != 0
            inside |= g > 0 and v0 % row_len != 0
        return tiles, rest, inside

    if epc % 4 == 0 and epc >= 64 and aligned and bins <= K_MAX_LDS_BINS:
        vpr = epc // 4
        s = splits_for((outer * vpr) // K_TILE_VEC)
        tiles, rest, inside = walk(vpr, s, K_TILE_VEC)
        flush = 'rows_add' if (s == 1 and n > K_SMALL_ELEMS) else 'atomic'
        return Path('float4', None, s, tiles, rest, inside, flush, n >= K_NT_ELEMS, copies)
    entry = 'bins' if bins > K_MAX_LDS_BINS else 'epc%4' if epc % 4 != 0 else 'epc<64' if epc < 64 else 'unaligned'
    if n // C >= 256 and bins <= K_MAX_LDS_BINS:
        s = splits_for((outer * epc) // (K_HIST_BLOCK * 8))
        tiles, rest, inside = walk(epc, s, K_HIST_BLOCK)
        return Path('scalar', entry, s, tiles, rest, inside, 'rows_add' if s == 1 else 'atomic', False, copies)
    if entry != 'bins': entry = 'short'
    return Path('global', entry, 1, False, False, False, 'atomic', False, None)


# ------------------------------------------------------------------------------------------------------------- the case table
Case = namedtuple('Case', 'name shape axis offset size')       # offset: floats into a larger buffer (1: a misaligned view)

CASES = [
    Case('f4_rest_one_wave', (1, 3, 64), 1, 0, 'small'),
    Case('f4_tile_rest', (1, 256, 4164), 1, 0, 'small'),
    Case('f4_splits_inside_rows', (2, 5, 6160), 1, 0, 'small'),
    Case('f4_rows_add_c_eq_cu', (1, 256, 16388), 1, 0, 'large'),
    Case('f4_rows_add_c_gt_cu', (1, 600, 7000), 1, 0, 'large'),
    Case('f4_nontemporal', (3, 256, 65536), 1, 0, 'huge'),
    Case('scalar_epc_mod4', (8, 6, 7, 7), 1, 0, 'small'),
    Case('scalar_epc_mod4_splits', (3, 4, 3001), 1, 0, 'small'),
    Case('scalar_epc_lt64', (40, 3, 4, 8), 1, 0, 'small'),
    Case('scalar_epc_lt64_splits', (300, 3, 4, 8), 1, 0, 'small'),
    Case('scalar_unaligned_splits', (2, 5, 6160), 1, 1, 'small'),
    Case('scalar_unaligned', (1, 3, 256), 1, 1, 'small'),
    # 300 single-element rows per channel: n / C = 300 >= 256, so this one takes the scalar kernel, not the global one;
    # (6, 40, 4) below is the last-axis case of the global kernel
    Case('scalar_last_axis', (6, 50, 4), 2, 0, 'small'),
    Case('global_short', (5, 7, 9), 1, 0, 'small'),
    Case('global_first_axis', (4, 3), 0, 0, 'small'),
    Case('global_last_axis', (6, 40, 4), 2, 0, 'small'),
    Case('limit_bins', (2, 3, 4096), 1, 0, 'limit'),              # bins 16384 (float4, 64 KiB of LDS) and 16385 (global)
]
CASE = {c.name: c for c in CASES}

BINS = (50, 128, 2048, 4096)
LIMIT_BINS = (16384, 16385)
ALL_BINS = BINS + LIMIT_BINS
# the shapes above 4 M elements: every rule form and clip mode once, the bin counts rotating over them
LARGE_RUNS = [('shared', True, 2048), ('shared', False, 50), ('scales', True, 128), ('scales', False, 4096),
              ('ranges', True, 4096), ('ranges', False, 128)]
# the 48 Mi element shape: these two only (about a second of numpy each)
HUGE_RUNS = [('shared', True, 2048), ('ranges', False, 128)]


def runs():
    """Every (case, form, clip, bins) of test_counts_equal_the_reference."""
    out = []
    for case in CASES:
        if case.size == 'small':
            out += [(case, f, clip, b) for f in FORMS for clip in (True, False) for b in BINS]
        elif case.size == 'limit':
            out += [(case, f, clip, b) for f in FORMS for clip in (True, False) for b in LIMIT_BINS]
        else:
            out += [(case, f, clip, b) for f, clip, b in (LARGE_RUNS if case.size == 'large' else HUGE_RUNS)]
    return out


def run_id(run) -> str:
    case, form, clip, bins = run
    return f'{case.name}-{form}-{"clip" if clip else "clamp"}-{bins}'


# --------------------------------------------------------------------------------------------------------- the data generator
Roles = namedtuple('Roles', 'relu dead saturated unbounded specials')
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38], np.float32)


def roles(C: int) -> Roles:
    """Which channel plays which part.  Every third channel (0, 3, ..) is ReLU'd; 1 is dead; the last carries the planted
    specials; with few channels the saturated and the unbounded one share a ReLU channel (C == 3: both sit on channel 0)."""
    relu = tuple(range(0, C, 3))
    dead = 1 if C >= 2 else None
    specials = C - 1 if C >= 3 else None
    saturated = 2 if C >= 4 else 0
    unbounded = 4 if C >= 6 else 3 if C == 5 else 0
    return Roles(relu, dead, saturated, unbounded, specials)


Planted = namedtuple('Planted', 'x axis roles sym_range lo hi shared_range')


def scales_of(p: Planted, bins: int):
    """The rules of a planted tensor at ``bins`` bins: (shared hs, scales[C], mins[C], maxs[C]), float32.  Ranges are 0.9 x the
    channel's true range (before anything was planted); the dead channel has scale 0 and min == max == 0, the unbounded one
    scale inf."""
    with np.errstate(all='ignore'):
        hs = np.float32(p.shared_range) / np.float32(bins)
        scales = (p.sym_range / np.float32(bins)).astype(np.float32)
    r = p.roles
    if r.dead is not None: scales[r.dead] = 0.0
    scales[r.unbounded] = np.inf
    return hs, scales, p.lo.copy(), p.hi.copy()


def planted(shape, axis, seed=0) -> Planted:
    """Seeded test tensor of ``shape``: randn scaled per channel by 1 .. C.  Every third channel is ReLU'd (the odd ones of them
    then lifted by (c + 1) / 4, which makes an INTERIOR bin the hot one); one channel is saturated, one dead, one carries special
    values and bin edges (of every rule form at every bin count of ALL_BINS) +- 1 ulp.  See ``roles`` and ``scales_of``."""
    shape = tuple(int(s) for s in shape)
    C = shape[axis]
    per = int(np.prod(shape)) // C
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape, dtype=np.float32)
    xs = np.moveaxis(x, axis, 0)                                            # a view: [C, ...]
    xs *= np.arange(1, C + 1, dtype=np.float32).reshape((C,) + (1,) * (x.ndim - 1))
    r = roles(C)
    for c in r.relu:
        np.maximum(xs[c], 0, out=xs[c])
        if c % 2: xs[c] += np.float32(0.25 * (c + 1))
    if r.dead is not None: xs[r.dead] = 0.0
    lo = np.array([xs[c].min() for c in range(C)], np.float32) * np.float32(0.9)
    hi = np.array([xs[c].max() for c in range(C)], np.float32) * np.float32(0.9)
    sym_range = np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)
    p = Planted(x, axis, r, sym_range, lo, hi, np.float32(sym_range.max()))

    def put(c, positions, values):                                          # into the channel's elements in tensor order
        sl = np.ascontiguousarray(xs[c]).reshape(-1)
        sl[positions] = values
        xs[c] = sl.reshape(xs[c].shape)

    # the saturated channel: 30 % at a constant beyond maxs[c], 30 % at one below mins[c] (for the symmetric rules both lie
    # beyond the last bin)
    c = r.saturated
    pos = rng.permutation(per)
    n30 = (per * 3) // 10
    top = np.float32(1.5) * max(np.float32(1.0), sym_range[c])
    put(c, pos[:n30], top)
    put(c, pos[n30:2 * n30], -top)
    # the specials, spread evenly over the channel's elements, the first and the last one included
    c = r.specials
    if c is not None:
        vals = [SPECIALS]
        for bins in ALL_BINS:
            hs, scales, mins, maxs = scales_of(p, bins)
            ha = asym_scale(mins[c], maxs[c], bins)
            for k in (1, bins // 2, bins - 1, bins):
                kf = np.float32(k)
                for edge in (kf * hs, -(kf * scales[c]), mins[c] + kf * ha):
                    edge = np.float32(edge)
                    vals.append(np.array([edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))],
                                         np.float32))
        vals = np.concatenate(vals)[:per]
        pos = np.unique(np.linspace(0, per - 1, vals.size).astype(np.int64))
        put(c, pos, vals[:pos.size])
    return p


def reference(p: Planted, form: str, clip: bool, bins: int) -> np.ndarray:
    hs, scales, mins, maxs = scales_of(p, bins)
    return hist_c(p.x, p.axis, bins, clip, form, hs=hs, scales=scales, mins=mins, maxs=maxs)


def observer_batches(shape, count_, seed):
    """Calibration batches for the observer test: randn scaled per channel (axis 1) and per batch, every third channel ReLU'd,
    channel 1 all zero."""
    rng = np.random.default_rng(seed)
    C = shape[1]
    out = []
    for i in range(count_):
        x = rng.standard_normal(shape, dtype=np.float32)
        x *= np.arange(1, C + 1, dtype=np.float32).reshape((1, C) + (1,) * (len(shape) - 2)) * np.float32(1 + 0.25 * i)
        x[:, 0::3] = np.maximum(x[:, 0::3], 0)
        x[:, 1] = 0.0
        out.append(x)
    return out
