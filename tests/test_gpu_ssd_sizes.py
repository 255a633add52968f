"""The three SSD entry points (csrc/ssd.hip) at the sizes where their loops, their cross-wave reductions and their launch
chunking decide the result, against the NumPy oracle tests/ssd_reference.py.  The golden-driven tests (test_gpu_ssd.py) stay
below one workgroup of 256 lanes: C <= 16 channels, at most 108 elements per channel and 864 per tensor.  Here:

* ranges and scales at C = 300 -- two trips over the elements of a channel and over the channels, the extremes PLANTED in the
  second trip, in waves 2 and 3 and in the last element, so that a dropped trip or a reduction that forgets a wave changes a bit;
* apply beyond the 1024 workgroups a job gets (the grid-strided loop), float4 and scalar body, aligned and 4 bytes off;
* more jobs than one launch carries (24 / 32 / 32), and one scales + apply sequence replayed from a HIP graph.

Everything is exact: ``==`` on bits; where a NaN is expected, the NaN positions and the bits of everything else."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import ssd_cases as SC  # noqa: E402
import ssd_reference as REF  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
BLOCK, WAVE = 256, 64                      # csrc/common.hpp kBlock, the wave of gfx950
MAX_BLOCKS = 1024                          # csrc/channel_scale.hpp kScaleMaxBlocksPerJob
SENTINEL = 0x5A5A5A5A                      # as float32: 1.5e16, no value any test computes
RATIO = SC.CHANNEL_RATIO


# ---- comparisons ------------------------------------------------------------------------------------------------------
def _np(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=F)


def _same(a, b) -> bool:
    a, b = _np(a), _np(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same_or_nan(a, b) -> bool:
    """NaN exactly where ``b`` has one, the bits of ``b`` everywhere else."""
    a, b = _np(a), _np(b)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(DEV)


def _filled(n: int) -> torch.Tensor:
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


# ---- pairs ------------------------------------------------------------------------------------------------------------
def _op(kind: str, w, **attributes):
    """What ``equalization.endpoint_layout`` reads of an operation."""
    return types.SimpleNamespace(type=kind, name=kind.lower(), attributes=attributes,
                                 inputs=[None, types.SimpleNamespace(value=w, is_parameter=True, name='w')])


def _axes(first, last):
    """(first channel axis, last channel axis, groups) from the operation kinds alone: a Conv stores [out, in / G, k, k], a Gemm
    [out, in] under transB and [in, out] without."""
    (kind1, _, attr1), (kind2, _, attr2) = first, last
    return (0 if kind1 == 'Conv' or attr1['transB'] else 1), (1 if kind2 == 'Conv' or attr2['transB'] else 0), attr2.get('group', 1)


def _imbalanced(rng, shape, out_axis: int, in_axis: int) -> np.ndarray:
    """Seeded normal values times the ROWMUL / COLMUL factors of ssd_cases.py over the output and the input channels."""
    w = rng.standard_normal(shape).astype(F) * F(0.3)
    for axis, mul in ((out_axis, SC.ROWMUL), (in_axis, SC.COLMUL)):
        f = np.array([mul[i % len(mul)] for i in range(shape[axis])], dtype=F)
        w = w * f.reshape([-1 if d == axis else 1 for d in range(len(shape))])
    return np.ascontiguousarray(w, dtype=F)


def _elements(w: np.ndarray, axis: int, group: int) -> np.ndarray:
    """[C, n] flat indices into ``w``: the n elements of every channel in the order the ranges kernel walks them
    (i = outer * run + e)."""
    if axis == 0: return np.arange(w.size).reshape(w.shape[0], -1)
    if w.ndim == 2: return np.arange(w.size).reshape(w.shape).T
    G, og, ipg = group, w.shape[0] // group, w.shape[1]
    return np.arange(w.size).reshape(G, og, ipg, -1).transpose(0, 2, 1, 3).reshape(G * ipg, -1)


# name -> (first, last, channels of max(first), max(last), max(act) and the minimum of algorithm 2): four different waves of
# the scales kernel's workgroup, one of them met in its second trip over the channels
PAIRS = {
    'conv': (('Conv', (300, 33, 3, 3), {}), ('Conv', (40, 300, 3, 3), {'group': 1}), (200, 150, 70, 290)),
    'gemm': (('Gemm', (300, 300), {'transB': 0}), ('Gemm', (264, 300), {'transB': 1}), (280, 100, 170, 250)),
    'grouped': (('Conv', (300, 33, 3, 3), {}), ('Conv', (24, 150, 3, 3), {'group': 2}), (130, 75, 290, 230)),
}
ZERO_FIRST, ZERO_LAST = 5, 6               # channels whose first weight is +-0 and one subnormal / whose last weight is all -0.0


def _plants(n: int):
    """(channel, element index) pairs for the channel's largest |w|: in the second trip over the elements (index >= 256), in waves
    2 and 3 of the first trip, in the last element; a channel of fewer than 256 elements has waves 0 and 1 only."""
    if n > BLOCK: return [(20, BLOCK + (n - BLOCK) // 2), (21, 2 * WAVE + 2), (257, 3 * WAVE + 8), (22, n - 1), (299, n - 1)]
    return [(20, WAVE + 6), (21, n - 2), (257, WAVE + 1), (22, n - 1), (299, n - 1)]


@pytest.fixture(scope='module')
def wide():
    """{name: dict(first, last, act, axes, plants, ranges, scales)}: the three pairs of C = 300 with everything planted, and the
    oracle's answer.  Built once; nothing changes it."""
    out = {}
    for seed, (name, (first, last, extremes)) in enumerate(PAIRS.items()):
        rng = np.random.default_rng(900 + seed)
        ax1, ax2, group = _axes(first, last)
        w1 = _imbalanced(rng, first[1], ax1, 1 - ax1)
        w2 = _imbalanced(rng, last[1], 1 - ax2, ax2)
        act = rng.uniform(0.02, 3.0, 300).astype(F)
        act[9], act[260] = F(0.004), F(0.00999)                              # under the 0.01 floor, one in each trip over the channels
        e1, e2 = _elements(w1, ax1, 1), _elements(w2, ax2, group)
        f1, f2 = w1.reshape(-1), w2.reshape(-1)                              # views: writes go through
        plants = {0: _plants(e1.shape[1]), 1: _plants(e2.shape[1])}
        for side, (flat, elems) in enumerate(((f1, e1), (f2, e2))):
            for k, (c, i) in enumerate(plants[side]):
                flat[elems[c, i]] = F(1.5) * np.abs(flat[elems[c]]).max() * F(-1 if k % 2 else 1)
        f1[e1[ZERO_FIRST]] = 0; f1[e1[ZERO_FIRST, 1]] = F(-0.0); f1[e1[ZERO_FIRST, -2]] = F(-1e-40)      # range: a subnormal
        f2[e2[ZERO_LAST]] = F(-0.0)                                                                      # range: +0
        cA, cB, cC, cD = extremes

        def set_range(flat, elems, c, value):
            flat[elems[c]] *= F(value) / np.abs(flat[elems[c]]).max()
        M1, M2 = np.abs(f1).max() * F(1.25), np.abs(f2).max() * F(1.25)
        set_range(f1, e1, cA, M1); set_range(f2, e2, cB, M2)
        act[cC] = act.max() * F(1.25)
        set_range(f1, e1, cD, M1 * F(0.95)); set_range(f2, e2, cD, M2 * F(0.01))   # ks ~ 1.05, nks = 1 / ratio: the smallest quotient
        set_range(f2, e2, cA, M2 * F(0.8)); set_range(f2, e2, cC, M2 * F(0.8))     # ks = 1 (as = 1) over nks = 1.25
        r = REF.ranges(w1, w2, group, ax1, ax2)
        out[name] = dict(first=first, last=last, w1=w1, w2=w2, act=act, axes=(ax1, ax2, group), plants=plants, elements=(e1, e2),
                         extremes=extremes, ranges=r, scales=REF.scales(r[0], r[1], act, RATIO))
    return out


def _segments(case, w1: torch.Tensor, w2: torch.Tensor):
    from ppq_amd.equalization import endpoint_layout
    (kind1, _, attr1), (kind2, _, attr2) = case['first'], case['last']
    _, ax1, C1, seg1, _ = endpoint_layout(_op(kind1, w1, **attr1), False)
    _, ax2, C2, seg2, _ = endpoint_layout(_op(kind2, w2, **attr2), True, reference_key_order=False)
    assert (ax1, ax2) == case['axes'][:2] and C1 == C2
    return C1, (w1, *seg1), (w2, *seg2)


def _scales_call(case, w1: np.ndarray, w2: np.ndarray, act: np.ndarray):
    from ppq_amd import ffi
    C, seg1, seg2 = _segments(case, _dev(w1), _dev(w2))
    scales, ranges = _filled(4 * C).view(4, C), _filled(2 * C).view(2, C)
    ffi.ssd_scales_multi([(seg1, seg2, _dev(act), RATIO, scales, ranges)])
    return ranges.cpu().numpy(), scales.cpu().numpy()


def test_planted_values_hold_the_extremes(wide):
    """Without this the size tests are vacuous: every planted element is the one largest |w| of its channel, the four
    cross-channel extremes lie in the four channels chosen for them -- alone -- and all the clips act."""
    for name, case in wide.items():
        r, s = case['ranges'], case['scales']
        for side, w in enumerate((case['w1'], case['w2'])):
            elems = case['elements'][side]
            n = elems.shape[1]
            want = {'last element'} | ({'second trip', 'wave 2', 'wave 3'} if n > BLOCK else {'wave 1'})
            seen = set()
            for c, i in case['plants'][side]:
                a = np.abs(w.reshape(-1)[elems[c]])
                assert a.argmax() == i and (a == a[i]).sum() == 1 and r[side][c] == a[i], (name, side, c, i)
                if i >= BLOCK: seen.add('second trip')
                else: seen.add(f'wave {i // WAVE}')
                if i == n - 1: seen.add('last element')
            assert want <= seen, (name, side, seen)
        assert r[0][ZERO_FIRST] == F(1e-40) and 0 < r[0][ZERO_FIRST] < np.finfo(F).tiny                  # a subnormal range
        assert r[1][ZERO_LAST] == 0 and not np.signbit(r[1][ZERO_LAST])
        assert np.signbit(case['w1'].reshape(-1)[case['elements'][0][ZERO_FIRST, 1]])
        cA, cB, cC, cD = case['extremes']
        low = REF.algo2_before_normalisation(r[0], r[1], case['act'], RATIO)
        for what, v, c, pick in (('max first', r[0], cA, np.argmax), ('max last', r[1], cB, np.argmax),
                                 ('max act', case['act'], cC, np.argmax), ('min algo 2', low, cD, np.argmin)):
            assert pick(v) == c and (v == v[c]).sum() == 1, (name, what, int(pick(v)), c)
        lanes = [c % BLOCK // WAVE for c in case['extremes']]
        assert sorted(lanes) == [0, 1, 2, 3] and max(case['extremes']) >= BLOCK, (name, lanes)
        assert (s[0] == F(0.1)).any() and (s[0] == F(10)).any() and (s[2:] == 1).any() and (s[2:] == 2).any(), name
        assert ((s[2] > 1) & (s[2] < 2)).any() and ((s[3] > 1) & (s[3] < 2)).any() and (case['act'] < F(0.01)).any(), name
        assert not np.isnan(s).any() and not np.isnan(r).any()


@pytest.mark.parametrize('name', list(PAIRS))
def test_ranges_and_scales_at_300_channels(wide, name):
    case = wide[name]
    ranges, scales = _scales_call(case, case['w1'], case['w2'], case['act'])
    assert _same(ranges, case['ranges']), np.flatnonzero(ranges.view(np.uint32) != case['ranges'].view(np.uint32))[:8]
    for algo in range(4):
        bad = np.flatnonzero(scales[algo].view(np.uint32) != case['scales'][algo].view(np.uint32))
        assert bad.size == 0, (name, algo, bad[:8], scales[algo][bad[:4]], case['scales'][algo][bad[:4]])


@pytest.mark.parametrize('where', ['first', 'act', 'last'])
def test_one_nan_at_300_channels(wide, where):
    """A NaN in the second trip over the elements of a channel of the second trip over the channels (first weight), in the
    activation range, in the second trip of a channel of the last weight: ranges [2, C] and scales [4, C] as the oracle has them
    -- that channel's range and algorithm-0 scale, and every channel of the algorithms that read the range."""
    case = wide['conv']
    w1, w2, act = case['w1'].copy(), case['w2'].copy(), case['act'].copy()
    e1, e2 = case['elements']
    if where == 'first': w1.reshape(-1)[e1[290, 270]] = np.nan
    elif where == 'last': w2.reshape(-1)[e2[150, 300]] = np.nan
    else: act[131] = np.nan
    r = REF.ranges(w1, w2)
    s = REF.scales(r[0], r[1], act, RATIO)
    assert int(np.isnan(r).sum()) == (0 if where == 'act' else 1) and int(np.isnan(s[0]).sum()) == (0 if where == 'act' else 1)
    assert np.isnan(s[2:]).all() and np.isnan(s[1]).all() == (where != 'last') and np.isnan(s[1]).any() == (where != 'last')
    ranges, scales = _scales_call(case, w1, w2, act)
    assert _same_or_nan(ranges, r)
    for algo in range(4): assert _same_or_nan(scales[algo], s[algo]), (where, algo)


# ---- apply beyond 1024 workgroups ------------------------------------------------------------------------------------
# name -> (kind, weight shape, attributes, downstream, the run the issue of this test names, float4 body when aligned)
APPLIES = {
    'upstream_conv_run891': ('Conv', (300, 99, 3, 3), {}, False, 891, False),
    'downstream_gemm_column': ('Gemm', (600, 500), {'transB': 1}, True, 1, False),
    'upstream_gemm_run1000': ('Gemm', (1100, 1000), {'transB': 1}, False, 1000, True),
    'downstream_grouped_conv_run16': ('Conv', (448, 150, 4, 4), {'group': 2}, True, 16, True),
}


def _apply_scales(rng, C: int) -> np.ndarray:
    s = np.exp(rng.uniform(np.log(0.1), np.log(10.0), (4, C))).astype(F)
    s[0, 0], s[1, 1 % C], s[2, 2 % C], s[3, 3 % C], s[2, C - 1] = F(1), F(2), F(0.1), F(10), F(3)
    return s


def _apply_input(rng, shape) -> np.ndarray:
    x = rng.standard_normal(shape).astype(F)
    flat = x.reshape(-1)
    flat[7], flat[-1], flat[flat.size // 2] = F(-0.0), F(1e-40), F(-1.2e-38)    # -0, a subnormal, a normal whose quotient is subnormal
    flat[11], flat[-5] = F(3e38), F(-2.5e-39)                                   # a product that overflows, a subnormal whose product is normal
    return x


@pytest.fixture(scope='module')
def apply_cases():
    out = {}
    for seed, (name, (kind, shape, attrs, down, run, vec)) in enumerate(APPLIES.items()):
        rng = np.random.default_rng(950 + seed)
        axis = (1 if kind == 'Conv' or attrs['transB'] else 0) if down else (0 if kind == 'Conv' or attrs['transB'] else 1)
        group = attrs.get('group', 1)
        C = shape[axis] * (group if kind == 'Conv' and down else 1)
        x, s = _apply_input(rng, shape), _apply_scales(rng, C)
        out[name] = dict(x=x, scales=s, want=REF.apply(x, s, axis, down, group))
    return out


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', '4_bytes_off'])
@pytest.mark.parametrize('name', list(APPLIES))
def test_apply_strides_beyond_1024_workgroups(apply_cases, name, off):
    """n (or n / 4 in the float4 body) exceeds 1024 workgroups x 256 lanes: every lane takes a second trip somewhere.  All four
    candidates equal the oracle, x keeps its bits, and a sentinel border around x and around out is untouched."""
    from ppq_amd import ffi
    from ppq_amd.equalization import endpoint_layout
    kind, shape, attrs, down, run, vec = APPLIES[name]
    case = apply_cases[name]
    x_np, s_np = case['x'], case['scales']
    n, pad = x_np.size, 64
    xa, oa = _filled(n + 2 * pad), _filled(4 * n + 2 * pad)
    x = xa[pad + off: pad + off + n].view(shape)
    out = oa[pad + off: pad + off + 4 * n].view((4,) + tuple(shape))
    x.copy_(torch.from_numpy(x_np))
    assert xa.data_ptr() % 16 == 0 and oa.data_ptr() % 16 == 0 and (x.data_ptr() % 16 == 0) == (off == 0)
    _, _, C, _, (g_run, inner, og) = endpoint_layout(_op(kind, x, **attrs), down, reference_key_order=False)
    assert g_run == run and C == s_np.shape[1] and (run % 4 == 0) == vec
    work = n // 4 if vec and off == 0 else n
    assert work > MAX_BLOCKS * BLOCK, (name, work)                             # the loop strides
    before = xa.clone()
    ffi.ssd_apply_multi([(x, out, _dev(s_np), g_run, inner, og, down)])
    torch.cuda.synchronize()
    assert torch.equal(xa.view(torch.int32), before.view(torch.int32))         # x and its border
    got = out.cpu().numpy()
    for cand in range(4):
        bad = np.flatnonzero(got[cand].view(np.uint32).ravel() != case['want'][cand].view(np.uint32).ravel())
        assert bad.size == 0, (name, off, cand, bad.size, bad[:4], got[cand].ravel()[bad[:4]], case['want'][cand].ravel()[bad[:4]])
    border = torch.cat([oa[:pad + off], oa[pad + off + 4 * n:]]).view(torch.int32)
    assert bool((border == SENTINEL).all())


# ---- more jobs than one launch carries ---------------------------------------------------------------------------------
def _small_pair(rng, C: int, form: str):
    if form == 'gemm': first, last = ('Gemm', (7, C), {'transB': 0}), ('Gemm', (6, C), {'transB': 1})
    elif form == 'grouped': first, last = ('Conv', (C, 2, 3, 3), {}), ('Conv', (6, C // 2, 3, 3), {'group': 2})
    elif form == 'long': first, last = ('Conv', (C, 33, 3, 3), {}), ('Conv', (31, C, 3, 3), {'group': 1})      # two trips per channel
    else: first, last = ('Conv', (C, 2, 3, 3), {}), ('Conv', (5, C, 3, 3), {'group': 1})
    ax1, ax2, group = _axes(first, last)
    w1, w2 = _imbalanced(rng, first[1], ax1, 1 - ax1), _imbalanced(rng, last[1], 1 - ax2, ax2)
    return dict(first=first, last=last, axes=(ax1, ax2, group), w1=w1, w2=w2, act=rng.uniform(0.005, 3.0, C).astype(F))


def test_scales_of_25_pairs_in_one_call():
    """kSsdMaxJobs = 24: the 25th pair rides in a second pair of launches, with its own table and first_block restarted.  Every
    pair equals its own single-pair call and the oracle."""
    from ppq_amd import ffi
    rng = np.random.default_rng(77)
    widths = [3, 8, 16, 300, 257, 12, 40, 64, 100, 5, 271, 33, 1, 2, 129, 256, 7, 9, 513, 31, 17, 65, 128, 15, 290]
    assert len(widths) == 25 and sum(c <= 16 for c in widths) >= 5 and sum(c > 256 for c in widths) >= 5 and widths[24] > 256
    items, wants, keep = [], [], []
    for k, C in enumerate(widths):
        form = 'long' if k in (3, 24) else ('gemm' if k % 3 == 1 else ('grouped' if k % 3 == 2 and C % 2 == 0 else 'conv'))
        case = _small_pair(rng, C, form)
        _, seg1, seg2 = _segments(case, _dev(case['w1']), _dev(case['w2']))
        scales, ranges = _filled(4 * C).view(4, C), _filled(2 * C).view(2, C)
        items.append((seg1, seg2, _dev(case['act']), RATIO, scales, ranges))
        r = REF.ranges(case['w1'], case['w2'], case['axes'][2], case['axes'][0], case['axes'][1])
        wants.append((r, REF.scales(r[0], r[1], case['act'], RATIO)))
        keep.append(case)
    ffi.ssd_scales_multi(items)
    for k, (item, (r, s)) in enumerate(zip(items, wants)):
        assert _same(item[5], r) and _same(item[4], s), (k, widths[k])
        alone = (_filled(4 * widths[k]).view(4, -1), _filled(2 * widths[k]).view(2, -1))
        ffi.ssd_scales_multi([item[:4] + alone])
        assert _same(alone[0], item[4]) and _same(alone[1], item[5]), k


def test_apply_of_33_jobs_in_one_call():
    """kSsdApMaxJobs = 32: job 33 is a launch of its own.  Upstream and downstream tensors, a bias, float4 and scalar bodies."""
    from ppq_amd import ffi
    from ppq_amd.equalization import endpoint_layout
    rng = np.random.default_rng(78)
    kinds = [('Conv', lambda C: (C, 5, 3, 3), {}, False), ('bias', lambda C: (C,), {}, False), ('Gemm', lambda C: (C, 16), {'transB': 1}, False),
             ('Conv', lambda C: (8, C // 2, 2, 2), {'group': 2}, True), ('Gemm', lambda C: (9, C), {'transB': 1}, True),
             ('Gemm', lambda C: (C, 6), {'transB': 0}, True), ('Conv', lambda C: (7, C, 3, 3), {'group': 1}, True)]
    items, wants, xs = [], [], []
    for k in range(33):
        kind, shape_of, attrs, down = kinds[k % len(kinds)]
        C = 2 * (5 + 3 * k)
        shape = shape_of(C)
        x_np, s_np = _apply_input(rng, shape), _apply_scales(rng, C)
        x = _dev(x_np)
        if kind == 'bias': axis, group, geometry = 0, 1, (1, C, 0)
        else:
            axis = (1 if kind == 'Conv' or attrs['transB'] else 0) if down else (0 if kind == 'Conv' or attrs['transB'] else 1)
            group = attrs.get('group', 1)
            _, got_axis, got_C, _, geometry = endpoint_layout(_op(kind, x, **attrs), down, reference_key_order=False)
            assert got_axis == axis and got_C == C
        out = _filled(4 * x_np.size).view((4,) + tuple(shape))
        items.append((x, out, _dev(s_np), *geometry, down))
        wants.append(REF.apply(x_np, s_np, axis, down, group))
        xs.append(x_np)
    assert len(items) == 33 and any(it[3] % 4 == 0 for it in items) and any(it[3] % 4 for it in items)
    ffi.ssd_apply_multi(items)
    for k, (item, want) in enumerate(zip(items, wants)):
        assert _same(item[1], want), k
        assert _same(item[0], xs[k]), k


def _fq_then_measure(y, r, scale, offset, axis, qmin, qmax, rounding):
    from ppq_amd import ffi
    from ppq_amd.ffi import CUDA
    if axis is None: q = CUDA.LinearQuantize_T(y, scale, offset, qmin, qmax, rounding)
    else: q = CUDA.LinearQuantize_C(y, scale, offset, axis, qmin, qmax, rounding)
    return ffi.measure_rows_multi([(q, r, None)])[0]


def test_fq_measure_rows_of_33_jobs_in_one_call():
    """kFqMsMaxJobs = 32: the 33rd job takes a second FqX table, first_block restarted and a second request for scratch partials
    -- both launches hold split rows (count > 8192).  Wave-per-row, workgroup-per-row and split rows; per-tensor jobs and
    per-channel jobs whose channels are no multiple of 4 long.  Bit-identical to fake-quant-then-measure and to one call per job."""
    from ppq_amd import ffi
    gen = torch.Generator().manual_seed(79)
    shapes = [(2, 3, 55, 57), (3, 5, 7, 9), (1, 4, 70, 70), (2, 6, 25, 27)]            # split x 2, a wave per row, split x 3, a workgroup per row
    counts = [int(np.prod(s[1:])) for s in shapes]
    assert counts[0] > 8192 and counts[2] > 2 * 8192 and counts[1] <= 1024 < counts[3] <= 8192
    assert all((c // s[1]) % 4 for c, s in zip(counts[:2] + counts[3:], shapes[:2] + shapes[3:]))      # elem_per_channel % 4 != 0
    items = []
    for k in range(33):
        shape = shapes[k % 4]
        y = (torch.randn(shape, generator=gen) * 3).to(DEV)
        r = (torch.randn(shape, generator=gen) * 3).to(DEV)
        y.view(-1)[::17] = torch.round(y.view(-1)[::17] * 8) / 16                       # rounding ties under scale 1 / 16
        axis = None if (k // 4) % 2 == 0 else 1
        n = 1 if axis is None else shape[1]
        scale = torch.full((1,), 0.0625, device=DEV) if axis is None else (torch.rand(n, generator=gen) * 0.05 + 0.0625 / 4).to(DEV)
        qmin, qmax = ((-128, 127), (0, 255), (0, 15))[k % 3]
        offset = (torch.randint(0, 200, (n,), generator=gen).float() if qmin == 0 else torch.zeros(n)).to(DEV)
        if qmax == 15: offset = offset + 300.0                                          # fake_quant(0) != 0: the padded slots
        items.append((y, r, scale, offset, axis, qmin, qmax, k % 8))
    split = [k for k, it in enumerate(items) if it[0][0].numel() > 8192]
    assert any(k < 32 for k in split) and 32 in split                                    # both launches ask for partials
    assert {it[4] for it in items} == {None, 1}
    sums = [torch.full((it[0].shape[0], 4), float('nan'), dtype=torch.float64, device=DEV) for it in items]
    ffi.fq_measure_rows_multi(items, sums)
    for k, (item, got) in enumerate(zip(items, sums)):
        want = _fq_then_measure(*item)
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (k, tuple(item[0].shape), item[4])
        alone = ffi.fq_measure_rows_multi([item])[0]
        assert torch.equal(got.view(torch.int64), alone.view(torch.int64)), k


# ---- HIP graph ---------------------------------------------------------------------------------------------------------
def test_graph_replay_of_a_wide_scales_and_apply_sequence(wide):
    """The scales of the C = 300 Conv pair and the four candidates of its first weight (scalar body) and of its last weight,
    captured after one eager warm-up on the capture stream: one replay into cleared outputs repeats the eager bits."""
    from ppq_amd import ffi
    from ppq_amd.equalization import endpoint_layout
    case = wide['conv']
    w1, w2, act = _dev(case['w1']), _dev(case['w2']), _dev(case['act'])
    C, seg1, seg2 = _segments(case, w1, w2)
    scales, ranges = _filled(4 * C).view(4, C), _filled(2 * C).view(2, C)
    o1, o2 = _filled(4 * w1.numel()).view((4,) + tuple(w1.shape)), _filled(4 * w2.numel()).view((4,) + tuple(w2.shape))
    g1 = endpoint_layout(_op('Conv', w1), False)[4]
    g2 = endpoint_layout(_op('Conv', w2, group=1), True, reference_key_order=False)[4]

    def work():
        ffi.ssd_scales_multi([(seg1, seg2, act, RATIO, scales, ranges)])
        ffi.ssd_apply_multi([(w1, o1, scales, *g1, False), (w2, o2, scales, *g2, True)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side): work()
    side.synchronize()
    eager = [t.clone() for t in (ranges, scales, o1, o2)]
    assert _same(eager[0], case['ranges']) and _same(eager[1], case['scales'])
    assert _same(eager[2], REF.apply(case['w1'], case['scales'], 0)) and _same(eager[3], REF.apply(case['w2'], case['scales'], 1, True))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side): work()
    for t in (ranges, scales, o1, o2): t.view(torch.int32).fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip((ranges, scales, o1, o2), eager): assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert _same(w1, case['w1']) and _same(w2, case['w2'])
