"""The histogram sinks of the convolution epilogues (ppqhip_bias_act_hist / ppqhip_bias_add_act_hist) and the store elision of
the residual launches (their `elide` mask, and ppqhip_bias_add_act_stats2 for the min/max sinks): what they store must equal,
bit for bit, the plain epilogue launch, and what they count / fold must equal the observers' own launch
(CUDA.Histogram_T_Rows / Histogram_Asymmetric_T_Rows, CUDA.MinMax_T_Slots) on the tensors the plain launch wrote.  Everything is
exact: integer counts, min/max bit patterns, identical tensors.

Tensors of 2^20 elements or fewer are, by design, not fused by the histogram entry points (they launch nothing and the tensor
stays with the observers' end-of-forward launch): the three small shapes of the min/max test check exactly that here, and
each of the kernel paths they stand for (n % 4 tail with per-element channels, 7x7 planes) has a shape just above 2^20."""
import pytest
import torch

from ppq_amd import CUDA, ffi
from ppq_amd.observer import _range_seed

DEV = 'cuda:0'
gpu = pytest.mark.gpu

# (shape, fused by the histogram entry points).  [1,8,4,4]: fewer tiles than workgroups; [1,3,5,7]: n % 4 tail, per-element
# channels; [2,16,7,7]: 7x7 planes; [2,64,96,96]: 1.18 M elements, a ragged last tile; [4,64,96,96]: 576 tiles, more than the
# 512-workgroup grid cap (several tiles per workgroup: the ping-pong loop); [1,3,599,601]: 1 079 997 elements, n % 4 = 1,
# per-element channels; [8,2700,7,7]: 1 058 400 elements in 7x7 planes
SHAPES = [((1, 8, 4, 4), False), ((1, 3, 5, 7), False), ((2, 16, 7, 7), False), ((2, 64, 96, 96), True), ((4, 64, 96, 96), True),
          ((1, 3, 599, 601), True), ((8, 2700, 7, 7), True)]
CHANNELS_LAST = (2, 24, 150, 150)            # 1.08 M elements
SMALL_LIMIT = 1 << 20


def _bits_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _inputs(shape, gen, special=True):
    """(conv output, bias): channel 0 has bias 0 and its first elements are -0.0, +0.0, NaN and +-inf."""
    y = torch.randn(shape, generator=gen)
    bias = torch.randn(shape[1], generator=gen) * 0.3
    if special:
        bias[0] = 0.0
        flat = y.view(-1)
        vals = [-0.0, 0.0, float('nan'), float('inf'), float('-inf')]
        n = min(len(vals), shape[2] * shape[3], flat.numel())
        flat[:n] = torch.tensor(vals[:n])
    return y.to(DEV), bias.to(DEV)


_DATA = {}


def _data(shape):
    """The operands of one shape, made once and never modified: (a, bias_a, b, bias_b)."""
    if shape not in _DATA:
        gen = torch.Generator().manual_seed(hash(shape) % 1000)
        _DATA[shape] = _inputs(shape, gen) + _inputs(shape, gen)
    return _DATA[shape]


class _Rows:
    """One observer-shaped histogram accumulator.  The rule puts part of N(0, 1) + bias beyond the last bin (symmetric:
    |x| > 2; asymmetric: x < -1.5 or x > 2) and ReLU's zeros into the hot bin 0 (symmetric)."""
    def __init__(self, asym, clip, bins):
        self.asym, self.clip, self.bins = asym, clip, bins
        self.p0, self.p1 = (-1.5, 2.0) if asym else (2.0 / bins, 0.0)
        self.rows = torch.zeros(CUDA.hist_rows(), bins, dtype=torch.int32, device=DEV)

    def job(self): return ('hist_rows', self.rows, self.asym, self.p0, self.p1, self.clip)

    def observe(self, t):                          # the observers' own launch
        if self.asym: CUDA.Histogram_Asymmetric_T_Rows(self.p0, self.p1, tensor=t, rows=self.rows, clip_outliers=self.clip)
        else: CUDA.Histogram_T_Rows(tensor=t, rows=self.rows, scale=self.p0, clip_outliers=self.clip)

    def folded(self): return self.rows.sum(0)


class _Slots:
    """One observer-shaped running range."""
    def __init__(self): self.buf = _range_seed(torch.device(DEV))[1].clone()

    def job(self): return ('minmax', self.buf)

    def observe(self, t): CUDA.MinMax_T_Slots(t, self.buf)

    def folded(self): return CUDA.MinMax_Slots_Finish(self.buf, _range_seed(torch.device(DEV))[0].clone())


def _same(s0, s1):
    a, b = s0.folded(), s1.folded()
    if a.dtype == torch.int32: assert torch.equal(a, b), (int((a != b).sum()), int(a.sum()), int(b.sum()))
    else: assert _bits_equal(a, b), (a, b)


def _reference(ops, mode, sinks):
    """The plain launch on clones of `ops`, then the observers' own launch on what it stored.  Returns the stored tensors."""
    a, bias_a, b, bias_b = ops
    a, b = a.clone(memory_format=torch.preserve_format), b.clone(memory_format=torch.preserve_format)
    if mode == 'p1':
        assert ffi.bias_act_(a, bias_a, relu=True)
        sinks[0].observe(a)
        return [a]
    out = ffi.bias_add_act(a, bias_a, b, bias_b if mode == 'p2b' else None, relu=True)
    stored = [a, b, out] if mode == 'p2b' else [a, out]
    for s, t in zip(sinks, stored): s.observe(t)
    return stored


def _fused(ops, mode, sinks, elide=0):
    """The sink launch on clones of `ops`.  Returns (the tensors a, b, out after it -- or None when nothing was launched,
    the clones it was given)."""
    a, bias_a, b, bias_b = ops
    a, b = a.clone(memory_format=torch.preserve_format), b.clone(memory_format=torch.preserve_format)
    hist = isinstance(sinks[0], _Rows)
    if mode == 'p1':
        ok = (ffi.bias_act_hist_ if hist else ffi.bias_act_stats_)(a, bias_a, True, sinks[0].job())
        return ([a] if ok else None), (a, b)
    jobs = [s.job() for s in sinks]
    launch = ffi.bias_add_act_hist if hist else ffi.bias_add_act_stats
    out = launch(a, bias_a, b, bias_b if mode == 'p2b' else None, True, jobs[0], jobs[1] if mode == 'p2b' else None, jobs[-1], elide)
    if out is None: return None, (a, b)
    return ([a, b, out] if mode == 'p2b' else [a, out]), (a, b)


N_SINKS = {'p1': 1, 'p2': 2, 'p2b': 3}


def _check_hist(shape, fused, mode, asym, clip, bins, ops=None, launches=1):
    ops = ops or _data(shape)
    ref = [_Rows(asym, clip, bins) for _ in range(N_SINKS[mode])]
    got = [_Rows(asym, clip, bins) for _ in range(N_SINKS[mode])]
    for k in range(launches):                          # several launches accumulate
        cur = ops if k == 0 else tuple(t.flip(0) if t.dim() == 4 else t for t in ops)
        want = _reference(cur, mode, ref)
        have, given = _fused(cur, mode, got)
        if not fused:                                  # at most 2^20 elements: nothing is launched, nothing is touched
            assert have is None
            assert _bits_equal(given[0], cur[0]) and _bits_equal(given[1], cur[2])
            assert all(int(s.rows.sum()) == 0 for s in got)
            return
        assert have is not None, (shape, mode)
        for w, h in zip(want, have): assert _bits_equal(w, h), (shape, mode)
    for s0, s1 in zip(ref, got): _same(s0, s1)
    assert int(ref[-1].folded().sum()) > 0


@gpu
@pytest.mark.parametrize('asym', [False, True])
@pytest.mark.parametrize('mode', ['p1', 'p2', 'p2b'])
def test_hist_sinks_equal_epilogue_then_observer_launch(mode, asym):
    for shape, fused in SHAPES:
        assert fused == (torch.Size(shape).numel() > SMALL_LIMIT)
        for clip in (True, False):
            for bins in (2048, 128):
                _check_hist(shape, fused, mode, asym, clip, bins)


@gpu
def test_hist_sinks_accumulate_over_consecutive_launches():
    for mode in ('p1', 'p2b'):
        _check_hist((2, 64, 96, 96), True, mode, False, True, 2048, launches=2)
        _check_hist((8, 2700, 7, 7), True, mode, True, True, 128, launches=2)
    # above 2048 bins a workgroup's row is no longer read ahead into registers: one sink of 4096 bins still fits the counters
    _check_hist((2, 64, 96, 96), True, 'p1', False, True, 4096, launches=2)
    _check_hist((2, 64, 96, 96), True, 'p1', True, False, 4096, launches=2)


@gpu
@pytest.mark.parametrize('mode', ['p1', 'p2b'])
def test_hist_sinks_channels_last_layout(mode):
    gen = torch.Generator().manual_seed(9)
    ops = tuple(t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t
                for t in _inputs(CHANNELS_LAST, gen) + _inputs(CHANNELS_LAST, gen))
    for asym in (False, True):
        _check_hist(CHANNELS_LAST, True, mode, asym, True, 2048, ops=ops)


@gpu
def test_hist_sinks_do_not_fuse_what_they_have_no_path_for():
    """An unaligned view, more counters than the LDS budget, sinks of different rules in one launch, and the tuple shape
    the min/max entry point refuses: NOTHING is launched, neither tensor nor rows change."""
    shape = (2, 64, 96, 96)
    a, bias_a, b, bias_b = _data(shape)
    base = torch.empty(1 + a.numel(), device=DEV)
    view = base[1:].view(shape)                  # a one-float offset: not 16-B aligned
    view.copy_(a)
    r = _Rows(False, True, 2048)
    assert not ffi.bias_act_hist_(view, bias_a, True, r.job())
    assert ffi.bias_add_act_hist(view, bias_a, b.clone(), None, True, r.job(), None, None) is None
    assert _bits_equal(view, a) and int(r.rows.sum()) == 0
    y = a.clone()
    big = _Rows(False, True, 8192)               # 8192 counters: above the budget of 6144
    assert not ffi.bias_act_hist_(y, bias_a, True, big.job())
    r2, r3 = _Rows(False, True, 2048), _Rows(False, True, 128)
    bb = b.clone()
    assert ffi.bias_add_act_hist(y, bias_a, bb, None, True, r2.job(), None, r3.job()) is None      # two bin counts
    r4 = _Rows(True, True, 2048)
    assert ffi.bias_add_act_hist(y, bias_a, bb, None, True, r2.job(), None, r4.job()) is None      # two rules
    assert ffi.bias_add_act_hist(y, bias_a, bb, None, True, None, None, None) is None              # no sink at all
    assert not ffi.bias_act_stats_(y, bias_a, True, r2.job())                                      # wrong entry point
    assert not ffi.bias_act_hist_(y, bias_a, True, _Slots().job())
    assert _bits_equal(y, a) and _bits_equal(bb, b)
    assert all(int(s.rows.sum()) == 0 for s in (big, r2, r3, r4))


# ---------------------------------------------------------------------------------------------- store elision
def _check_elision(shape, mode, make_sink, elide):
    ops = _data(shape)
    ref = [make_sink() for _ in range(N_SINKS[mode])]
    got = [make_sink() for _ in range(N_SINKS[mode])]
    want = _reference(ops, mode, ref)
    have, _ = _fused(ops, mode, got, elide)
    assert have is not None, (shape, mode)
    assert _bits_equal(want[-1], have[-1])                                  # out
    a_after, b_after = have[0], (have[1] if mode == 'p2b' else None)
    # an elided operand keeps the convolution output it held; a stored one is the plain launch's
    assert _bits_equal(a_after, ops[0] if elide & ffi.ELIDE_A else want[0])
    if mode == 'p2b': assert _bits_equal(b_after, ops[2] if elide & ffi.ELIDE_B else want[1])
    for s0, s1 in zip(ref, got): _same(s0, s1)                              # every statistic as without elision


@gpu
@pytest.mark.parametrize('mode,elide', [('p2', 1), ('p2b', 1), ('p2b', 2), ('p2b', 3)])
def test_elided_stores_minmax_sinks(mode, elide):
    for shape, _ in SHAPES: _check_elision(shape, mode, _Slots, elide)


@gpu
@pytest.mark.parametrize('mode,elide', [('p2', 1), ('p2b', 1), ('p2b', 2), ('p2b', 3)])
def test_elided_stores_hist_sinks(mode, elide):
    for shape, fused in SHAPES:
        if not fused: continue                     # (not fused at all: test_hist_sinks_equal_epilogue_then_observer_launch)
        for asym in (False, True): _check_elision(shape, mode, lambda: _Rows(asym, True, 2048), elide)


@gpu
@pytest.mark.parametrize('make_sink', [_Slots, lambda: _Rows(False, True, 2048)])
def test_elision_without_a_sink_is_refused(make_sink):
    shape = (2, 64, 96, 96)
    a, bias_a, b, bias_b = _data(shape)
    a1, b1 = a.clone(), b.clone()
    s_a, s_out = make_sink(), make_sink()
    launch = ffi.bias_add_act_hist if isinstance(s_a, _Rows) else ffi.bias_add_act_stats
    state = lambda s: (s.rows if isinstance(s, _Rows) else s.buf).clone()
    before = state(s_a), state(s_out)
    with pytest.raises(RuntimeError):              # a is elided but has no sink
        launch(a1, bias_a, b1, bias_b, True, None, None, s_out.job(), ffi.ELIDE_A)
    with pytest.raises(RuntimeError):              # b is elided but has no sink
        launch(a1, bias_a, b1, bias_b, True, s_a.job(), None, s_out.job(), ffi.ELIDE_B)
    with pytest.raises(RuntimeError):              # without bias_b, b is not computed: nothing to elide
        launch(a1, bias_a, b1, None, True, s_a.job(), None, s_out.job(), ffi.ELIDE_B)
    torch.cuda.synchronize()
    assert _bits_equal(a1, a) and _bits_equal(b1, b)
    assert torch.equal(state(s_a), before[0]) and torch.equal(state(s_out), before[1])


@gpu
def test_two_sinks_on_one_accumulator_are_refused():
    """A workgroup reads its row of every sink ahead and writes it back at the end, so the sinks of a launch must be
    distinct accumulators: the same rows twice is an error, and nothing is launched."""
    shape = (2, 64, 96, 96)
    a, bias_a, b, bias_b = _data(shape)
    a1, b1, r = a.clone(), b.clone(), _Rows(False, True, 2048)
    for jobs in ((r.job(), None, r.job()), (r.job(), r.job(), None), (None, r.job(), r.job())):
        with pytest.raises(RuntimeError):
            ffi.bias_add_act_hist(a1, bias_a, b1, bias_b, True, *jobs)
    torch.cuda.synchronize()
    assert _bits_equal(a1, a) and _bits_equal(b1, b) and int(r.rows.sum()) == 0
