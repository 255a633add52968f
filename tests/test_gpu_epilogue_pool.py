"""The pooled epilogue launches (ppqhip_bias_act_pool / _pool_stats / _pool_hist): Conv(bias) -> Relu -> MaxPool in one launch.

Everything is exact.  The pooled tensor must equal ``F.max_pool2d(F.relu(y + b.view(1, -1, 1, 1)), k, s, p)`` bit for bit (signed
zeros and NaN included: compared as int32), ``y`` must come out as the plain epilogue leaves it -- or untouched when the store is
elided -- and what the sinks fold / count must equal what the existing ppqhip_bias_act_stats / ppqhip_bias_act_hist launch folds /
counts on a copy of the same input.  Which slot or row a value lands in is unspecified for both launches (their grids differ),
so ranges are compared after ppqhip_minmax_slots_finish and histograms as column sums.  ppqhip_bias_act_hist launches nothing
for tensors of 2^20 elements or fewer; there the counts are compared with the observers' own launch on what the plain epilogue
stored -- the reference tests/test_gpu_epilogue_hist.py holds ppqhip_bias_act_hist itself to -- and one shape above 2^20
elements is compared with both."""
import pytest
import torch
import torch.nn.functional as F

from ppq_amd import CUDA, _lib, ffi
from ppq_amd.observer import _range_seed

DEV = 'cuda:0'
gpu = pytest.mark.gpu

# [2,3,8,8], [3,4,12,12], [2,2,6,10] (pooled planes of 15 elements with stride 2: element-wise stores), [1,2,112,112] (one real
# stem plane: four steps per plane, the last one ragged): fewer planes than workgroups.  [2,300,8,8]: 600 planes, more than the
# 512-workgroup grid cap (several planes per workgroup).  [2,48,112,112]: 1.2 M elements, where ppqhip_bias_act_hist launches
SHAPES = [(2, 3, 8, 8), (3, 4, 12, 12), (1, 2, 112, 112), (2, 2, 6, 10), (2, 300, 8, 8)]
LARGE = (2, 48, 112, 112)
WINDOWS = [(3, 2, 1), (2, 2, 0), (3, 1, 1)]


def _bits(t): return t.contiguous().view(torch.int32)


def _bits_equal(x, y): return x.shape == y.shape and torch.equal(_bits(x), _bits(y))


_DATA = {}


def _data(shape):
    """(y, bias) of one shape, made once and never modified.  Channel 0 has bias -0.0, so what is planted in plane (0, 0)
    survives the add: the plane is negative throughout (every window of relu's output is all +0.0; without relu the zeros
    planted below are the maxima and the scan order decides whose sign comes out), with -0.0 left of +0.0, +0.0 left of -0.0,
    +0.0 above -0.0, a NaN, +inf and -inf."""
    if shape not in _DATA:
        gen = torch.Generator().manual_seed(sum(shape))
        y = torch.randn(shape, generator=gen)
        bias = torch.randn(shape[1], generator=gen) * 0.3
        bias[0] = -0.0
        p = y[0, 0]
        p.copy_(-p.abs() - 0.5)
        p[1, 0], p[1, 1] = -0.0, 0.0
        p[3, 2], p[3, 3] = 0.0, -0.0
        p[4, 0], p[5, 0] = 0.0, -0.0
        p[0, 3] = float('nan')
        p[-1, -1] = float('inf')
        p[0, -1] = float('-inf')
        _DATA[shape] = (y.to(DEV), bias.to(DEV))
    return _DATA[shape]


_REF = {}


def _reference(shape, window, relu=True):
    """(act(y + b), its max pool) by PyTorch, computed once."""
    key = (shape, window, relu)
    if key not in _REF:
        y, b = _data(shape)
        x = y + b.view(1, -1, 1, 1)
        if relu: x = F.relu(x)
        _REF[key] = (x, F.max_pool2d(x, *window))
    return _REF[key]


@gpu
@pytest.mark.parametrize('window', WINDOWS)
def test_plain_pooled_launch_equals_torch(window):
    for shape in SHAPES:
        for relu in (True, False):
            y, b = _data(shape)
            act, want = _reference(shape, window, relu)
            got_y = y.clone()
            got = ffi.bias_act_(got_y, b, relu=relu, pool=window)
            assert got is not None, (shape, window)
            assert _bits_equal(got, want), (shape, window, relu, int((_bits(got) != _bits(want)).sum()))
            assert _bits_equal(got_y, act), (shape, window, relu)              # y is overwritten as ppqhip_bias_act does
            plain = y.clone()
            assert ffi.bias_act_(plain, b, relu=relu) and _bits_equal(plain, got_y)


@gpu
def test_planted_values_reach_the_pooled_tensor():
    """The reference itself shows what the planted values are for: the cases below would pass vacuously otherwise."""
    _, want = _reference((2, 3, 8, 8), (3, 2, 1), True)
    plane = want[0, 0]
    assert torch.isnan(plane).any() and torch.isinf(plane).any()
    zero = plane == 0
    assert zero.any() and (_bits(plane)[zero] == 0).all()                      # all-negative windows pool relu's +0.0
    _, raw = _reference((2, 3, 8, 8), (2, 2, 0), False)
    signs = _bits(raw[0, 0])[raw[0, 0] == 0]
    assert (signs == 0).any() and (signs != 0).any()                           # without relu both zeros win somewhere


class _Slots:
    """One observer-shaped running range."""
    def __init__(self): self.buf = _range_seed(torch.device(DEV))[1].clone()

    def job(self): return ('minmax', self.buf)

    def existing(self, y, b):                      # the existing sink launch on y, in place
        assert ffi.bias_act_stats_(y, b, True, self.job())

    def folded(self): return CUDA.MinMax_Slots_Finish(self.buf, _range_seed(torch.device(DEV))[0].clone())

    def untouched(self): return _bits_equal(self.buf, _range_seed(torch.device(DEV))[1])


class _Rows:
    """One observer-shaped histogram accumulator; the rule puts part of the values beyond the last bin and relu's zeros into
    the hot bin (symmetric)."""
    def __init__(self, asym, clip, bins):
        self.asym, self.clip, self.bins = asym, clip, bins
        self.p0, self.p1 = (-0.5, 2.0) if asym else (2.0 / bins, 0.0)
        self.rows = torch.zeros(CUDA.hist_rows(), bins, dtype=torch.int32, device=DEV)

    def job(self): return ('hist_rows', self.rows, self.asym, self.p0, self.p1, self.clip)

    def existing(self, y, b):
        """ppqhip_bias_act_hist on y, in place; below its size limit the plain epilogue and the observers' own launch.
        Returns whether the existing sink launch took place."""
        before = int(self.rows.sum())
        if ffi.bias_act_hist_(y, b, True, self.job()): return True
        assert y.numel() <= 1 << 20 and int(self.rows.sum()) == before
        assert ffi.bias_act_(y, b, relu=True)
        self.observe(y)
        return False

    def observe(self, t):
        if self.asym: CUDA.Histogram_Asymmetric_T_Rows(self.p0, self.p1, tensor=t, rows=self.rows, clip_outliers=self.clip)
        else: CUDA.Histogram_T_Rows(tensor=t, rows=self.rows, scale=self.p0, clip_outliers=self.clip)

    def folded(self): return self.rows.sum(0)

    def untouched(self): return int(self.rows.abs().sum()) == 0


def _check_sinks(shape, window, make, store, launches=1):
    y, b = _data(shape)
    act, want = _reference(shape, window)
    ref, got = make(), make()
    launch = ffi.bias_act_hist_ if isinstance(got, _Rows) else ffi.bias_act_stats_
    took_place = None
    for k in range(launches):                      # several launches accumulate
        cur = y if k == 0 else y.flip(0)
        mine, theirs = cur.clone(), cur.clone()
        took_place = ref.existing(theirs, b)
        pooled = launch(mine, b, True, got.job(), pool=window, store=store)
        assert pooled is not None, (shape, window)
        assert _bits_equal(pooled, want if k == 0 else want.flip(0)), (shape, window, store)
        if store: assert _bits_equal(mine, theirs) and _bits_equal(mine, act if k == 0 else act.flip(0))
        else: assert _bits_equal(mine, cur)        # the elided store: y keeps the convolution output
    a, c = ref.folded(), got.folded()
    if a.dtype == torch.int32:
        assert torch.equal(a, c), (shape, window, store, int((a != c).sum()), int(a.sum()), int(c.sum()))
        assert int(a.sum()) > 0
    else:
        assert _bits_equal(a, c), (shape, window, store, a, c)
    return took_place


@gpu
@pytest.mark.parametrize('store', [True, False], ids=['stored', 'elided'])
@pytest.mark.parametrize('window', WINDOWS)
def test_minmax_sink_equals_the_existing_stats_launch(window, store):
    for shape in SHAPES + [LARGE]:
        _check_sinks(shape, window, _Slots, store)
    _check_sinks((3, 4, 12, 12), window, _Slots, store, launches=2)


@gpu
@pytest.mark.parametrize('store', [True, False], ids=['stored', 'elided'])
@pytest.mark.parametrize('window', WINDOWS)
def test_histogram_sink_equals_the_existing_hist_launch(window, store):
    for asym in (False, True):
        for clip in (True, False):
            for bins in (2048, 126):               # (126: the plane in LDS starts behind counters that are padded to 16 B)
                for shape in SHAPES:
                    assert not _check_sinks(shape, window, lambda: _Rows(asym, clip, bins), store)
    for asym in (False, True):                     # above 2^20 elements the existing histogram sink launch is the reference
        assert _check_sinks(LARGE, window, lambda: _Rows(asym, True, 2048), store)
    _check_sinks((3, 4, 12, 12), window, lambda: _Rows(False, True, 2048), store, launches=2)


def _unaligned(shape):
    y, b = _data(shape)
    buf = torch.empty(y.numel() + 1, device=DEV)
    view = buf[1:].view(shape)
    view.copy_(y)
    return view, b


@gpu
def test_what_has_no_exact_path_launches_nothing():
    """H * W = 63, a pointer that is not 16-B aligned, windows the kernel has no form for, a plane that does not fit the LDS
    beside the counters: None, with y, the slots and the rows untouched."""
    odd = (1, 5, 7, 9)
    y = torch.randn(odd, generator=torch.Generator().manual_seed(5)).to(DEV)
    b = torch.randn(5, generator=torch.Generator().manual_seed(6)).to(DEV)
    cases = [(y, b, (3, 2, 1)), (*_unaligned((2, 3, 8, 8)), (3, 2, 1))]
    cases += [(*_data((3, 4, 12, 12)), w) for w in ((5, 1, 2), (4, 2, 1), (3, 2, 2))]
    big = torch.randn(1, 2, 128, 128, generator=torch.Generator().manual_seed(7)).to(DEV)       # 64 KB per plane
    cases.append((big, b[:2].contiguous(), (3, 2, 1)))
    for t, bias, window in cases:
        for form in ('plain', 'stats', 'hist'):
            for store in ((True,) if form == 'plain' else (True, False)):
                given = t.clone() if t.data_ptr() % 16 == 0 else _unaligned(tuple(t.shape))[0]
                before = given.clone()
                slots, rows = _Slots(), _Rows(False, True, 2048)
                if form == 'plain': out = ffi.bias_act_(given, bias, relu=True, pool=window)
                elif form == 'stats': out = ffi.bias_act_stats_(given, bias, True, slots.job(), pool=window, store=store)
                else: out = ffi.bias_act_hist_(given, bias, True, rows.job(), pool=window, store=store)
                assert out is None, (tuple(t.shape), window, form)
                assert _bits_equal(given, before) and slots.untouched() and rows.untouched()
    # a plane that fits beside 126 counters but not beside 2048: the histogram form decides by its counters
    fits = torch.randn(1, 2, 120, 124, generator=torch.Generator().manual_seed(8)).to(DEV)      # 59 520 B per plane
    bias = b[:2].contiguous()
    want = F.max_pool2d(F.relu(fits + bias.view(1, -1, 1, 1)), 3, 2, 1)
    assert ffi.bias_act_hist_(fits.clone(), bias, True, _Rows(False, True, 2048).job(), pool=(3, 2, 1)) is None
    got = ffi.bias_act_hist_(fits.clone(), bias, True, _Rows(False, True, 126).job(), pool=(3, 2, 1))
    assert got is not None and _bits_equal(got, want)
    # relu = 0 has no histogram form, as for ppqhip_bias_act_hist
    y0, b0 = _data((2, 3, 8, 8))
    assert ffi.bias_act_hist_(y0.clone(), b0, False, _Rows(False, True, 2048).job(), pool=(3, 2, 1)) is None


@gpu
def test_an_elided_store_needs_a_sink():
    y, b = _data((2, 3, 8, 8))
    y = y.clone()
    before = y.clone()
    pool = torch.zeros(2, 3, 4, 4, device=DEV)
    status = _lib.lib.ppqhip_bias_act_pool_stats(y.data_ptr(), b.data_ptr(), pool.data_ptr(), y.numel(), 3, 8, 8, 1, 3, 2, 1, 1, 0,
                                                 None, 0, None)
    assert status == -1 and b'needs a sink' in _lib.lib.ppqhip_last_error()
    status = _lib.lib.ppqhip_bias_act_pool_hist(y.data_ptr(), b.data_ptr(), pool.data_ptr(), y.numel(), 3, 8, 8, 1, 3, 2, 1, 1, 0,
                                                None, 0.01, 0.0, 2048, 0, 1, 0, None)
    assert status == -1 and b'needs a sink' in _lib.lib.ppqhip_last_error()
    torch.cuda.synchronize()
    assert _bits_equal(y, before) and int(pool.abs().sum()) == 0
