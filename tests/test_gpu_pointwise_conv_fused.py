"""ppqhip_conv1x1_epilogue (ffi.conv1x1_epilogue): the native 1x1 convolution with its epilogue group -- bias, residual Add, ReLU --
and the group's calibration sinks in the GEMM's store.  Reference: today's path, ``ffi.conv1x1(x, w, None, stride)`` followed by the
sink epilogue launch (``bias_act_stats_`` / ``bias_add_act_stats`` / ``bias_act_hist_`` / ``bias_add_act_hist``) with the same
jobs and every tensor the fused launch does not store elided; where that launch takes nothing in (by design the histogram sinks
leave tensors of 2^20 elements or fewer alone) the plain epilogue launch followed by the observers' own launch on what it stored,
which is what the sink launches are themselves tested against.  Everything is exact: ``out`` bit for bit, the folded min/max
slots bit for bit, the histogram rows as integers.

Shapes are the smallest at which each mechanism can break: c in {8, 33, 64} (a partial last K tile, dword loads), o in {8, 40, 72}
(a partial row tile of the 64 x 128 block), planes 7x7 (dword loads, C/D-map lanes off the edge) and 8x8 (16-byte loads), stride 2
on 9x9, n = 3; a 10-tile tensor walked by 1 and by 3 workgroups."""
import itertools

import pytest
import torch

from ppq_amd import CUDA, ffi
from ppq_amd.observer import _range_seed

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
BINS = 2048


def _bits_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


class _Rows:
    """One observer-shaped histogram accumulator; the rule leaves part of the values beyond the last bin."""
    def __init__(self, asym, clip, bins=BINS):
        self.asym, self.clip = asym, clip
        self.p0, self.p1 = (-1.5, 2.0) if asym else (2.0 / bins, 0.0)
        self.rows = torch.zeros(CUDA.hist_rows(), bins, dtype=torch.int32, device=DEV)

    def job(self): return ('hist_rows', self.rows, self.asym, self.p0, self.p1, self.clip)

    def observe(self, t):
        if self.asym: CUDA.Histogram_Asymmetric_T_Rows(self.p0, self.p1, tensor=t, rows=self.rows, clip_outliers=self.clip)
        else: CUDA.Histogram_T_Rows(tensor=t, rows=self.rows, scale=self.p0, clip_outliers=self.clip)

    def folded(self): return self.rows.sum(0, dtype=torch.int64)


class _Slots:
    """One observer-shaped running range."""
    def __init__(self): self.buf = _range_seed(torch.device(DEV))[1].clone()

    def job(self): return ('minmax', self.buf)

    def observe(self, t): CUDA.MinMax_T_Slots(t, self.buf)

    def folded(self): return CUDA.MinMax_Slots_Finish(self.buf, _range_seed(torch.device(DEV))[0].clone())


def _same(s0, s1):
    a, b = s0.folded(), s1.folded()
    if a.dtype == torch.int64: assert torch.equal(a, b), (int((a != b).sum()), int(a.sum()), int(b.sum()))
    else: assert _bits_equal(a, b), (a, b)


_DATA = {}


def _data(n, c, o, h, w, stride, special=False):
    """(x, weight, bias_a, resid, bias_b) of one shape, made once and never modified."""
    key = (n, c, o, h, w, stride, special)
    if key not in _DATA:
        gen = torch.Generator().manual_seed(sum(v * 31 ** k for k, v in enumerate(key[:6])) % 10007)
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        x = torch.randn(n, c, h, w, generator=gen)
        wt = torch.randn(o, c, 1, 1, generator=gen) * (1.0 / c ** 0.5)
        resid = torch.randn(n, o, ho, wo, generator=gen)
        bias_a, bias_b = torch.randn(o, generator=gen) * 0.3, torch.randn(o, generator=gen) * 0.3
        if special:
            bias_a[0] = 0.0
            x[0, :, 0, 0] = 0.0; x[0, 0, 0, 0] = -0.0               # an all-zero column: +0 from the chain, -0 never survives it
            x[0, 1, 0, 2] = float('nan'); x[0, 2, 2, 0] = float('inf'); x[1, 0, 2, 2] = float('-inf')
            r = resid.view(-1)
            r[:5] = torch.tensor([-0.0, 0.0, float('nan'), float('inf'), float('-inf')])
        _DATA[key] = tuple(t.to(DEV) for t in (x, wt, bias_a, resid, bias_b))
    return _DATA[key]


def _sinks(kind, count):
    if kind == 'minmax': return [_Slots() for _ in range(count)]
    return [_Rows(kind[1], kind[2]) for _ in range(count)]


def _reference(ops, stride, form, relu, sinks, times=1):
    """Today's path.  `sinks`: [out] (p1), [a, out] (p2), [a, r, out] (p2b), None where a tensor has no sink.  Returns out."""
    x, wt, bias_a, resid, bias_b = ops
    hist = any(isinstance(s, _Rows) for s in sinks if s is not None)
    jobs = [None if s is None else s.job() for s in sinks]
    for _ in range(times):
        y = ffi.conv1x1(x, wt, None, stride)
        assert y is not None
        if form == 'p1':
            done = (ffi.bias_act_hist_ if hist else ffi.bias_act_stats_)(y, bias_a, relu, jobs[0])
            if not done:
                assert ffi.bias_act_(y, bias_a, relu=relu)
                sinks[0].observe(y)
            out = y
            continue
        b, bb = resid.clone(), (bias_b if form == 'p2b' else None)
        job_a, job_b, job_out = jobs[0], (jobs[1] if form == 'p2b' else None), jobs[-1]
        elide = (ffi.ELIDE_A if job_a is not None else 0) | (ffi.ELIDE_B if job_b is not None else 0)
        out = (ffi.bias_add_act_hist if hist else ffi.bias_add_act_stats)(y, bias_a, b, bb, relu, job_a, job_b, job_out, elide)
        if out is None:
            out = ffi.bias_add_act(y, bias_a, b, bb, relu=relu)
            assert out is not None
            stored = [y, b, out] if form == 'p2b' else [y, out]
            for s, t in zip(sinks, stored):
                if s is not None: s.observe(t)
    return out


def _fused(ops, stride, form, relu, sinks, max_workgroups=0, times=1):
    x, wt, bias_a, resid, bias_b = ops
    jobs = [None if s is None else s.job() for s in sinks]
    for _ in range(times):
        if form == 'p1': out = ffi.conv1x1_epilogue(x, wt, stride, bias_a, None, None, relu, None, None, jobs[0], max_workgroups)
        elif form == 'p2': out = ffi.conv1x1_epilogue(x, wt, stride, bias_a, resid, None, relu, jobs[0], None, jobs[1], max_workgroups)
        else: out = ffi.conv1x1_epilogue(x, wt, stride, bias_a, resid, bias_b, relu, jobs[0], jobs[1], jobs[2], max_workgroups)
    return out


NS = {'p1': 1, 'p2': 2, 'p2b': 3}


def _check(shape, form, kind, subset=None, relu=True, max_workgroups=0, times=1, special=False):
    n, c, o, h, w, stride = shape
    ops = _data(n, c, o, h, w, stride, special)
    subset = subset if subset is not None else (True,) * NS[form]
    ref = [s if on else None for s, on in zip(_sinks(kind, NS[form]), subset)]
    got = [s if on else None for s, on in zip(_sinks(kind, NS[form]), subset)]
    resid_before = ops[3].clone()
    want = _reference(ops, stride, form, relu, ref, times)
    out = _fused(ops, stride, form, relu, got, max_workgroups, times)
    assert out is not None
    assert _bits_equal(out, want), int((out.view(torch.int32) != want.view(torch.int32)).sum())
    assert _bits_equal(ops[3], resid_before)                       # the residual is only read
    for s0, s1 in zip(ref, got):
        if s0 is not None: _same(s0, s1)


KINDS = ['minmax', ('hist', False, False), ('hist', False, True), ('hist', True, False), ('hist', True, True)]
# (n, c, o, h, w, stride): every c and o of the docstring, each plane, the stride-2 form
SHAPES = [(3, 8, 8, 7, 7, 1), (3, 33, 40, 7, 7, 1), (3, 64, 72, 8, 8, 1), (3, 33, 72, 8, 8, 1), (3, 8, 40, 8, 8, 1),
          (3, 64, 40, 9, 9, 2), (3, 33, 8, 9, 9, 2)]


@pytest.mark.parametrize('kind', KINDS, ids=lambda k: k if isinstance(k, str) else f'hist-asym{int(k[1])}-clip{int(k[2])}')
@pytest.mark.parametrize('form', ['p1', 'p2', 'p2b'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_fused_equals_unfused(shape, form, kind):
    _check(shape, form, kind)


@pytest.mark.parametrize('kind', ['minmax', ('hist', False, True)], ids=['minmax', 'hist'])
def test_every_sink_subset(kind):
    """Every non-empty subset of the sinks of each form (the executor produces those with a job for every tensor that is not stored;
    the entry point takes them all)."""
    shape = (3, 33, 40, 8, 8, 1)
    for form in ('p2', 'p2b'):
        for subset in itertools.product((False, True), repeat=NS[form]):
            if any(subset): _check(shape, form, kind, subset)


@pytest.mark.parametrize('kind', ['minmax', ('hist', True, False)], ids=['minmax', 'hist'])
@pytest.mark.parametrize('form', ['p1', 'p2b'])
def test_without_relu(form, kind):
    _check((3, 33, 40, 7, 7, 1), form, kind, relu=False)


@pytest.mark.parametrize('max_workgroups', [1, 3])
@pytest.mark.parametrize('kind', ['minmax', ('hist', False, False)], ids=['minmax', 'hist'])
@pytest.mark.parametrize('form', ['p1', 'p2b'])
def test_several_tiles_per_workgroup(form, kind, max_workgroups):
    """o = 72 is two row tiles, 3 x 12 x 16 = 576 columns are five column tiles: ten tiles, so one workgroup walks all of them and
    of three the first owns four and the others three -- the prefetch of the next tile, both halves of the bias staging, a
    partial row tile and a partial column tile."""
    _check((3, 64, 72, 12, 16, 1), form, kind, max_workgroups=max_workgroups)
    _check((3, 33, 72, 15, 13, 1), form, kind, max_workgroups=max_workgroups)      # the same with dword loads (585 columns)


@pytest.mark.parametrize('kind', ['minmax', ('hist', False, True)], ids=['minmax', 'hist'])
def test_two_launches_accumulate(kind):
    """The slot / row is read and added to, not overwritten."""
    _check((3, 64, 72, 8, 8, 1), 'p2b', kind, times=2)
    _check((3, 33, 40, 7, 7, 1), 'p1', kind, times=2, max_workgroups=1)


@pytest.mark.parametrize('kind', KINDS, ids=lambda k: k if isinstance(k, str) else f'hist-asym{int(k[1])}-clip{int(k[2])}')
@pytest.mark.parametrize('form', ['p1', 'p2b'])
def test_special_values(form, kind):
    """NaN, +-Inf and -0 in x and in the residual come out, and are folded / counted, as on today's path."""
    _check((3, 8, 8, 8, 8, 1), form, kind, special=True)
    _check((3, 33, 40, 7, 7, 1), form, kind, special=True, relu=False)


def test_plane_width_no_multiple_of_32():
    """5 x 13 = 65 columns per image: the 32 C/D-map lanes of a store straddle images and fall off the last column tile."""
    for form in ('p1', 'p2'):
        _check((3, 8, 40, 5, 13, 1), form, 'minmax')
        _check((3, 8, 40, 5, 13, 1), form, ('hist', False, False))


@pytest.mark.parametrize('kind', ['minmax', ('hist', False, True)], ids=['minmax', 'hist'])
def test_hip_graph_replay(kind):
    """One capture and one replay give what one eager launch gives."""
    shape, form = (3, 64, 72, 8, 8, 1), 'p2b'
    ops = _data(*shape)
    eager, replayed, warm = _sinks(kind, 3), _sinks(kind, 3), _sinks(kind, 3)
    want = _fused(ops, 1, form, True, eager)
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream): _fused(ops, 1, form, True, warm)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph): out = _fused(ops, 1, form, True, replayed)
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert _bits_equal(out, want)
    for s0, s1 in zip(eager, replayed): _same(s0, s1)


def test_nothing_launched():
    """PPQHIP_NOT_FUSED and the binding's own refusals return None; a call the entry point refuses raises."""
    ops = _data(3, 8, 8, 8, 8, 1)
    x, wt, bias_a, resid, bias_b = ops
    assert ffi.conv1x1_epilogue(x, wt, 1, bias_a, None, None, True, None, None, None) is None                    # no job
    big = [_Rows(False, False, bins=4096) for _ in range(3)]                                                    # 3 x 4096 counters
    assert ffi.conv1x1_epilogue(x, wt, 1, bias_a, resid, bias_b, True, *(s.job() for s in big)) is None
    assert all(int(s.rows.sum()) == 0 for s in big)
    mixed = [_Slots().job(), None, _Rows(False, False).job()]
    assert ffi.conv1x1_epilogue(x, wt, 1, bias_a, resid, None, True, *mixed) is None                             # two kinds
    assert ffi.conv1x1_epilogue(x, wt, 1, bias_a, resid[:, :, :4], None, True, _Slots().job(), None, None) is None
    with pytest.raises(RuntimeError, match='only out has a sink'):
        ffi.conv1x1_epilogue(x, wt, 1, bias_a, None, None, True, _Slots().job(), None, None)
    shared = _Slots().job()
    with pytest.raises(RuntimeError, match='two sinks share one accumulator'):
        ffi.conv1x1_epilogue(x, wt, 1, bias_a, resid, None, True, shared, None, shared)
