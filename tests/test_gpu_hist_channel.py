"""The per-channel histogram kernels of hist.hip (hist_c_channel_kernel, hist_c_channel_scalar_kernel, hist_c_global_kernel) on
every launch path of hist_c_impl, for the three rule forms (shared scale, per-channel scales, per-channel asymmetric ranges)
clipped and clamped: the whole [C, bins] histogram equals the plain numpy reference of tests/hist_c_reference.py, integer for
integer.  The case table, its data (ReLU, saturated, dead, unbounded channels; NaN, Inf, denormals and bin edges +- 1 ulp) and
the reference live there; tests/test_host_hist_channel.py pins the reference to the C oracle and shows which launch path each
case takes on a 256-CU device.  Nothing here branches on that path: the counts must hold wherever a case lands."""
import numpy as np
import pytest
import torch

import hist_c_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def CUDA():
    from ppq_amd import CUDA as C
    yield C
    for store in (_small, _big, _wants): store.clear()                      # hand the tensors back when the module is done


# ---- data and references: built once per shape, shared by the tests below, never written to ------------------------------------
_small, _big, _wants = {}, {}, {}


def _data(case):
    """(Planted, device tensor of the case's shape -- for offset 1 a view one float into a larger buffer)."""
    store = _small if case.size in ('small', 'limit') else _big
    if case.name not in store:
        if store is _big: store.clear()                                     # one large tensor at a time
        p = R.planted(case.shape, case.axis)
        n = p.x.size
        buf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
        x = buf[case.offset:case.offset + n].view(*case.shape)
        x.copy_(torch.from_numpy(p.x))
        p.x.setflags(write=False)
        assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == (case.offset % 4 == 0)
        store[case.name] = (p, x)
    return store[case.name]


def _want(case, form, clip, bins):
    key = (case.name, form, clip, bins)
    if key in _wants: return _wants[key]
    w = R.reference(_data(case)[0], form, clip, bins)
    w.setflags(write=False)
    if w.nbytes <= (1 << 20): _wants[key] = w
    return w


def _launch(CUDA, x, axis, form, clip, bins, rules, hist):
    hs, scales, mins, maxs = rules
    if form == 'shared': CUDA.Histogram_C(x, axis, hist, float(hs), clip)
    elif form == 'scales': CUDA.Histogram_C_Scales(x, axis, hist, scales, clip)
    else: CUDA.Histogram_Asymmetric_C_Ranges(x, axis, hist, mins, maxs, clip)


def _rules(p, bins):
    hs, scales, mins, maxs = R.scales_of(p, bins)
    return hs, torch.from_numpy(scales).to(DEV), torch.from_numpy(mins).to(DEV), torch.from_numpy(maxs).to(DEV)


def _assert_equal(got: torch.Tensor, want: np.ndarray, what):
    g = got.cpu().numpy().astype(np.int64)
    assert g.shape == want.shape, (g.shape, want.shape)
    if not np.array_equal(g, want):
        bad = np.argwhere(g != want)
        c, b = (int(v) for v in bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {g.size} counts differ in {len(set(bad[:, 0].tolist()))} channels; first at '
                             f'channel {c} bin {b}: {g[c, b]} against {want[c, b]}; row sums {g[c].sum()} against {want[c].sum()}')


# ---- 1. every case x rule form x clip x bins, into a zeroed histogram ----------------------------------------------------------
@pytest.mark.parametrize('run', R.runs(), ids=R.run_id)
def test_counts_equal_the_reference(CUDA, run):
    case, form, clip, bins = run
    p, x = _data(case)
    C = case.shape[case.axis]
    hist = torch.zeros(C, bins, dtype=torch.int32, device=DEV)
    _launch(CUDA, x, case.axis, form, clip, bins, _rules(p, bins), hist)
    _assert_equal(hist, _want(case, form, clip, bins), R.run_id(run))


# ---- 2. += into a histogram that is not zero, twice ----------------------------------------------------------------------------
ACCUMULATE = ([(R.CASE[n], f, clip, b) for n, f, clip, b in [
    ('f4_splits_inside_rows', 'scales', True, 2048), ('f4_rest_one_wave', 'ranges', False, 128),
    ('f4_tile_rest', 'shared', True, 50), ('limit_bins', 'scales', False, 16384),
    ('scalar_epc_mod4', 'scales', False, 128), ('scalar_epc_mod4_splits', 'ranges', True, 50),
    ('scalar_unaligned_splits', 'shared', False, 4096), ('scalar_epc_lt64', 'ranges', False, 2048),
    ('global_short', 'shared', True, 128), ('global_last_axis', 'scales', True, 50), ('limit_bins', 'ranges', True, 16385)]]
    # the plain read-modify-write flush of the float4 kernel: a lost or doubled add shows here only
    + [(R.CASE[n], f, clip, b) for n in ('f4_rows_add_c_eq_cu', 'f4_rows_add_c_gt_cu')
       for f, clip, b in (('shared', True, 2048), ('scales', False, 128), ('ranges', True, 4096))])


@pytest.mark.parametrize('run', ACCUMULATE, ids=R.run_id)
def test_accumulates_into_a_nonzero_histogram(CUDA, run):
    case, form, clip, bins = run
    p, x = _data(case)
    C = case.shape[case.axis]
    seed = torch.randint(0, 5, (C, bins), dtype=torch.int32, generator=torch.Generator().manual_seed(bins + C))
    hist = seed.to(DEV)
    rules = _rules(p, bins)
    _launch(CUDA, x, case.axis, form, clip, bins, rules, hist)
    _launch(CUDA, x, case.axis, form, clip, bins, rules, hist)
    _assert_equal(hist, seed.numpy().astype(np.int64) + 2 * _want(case, form, clip, bins), R.run_id(run))


# ---- 3. nothing outside [C, bins] is written, nothing outside x is counted ------------------------------------------------------
GUARDED = [(R.CASE[n], f, clip) for n in ('f4_rest_one_wave', 'f4_tile_rest', 'f4_splits_inside_rows', 'scalar_epc_mod4',
                                          'scalar_epc_mod4_splits', 'scalar_unaligned_splits', 'scalar_last_axis', 'global_short')
           for f in R.FORMS for clip in (True, False)]
SENTINEL = 0x5A5A5A5A


@pytest.mark.parametrize('case,form,clip', GUARDED, ids=lambda v: v.name if isinstance(v, R.Case) else str(v))
def test_rows_around_the_histogram_are_left_alone(CUDA, case, form, clip):
    bins = 128
    p, x0 = _data(case)
    C, n = case.shape[case.axis], p.x.size
    pad = 1024
    # x inside a float buffer whose surroundings WOULD be counted (0.5 is inside every rule's range), at the case's alignment
    fbuf = torch.full((pad + n + pad,), 0.5, dtype=torch.float32, device=DEV)
    x = fbuf[pad + case.offset:pad + case.offset + n].view(*case.shape)
    x.copy_(x0)
    assert (x.data_ptr() % 16 == 0) == (case.offset % 4 == 0)
    ibuf = torch.full((3 * C * bins,), SENTINEL, dtype=torch.int32, device=DEV)
    hist = ibuf[C * bins:2 * C * bins].view(C, bins)
    hist.zero_()
    _launch(CUDA, x, case.axis, form, clip, bins, _rules(p, bins), hist)
    _assert_equal(hist, _want(case, form, clip, bins), (case.name, form, clip))
    out = ibuf.cpu().numpy()
    assert (out[:C * bins] == SENTINEL).all() and (out[2 * C * bins:] == SENTINEL).all()
    f = fbuf.cpu().numpy()
    assert (f[:pad + case.offset] == 0.5).all() and (f[pad + case.offset + n:] == 0.5).all()


# ---- 4. a second witness: the per-tensor kernels on each channel's contiguous slice ---------------------------------------------
WITNESS = [(R.CASE[n], f, clip, b) for n, b in (('f4_splits_inside_rows', 2048), ('f4_tile_rest', 128), ('scalar_epc_mod4_splits', 50),
                                                ('scalar_epc_mod4', 4096), ('scalar_unaligned_splits', 128))
           for f in ('scales', 'ranges') for clip in (True, False)]


@pytest.mark.parametrize('run', WITNESS, ids=R.run_id)
def test_each_channel_equals_the_per_tensor_kernel_on_its_slice(CUDA, run):
    """Row c == Histogram_T / Histogram_Asymmetric_T on channel c's slice (those kernels are pinned to the oracle bit for bit in
    test_gpu_kernels.py), the dead (hist_scale 0, min == max) and unbounded (hist_scale inf) channels included: the rule set on
    the device (Binner::set_rule) against the rule made on the host (make_rule)."""
    case, form, clip, bins = run
    p, x = _data(case)
    C = case.shape[case.axis]
    hs, scales, mins, maxs = R.scales_of(p, bins)
    assert scales[p.roles.dead] == 0 and np.isinf(scales[p.roles.unbounded]) and mins[p.roles.dead] == maxs[p.roles.dead]
    hist = torch.zeros(C, bins, dtype=torch.int32, device=DEV)
    _launch(CUDA, x, case.axis, form, clip, bins, _rules(p, bins), hist)
    xs = x.movedim(case.axis, 0).reshape(C, -1).contiguous()
    per_tensor = torch.zeros(C, bins, dtype=torch.int32, device=DEV)
    for c in range(C):
        if form == 'scales': CUDA.Histogram_T(xs[c], per_tensor[c], float(scales[c]), clip)
        else: CUDA.Histogram_Asymmetric_T(float(mins[c]), float(maxs[c]), xs[c], per_tensor[c], clip)
    _assert_equal(hist, per_tensor.cpu().numpy().astype(np.int64), R.run_id(run))
    _assert_equal(per_tensor, _want(case, form, clip, bins), 'per-tensor kernels, ' + R.run_id(run))


# ---- 5. the observers that these kernels feed -----------------------------------------------------------------------------------
def _cfg(alg, sym=True, per_channel_axis=None, bins=None):
    from ppq_amd import LinearQuantizationConfig
    qmin, qmax = (-128, 127) if sym else (0, 255)
    c = LinearQuantizationConfig(symmetrical=sym, quant_min=qmin, quant_max=qmax, num_of_bits=8, calibration=alg,
                                 channel_axis=per_channel_axis, power_of_2=False)
    if bins: c.detail['OBSERVER_KL_HIST_BINS_MANUL_OVERRIDE'] = bins
    return c


def _outcome(ob, cfg):
    """What the last render does: ('raises', exception type) or ('ok', scales, offsets) as float32 bit patterns."""
    try:
        ob.render_quantization_config()
    except Exception as e:                                                  # noqa: BLE001 -- the type IS the result
        return ('raises', type(e).__name__)
    s = np.atleast_1d(cfg.scale.detach().cpu().numpy().astype(np.float32))
    o = np.atleast_1d(cfg.offset.detach().cpu().numpy().astype(np.float32))
    return ('ok', s.view(np.uint32).tolist(), o.view(np.uint32).tolist())


def _calibrate(alg, sym, axis, batches, bins):
    from ppq_amd.observer import TensorObserverFactroy
    cfg = _cfg(alg, sym, axis, bins)
    ob = TensorObserverFactroy.build_observer('x', cfg)
    for d in batches: ob.observe(d)
    ob.render_quantization_config()                                          # ranges -> histogram phase
    for d in batches: ob.observe(d)
    return ob, cfg, _outcome(ob, cfg)


@pytest.mark.parametrize('shape,count', [((2, 5, 6160), 2), ((1, 256, 4164), 1)], ids=['split_rows', 'tile_and_rest'])
@pytest.mark.parametrize('alg,sym', [('kl', True), ('mse', True), ('mse', False)], ids=['kl', 'mse_sym', 'mse_asym'])
def test_channelwise_observers_on_split_rows_and_a_dead_channel(CUDA, alg, sym, shape, count):
    """'kl_channel' / 'mse_channel' over batches whose rows are split over workgroups (and run full tiles), one channel all zero:
    the observer's histogram is the numpy reference summed over the batches, and every channel gets the (scale, offset) the
    per-tensor observer renders on that channel's slice.  The dead channel (hist_scale 0, min == max) is held to whatever the
    per-tensor observer does with it: on an MI355X both render, for kl and for mse symmetric and asymmetric, the finite floor
    scale 1e-8 (OBSERVER_MIN_SCALE) with offset 0 and neither raises -- the assertion at the end pins that."""
    host = R.observer_batches(shape, count, seed=7)
    batches = [torch.from_numpy(b).to(DEV) for b in host]
    C, DEAD = shape[1], 1
    bins = 2048
    ob, cfg, got = _calibrate(alg + '_channel', sym, 1, batches, bins if alg == 'kl' else None)
    assert ob._hist_bins == bins
    # the histogram against the reference, with the rules worked out from the data alone
    lo = np.min([R.channel_slices(b, 1).min(axis=1) for b in host], axis=0).astype(np.float32)
    hi = np.max([R.channel_slices(b, 1).max(axis=1) for b in host], axis=0).astype(np.float32)
    if sym:
        scales = np.array([max(abs(float(h)), abs(float(l))) / bins for l, h in zip(lo, hi)]).astype(np.float32)
        want = sum(R.hist_c(b, 1, bins, True, 'scales', scales=scales) for b in host)
        assert scales[DEAD] == 0
    else:
        want = sum(R.hist_c(b, 1, bins, True, 'ranges', mins=lo, maxs=hi) for b in host)
        assert lo[DEAD] == 0 and hi[DEAD] == 0
    _assert_equal(ob.histogram(), want, (alg, sym, shape))
    assert want[DEAD, 0] == sum(b.size for b in host) // C
    # every channel against the per-tensor observer on its slice
    per = [_calibrate(alg, sym, None, [d[:, c].contiguous() for d in batches], bins if alg == 'kl' else None)[2] for c in range(C)]
    dead = per[DEAD]
    print(f'dead channel, {alg} sym={sym} {shape}: per tensor {dead}, per channel {got[0]} '
          f'{(got[1][DEAD], got[2][DEAD]) if got[0] == "ok" else got[1]}')
    assert got[0] == dead[0], (got[:2], dead)
    if dead[0] == 'raises':                      # both refuse: the same exception, and only the dead channel is the reason
        assert got[1] == dead[1] and all(per[c][0] == 'ok' for c in range(C) if c != DEAD), (got, dead)
        return
    for c in range(C):
        assert per[c][0] == 'ok' and (got[1][c], got[2][c]) == (per[c][1][0], per[c][2][0]), (c, got[1][c], per[c])
    dead_scale = np.array(got[1][DEAD], np.uint32).view(np.float32)
    assert np.isfinite(dead_scale) and dead_scale == np.float32(1e-8), dead_scale       # OBSERVER_MIN_SCALE: the recorded behaviour
