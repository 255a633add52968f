"""GPU tests of the channelwise split: the plan and gather kernels (csrc/split.hip) and the pass that drives them
(ppq_amd/channel_split.py) against the reference's recorded masks and parameters (tests/golden/channel_split.npz, written on the
CPU by tests/golden/make_channel_split.py), against numpy / torch on the CPU for synthetic jobs, and against the torch arm on
the device."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import channel_split_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DRIFT_FACTOR = 4                     # times the reference's own recorded drift: see test_graph_outputs_are_preserved_on_the_device
INVALID_VALUE = -1                   # PPQHIP_ERR_INVALID_VALUE
RESNET_THRESHOLD = 0.2               # He-initialised weights: the reference's default of 2 splits nothing there


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'channel_split.npz')))


@pytest.fixture(scope='module')
def book():
    with open(os.path.join(HERE, 'golden', 'channel_split.json')) as f: return json.load(f)


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same(a, b) -> bool:
    """Same shape and bit equality; NaN equals NaN whatever its payload (the nan_key case)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)): return False
    keep = ~np.isnan(a)
    return np.array_equal(_bits(a[keep]), _bits(b[keep]))


def _to_device(g):
    for v in g.variables.values():
        if v.is_parameter: v.value = v.value.to(DEV)
    return g


def _case_graph(golden, k, at: str = 'init'):
    """Case k on the device with the recorded parameters of `at` ('init' or 'it<n>')."""
    params = {n[len(f'c{k}_{at}_'):]: torch.from_numpy(v.copy()) for n, v in golden.items() if n.startswith(f'c{k}_{at}_')}
    return _to_device(CC.harness_graph(k, params))


def _activations(golden, k):
    case = CC.CASES[k]
    if not case['including_act']: return None
    out = []
    for it in range(1, case['iterations'] + 1):
        pre = f'c{k}_act_it{it}_'
        out.append({n[len(pre):]: torch.from_numpy(v).to(DEV) for n, v in golden.items() if n.startswith(pre)})
    return out


def _pass(k, **kw):
    from ppq_amd.channel_split import ChannelwiseSplitPass
    case = CC.CASES[k]
    return ChannelwiseSplitPass(iterations=case['iterations'], threshold=case['threshold'], including_bias=case['including_bias'],
                                including_act=case['including_act'], **kw)


def _plan(item_of, sizes):
    """The plans of len(sizes) jobs in ONE call: item_of(k, src_of, count) builds job k.  Returns the counts and the plans
    (cut at their counts) on the host and the whole plan buffers on the device; the buffers are poisoned first."""
    from ppq_amd import ffi
    plans = [torch.full((2 * C,), -7, dtype=torch.int32, device=DEV) for C in sizes]
    counts = torch.full((len(sizes),), -7, dtype=torch.int32, device=DEV)
    ffi.split_plan_multi([item_of(k, plans[k], counts[k:k + 1]) for k in range(len(sizes))])
    counts = counts.tolist()
    return counts, [p[:n].cpu().numpy() for p, n in zip(plans, counts)], plans


def _expected_plan(mask) -> np.ndarray:
    """numpy.cumsum: entry d[c] = exclusive prefix sum of 1 + mask holds c, and so does d[c] + 1 where mask[c], bit 31 on both."""
    mask = np.asarray(mask).astype(np.int64)
    width = 1 + mask
    d = np.cumsum(width) - width
    out = np.zeros(int(width.sum()), dtype=np.int64)
    c = np.arange(mask.size)
    out[d] = c | (mask << 31)
    out[(d + 1)[mask == 1]] = c[mask == 1] | (1 << 31)
    return out.astype(np.uint32).view(np.int32)


@pytest.mark.parametrize('k', range(len(CC.CASES)))
def test_plan_kernel_equals_the_recorded_masks(golden, book, k):
    """Every split pair of every case in every iteration: the parameters the reference had BEFORE the step go in, count and plan
    of its recorded mask must come out.  (Within an iteration pair q sees what the pairs before it did: the recorded state is
    per iteration, so the pairs are walked in order and each plan is applied with the gather kernel; the parameters after the
    iteration must then be the recorded ones.)"""
    from ppq_amd import ffi
    from ppq_amd.channel_split import split_tensors
    case = CC.CASES[k]
    acts = _activations(golden, k)
    info = book['cases'][case['name']]
    for it in range(1, case['iterations'] + 1):
        g = _case_graph(golden, k, 'init' if it == 1 else f'it{it - 1}')
        p = _pass(k)
        pairs = p.find_equalization_pair(g, p.interested_operations(g))
        if acts: p.activations = acts[it - 1]
        for q, pair in enumerate(pairs):
            if q in info['skipped']: continue
            want = golden[f'c{k}_mask_it{it}_p{q}']
            C = pair.num_channel()
            assert C == want.size
            counts, plans, raw = _plan(lambda _, s, c: p.plan_items(pair, s, c), [C])
            assert counts[0] == int(want.sum()) + C, (case['name'], it, q)
            assert np.array_equal(plans[0], CC.split_map(want)) and np.array_equal(plans[0], _expected_plan(want)), (case['name'], it, q)
            if counts[0] == C: continue
            jobs = []
            for var, axis in split_tensors(pair):
                x = var.value
                out = torch.empty(x.shape[:axis] + (counts[0],) + x.shape[axis + 1:], device=DEV)
                jobs.append((x, out, raw[0], C, counts[0], int(np.prod(x.shape[axis + 1:], dtype=np.int64))))
                var.value = out
            ffi.split_apply_multi(jobs)
        for v in g.variables.values():
            if v.is_parameter: assert _same(v.value, golden[f'c{k}_it{it}_{v.name}']), (case['name'], it, v.name)


def _mask_job(mask: np.ndarray, threshold: float = 0.5, extra: bool = False):
    """A synthetic pair whose mask is `mask`: upstream key 1 where set (0.25 elsewhere), downstream key 1 everywhere (`extra`: a
    second downstream segment under the threshold)."""
    up = torch.from_numpy(np.where(mask, 1.0, 0.25).astype(np.float32)).to(DEV)
    down = torch.ones(mask.size, device=DEV)
    segments = [(up, 1, 1, 0, 1, 0, 1, 1.0, False), (down, 1, 1, 0, 1, 0, 1, 1.0, True)]
    if extra: segments.append((down, 1, 1, 0, 1, 0, 1, 0.125, True))
    return lambda _, s, c: (s, c, threshold, segments)


@pytest.mark.parametrize('density', [0.3, 0.0, 1.0])
def test_plan_kernel_scan_crosses_chunk_carries(density):
    """C = 600: three chunks of 256 channels, two carries; a random mask, the all-false and the all-true one."""
    C = 600
    mask = np.random.default_rng(11).random(C) < density
    if density == 0.3: assert 120 < mask.sum() < 240
    else: assert mask.sum() == int(density) * C
    counts, plans, _ = _plan(_mask_job(mask), [C])
    assert counts[0] == C + int(mask.sum())
    assert np.array_equal(plans[0], _expected_plan(mask))


def test_plan_kernel_chunks_its_table():
    """70 jobs -- 30 of 3 segments, then 40 of 2 -- in ONE call equal the single-job calls: the first launch is full at 72
    segments (24 jobs), the second at 32 jobs (70 segments), the third takes the rest."""
    from ppq_amd import ffi
    rng = np.random.default_rng(3)
    sizes = [int(rng.integers(5, 300)) for _ in range(70)]
    masks = [rng.random(C) < 0.4 for C in sizes]
    makers = [_mask_job(m, extra=k < 30) for k, m in enumerate(masks)]
    counts, plans, _ = _plan(lambda k, s, c: makers[k](k, s, c), sizes)
    for k in range(len(sizes)):
        one_count, one_plan, _ = _plan(makers[k], [sizes[k]])
        assert counts[k] == one_count[0] == sizes[k] + int(masks[k].sum())
        assert np.array_equal(plans[k], one_plan[0]) and np.array_equal(plans[k], _expected_plan(masks[k])), k
    items = [makers[k](k, None, None) for k in range(len(sizes))]
    assert ffi.split_plan_launches(items) == 2 * 3 and ffi.split_plan_launches(items[:1]) == 2


C_APPLY = 7
APPLY_KINDS = [                                                            # (shape, channel axis): the view table of include/ppq_hip.h
    ((C_APPLY, 3, 3, 3), 0), ((C_APPLY, 4, 1, 1), 0), ((C_APPLY, 1, 3, 3), 0), ((C_APPLY, 1, 1, 1), 0),     # upstream Conv: run 27, 4, 9, 1
    ((C_APPLY,), 0),                                                                                         # bias
    ((5, C_APPLY), 1),                                                                                       # upstream Gemm stored [I, O]
    ((6, C_APPLY, 3, 3), 1), ((6, C_APPLY, 2, 2), 1), ((6, C_APPLY, 1, 1), 1), ((3, C_APPLY, 3, 9), 1),     # downstream Conv: run 9, 4, 1, 27
    ((9, C_APPLY), 1),                                                                                       # downstream Gemm [O, I]
    ((C_APPLY, 12), 0), ((C_APPLY, 27), 0), ((C_APPLY, 9), 0)]                                               # downstream Gemm [I, O]


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_apply_kernel_equals_torch_for_every_tensor_kind_and_pointer_offset(offset):
    """index_select and ONE fp32 multiply on the CPU are the reference.  Every tensor kind, run in {1, 4, 9, 27}, the source
    `offset` floats off 16 bytes and the destination 0, 1, 2 and 3 floats off: 56 jobs (more than one launch holds) in ONE call.
    Unsplit channels are the source's bits."""
    from ppq_amd import ffi
    gen = torch.Generator().manual_seed(70 + offset)
    mask = np.array([1, 0, 0, 1, 1, 0, 1], dtype=bool)
    plan = CC.split_map(mask)
    count = plan.size
    src_of = torch.from_numpy(plan).to(DEV)

    def place(t, off, fill=None):
        buf = torch.full((t.numel() + 8,), -7.0, device=DEV)
        v = buf[off:off + t.numel()].view(t.shape)
        if fill is None: v.copy_(t)
        assert v.data_ptr() % 16 == (4 * off) % 16
        return v, buf
    jobs, wants, guards = [], [], []
    for shape, axis in APPLY_KINDS:
        for out_offset in range(4):
            x = torch.randn(shape, generator=gen)
            want = CC.split_reference(x, plan, axis)
            out, buf = place(want, out_offset, fill=False)
            jobs.append((place(x, offset)[0], out, src_of, C_APPLY, count, int(np.prod(shape[axis + 1:], dtype=np.int64))))
            wants.append((want, x, axis)); guards.append((buf, out_offset, want.numel()))
    assert len(jobs) > 32 and {j[5] for j in jobs} >= {1, 4, 9, 27}
    ffi.split_apply_multi(jobs)
    single = torch.from_numpy(np.flatnonzero(plan >= 0))
    for (_, out, *_), (want, x, axis), (buf, off, n) in zip(jobs, wants, guards):
        assert _same(out, want), (tuple(x.shape), off)
        assert _same(out.cpu().index_select(axis, single), x.index_select(axis, torch.from_numpy(plan[plan >= 0].astype(np.int64))))
        assert bool((buf[:off] == -7).all()) and bool((buf[off + n:] == -7).all()), (tuple(x.shape), off)      # nothing written around it


def test_library_refuses_bad_apply_jobs_without_launching():
    from ppq_amd import ffi
    from ppq_amd._lib import last_error
    C, run = 8, 9
    plan = CC.split_map(np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=bool))
    src_of = torch.from_numpy(plan).to(DEV)
    buf = torch.full((400,), -7.0, device=DEV)
    x = buf[:C * run]
    stream = torch.cuda.current_stream().cuda_stream

    def status(item):
        t = ffi.split_apply_table([item])
        return t.entry(t.jobs.ctypes.data, 1, stream)
    far = torch.full((10 * run,), -7.0, device=DEV)
    assert status((x, buf[40:40 + 10 * run], src_of, C, 10, run)) == INVALID_VALUE and 'overlaps an input' in last_error()
    assert status((x, far[:7 * run], src_of, C, 7, run)) == INVALID_VALUE and 'count 7 is outside' in last_error()
    assert status((x, far, src_of, C, 17, run)) == INVALID_VALUE and 'count 17 is outside' in last_error()
    assert status((x, far, src_of, 5, 10, run)) == INVALID_VALUE and 'bad geometry' in last_error()          # 72 % (5 * 9) != 0
    assert status((x, far, src_of, C, 10, 1 << 62)) == INVALID_VALUE and 'bad geometry' in last_error()      # a run the product would overflow with
    t = ffi.split_apply_table([(x, far, src_of, C, 10, run), (x, far, src_of, C, 10, run)])
    assert t.entry(t.jobs.ctypes.data, 2, stream) == INVALID_VALUE and 'two outputs overlap' in last_error()
    with pytest.raises(RuntimeError, match='count 7 is outside'): ffi.split_apply_multi([(x, far[:7 * run], src_of, C, 7, run)])
    with pytest.raises(RuntimeError, match='not on the GPU'): ffi.split_apply_multi([(x.cpu(), far, src_of, C, 10, run)])
    torch.cuda.synchronize()
    assert bool((buf == -7).all()) and bool((far == -7).all())              # nothing was launched
    up = torch.ones(C, device=DEV)
    plan_buf, cnt = torch.zeros(2 * C, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='upstream and a downstream'):
        ffi.split_plan_multi([(plan_buf, cnt, 0.5, [(up, 1, 1, 0, 1, 0, 1, 1.0, False)])])
    with pytest.raises(RuntimeError, match='reads element'):
        ffi.split_plan_multi([(plan_buf, cnt, 0.5, [(up, 1, 2, 0, 1, 0, 1, 1.0, False), (up, 1, 1, 0, 1, 0, 1, 1.0, True)])])
    with pytest.raises(RuntimeError, match='an output overlaps an input'):                                # the plan inside a key tensor
        ffi.split_plan_multi([(plan_buf, cnt, 0.5, [(up, 1, 1, 0, 1, 0, 1, 1.0, False), (plan_buf.view(torch.float32), 1, 1, 0, 1, 0, 1, 1.0, True)])])
    with pytest.raises(RuntimeError, match='two outputs overlap'):
        ffi.split_plan_multi([(plan_buf, plan_buf[3:4], 0.5, [(up, 1, 1, 0, 1, 0, 1, 1.0, False), (up, 1, 1, 0, 1, 0, 1, 1.0, True)])])


@pytest.mark.parametrize('schedule', ['levelled', 'sequential'])
@pytest.mark.parametrize('k', range(len(CC.CASES)))
def test_pass_with_kernels_equals_the_goldens_and_the_torch_arm(golden, book, k, schedule):
    """The kernel arm on the device against the recorded masks and parameters and against the torch arm on the device, bit for
    bit; and its launches and copies: per level the plan's two launches and ONE copy, one gather launch more where the level
    splits something."""
    case = CC.CASES[k]
    info = book['cases'][case['name']]
    g = _case_graph(golden, k)
    before = {n: v.value for n, v in g.variables.items() if v.is_parameter}
    p = _pass(k, schedule=schedule)
    p.keep_masks = True
    p.optimize(g, dataloader=[], executor=None, activations=_activations(golden, k))
    recorded = {n: v for n, v in golden.items() if n.startswith(f'c{k}_mask_')}
    assert {f'c{k}_mask_it{it + 1}_p{q}' for it, q in p.masks} == set(recorded)
    for (it, q), m in p.masks.items():
        assert np.array_equal(m.cpu().numpy().astype(np.uint8), recorded[f'c{k}_mask_it{it + 1}_p{q}']), (case['name'], it, q)
    for v in g.variables.values():
        if v.is_parameter:
            assert _same(v.value, golden[f'c{k}_it{case["iterations"]}_{v.name}']), (case['name'], v.name)
            assert v.value.is_contiguous() and v.value.is_cuda
    t = _case_graph(golden, k)
    pt = _pass(k, schedule=schedule, use_kernels=False)
    pt.optimize(t, dataloader=[], executor=None, activations=_activations(golden, k))
    for name, v in g.variables.items():
        if v.is_parameter: assert _same(v.value, t.variables[name].value), (case['name'], name)
    for key in ('pairs', 'skipped_pairs', 'levels', 'channels_before', 'channels_after', 'split_channels'): assert p.stats[key] == pt.stats[key], key
    assert pt.stats['launches'] == 0 and pt.stats['copies'] == 0
    # launch accounting: the schedule the pass walked, rebuilt here; a level is the plan's two launches and ONE copy, and one
    # gather launch more where a recorded mask of one of its pairs splits something (tables this small are never chunked)
    from ppq_amd.equalization import build_schedule
    active = [q for q in range(len(info['pairs'])) if q not in info['skipped']]
    active_pairs = [p.pairs[q] for q in active]
    if case['including_act']:
        walked = [[(it, active[q]) for _, q in level] for it in range(case['iterations']) for level in build_schedule(active_pairs, 1, schedule)]
    else: walked = [[(it, active[q]) for it, q in level] for level in build_schedule(active_pairs, case['iterations'], schedule)]
    splitting = sum(any(recorded[f'c{k}_mask_it{it + 1}_p{q}'].any() for it, q in level) for level in walked)
    levels = p.stats['levels']
    assert levels == len(walked) and p.stats['copies'] == levels and p.stats['launches'] == 2 * levels + splitting
    if schedule == 'sequential': assert levels == case['iterations'] * len(active)
    if not any(v.any() for v in recorded.values()):                        # grouped, no_split: no gather launch, the same objects
        assert p.stats['launches'] == 2 * levels
        for n, x in before.items(): assert g.variables[n].value is x, n
    if case['name'] == 'chain':                                            # pair 0 never splits: c1's tensors stay the objects they were
        assert g.variables['c1_w'].value is before['c1_w'] and g.variables['c1_b'].value is before['c1_b']
        assert g.variables['c2_w'].value is not before['c2_w']


def test_kernel_arm_refuses_what_it_cannot_read(golden):
    g = _case_graph(golden, 0)
    g.variables['c2_w'].value = g.variables['c2_w'].value.double()
    with pytest.raises(TypeError, match='must be a contiguous float32 tensor for the kernels'): _pass(0).optimize(g)
    g = _case_graph(golden, 0)
    g.variables['c3_w'].value = g.variables['c3_w'].value.cpu()
    with pytest.raises(TypeError, match='partly on the GPU and partly not'): _pass(0).optimize(g)


@pytest.mark.parametrize('k', [k for k, c in enumerate(CC.CASES) if c['executable']])
def test_graph_outputs_are_preserved_on_the_device(golden, book, k):
    """Graph outputs on the recorded batch before and after the kernel arm: max |after - before| / max |before| within 4 x the
    drift of the REFERENCE's own outputs on the CPU (channel_split.json).  Why 4: the device's convolutions sum in another order
    than the CPU's, and the channel count -- the summation length -- grows by up to 2 x per iteration; a judgement, not a
    measurement.  A case in which nothing splits recorded 0: its tensors stay the same objects and the outputs must repeat."""
    from ppq_amd import harness
    case = CC.CASES[k]
    g = CC.harness_graph(k)
    ex = harness.TorchExecutor(g, DEV)
    x = torch.from_numpy(golden[f'c{k}_x']).to(DEV)
    before = [y.clone() for y in ex.forward(x)]
    p = _pass(k)
    p.optimize(g, dataloader=[b.to(DEV) for b in CC.case_batches(k)], executor=ex, activations=_activations(golden, k))
    assert p.stats['split_channels'] == [int(sum(v.sum() for n, v in golden.items() if n.startswith(f'c{k}_mask_it{it}_')))
                                         for it in range(1, case['iterations'] + 1)]
    bound = DRIFT_FACTOR * book['cases'][case['name']]['drift']
    for y0, y1 in zip(before, ex.forward(x)):
        drift = float((y1 - y0).abs().max() / y0.abs().max())
        print(case['name'], 'drift', drift, 'bound', bound)
        assert y1.shape == y0.shape and drift <= bound, (case['name'], drift, bound)


def test_own_collection_on_the_device_is_one_launch_per_forward(golden):
    """including_act without maxima handed in: collected at the start of every iteration on the graph as it then is, ONE
    per-channel min/max launch per forward, nothing written into the graph."""
    from ppq_amd import harness
    k = [c['name'] for c in CC.CASES].index('zero_act')
    g = CC.harness_graph(k)
    ex = harness.TorchExecutor(g, DEV)
    batches = [b.to(DEV) for b in CC.case_batches(k)]
    p = _pass(k)
    p.optimize(g, dataloader=batches, executor=ex)
    assert p.stats['collect_launches'] == 2 * len(batches) and p.stats['copies'] == p.stats['levels']
    assert p.activations['c1_out'].numel() == 10                          # the second collection saw the first split
    assert sum(p.stats['split_channels']) > 0 and p.stats['channels_after'] == p.stats['channels_before'] + sum(p.stats['split_channels'])
    assert all(v.value is None for v in g.variables.values() if not v.is_parameter)
    assert all(torch.isfinite(y).all() for y in ex.forward(batches[0]))


def test_resnet50_kernel_arm_equals_torch_arm_on_the_device():
    """Real sizes: pairs of up to 2048 channels (eight scan chunks), tables of more than one launch, 16-byte and 4-byte gathers.
    One iteration at a threshold under which He-initialised weights split."""
    from ppq_amd import harness
    from ppq_amd.channel_split import ChannelwiseSplitPass
    graphs, stats = {}, {}
    for arm, kw in (('torch', dict(use_kernels=False)), ('levelled', dict(schedule='levelled')), ('sequential', dict(schedule='sequential'))):
        g = _to_device(harness.resnet50_graph(num_classes=10))
        p = ChannelwiseSplitPass(iterations=1, threshold=RESNET_THRESHOLD, including_bias=True, **kw)
        p.optimize(g, dataloader=[], executor=None)
        graphs[arm], stats[arm] = g, p.stats
    print('resnet50', stats['levelled'])
    assert 0 < stats['levelled']['split_channels'][0] < stats['levelled']['channels_before']
    assert stats['levelled']['levels'] < stats['sequential']['levels'] and stats['levelled']['copies'] == stats['levelled']['levels']
    for name, v in graphs['levelled'].variables.items():
        if not v.is_parameter: continue
        assert _same(v.value, graphs['sequential'].variables[name].value), name
        assert _same(v.value, graphs['torch'].variables[name].value), name
    for key in ('pairs', 'skipped_pairs', 'channels_before', 'channels_after', 'split_channels'): assert stats['levelled'][key] == stats['torch'][key], key
    ex = harness.TorchExecutor(graphs['levelled'], DEV)
    assert all(torch.isfinite(y).all() for y in ex.forward(torch.rand(1, 3, 64, 64, device=DEV)))

