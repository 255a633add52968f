"""The error analysis on the GPU: the three launches of csrc/measure.hip against float64 / index_select, the measures and the
recorder against the reference's recorded values (tests/golden/analyse.npz), the two analyses end to end against torch
restatements, and what they launch and copy."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import analyse_cases as C  # noqa: E402

GOLD = np.load(os.path.join(HERE, 'golden', 'analyse.npz'))
DEV = 'cuda:0'


def _misaligned(t: torch.Tensor, floats: int = 1) -> torch.Tensor:
    """The same values in a contiguous tensor whose first element sits `floats` * 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = buf[floats:floats + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * floats and view.is_contiguous()
    return view


def _pair(rows, count, seed):
    gen = torch.Generator().manual_seed(seed)
    real = (torch.randn(rows, count, generator=gen) * 1.5 + 0.25).to(DEV)
    return real + (torch.randn(rows, count, generator=gen) * 0.05).to(DEV), real


def _expected_sums(p, r):
    """The float64 sums of the SAME fp32 terms: one fp32 operation each, as torch computes them elementwise."""
    d = p - r
    return torch.stack([(d * d).double().sum(1), (r * r).double().sum(1), (p * p).double().sum(1), (p * r).double().sum(1)], dim=1)


def _check_sums(got, p, r, count, what):
    want = _expected_sums(p, r).cpu().numpy()
    got = got.cpu().numpy()
    assert got.shape == want.shape, what
    rel = count * 2.0 ** -52
    for k in range(3):
        assert (np.abs(got[:, k] - want[:, k]) <= rel * want[:, k]).all(), (what, k, got[:, k], want[:, k])
    assert (np.abs(got[:, 3] - want[:, 3]) <= rel * np.sqrt(want[:, 2] * want[:, 1])).all(), (what, got[:, 3], want[:, 3])


# (rows, count): one-wave rows (<= 1024), one-workgroup rows (<= 8192), split rows; row lengths that are no multiple of 4 put
# every row but the first off the 16-byte grid
DENSE = [(5, 1000), (3, 37), (1, 1024), (7, 1023), (4, 4096), (1, 1025), (3, 8192), (6, 4099), (2, 100352), (1, 8193), (3, 20003),
         (1, 802816), (5, 1), (9, 9000), (6, 140000)]


@pytest.mark.parametrize('rows,count', DENSE)
def test_dense_row_sums_against_float64(rows, count):
    from ppq_amd import ffi
    p, r = _pair(rows, count, 10 * rows + count)
    got = ffi.measure_rows_multi([(p, r, None)])[0]
    _check_sums(got, p, r, count, 'aligned')
    again = ffi.measure_rows_multi([(p, r, None)])[0]
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                 # identical bits on a second run
    # the element -> lane assignment does not depend on the pointers: tensors that start off the 16-byte grid give the same bits
    for shift_p, shift_r in ((1, 1), (3, 2), (0, 1)):
        moved = ffi.measure_rows_multi([(_misaligned(p, shift_p) if shift_p else p, _misaligned(r, shift_r), None)])[0]
        assert torch.equal(got.view(torch.int64), moved.view(torch.int64)), (shift_p, shift_r)


# (rows, row_len, count): gathered p -- one-wave, one-workgroup (the analysis' 4096 samples) and split index tables, more
# fetches than elements, a table off the 16-byte grid
GATHERED = [(3, 5000, 512), (4, 150528, 4096), (2, 7, 4096), (1, 802816, 4096), (2, 1000, 10001), (3, 4096, 1024), (32, 100352, 4096)]


@pytest.mark.parametrize('rows,row_len,count', GATHERED)
def test_gathered_row_sums_against_float64(rows, row_len, count):
    from ppq_amd import analyse, ffi
    x, _ = _pair(rows, row_len, rows + row_len)
    index = analyse.device_indexer(count, row_len, 10086, torch.device(DEV))
    assert index.dtype == torch.int32 and int(index.max()) < row_len
    p = x.index_select(1, index.long())
    r = p + (torch.randn(rows, count, generator=torch.Generator().manual_seed(count)) * 0.05).to(DEV)
    got = ffi.measure_rows_multi([(x, r, index)])[0]
    _check_sums(got, p, r, count, 'gathered')
    assert torch.equal(got.view(torch.int64), ffi.measure_rows_multi([(x, r, index)])[0].view(torch.int64))
    assert torch.equal(got.view(torch.int64), ffi.measure_rows_multi([(p, r, None)])[0].view(torch.int64))      # fused fetch == fetch, then dense
    off = torch.empty(count + 4, dtype=torch.int32, device=DEV)[1:count + 1]
    off.copy_(index)
    assert torch.equal(got.view(torch.int64), ffi.measure_rows_multi([(_misaligned(x), _misaligned(r, 2), off)])[0].view(torch.int64))


def test_many_jobs_cross_the_per_launch_limit():
    """More jobs than one launch's argument table holds (56 measure jobs, 80 fetch jobs), of every path, split jobs on both
    sides of the boundary: each job's result equals the one it gets alone."""
    from ppq_amd import analyse, ffi
    shapes = [(2, 100352), (3, 700)] + [(1 + k % 4, 50 + 37 * k) for k in range(52)] + [(2, 9000), (3, 4096), (2, 30000)] + \
             [(2, 300 + k) for k in range(30)] + [(1, 8193)]
    assert len(shapes) > 80
    items = []
    for k, (rows, count) in enumerate(shapes):
        p, r = _pair(rows, count, 500 + k)
        items.append((p, r, None))
    x, _ = _pair(3, 5000, 1)
    index = analyse.device_indexer(4096, 5000, 10086, torch.device(DEV))
    items.insert(55, (x, x.index_select(1, index.long()) * 1.01, index))
    items.insert(56, (x, x.index_select(1, index.long()) * 0.99, index))
    got = ffi.measure_rows_multi(items)
    for k, (item, g) in enumerate(zip(items, got)):
        alone = ffi.measure_rows_multi([item])[0]
        assert torch.equal(g.view(torch.int64), alone.view(torch.int64)), k
        if item[2] is None: _check_sums(g, item[0], item[1], item[1].shape[1], k)
    fetch_items = [(p, analyse.device_indexer(33 + k, p.shape[1], 10086, torch.device(DEV))) for k, (p, _, _) in enumerate(items)]
    for (x_k, index_k), out in zip(fetch_items, ffi.fetch_rows_multi(fetch_items)):
        assert torch.equal(out, x_k.index_select(1, index_k.long()))


@pytest.mark.parametrize('rows,row_len,count', [(4, 150528, 4096), (1, 7, 4096), (3, 1000, 1023), (2, 5000, 5), (5, 4096, 4097), (32, 802816, 4096)])
def test_fetch_rows_equals_index_select(rows, row_len, count):
    from ppq_amd import analyse, ffi
    x, _ = _pair(rows, row_len, row_len + count)
    index = analyse.device_indexer(count, row_len, 10086, torch.device(DEV))
    want = x.index_select(1, index.long())
    assert torch.equal(ffi.fetch_rows_multi([(x, index)])[0], want)
    assert torch.equal(analyse.batch_random_fetch(x.view(rows, 1, row_len), fetches_per_batch=count, seed=10086), want)
    out = _misaligned(torch.zeros(rows, count, device=DEV), 3)
    off = torch.empty(count + 4, dtype=torch.int32, device=DEV)[1:count + 1]
    off.copy_(index)
    ffi.fetch_rows_multi([(_misaligned(x, 2), off)], [out])
    assert torch.equal(out, want)


def test_the_three_launches_replay_from_a_hip_graph():
    """No upload, no synchronisation, no allocation inside the launches: fetch, fused measure (one-workgroup and split rows) and
    finish are captured once and replayed; the replays read the tensors as they are then and equal the eager results."""
    from ppq_amd import analyse, ffi
    side = torch.cuda.Stream()
    x, _ = _pair(4, 150528, 3)
    big_p, big_r = _pair(3, 50000, 4)
    index = analyse.device_indexer(4096, 150528, 10086, torch.device(DEV))
    fetched = torch.empty(4, 4096, device=DEV)
    sums = [torch.empty(4, 4, dtype=torch.float64, device=DEV), torch.empty(3, 4, dtype=torch.float64, device=DEV)]
    acc = torch.zeros(2, 2, dtype=torch.float64, device=DEV)

    def work():
        ffi.fetch_rows_multi([(x, index)], [fetched])
        ffi.measure_rows_multi([(x, fetched, index), (big_p, big_r, None)], sums)
        ffi.measure_finish_multi([(sums[0], 4096, acc[0], None), (sums[1], 50000, acc[1], None)], 'snr')
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side): work()                                   # eager once on the stream: its scratch is sized
    side.synchronize()
    eager_sums = [s.clone() for s in sums]
    assert float(eager_sums[0][:, 0].abs().max()) == 0.0                   # x against its own samples: no noise
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side): work()
    big_r.mul_(1.5)
    acc.zero_()
    graph.replay(); graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sums[0], eager_sums[0]) and not torch.equal(sums[1], eager_sums[1])
    assert torch.equal(sums[1].view(torch.int64), ffi.measure_rows_multi([(big_p, big_r, None)])[0].view(torch.int64))
    assert acc[:, 1].tolist() == [8.0, 6.0]                                # two replays, 4 and 3 rows each


def test_bad_arguments_are_errors():
    from ppq_amd import ffi
    p, r = _pair(2, 64, 0)
    index = torch.zeros(16, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError): ffi.measure_rows_multi([(p, r[:, :32].contiguous(), None)])
    with pytest.raises(RuntimeError): ffi.measure_rows_multi([(p, r, index)])
    with pytest.raises(RuntimeError): ffi.measure_rows_multi([(p.cpu(), r.cpu(), None)])
    with pytest.raises(RuntimeError): ffi.measure_rows_multi([(p.double(), r.double(), None)])
    with pytest.raises(RuntimeError): ffi.fetch_rows_multi([(p, index.long())])
    with pytest.raises(RuntimeError): ffi.measure_finish_multi([(torch.zeros(2, 4, device=DEV), 64, None, None)], 'snr')


# ---- measures and recorder against the reference's recorded values ----------------------------------------------------------
def _fn(method):
    from ppq_amd import measure
    return {'snr': measure.torch_snr_error, 'mse': measure.torch_mean_square_error, 'cosine': measure.torch_cosine_similarity}[method]


@pytest.mark.parametrize('method', C.METHODS)
@pytest.mark.parametrize('k', range(len(C.MEASURE_CASES)))
def test_measures_on_the_device_match_the_reference(k, method):
    from ppq_amd import measure
    name, shape = C.MEASURE_CASES[k]
    pred, real = (t.to(DEV) for t in C.measure_tensors(k))
    assert measure.kernel_path(pred, real)
    count = int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])
    rows_ref = GOLD[f'measure_{name}_{method}_none']
    got = _fn(method)(pred, real, 'none')
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == rows_ref.shape
    err = np.abs(got.cpu().numpy().astype(np.float64) - rows_ref)
    ulps = err / (2.0 ** -23 if method == 'cosine' else np.spacing(np.abs(rows_ref)))
    print(f'measure {name} {method}: count {count}, max difference {float(ulps.max()):.2f} fp32 ulps '
          f'({float((err / C.measure_bound(method, count, rows_ref)).max()):.2e} of the bound)')
    assert (err <= C.measure_bound(method, count, rows_ref)).all()
    for reduction in ('mean', 'sum'):
        want = float(GOLD[f'measure_{name}_{method}_{reduction}'])
        assert abs(float(_fn(method)(pred, real, reduction)) - want) <= C.reduced_bound(method, count, rows_ref, reduction)


@pytest.mark.parametrize('method', C.METHODS)
def test_all_zero_rows_are_exact(method):
    zero = torch.zeros(3, 5000, device=DEV)
    assert torch.equal(_fn(method)(zero, zero, 'none').cpu(), torch.zeros(3))            # snr 0, mse 0, cosine 0
    assert np.array_equal(_fn(method)(zero[:2, :64].contiguous(), zero[:2, :64].contiguous(), 'none').cpu().numpy(),
                          GOLD[f'measure_zero_{method}_none'])


@pytest.mark.parametrize('method', C.METHODS)
def test_measure_recorder_on_device_tensors(method):
    from ppq_amd.analyse import MeasureRecorder
    rec, stepwise, top = MeasureRecorder(method), MeasureRecorder(method), MeasureRecorder(method, reduce='max')
    want_mean, running_max, rows_seen, bound = GOLD[f'recorder_{method}_mean'], 0.0, 0, 0.0
    for i, batch in enumerate(C.RECORDER_BATCHES):
        pred, real = (t.to(DEV) for t in C.recorder_tensors(i))
        for r in (rec, stepwise, top): r.update(y_pred=pred, y_real=real)
        rows_ref = GOLD[f'recorder_{method}_rows_{i}']
        bound = (bound * rows_seen + C.reduced_bound(method, C.RECORDER_ROW, rows_ref, 'mean') * batch) / (rows_seen + batch)
        rows_seen += batch
        assert abs(stepwise.measure - want_mean[i]) <= bound + 1e-12 * abs(want_mean[i]), i
        assert stepwise.num_of_elements == rows_seen and stepwise.device_reads == i + 1
        running_max = max(running_max, float(rows_ref.max()))
        assert abs(top.measure - running_max) <= C.measure_bound(method, C.RECORDER_ROW, rows_ref).max()
    # nothing came back from the device until the value is asked for: the state says so
    assert rec.device_reads == 0 and rec._stale and rec._acc.is_cuda
    assert abs(rec.measure - want_mean[-1]) <= bound + 1e-12 * abs(want_mean[-1])
    assert rec.device_reads == 1 and rec.measure == rec.measure and rec.device_reads == 1
    assert rec.measure == stepwise.measure
    with pytest.raises(RuntimeError): rec.update(torch.zeros(2, 4), torch.zeros(2, 4))   # a device recorder takes no CPU tensor


# ---- end to end -------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _deterministic():
    """Repeatable forwards, so that two analyses see the same activations bit for bit: PyTorch's native convolutions instead of
    MIOpen (which does not repeat every convolution between calls) and PyTorch's deterministic algorithms."""
    prev = (torch.backends.cudnn.enabled, torch.are_deterministic_algorithms_enabled(),
            torch.is_deterministic_algorithms_warn_only_enabled())
    torch.backends.cudnn.enabled = False
    torch.use_deterministic_algorithms(True, warn_only=True)
    try: yield
    finally:
        torch.backends.cudnn.enabled = prev[0]
        torch.use_deterministic_algorithms(prev[1], warn_only=prev[2])


def _calibrated(kind):
    from ppq_amd import harness
    from ppq_amd.calibration import RuntimeCalibrationPass
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(7)
    if kind == 'small_cnn':
        graph = harness.small_cnn_graph(seed=5, width=16)
        batches = [torch.rand(8 if i != 1 else 5, 3, 24, 24, generator=gen).to(DEV) for i in range(4)]
    else:
        graph = harness.resnet50_graph(seed=0)
        batches = [torch.rand(2, 3, 64, 64, generator=gen).to(DEV) for _ in range(3)]
    harness.quantize_graph(graph, 'minmax')
    ex = harness.TorchExecutor(graph, DEV)
    harness.ParameterQuantizePass().optimize(graph)
    RuntimeCalibrationPass(check_steps=False).optimize(graph, dataloader=batches, executor=ex, calib_steps=len(batches))
    return graph, ex, batches


def _bits(t): return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).numpy().copy()


def _snapshot(graph):
    snap = {}
    for op in graph.operations.values():
        for v in op.inputs:
            if v.is_parameter and isinstance(v.value, torch.Tensor):
                snap[('value', v.name)] = _bits(v.value)
                if v.stored_value is not None: snap[('stored', v.name)] = _bits(v.stored_value)
        if hasattr(op, 'config'):
            for i, (c, _) in enumerate(op.config_with_variable):
                snap[('state', op.name, i)] = (c.state, 'Stored State' in c.detail)
                if isinstance(c.scale, torch.Tensor): snap[('scale', op.name, i)] = _bits(c.scale)
                if isinstance(c.offset, torch.Tensor): snap[('offset', op.name, i)] = _bits(c.offset)
    return snap


def _assert_untouched(graph, snap):
    now = _snapshot(graph)
    assert now.keys() == snap.keys()
    for key, was in snap.items():
        assert np.array_equal(now[key], was) if isinstance(was, np.ndarray) else now[key] == was, key


class _Keep:
    """The restatement's hook: the whole first output after the output quantisation, as rows."""
    def __init__(self): self.value = None
    def pre_forward_hook(self, inputs, quant_inputs, quant_configs): return quant_inputs

    def post_forward_hook(self, outputs, quant_outputs, quant_configs):
        self.value = quant_outputs[0].clone().flatten(start_dim=1)
        return quant_outputs


def _whole_tensor_restatement(graph, ex, batches, method, steps):
    """The reference's two phases over WHOLE tensors with torch operations on the device, the running mean in Python."""
    from ppq_amd import harness, measure
    ops = [op for op in graph.operations.values() if hasattr(op, 'config') and op.type in harness.COMPUTING_OP]
    quantable = [op for op in graph.operations.values() if hasattr(op, 'config')]
    hooks = {op.name: _Keep() for op in ops}
    total, seen = {op.name: 0.0 for op in ops}, 0
    for idx, batch in enumerate(batches):
        for op in quantable: op.dequantize()
        ex.forward(inputs=batch, hooks=hooks)
        fp = {name: h.value for name, h in hooks.items()}
        for op in quantable: op.restore_quantize_state()
        ex.forward(inputs=batch, hooks=hooks)
        for name, h in hooks.items():
            total[name] += measure.reference_formula(method, h.value, fp[name], 'mean').item() * batch.shape[0]
        seen += batch.shape[0]
        if idx >= steps: break
    return {name: total[name] / seen for name in total}, {op.name: op.outputs[0] for op in ops}


@pytest.mark.parametrize('method', C.METHODS)
@pytest.mark.parametrize('kind', ['small_cnn', 'resnet50'])
def test_graphwise_analysis_with_kernels_against_torch(kind, method):
    from ppq_amd import analyse, harness
    graph, ex, batches = _calibrated(kind)
    snap = _snapshot(graph)
    rows = batches[0].shape[0]
    with _deterministic():
        ours = analyse.graphwise_error_analyse(graph, DEV, batches, method=method, steps=2, verbose=False, fetchs=4096, executor=ex)
        stats = dict(analyse.last_analysis_stats)
        _assert_untouched(graph, snap)
        torch_arm = analyse.graphwise_error_analyse(graph, DEV, batches, method=method, steps=2, verbose=False, fetchs=4096,
                                                    executor=ex, use_kernels=False)
        _assert_untouched(graph, snap)
        whole = analyse.graphwise_error_analyse(graph, DEV, batches, method=method, steps=2, verbose=False, fetchs=None, executor=ex)
        whole_stats = dict(analyse.last_analysis_stats)
        _assert_untouched(graph, snap)
        whole_want, _ = _whole_tensor_restatement(graph, ex, batches, method, 2)
        _assert_untouched(graph, snap)
    n_ops = sum(1 for op in graph.operations.values() if hasattr(op, 'config') and op.type in harness.COMPUTING_OP)
    assert list(ours) == list(torch_arm) == list(whole) == list(whole_want) and len(ours) == n_ops
    assert stats == {'forwards': 6, 'fetch_launches': 3, 'measure_launches': 3, 'finish_launches': 3, 'device_reads': 1}
    assert whole_stats == {'forwards': 6, 'fetch_launches': 0, 'measure_launches': 3, 'finish_launches': 3, 'device_reads': 1}
    worst = 0.0
    for name in ours:
        bound = C.analysis_bound(method, 4096, rows, torch_arm[name])
        worst = max(worst, abs(ours[name] - torch_arm[name]) / bound)
        assert abs(ours[name] - torch_arm[name]) <= bound, (name, ours[name], torch_arm[name])
        assert np.isfinite(ours[name]) and (method == 'cosine' or ours[name] > 0)
    print(f'graphwise {kind} {method}: sampled, worst difference {worst:.2e} of the bound')
    worst = 0.0
    shapes = {}
    with _deterministic(), torch.no_grad():
        hooks = {name: _Keep() for name in ours}
        ex.forward(inputs=batches[0], hooks=hooks)
        shapes = {name: h.value.shape[1] for name, h in hooks.items()}
    for name in whole:
        bound = C.analysis_bound(method, shapes[name], rows, whole_want[name])
        worst = max(worst, abs(whole[name] - whole_want[name]) / bound)
        assert abs(whole[name] - whole_want[name]) <= bound, (name, whole[name], whole_want[name], shapes[name])
    print(f'graphwise {kind} {method}: whole tensors, worst difference {worst:.2e} of the bound')


@pytest.mark.parametrize('method', C.METHODS)
def test_layerwise_analysis_with_kernels_against_torch(method):
    from ppq_amd import analyse
    graph, ex, batches = _calibrated('small_cnn')
    snap = _snapshot(graph)
    with _deterministic():
        ours = analyse.layerwise_error_analyse(graph, batches, running_device=DEV, method=method, steps=2, verbose=False, executor=ex)
        stats = dict(analyse.last_analysis_stats)
        _assert_untouched(graph, snap)
        torch_arm = analyse.layerwise_error_analyse(graph, batches, running_device=DEV, method=method, steps=2, verbose=False,
                                                    executor=ex, use_kernels=False)
        _assert_untouched(graph, snap)
    assert list(ours) == list(torch_arm) == ['c1', 'c2', 'fc']
    assert stats == {'forwards': 3 + 3 * 3, 'fetch_launches': 0, 'measure_launches': 9, 'finish_launches': 9, 'device_reads': 1}
    for name in ours:                                                          # the graph output: 10 logits per row
        assert abs(ours[name] - torch_arm[name]) <= C.analysis_bound(method, 10, batches[0].shape[0], torch_arm[name]), name
        assert method == 'cosine' or ours[name] > 0


def test_launches_and_copies_of_one_sampled_analysis(capsys):
    """Per forward: ONE fetch launch in phase 1, one measure and one finish launch in phase 2 (the library's own launch
    counters); one device-to-host copy, after the last forward."""
    from ppq_amd import _lib, analyse
    graph, ex, batches = _calibrated('small_cnn')
    analyse.graphwise_error_analyse(graph, DEV, batches, steps=0, verbose=False, executor=ex)        # warm: tables, scratch
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    try:
        got = analyse.graphwise_error_analyse(graph, DEV, batches, method='snr', steps=2, verbose=True, executor=ex)
    finally:
        torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 32)()
    n = _lib.lib.ppqhip_prof_collect(arr, 32)
    launches = {arr[i].name.decode(): arr[i].launches for i in range(n)}
    assert launches.get('fetch_rows', 0) == 3 and launches.get('measure_rows', 0) == 3 and launches.get('measure_finish', 0) == 3, launches
    assert analyse.last_analysis_stats['device_reads'] == 1 and analyse.last_analysis_stats['forwards'] == 6
    text = capsys.readouterr().out
    assert 'NOISE:SIGNAL POWER RATIO' in text and all(f'{name}:' in text for name in got)
