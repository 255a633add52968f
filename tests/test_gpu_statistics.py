"""The statistical reports on the GPU: the two kernels of csrc/stats.hip against float64 and against their own arithmetic
contract restated with elementwise torch operations, the recorded reference series (tests/golden/statistics.npz) on the
device, the reports end to end against their torch arms, and what they launch and copy.

Bounds (tests/golden/statistics_cases.py has the reasoning): min and max exact; mean_f and std_f within one float32 ulp of the
rounded float64 value plus the double accumulation error n * 2^-52; the sums of t^3 and t^4 within n * 2^-52 * sum |term| of
the float64 sum of the same fp32 terms; histogram counts equal to the bincount of the same fp32 position rule -- and, against
a CPU ``torch.histc``, at most the series' edge samples apart."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import statistics_cases as C  # noqa: E402
from test_gpu_analyse import _assert_untouched, _calibrated, _deterministic, _misaligned, _snapshot  # noqa: E402

GOLD = np.load(os.path.join(HERE, 'golden', 'statistics.npz'))
with open(os.path.join(HERE, 'golden', 'statistics.json')) as _f: BOOK = json.load(_f)
DEV = 'cuda:0'
SIZES = [1, 2, 63, 64, 65, 1024, 1025, 3072, 9216, 9217, 589824, 2359296 + 3]
DATA = ['normal', 'offset', 'constant', 'pair']


def _series(kind: str, n: int):
    """(p, r): the series is p (r None) or p - r."""
    gen = torch.Generator().manual_seed(1000 * DATA.index(kind) + n % 9973)
    if kind == 'normal': return (torch.randn(n, generator=gen) * 1.5 + 0.25).to(DEV), None
    if kind == 'offset': return (torch.randn(n, generator=gen, dtype=torch.float64) * 1e-2 + 1e4).float().to(DEV), None      # mean 1e4, std 1e-2
    if kind == 'constant': return torch.full([n], -3.75, device=DEV), None      # x - 1 and x + 1 are exact
    real = (torch.randn(n, generator=gen) * 1.5 + 0.25).to(DEV)
    return real + (torch.randn(n, generator=gen) * 0.05 + 0.01).to(DEV), real


def _moments(items, bins=0):
    from ppq_amd import ffi
    table = ffi.stat_table(len(items), bins, torch.device(DEV))
    return ffi.stat_moments_multi(items, table)


def _check_moments(rec: np.ndarray, x: torch.Tensor, what):
    """One record against float64 on the device: x is the float32 series itself."""
    n = x.numel()
    x64 = x.double()
    mean = float(x64.sum() / n)
    assert rec[2] == float(x.min()) and rec[3] == float(x.max()), (what, rec[2:4])
    bound = C.moment_bound(mean, n, scale=float(x64.abs().sum() / n))
    assert abs(float(rec[0]) - float(np.float32(mean))) <= bound, (what, 'mean', rec[0], mean, bound)
    if n == 1:
        assert math.isnan(rec[1]), (what, rec[1])
        return 0.0, 0.0
    std = math.sqrt(float(((x64 - mean) ** 2).sum() / (n - 1)))
    assert abs(float(rec[1]) - float(np.float32(std))) <= C.moment_bound(std, n), (what, 'std', rec[1], std)
    return abs(float(rec[0]) - mean) / C.ulp32(np.float32(mean)), abs(float(rec[1]) - std) / C.ulp32(np.float32(std)) if std > 0 else float(rec[1] != 0)


@pytest.mark.parametrize('kind', DATA)
@pytest.mark.parametrize('n', SIZES)
def test_moments_against_float64(n, kind):
    p, r = _series(kind, n)
    x = p if r is None else p - r
    table = _moments([(p, r)])
    rec = table.cpu().numpy()[0]
    worst = _check_moments(rec, x, (kind, n))
    if kind == 'constant': assert rec[0] == np.float32(-3.75) and (n == 1 or rec[1] == 0.0)
    if r is not None:
        d = p - r
        snr64 = float((d * d).double().sum() / ((r * r).double().sum() + 1e-7))
        assert abs(float(rec[6]) - snr64) <= C.snr_bound(snr64, n), (rec[6], snr64)
    else: assert rec[6] == 0.0
    assert rec[7] == 0.0
    print(f'moments {kind} n={n}: mean {worst[0]:.3f} ulp, std {worst[1]:.3f} ulp off float64')
    # identical bits on a second call, and for pointers off the 16-byte grid (each of p and r on its own offset)
    bits = table.view(torch.int32)
    assert torch.equal(bits, _moments([(p, r)]).view(torch.int32))
    for shift_p, shift_r in ((1, 1), (3, 2), (0, 1), (2, 0)):
        if r is None and shift_p == 0: continue
        moved = _moments([(_misaligned(p, shift_p) if shift_p else p, None if r is None else (_misaligned(r, shift_r) if shift_r else r))])
        assert torch.equal(bits, moved.view(torch.int32)), (shift_p, shift_r)


def _shape_restatement(x: torch.Tensor, rec: torch.Tensor, bins: int):
    """The contract of ppqhip_stat_shape_multi with elementwise torch operations on the device, from the record's own mean_f,
    std_f: the fp32 terms t3, t4 (each step one fp32 operation; the quotient through float64, which rounds to the IEEE
    quotient) and the counts of the position rule."""
    t = C.quotient32(x - rec[0], rec[1].expand_as(x))
    t2 = t * t
    return t2 * t, t2 * t2, C.position_bins(x, bins)


@pytest.mark.parametrize('kind', ['normal', 'constant', 'pair', 'grid'])
@pytest.mark.parametrize('bins', [32, 64])
@pytest.mark.parametrize('n', [1, 2, 65, 1024, 3072, 9217, 589824, 2359296 + 3])
def test_shape_kernel_against_its_contract(n, bins, kind):
    from ppq_amd import ffi
    if kind == 'grid':                                  # values on a coarse grid: many samples exactly on bin edges
        gen = torch.Generator().manual_seed(n)
        p, r = (torch.randint(-64, 65, [n], generator=gen).float() / 16.0).to(DEV), None
    else: p, r = _series(kind, n)
    x = p if r is None else p - r
    table = _moments([(p, r)], bins)
    before = table.clone()
    ffi.stat_shape_multi([(p, r)], table)
    assert torch.equal(table[:, :4].view(torch.int32), before[:, :4].view(torch.int32))          # the moments are only read
    rec = table[0]
    counts = ffi.stat_counts(table)[0].long()
    t3, t4, want_counts = _shape_restatement(x, rec, bins)
    assert int(counts.sum()) == n and torch.equal(counts, want_counts), (counts.tolist(), want_counts.tolist())
    if bool(x.min() == x.max()):
        assert int(counts[bins // 2]) == n              # lo - 1, hi + 1 (both exact here): the middle
        assert math.isnan(float(rec[4])) and math.isnan(float(rec[5]))
    elif n > 1:
        for got, terms, shift in ((rec[4], t3, 0.0), (rec[5], t4, 3.0)):
            want = float(terms.double().sum() / n)
            slack = n * 2.0 ** -52 * float(terms.double().abs().sum() / n)
            want32 = float(np.float32(np.float32(want) - np.float32(shift)))
            lo32 = float(np.float32(np.float32(want - slack) - np.float32(shift)))
            hi32 = float(np.float32(np.float32(want + slack) - np.float32(shift)))
            assert min(lo32, want32) <= float(got) <= max(hi32, want32), (kind, n, float(got), want32, slack)
    on_device = torch.histc(x, bins=bins, min=float(x.min()), max=float(x.max()))
    print(f'shape {kind} n={n} bins={bins}: torch.histc on the device '
          f'{"equal" if torch.equal(on_device.long(), counts) else "differs in " + str(int((on_device.long() - counts).abs().sum()) // 2) + " samples"}')
    again = _moments([(p, r)], bins)
    ffi.stat_shape_multi([(p, r)], again)
    assert torch.equal(again.view(torch.int32), table.view(torch.int32))
    if n > 4:
        moved = _moments([(_misaligned(p, 3), None if r is None else _misaligned(r, 1))], bins)
        ffi.stat_shape_multi([(_misaligned(p, 3), None if r is None else _misaligned(r, 1))], moved)
        assert torch.equal(moved.view(torch.int32), table.view(torch.int32))


def test_many_series_cross_the_per_launch_limit():
    """More jobs than one launch's argument table holds (88), split series on both sides of the boundary: each record equals
    the one the series gets alone."""
    from ppq_amd import ffi
    sizes = [40000, 700] + [50 + 37 * k for k in range(84)] + [16385, 100000, 16384] + [300 + k for k in range(100)] + [70000]
    items = []
    for k, n in enumerate(sizes):
        p, r = _series('pair' if k % 3 == 0 else 'normal', n)
        items.append((p, r))
    table = _moments(items, 32)
    ffi.stat_shape_multi(items, table)
    for k, item in enumerate(items):
        alone = _moments([item], 32)
        ffi.stat_shape_multi([item], alone)
        assert torch.equal(alone[0].view(torch.int32), table[k].view(torch.int32)), k
    with pytest.raises(RuntimeError, match='Kernel Failure'): ffi.stat_moments_multi(items[:2], ffi.stat_table(3, 0, torch.device(DEV)))
    with pytest.raises(RuntimeError, match='Kernel Failure'): ffi.stat_table(1, 65, torch.device(DEV))
    with pytest.raises(RuntimeError, match='Kernel Failure'): _moments([(items[1][0].cpu(), None)])
    with pytest.raises(RuntimeError, match='Kernel Failure'): _moments([(items[0][0], items[0][1][:-1])])


def test_the_two_launches_replay_from_a_hip_graph():
    """No upload, no synchronisation, no allocation inside the launches: moments and shape (one-workgroup and split series) are
    captured once and replayed; the replay reads the series as they are then."""
    from ppq_amd import ffi
    side = torch.cuda.Stream()
    items = [_series('pair', 9216), _series('normal', 40000)]
    table = ffi.stat_table(2, 32, torch.device(DEV))

    def work():
        ffi.stat_moments_multi(items, table)
        ffi.stat_shape_multi(items, table)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side): work()                                   # eager once on the stream: its scratch is sized
    side.synchronize()
    eager = table.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side): work()
    items[1][0].mul_(1.5)
    table.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(table[0].view(torch.int32), eager[0].view(torch.int32)) and not torch.equal(table[1], eager[1])
    fresh = _moments(items, 32)
    ffi.stat_shape_multi(items, fresh)
    assert torch.equal(table.view(torch.int32), fresh.view(torch.int32))


# ---- the recorded reference series on the device --------------------------------------------------------------------------
def _check_records(records, pairs, reference_hist=None, cap=False):
    """Kernel-arm records against float64 of the same series; the histogram against `reference_hist(k, kind)` (a CPU histc of
    the same values): half the L1 distance is at most the series' edge samples, zero for a constant series."""
    worst = {'mean': 0.0, 'std': 0.0, 'skew': 0.0, 'kurt': 0.0, 'snr': 0.0, 'hist': 0}
    for k, (rec, (op, var, x_fp, x_qt)) in enumerate(zip(records, pairs)):
        assert list(rec) == C.KEYS
        fp, qt = x_fp.cpu().numpy(), x_qt.cpu().numpy()
        n = fp.size
        for kind, x in (('Noise', C.noise_of(qt, fp)), ('Quantized', qt), ('Float', fp)):
            what = (k, op.name, var.name, kind)
            f64 = C.float64_series(x)
            assert rec[f'{kind} Min'] == float(x.min()) and rec[f'{kind} Max'] == float(x.max()), what
            bound = C.moment_bound(f64['Mean'], n, scale=float(np.abs(x.astype(np.float64)).sum() / n))
            assert abs(rec[f'{kind} Mean'] - float(np.float32(f64['Mean']))) <= bound, (what, rec[f'{kind} Mean'], f64['Mean'])
            assert abs(rec[f'{kind} Std'] - float(np.float32(f64['Std']))) <= C.moment_bound(f64['Std'], n), (what, rec[f'{kind} Std'], f64['Std'])
            worst['mean'] = max(worst['mean'], abs(rec[f'{kind} Mean'] - f64['Mean']) / C.ulp32(np.float32(f64['Mean'])))
            constant = bool(x.min() == x.max())
            edges = C.edge_samples(x)
            hist = rec[f'{kind} Hist']
            assert len(hist) == C.BINS and sum(hist) == n and all(type(c) is float for c in hist), what
            if constant:
                assert math.isnan(rec[f'{kind} Skewness']) and math.isnan(rec[f'{kind} Kurtosis']) and rec[f'{kind} Std'] == 0.0, what
                assert hist[C.BINS // 2] == n, what
            else:
                if cap: assert edges <= C.EDGE_CAP * n, (what, edges)       # fails, does not skip
                worst['std'] = max(worst['std'], abs(rec[f'{kind} Std'] - f64['Std']) / C.ulp32(np.float32(f64['Std'])))
                skew_bound, kurt_bound = C.shape_bounds(x)
                assert abs(rec[f'{kind} Skewness'] - f64['Skewness']) <= skew_bound, (what, rec[f'{kind} Skewness'], f64['Skewness'], skew_bound)
                assert abs(rec[f'{kind} Kurtosis'] - f64['Kurtosis']) <= kurt_bound, (what, rec[f'{kind} Kurtosis'], f64['Kurtosis'], kurt_bound)
                worst['skew'] = max(worst['skew'], abs(rec[f'{kind} Skewness'] - f64['Skewness']))
                worst['kurt'] = max(worst['kurt'], abs(rec[f'{kind} Kurtosis'] - f64['Kurtosis']))
            if reference_hist is not None:
                moved = int(np.abs(np.asarray(hist) - np.asarray(reference_hist(k, kind))).sum()) // 2
                assert moved <= (0 if constant else edges), (what, moved, edges)
                worst['hist'] = max(worst['hist'], moved)
        snr64 = C.float64_snr(qt, fp)
        assert abs(rec['Noise:Signal Power Ratio'] - snr64) <= C.snr_bound(snr64, n), (k, rec['Noise:Signal Power Ratio'], snr64)
        if snr64 > 0: worst['snr'] = max(worst['snr'], abs(rec['Noise:Signal Power Ratio'] - snr64) / snr64)
    return worst


def test_golden_series_on_the_device():
    from ppq_amd import analyse
    from test_host_statistics import golden_pairs
    pairs = golden_pairs(DEV)
    records = analyse.series_statistics(pairs, bins=C.BINS)
    assert analyse.last_analysis_stats['stat_launches'] >= 2
    for rec, entry in zip(records, BOOK['records']):
        for key in C.KEYS[:6]: assert rec[key] == entry[key]
    kinds = {kind: s for s, kind in enumerate(C.KINDS)}
    worst = _check_records(records, pairs, lambda k, kind: GOLD['ref_hist'][k, kinds[kind]], cap=True)
    # the recorded float64 column is what the test recomputed
    for k, rec in enumerate(records):
        for s, kind in enumerate(C.KINDS):
            f64 = C.float64_series({'Noise': C.noise_of(GOLD[f'qt_{k}'], GOLD[f'fp_{k}']), 'Quantized': GOLD[f'qt_{k}'], 'Float': GOLD[f'fp_{k}']}[kind])
            for i, field in enumerate(C.SCALARS):
                a, b = GOLD['f64_scalars'][k, s, i], f64[field]
                assert (math.isnan(a) and math.isnan(b)) or a == b
    print('golden series on the device, worst against float64 / the reference histogram:', worst)


# ---- end to end -----------------------------------------------------------------------------------------------------------
_STAT_LAUNCHES = {}


@pytest.mark.parametrize('kind', ['small_cnn', 'resnet50'])
def test_statistical_analyse_with_kernels_against_torch(kind):
    from ppq_amd import analyse
    graph, ex, batches = _calibrated(kind)
    snap = _snapshot(graph)
    steps, ran = 1, 2
    with _deterministic():
        pairs = analyse.collect_samples(graph, DEV, batches, steps=steps, executor=ex)
        stats = dict(analyse.last_analysis_stats)
        _assert_untouched(graph, snap)
        torch_pairs = analyse.collect_samples(graph, DEV, batches, steps=steps, executor=ex, use_kernels=False)
        torch_stats = dict(analyse.last_analysis_stats)
        _assert_untouched(graph, snap)
        records = analyse.statistical_analyse(graph, DEV, batches, steps=steps, executor=ex)
        full = dict(analyse.last_analysis_stats)
        _assert_untouched(graph, snap)
    assert len(pairs) == len(torch_pairs) == len(records) > 6
    assert stats == {'forwards': 2 * ran, 'fetch_launches': 2 * ran, 'stat_launches': 0, 'device_reads': 0}
    assert torch_stats['device_reads'] == 2 * ran * len(pairs) and torch_stats['fetch_launches'] == 0
    assert full['fetch_launches'] == full['forwards'] == 2 * ran and full['device_reads'] == 1
    _STAT_LAUNCHES[kind] = full['stat_launches']
    if len(_STAT_LAUNCHES) == 2: assert _STAT_LAUNCHES['small_cnn'] == _STAT_LAUNCHES['resnet50']          # does not depend on V
    for (op, var, x_fp, x_qt), (t_op, t_var, t_fp, t_qt) in zip(pairs, torch_pairs):
        assert op is t_op and var is t_var and x_fp.is_cuda and not t_fp.is_cuda and x_fp.shape == (ran * 1024,)
        assert torch.equal(x_fp.cpu().view(torch.int32), t_fp.view(torch.int32)), (op.name, var.name)       # bit for bit
        assert torch.equal(x_qt.cpu().view(torch.int32), t_qt.view(torch.int32)), (op.name, var.name)
    assert any(not torch.equal(x_fp, x_qt) for _, _, x_fp, x_qt in pairs)
    torch_records = analyse.series_statistics(torch_pairs, use_kernels=False)
    again = analyse.series_statistics(pairs)
    assert json.dumps(again) == json.dumps(records)                         # the same samples, the same bits
    worst = _check_records(records, torch_pairs, lambda k, kind_: torch_records[k][f'{kind_} Hist'])
    for rec, t_rec in zip(records, torch_records):
        assert [rec[key] for key in C.KEYS[:6]] == [t_rec[key] for key in C.KEYS[:6]]
    print(f'statistical_analyse {kind}: {len(records)} records, worst against float64 / the CPU histogram:', worst)


def test_launches_and_copies_of_one_report():
    """The library's own launch counters: one fetch per forward, one moments and one shape call for the whole report."""
    from ppq_amd import _lib, analyse
    graph, ex, batches = _calibrated('small_cnn')
    analyse.statistical_analyse(graph, DEV, batches, steps=0, executor=ex)                              # warm: tables
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    try: records = analyse.statistical_analyse(graph, DEV, batches, steps=2, executor=ex)
    finally:
        torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 32)()
    n = _lib.lib.ppqhip_prof_collect(arr, 32)
    launches = {arr[i].name.decode(): arr[i].launches for i in range(n)}
    assert launches.get('fetch_rows', 0) == 6 and launches.get('stat_moments', 0) == 1 and launches.get('stat_shape', 0) == 1, launches
    assert analyse.last_analysis_stats == {'forwards': 6, 'fetch_launches': 6, 'stat_launches': 2, 'device_reads': 1}
    assert len(records) > 6


def test_parameter_analyse_with_kernels_against_torch(capsys):
    from ppq_amd import analyse
    graph, ex, _ = _calibrated('resnet50')
    snap = _snapshot(graph)
    got = analyse.parameter_analyse(graph)
    text = capsys.readouterr().out
    stats = dict(analyse.last_analysis_stats)
    want = analyse.parameter_analyse(graph, use_kernels=False)
    assert capsys.readouterr().out.count('\n') == text.count('\n') > 3
    _assert_untouched(graph, snap)
    assert stats == {'forwards': 0, 'fetch_launches': 0, 'stat_launches': 1, 'device_reads': 1}
    assert analyse.last_analysis_stats['device_reads'] == 4 * len(want['Value Std'])
    assert list(got) == list(want) == ['Value Range', 'Value Std', 'Value Mean(Abs)']
    params = {f'{v.name}[{op.name}]': v.value for op in graph.operations.values() for v in op.parameters if v.value.numel() > 1}
    assert list(got['Value Range']) == list(want['Value Range']) == list(params) and len(params) > 100
    worst = [0.0, 0.0]
    for label, value in params.items():
        n, x64 = value.numel(), value.double()
        assert got['Value Range'][label] == want['Value Range'][label], label                             # exact
        mean = float(x64.sum() / n)
        std = math.sqrt(float(((x64 - mean) ** 2).sum() / (n - 1)))
        assert abs(got['Value Mean(Abs)'][label] - float(np.float32(abs(mean)))) <= C.moment_bound(mean, n, scale=float(x64.abs().sum() / n)), label
        assert abs(got['Value Std'][label] - float(np.float32(std))) <= C.moment_bound(std, n), label
        worst[0] = max(worst[0], abs(want['Value Mean(Abs)'][label] - abs(mean)) / C.ulp32(np.float32(mean)))
        worst[1] = max(worst[1], abs(want['Value Std'][label] - std) / C.ulp32(np.float32(std)))
    print(f'parameter_analyse: {len(params)} parameters; the torch arm is up to {worst[0]:.2f} / {worst[1]:.2f} ulp (mean / std) off float64')


def test_variable_analyse_counts_follow_the_position_rule():
    from ppq_amd import analyse
    graph, ex, batches = _calibrated('small_cnn')
    snap = _snapshot(graph)
    names = [graph.operations['c1'].outputs[0].name, list(graph.outputs)[0]]
    with _deterministic():
        got = analyse.variable_analyse(graph, batches, names, running_device=DEV, samples_per_step=65536, steps=2, seed=10086, executor=ex)
        fp = analyse.variable_analyse(graph, batches, names[0], running_device=DEV, samples_per_step=4096, steps=2, dequantize=True,
                                      seed=10086, executor=ex)
        _assert_untouched(graph, snap)
        samples = {name: [] for name in names}
        for batch in batches[:3]:
            for name, y in zip(names, ex.forward(inputs=batch, output_names=names)):
                flat = y.contiguous().flatten()
                samples[name].append(flat.index_select(0, analyse.generate_indexer(65536, flat.numel(), 10086).to(DEV).long()))
    assert list(got) == names and list(fp) == names[:1]
    for name in names:
        x = torch.cat(samples[name])
        counts, lo, hi = got[name]
        assert len(counts) == 64 and sum(counts) == x.numel() == 3 * 65536
        assert lo == float(x.min()) and hi == float(x.max())
        assert counts == C.position_bins(x, 64).tolist(), name
    assert sum(fp[names[0]][0]) == 3 * 4096 and fp[names[0]][0] != got[names[0]][0]
    random = analyse.variable_analyse(graph, batches, names[1], running_device=DEV, samples_per_step=1000, steps=0, executor=ex)     # torch.randint tables
    assert sum(random[names[1]][0]) == 1000
