"""statistical_analyse and parameter_analyse on the ResNet-50 and the YOLOv6-s-like harness graphs (batch 32, minmax-calibrated
INT8, steps = 8: 9 batches per phase): wall time per report of the two arms, what a report launches, and the library's own
event timing of its three entry points.

  torch : use_kernels=False -- the reference's procedure on the same device: index_select and one copy to the CPU per tensor
          and forward, then about 30 torch calls and 24 .item() per variable on the CPU (the index tables are made once and
          kept, which the reference does not do: the arm is faster than the reference itself)
  hip   : one fetch launch per forward, one moments and one shape call per report, one copy

Wall time = host clock around one report that ends in a device synchronise, the arms ALTERNATED in one process.  The last line
printed is one JSON object with the medians and the run spread.

    python tools/statistics_bench.py [--repeats 3] [--out profiles/statistics.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 8


def setup(kind, batch=32):
    from ppq_amd import harness
    from ppq_amd.calibration import RuntimeCalibrationPass
    torch.manual_seed(0)
    graph, size = (harness.resnet50_graph(seed=0), 224) if kind == 'resnet50' else (harness.yolov6s_graph(seed=0), 160)
    harness.quantize_graph(graph, 'minmax')
    ex = harness.TorchExecutor(graph, 'cuda')
    harness.ParameterQuantizePass().optimize(graph)
    g = torch.Generator().manual_seed(9)
    batches = [torch.rand(batch, 3, size, size, generator=g).to('cuda') for _ in range(STEPS + 1)]
    RuntimeCalibrationPass(check_steps=False).optimize(graph, dataloader=batches, executor=ex, calib_steps=STEPS)
    return graph, ex, batches, size


def timed(fn):
    from ppq_amd import analyse
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, result, dict(analyse.last_analysis_stats)


def spread(values): return (max(values) - min(values)) / statistics.median(values)


def library_times(fn):
    """Launches and total milliseconds per entry point of one call of fn, by the library's own event pairs."""
    from ppq_amd import _lib
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    try: fn()
    finally:
        torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 32)()
    n = _lib.lib.ppqhip_prof_collect(arr, 32)
    return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(n)
            if arr[i].name.decode() in ('fetch_rows', 'stat_moments', 'stat_shape')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--graphs', default='resnet50,yolov6s')
    args = ap.parse_args()
    from ppq_amd import analyse
    lines = [f'# tools/statistics_bench.py --repeats {args.repeats}: batch 32, minmax-calibrated INT8, steps = {STEPS} ({STEPS + 1} batches per phase)',
             f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0), 'steps': STEPS, 'batch': 32}
    for kind in args.graphs.split(','):
        graph, ex, batches, size = setup(kind)
        arms = {'torch': lambda: analyse.statistical_analyse(graph, 'cuda', batches, steps=STEPS, executor=ex, use_kernels=False),
                'hip': lambda: analyse.statistical_analyse(graph, 'cuda', batches, steps=STEPS, executor=ex),
                'parameter torch': lambda: analyse.parameter_analyse(graph, verbose=False, use_kernels=False),
                'parameter hip': lambda: analyse.parameter_analyse(graph, verbose=False)}
        times, stats, results = {arm: [] for arm in arms}, {}, {}
        for arm, fn in arms.items(): timed(fn)                                             # warm every arm once
        for _ in range(args.repeats):
            for arm, fn in arms.items():                                                   # alternated
                t, results[arm], stats[arm] = timed(fn)
                times[arm].append(t)
                print(f'{kind} {arm} {t:.3f} s', file=sys.stderr, flush=True)
        records = results['hip']
        elements = sum(v.value.numel() for op in graph.operations.values() for v in op.parameters if v.value.numel() > 1)
        lines.append(f'{kind}: {size} x {size} input, {len(records)} records per report, {len(results["parameter hip"]["Value Std"])} parameters of {elements / 1e6:.1f} M elements')
        for arm, ts in times.items():
            lines.append(f'  {arm:16s} wall s: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {statistics.median(ts):.4f}  spread {spread(ts) * 100:.1f} %   {stats[arm]}')
        for a, b, what in (('torch', 'hip', 'statistical_analyse'), ('parameter torch', 'parameter hip', 'parameter_analyse')):
            ma, mb = statistics.median(times[a]), statistics.median(times[b])
            lines.append(f'  {what}: hip over torch {ma / mb:.2f}x by the medians ({(ma - mb) * 1e3:.1f} ms less per report)')
        fwd = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for b in batches: ex.forward(b)
            torch.cuda.synchronize(); fwd.append((time.perf_counter() - t0) / len(batches))
        lines.append(f'  for scale: one quantised forward without hooks {statistics.median(fwd) * 1e3:.1f} ms; a report runs {2 * (STEPS + 1)} (hooked: no fused epilogues)')
        for what, fn in (('statistical_analyse', arms['hip']), ('parameter_analyse', arms['parameter hip'])):
            lines.append(f'  {what}, the library\'s entry points (calls, total ms by event pairs): {library_times(fn)}')
        worst = 0.0
        for rec, ref in zip(records, results['torch']):
            for key in ('Quantized Std', 'Float Std', 'Noise Std'):
                if ref[key]: worst = max(worst, abs(rec[key] - ref[key]) / abs(ref[key]))
        lines.append(f'  hip vs torch std columns (MIOpen convolutions do not repeat bit for bit between runs): largest relative difference {worst:.2e}')
        summary[kind] = {'records': len(records),
                         'statistical_analyse_torch_s': statistics.median(times['torch']), 'statistical_analyse_hip_s': statistics.median(times['hip']),
                         'statistical_analyse_spread': max(spread(times['torch']), spread(times['hip'])),
                         'parameter_analyse_torch_s': statistics.median(times['parameter torch']), 'parameter_analyse_hip_s': statistics.median(times['parameter hip']),
                         'parameter_analyse_spread': max(spread(times['parameter torch']), spread(times['parameter hip']))}
        del graph, ex, batches
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
