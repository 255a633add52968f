"""ChannelwiseSplitPass on resnet50_graph and yolov6s_graph at optimize_level 1 and 2, at the reference's default threshold (2:
nothing splits on He-initialised weights, the pass is its plan launches and copies alone) and at one low enough that channels
split: ms per pass for two arms on the same device, and the kernel dispatches per arm.

  torch  : use_kernels=False on the device -- the reference's torch operations: mask.tolist() and one row per channel, per tensor
  kernel : the HIP plan and gather kernels, a level of independent pairs per plan launch pair, copy and gather launch (default)

ms per pass = device-synchronised wall time of ``optimize``; the parameters are rebound to the saved tensors before every run
(neither arm writes into a tensor it was given).  The arms are alternated in ONE process, --runs times after one warm-up run
each; the median with the smallest and largest run is reported, and whether the two spreads overlap.  Dispatches come from one
child per arm under `rocprofv3 --kernel-trace --stats` (kernel trace only; the program after `--`).

    python tools/channel_split_bench.py [--runs 5] [--iterations 2] [--out profiles/channel_split.txt]"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = {'torch': dict(use_kernels=False), 'kernel': dict(schedule='levelled')}
LOW_THRESHOLD = {'resnet50': 0.2, 'yolov6s': 0.1}       # about a tenth / a thirtieth of the channels split in the first iteration
DEFAULT_THRESHOLD = 2.0


class Workload:
    def __init__(self, name: str):
        from ppq_amd import harness
        self.name = name
        self.graph = getattr(harness, name + '_graph')()
        harness.TorchExecutor(self.graph, 'cuda')                          # places the parameters
        self.saved = {n: v.value for n, v in self.graph.variables.items() if v.is_parameter}

    def restore(self) -> None:
        for n, t in self.saved.items(): self.graph.variables[n].value = t

    def run(self, arm: str, threshold: float, level: int, iterations: int):
        from ppq_amd.channel_split import ChannelwiseSplitPass
        self.restore()
        p = ChannelwiseSplitPass(iterations=iterations, threshold=threshold, including_bias=True, optimize_level=level, **ARMS[arm])
        torch.cuda.synchronize(); t0 = time.perf_counter()
        p.optimize(self.graph)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, p.stats


def child(arm: str, name: str, threshold: float, level: int, iterations: int):
    w = Workload(name)
    ms, stats = w.run(arm, threshold, level, iterations)
    return {'arm': arm, 'ms': ms, **stats}


def traced(arm: str, name: str, threshold: float, level: int, iterations: int):
    """Child under rocprofv3: kernel trace rows, or (None, reason)."""
    rocprof = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if rocprof is None: return None, 'rocprofv3 not found'
    out = tempfile.mkdtemp(prefix='channel_split_trace_')
    cmd = [rocprof, '--kernel-trace', '--stats', '-d', out, '-o', 'run', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--child', arm, '--graph', name, '--threshold', str(threshold), '--level', str(level),
           '--iterations', str(iterations)]
    try:
        try: r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired: return None, 'timed out after 300 s'
        traces = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
        if r.returncode != 0 or not traces: return None, f'rc={r.returncode}; stderr tail {(r.stderr or "")[-300:]!r}'
        with open(traces[0]) as f: rows = list(csv.DictReader(f))
        return rows, r.stdout
    finally: shutil.rmtree(out, ignore_errors=True)


def _ns(row) -> int:
    return int(row['End_Timestamp']) - int(row['Start_Timestamp'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=2)
    ap.add_argument('--graph', default=None)
    ap.add_argument('--threshold', type=float, default=None)
    ap.add_argument('--level', type=int, default=2)
    ap.add_argument('--child', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        print(child(args.child, args.graph, args.threshold, args.level, args.iterations))
        return
    lines = [f'# tools/channel_split_bench.py --runs {args.runs} --iterations {args.iterations}: ChannelwiseSplitPass, including_bias; ms per pass, '
             'device-synchronised, parameters rebound before every run; one warm-up run per arm and setting, then the arms alternated',
             f'# device: {torch.cuda.get_device_name(0)}',
             f'# thresholds: {DEFAULT_THRESHOLD:g} (the reference\'s default) and, low enough that He-initialised weights split, '
             + ', '.join(f'{n} {t:g}' for n, t in LOW_THRESHOLD.items())]

    def emit(line):
        lines.append(line); print(line, flush=True)
    for name in ('resnet50', 'yolov6s'):
        w = Workload(name)
        for level in (1, 2):
            for threshold in (DEFAULT_THRESHOLD, LOW_THRESHOLD[name]):
                for arm in ARMS: w.run(arm, threshold, level, args.iterations)      # warm the allocator and the code objects
                runs = {arm: [] for arm in ARMS}
                for _ in range(args.runs):
                    for arm in ARMS: runs[arm].append(w.run(arm, threshold, level, args.iterations))
                med, spread = {}, {}
                for arm in ARMS:
                    ms = [r[0] for r in runs[arm]]
                    med[arm], spread[arm] = statistics.median(ms), (min(ms), max(ms))
                    s = runs[arm][-1][1]
                    emit(f'{name} level {level} threshold {threshold:g} {arm:6s} ms/pass median {med[arm]:.3f} (min {min(ms):.3f}, max {max(ms):.3f}, '
                         f'{len(ms)} runs); pairs {s["pairs"]}, skipped {s["skipped_pairs"]}, levels {s["levels"]}, launches {s["launches"]}, '
                         f'copies {s["copies"]}, channels {s["channels_before"]} -> {s["channels_after"]}, split per iteration {s["split_channels"]}')
                apart = spread['kernel'][1] < spread['torch'][0] or spread['torch'][1] < spread['kernel'][0]
                emit(f'{name} level {level} threshold {threshold:g} ratio of medians torch / kernel {med["torch"] / med["kernel"]:.2f}x; '
                     f'the spreads {"do not overlap" if apart else "OVERLAP: no difference shown"}')
        del w
        torch.cuda.empty_cache()
    for arm in ARMS:                                                       # where the time goes: resnet50, level 2, the low threshold
        rows, err = traced(arm, 'resnet50', LOW_THRESHOLD['resnet50'], 2, args.iterations)
        if rows is None:
            emit(f'trace resnet50 {arm}: not measured ({err})')
            break                                                          # a child that failed: nothing more is started on the GPU
        by = {}
        for r in rows: by.setdefault(r.get('Kernel_Name', '?').replace('(anonymous namespace)::', '').split('(')[0][:70], []).append(_ns(r))
        top = sorted(by.items(), key=lambda kv: -sum(kv[1]))[:5]
        emit(f'trace resnet50 level 2 threshold {LOW_THRESHOLD["resnet50"]:g} {arm}: {len(rows)} kernel dispatches for the whole child (graph upload '
             f'included), {sum(sum(v) for v in by.values()) / 1e6:.3f} ms of kernel time')
        for k, v in top: emit(f'    {len(v):6d} x {k}: sum {sum(v) / 1e6:.3f} ms, median {statistics.median(v) / 1e3:.2f} us')
    if args.out:
        with open(args.out, 'w') as f: f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
