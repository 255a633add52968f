"""LayerwiseEqualizationPass on resnet50_graph and yolov6s_graph, 10 iterations, with bias and activations both off and both
on: ms per pass for three arms, the kernel dispatches per arm, and the two launches of the largest pair against a copy of the
same bytes.

  torch      : use_kernels=False on the device -- the reference's torch operations, pair by pair
  sequential : the two HIP kernels, one pair instance per pair of launches (the reference's order)
  levelled   : the two HIP kernels, a level of independent pair instances per pair of launches (the default)

ms per pass = device-synchronised wall time of ``optimize`` on parameters restored in place before every run; with
activations on, the maxima are collected ONCE by the kernel path and handed to every arm, so the timed part is the
iterations alone (the collection is timed on its own, per arm).  The arms are alternated in ONE process, --runs times; the
median with the smallest and largest run is reported.  Dispatches come from one child per arm under
`rocprofv3 --kernel-trace --stats` (kernel trace only; the program after `--`).  The `floor` child launches the scale table and
the apply table of the pair that moves the most bytes, then `floor_copy` (tools/floor) over the same bytes, 20 times each.

    python tools/equalization_bench.py [--runs 5] [--iterations 10] [--out profiles/r11_equalization.txt]"""
import argparse
import ast
import csv
import ctypes
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
FLOOR_SO = os.path.join(ROOT, 'tools', 'floor', 'libfloor.so')
FLOOR_REPEATS = 20
ARMS = {'torch': dict(use_kernels=False), 'sequential': dict(schedule='sequential'), 'levelled': dict(schedule='levelled')}
SHAPES = {'resnet50': (2, 3, 224, 224), 'yolov6s': (2, 3, 160, 160)}


class Workload:
    def __init__(self, name: str):
        from ppq_amd import harness
        self.name = name
        self.graph = getattr(harness, name + '_graph')()
        self.executor = harness.TorchExecutor(self.graph, 'cuda')
        self.saved = {n: v.value.detach().clone() for n, v in self.graph.variables.items() if v.is_parameter}
        g = torch.Generator().manual_seed(9)
        self.batches = [torch.rand(SHAPES[name], generator=g).to('cuda') for _ in range(4)]
        self.activations = None

    def restore(self) -> None:
        for n, t in self.saved.items(): self.graph.variables[n].value.copy_(t)

    def make_pass(self, arm: str, on: bool, iterations: int):
        from ppq_amd.equalization import LayerwiseEqualizationPass
        return LayerwiseEqualizationPass(iterations=iterations, including_bias=on, including_act=on, **ARMS[arm])

    def collect(self, arm: str) -> float:
        """ms of the activation collection alone (iterations = 0)."""
        self.restore()
        p = self.make_pass(arm, True, 0)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        p.optimize(self.graph, dataloader=self.batches, executor=self.executor)
        torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
        if arm != 'torch': self.activations = p.activations
        return ms

    def run(self, arm: str, on: bool, iterations: int):
        self.restore()
        p = self.make_pass(arm, on, iterations)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        p.optimize(self.graph, dataloader=self.batches, executor=self.executor, activations=self.activations if on else None)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, p.stats


def child(arm: str, name: str, on: bool, iterations: int):
    w = Workload(name)
    if on: w.collect('levelled')
    if arm == 'floor': return run_floor(w, on)
    ms, stats = w.run(arm, on, iterations)
    return {'arm': arm, 'ms': ms, **stats}


def run_floor(w: Workload, on: bool):
    from ppq_amd import equalization as EQ
    from ppq_amd import ffi
    fl = ctypes.CDLL(FLOOR_SO)
    fl.floor_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    p = w.make_pass('levelled', on, 1)
    pairs = p.find_equalization_pair(w.graph, p.interested_operations(w.graph))
    size = lambda pair: sum(op.inputs[1].value.numel() for op in pair.operations)          # noqa: E731
    pair = max(pairs, key=size)
    scale = torch.empty(pair.num_channel(), device='cuda')
    item, applies = EQ.pair_jobs(pair, scale, 0.5, on, on, 0.5, 0.5, w.activations or {})
    st, at = ffi.equalize_scale_table([item]), ffi.equalize_apply_table(applies)
    n = size(pair)
    src, dst = torch.rand(n, device='cuda'), torch.empty(n, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for _ in range(FLOOR_REPEATS): ffi.equalize_scale_multi(st)
    for _ in range(FLOOR_REPEATS):                                     # the scale launch reads 4 n bytes: a copy of n / 2 floats moves as many
        if fl.floor_copy(src.data_ptr(), dst.data_ptr(), n // 2, 256, 2, 0, stream) != 0: raise RuntimeError('floor_copy failed')
    scale.fill_(1.0)                                                   # the apply launches leave the weights as they are
    for _ in range(FLOOR_REPEATS): ffi.equalize_apply_multi(at)
    for _ in range(FLOOR_REPEATS):                                     # reads and writes 8 n bytes: a copy of n floats
        if fl.floor_copy(src.data_ptr(), dst.data_ptr(), n, 256, 2, 0, stream) != 0: raise RuntimeError('floor_copy failed')
    torch.cuda.synchronize()
    return {'arm': 'floor', 'pair': repr(pair), 'elements': n, 'channels': pair.num_channel(), 'segments': len(item[2]), 'tensors': len(applies)}


def traced(arm: str, name: str, on: bool, iterations: int):
    """Child under rocprofv3: (kernel trace rows, child stdout) or (None, reason)."""
    rocprof = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if rocprof is None: return None, 'rocprofv3 not found'
    out = tempfile.mkdtemp(prefix='equalization_trace_')
    cmd = [rocprof, '--kernel-trace', '--stats', '-d', out, '-o', 'run', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--child', arm, '--graph', name, '--iterations', str(iterations)] + (['--on'] if on else [])
    try: r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired: return None, 'timed out after 300 s'
    traces = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
    if r.returncode != 0 or not traces: return None, f'rc={r.returncode}; stderr tail {(r.stderr or "")[-300:]!r}'
    rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r['Start_Timestamp']))
    shutil.rmtree(out, ignore_errors=True)
    return rows, r.stdout


def _ns(row) -> int:
    return int(row['End_Timestamp']) - int(row['Start_Timestamp'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--iterations', type=int, default=10)
    ap.add_argument('--graph', default=None)
    ap.add_argument('--on', action='store_true')
    ap.add_argument('--child', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        print(child(args.child, args.graph, args.on, args.iterations))
        return
    lines = [f'# tools/equalization_bench.py --runs {args.runs} --iterations {args.iterations}: LayerwiseEqualizationPass, value_threshold 0.5, '
             'optimize_level 2; ms per pass, device-synchronised, parameters restored in place before every run',
             f'# device: {torch.cuda.get_device_name(0)}']

    def emit(line):
        lines.append(line); print(line, flush=True)
    failed = False
    for name in ('resnet50', 'yolov6s'):
        w = Workload(name)
        for arm in ARMS: w.run(arm, False, 1)                          # warm the allocator and the code objects
        coll = {arm: [w.collect(arm) for _ in range(3)] for arm in ('torch', 'levelled')}
        emit(f'{name}: activation collection over {len(w.batches)} batches {SHAPES[name]} (forwards included): torch arm median '
             f'{statistics.median(coll["torch"]):.2f} ms, kernel arm median {statistics.median(coll["levelled"]):.2f} ms (3 runs each)')
        for on in (False, True):
            runs = {arm: [] for arm in ARMS}
            for _ in range(args.runs):                                 # alternated: drift of the box hits all arms alike
                for arm in ARMS: runs[arm].append(w.run(arm, on, args.iterations))
            med = {}
            for arm in ARMS:
                ms = [r[0] for r in runs[arm]]
                med[arm] = statistics.median(ms)
                s = runs[arm][-1][1]
                emit(f'{name} bias/act {"on " if on else "off"} {arm:10s} ms/pass median {med[arm]:.3f} (min {min(ms):.3f}, max {max(ms):.3f}, '
                     f'{len(ms)} runs); pairs {s["pairs"]}, levels {s["levels"]}, launches {s["launches"]}, channels {s["channels"]}, '
                     f'scaled {s["scaled_channels"]}, clipped {s["clipped_channels"]}')
            emit(f'{name} bias/act {"on " if on else "off"} ratio of medians: torch / sequential {med["torch"] / med["sequential"]:.2f}x, '
                 f'torch / levelled {med["torch"] / med["levelled"]:.2f}x, sequential / levelled {med["sequential"] / med["levelled"]:.2f}x')
        del w
        torch.cuda.empty_cache()
        for arm in ARMS:
            if failed: break
            rows, err = traced(arm, name, False, args.iterations)
            if rows is None:
                emit(f'trace {name} {arm}: not measured ({err})')
                failed = True                                          # a child that failed: nothing more is started on the GPU
                break
            mine = {k: [_ns(r) for r in rows if k in r.get('Kernel_Name', '')] for k in ('equalize_scale', 'equalize_apply')}
            emit(f'trace {name} bias/act off {arm}: {len(rows)} kernel dispatches for the whole child (graph upload included)'
                 + ''.join(f'; {k}: {len(v)} dispatches, median {statistics.median(v) / 1e3:.2f} us, sum {sum(v) / 1e6:.3f} ms' for k, v in mine.items() if v))
        if failed: break
        rows, out = traced('floor', name, False, 1)
        if rows is None:
            emit(f'floor {name}: not measured ({out})')
            break
        info = ast.literal_eval(out.strip().splitlines()[-1])
        sc = [_ns(r) for r in rows if 'equalize_scale' in r['Kernel_Name']][-FLOOR_REPEATS:]
        apl = [_ns(r) for r in rows if 'equalize_apply' in r['Kernel_Name']][-FLOOR_REPEATS:]
        cp = [_ns(r) for r in rows if 'floor_copy' in r['Kernel_Name']]
        if len(cp) != 2 * FLOOR_REPEATS or len(sc) != FLOOR_REPEATS or len(apl) != FLOOR_REPEATS:
            emit(f'floor {name}: the trace does not split into 4 x {FLOOR_REPEATS} launches: not reported')
            continue
        n = info['elements']
        m = [statistics.median(v) / 1e3 for v in (sc, cp[:FLOOR_REPEATS], apl, cp[FLOOR_REPEATS:])]
        emit(f'floor {name}: largest pair {info["pair"]}: {n} weight elements, {info["channels"]} channels, {info["segments"]} segments, '
             f'{info["tensors"]} tensors; same buffers every launch ({8 * n / 1e6:.1f} MB: cache resident or not by size)')
        emit(f'  equalize_scale {m[0]:.2f} us vs floor_copy of {4 * n / 1e6:.2f} MB {m[1]:.2f} us: ratio {m[0] / m[1]:.2f}')
        emit(f'  equalize_apply {m[2]:.2f} us vs floor_copy of {8 * n / 1e6:.2f} MB {m[3]:.2f} us: ratio {m[2] / m[3]:.2f}')
    if args.out:
        with open(args.out, 'w') as f: f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
