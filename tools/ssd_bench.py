"""SSDEqualizationPass on resnet50_graph and yolov6s_graph (per-tensor weights, batch 32): ms per pass for the two arms, their
forward and launch counts, and the three launches of csrc/ssd.hip against a copy of the same bytes.

  torch   : use_kernels=False on the device -- the reference's sequence, one executor.forward wherever it has one
  kernels : one prefix forward per distinct batch per (iteration, pair), the three HIP launches (the default)

ms per pass = device-synchronised wall time of ``optimize`` on parameters restored before every run.  The arms are alternated
in ONE process, --runs times; the median with the smallest and largest run is reported.  The `floor` child runs under
`rocprofv3 --kernel-trace --stats` (kernel trace only; the program after `--`): for the pair that holds the most weights it
launches the scales, the apply and -- on that pair's output of one batch -- the loss read, then `floor_copy` (tools/floor) over
the same bytes, 20 times each.

    python tools/ssd_bench.py [--runs 3] [--iteration 1] [--out profiles/r12_ssd.txt]"""
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
ARMS = {'torch': dict(use_kernels=False), 'kernels': dict(use_kernels=True)}
SHAPES = {'resnet50': (32, 3, 224, 224), 'yolov6s': (32, 3, 160, 160)}
BATCHES = 2


class Workload:
    def __init__(self, name: str):
        from ppq_amd import harness
        self.name = name
        self.graph = getattr(harness, name + '_graph')()
        harness.quantize_graph(self.graph, per_channel_weight=False)
        self.executor = harness.TorchExecutor(self.graph, 'cuda')
        self.saved = {n: v.value.detach().clone() for n, v in self.graph.variables.items() if v.is_parameter}
        g = torch.Generator().manual_seed(9)
        self.batches = [torch.rand(SHAPES[name], generator=g).to('cuda') for _ in range(BATCHES)]

    def restore(self) -> None:
        for n, t in self.saved.items(): self.graph.variables[n].value = t.clone()
        for op in self.graph.operations.values():
            if hasattr(op, 'store_parameter_value'): op.store_parameter_value()

    def run(self, arm: str, iteration: int, keep: bool = False):
        from ppq_amd.ssd import SSDEqualizationPass
        self.restore()
        p = SSDEqualizationPass(iteration=iteration, **ARMS[arm])
        torch.cuda.synchronize(); t0 = time.perf_counter()
        p.optimize(self.graph, dataloader=self.batches, executor=self.executor, collate_fn=None, calib_steps=BATCHES)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, (p if keep else p.stats)


def compare_arms(w: Workload, iteration: int) -> str:
    """One more run of each arm with the convolution library's deterministic algorithms: do the arms decide alike, and how far
    apart are their losses?  (Bit equality of the arms needs a forward that repeats its bits; a decision whose loss sits at the
    threshold can go either way when it does not.)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        names = [op.outputs[0].name for op in w.graph.operations.values() if op.type == 'Conv']
        first, second = w.executor.forward(w.batches[0], output_names=names), w.executor.forward(w.batches[0], output_names=names)
        repeats = all(torch.equal(a, b) for a, b in zip(first, second))
        a, b = w.run('torch', iteration, keep=True)[1], w.run('kernels', iteration, keep=True)[1]
    finally:
        torch.backends.cudnn.deterministic = before
    differ = [k for k in a.history if a.history[k]['best_idx'] != b.history[k]['best_idx']]
    worst = max(abs(x - y) / max(abs(x), 1e-30) for k in a.history
                for x, y in zip([a.history[k]['basic']] + a.history[k]['losses'], [b.history[k]['basic']] + b.history[k]['losses']))
    return (f'arms compared with deterministic convolutions: every Conv output repeats its bits over two forwards: {repeats}; '
            f'(iteration, pair) instances decided differently: {len(differ)} of {len(a.history)}; largest relative difference '
            f'between their losses {worst:.3e}')


def run_floor(name: str):
    from ppq_amd import ffi
    from ppq_amd import ssd as SSD
    w = Workload(name)
    fl = ctypes.CDLL(FLOOR_SO)
    fl.floor_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    p = SSD.SSDEqualizationPass()
    size = lambda pair: sum(v.value.numel() for op in (pair[0], pair[-1]) for v in op.parameters)      # noqa: E731
    pair = max(p.collect_all_pairs(w.graph), key=size)
    C, seg1, seg2, applies = SSD.pair_geometry(pair)
    n = size(pair)
    y = w.executor.forward(w.batches[0], output_names=[pair[-1].outputs[0].name])[0].contiguous()
    r = y + 0.01 * torch.randn_like(y)
    act = y.new_ones(C)
    scales, ranges = torch.empty((4, C), device='cuda'), torch.empty((2, C), device='cuda')
    outs = {var: torch.empty((4,) + tuple(var.value.shape), device='cuda') for var, *_ in applies}
    items = [(var.value, outs[var], scales, run, inner, og, divide) for var, run, inner, og, divide in applies]
    s, o = torch.full((1,), float(y.abs().max()) / 127, device='cuda'), torch.zeros(1, device='cuda')
    sums = [torch.empty((y.shape[0], 4), dtype=torch.float64, device='cuda')]
    big = max(5 * n // 2, y.numel())
    src, dst = torch.rand(big, device='cuda'), torch.empty(big, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def copy(count):
        for _ in range(FLOOR_REPEATS):
            if fl.floor_copy(src.data_ptr(), dst.data_ptr(), count, 256, 2, 0, stream) != 0: raise RuntimeError('floor_copy failed')
    torch.cuda.synchronize()
    for _ in range(FLOOR_REPEATS): ffi.ssd_scales_multi([(seg1, seg2, act, 0.5, scales, ranges)])
    copy(n // 2)                                                       # the scales read 4 n bytes: a copy of n / 2 floats moves as many
    for _ in range(FLOOR_REPEATS): ffi.ssd_apply_multi(items)
    copy(5 * n // 2)                                                   # reads 4 n, writes 16 n bytes: a copy of 2.5 n floats
    for _ in range(FLOOR_REPEATS): ffi.fq_measure_rows_multi([(y, r, s, o, None, -128, 127, 0)], sums)
    copy(y.numel())                                                    # reads y and r: a copy of y.numel() floats moves as many bytes
    torch.cuda.synchronize()
    return {'pair': '--'.join(op.name for op in pair), 'elements': n, 'channels': C, 'tensors': len(applies), 'output': list(y.shape)}


def traced(name: str):
    """The floor child under rocprofv3: (kernel trace rows, child stdout) or (None, reason)."""
    rocprof = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if rocprof is None: return None, 'rocprofv3 not found'
    out = tempfile.mkdtemp(prefix='ssd_trace_')
    cmd = [rocprof, '--kernel-trace', '--stats', '-d', out, '-o', 'run', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--child', 'floor', '--graph', name]
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
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--iteration', type=int, default=1)
    ap.add_argument('--graph', default=None)
    ap.add_argument('--child', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        print(run_floor(args.graph))
        return
    lines = [f'# tools/ssd_bench.py --runs {args.runs} --iteration {args.iteration}: SSDEqualizationPass (channel_ratio 0.5, loss_threshold 0.8) on '
             f'quantize_graph(per_channel_weight=False), {BATCHES} batches; ms per pass, device-synchronised, parameters restored before every run',
             f'# device: {torch.cuda.get_device_name(0)}']

    def emit(line):
        lines.append(line); print(line, flush=True)
    for name in ('resnet50', 'yolov6s'):
        w = Workload(name)
        runs = {arm: [] for arm in ARMS}
        for _ in range(args.runs):                                     # alternated: drift of the box hits both arms alike
            for arm in ARMS: runs[arm].append(w.run(arm, args.iteration))
        med = {}
        for arm in ARMS:
            ms = [r[0] for r in runs[arm]]
            med[arm] = statistics.median(ms)
            s = runs[arm][-1][1]
            emit(f'{name} batch {SHAPES[name][0]} {arm:8s} ms/pass median {med[arm]:.1f} (min {min(ms):.1f}, max {max(ms):.1f}, {len(ms)} runs); '
                 f'pairs {s["pairs"]}, calib_steps {s["calib_steps"]}, prefix_forwards {s["prefix_forwards"]}, pair_forwards {s["pair_forwards"]}, '
                 f'launches {s["launches"]}, accepted {dict(sorted(s["accepted"].items()))}')
        spread = max(max(r[0] for r in runs[a]) / min(r[0] for r in runs[a]) for a in ARMS)
        emit(f'{name} ratio of medians torch / kernels {med["torch"] / med["kernels"]:.2f}x (largest max / min within an arm {spread:.2f}x)')
        emit(f'{name} ' + compare_arms(w, args.iteration))
        del w
        torch.cuda.empty_cache()
        rows, out = traced(name)
        if rows is None:
            emit(f'floor {name}: not measured ({out})')
            break                                                      # a child that failed: nothing more is started on the GPU
        info = ast.literal_eval(out.strip().splitlines()[-1])
        pick = lambda word: [_ns(r) for r in rows if word in r['Kernel_Name']][-FLOOR_REPEATS:]       # noqa: E731
        rg, sc, apl, fq = pick('ssd_ranges_kernel'), pick('ssd_scales_kernel'), pick('ssd_apply_kernel'), pick('fq_measure_rows_kernel')
        cp = [_ns(r) for r in rows if 'floor_copy' in r['Kernel_Name']]
        if len(cp) != 3 * FLOOR_REPEATS or min(len(rg), len(sc), len(apl), len(fq)) != FLOOR_REPEATS:
            emit(f'floor {name}: the trace does not split into the expected launches: not reported')
            continue
        n, ny = info['elements'], 1
        for d in info['output']: ny *= d
        us = lambda v: statistics.median(v) / 1e3                     # noqa: E731
        c = [us(cp[i * FLOOR_REPEATS:(i + 1) * FLOOR_REPEATS]) for i in range(3)]
        emit(f'floor {name}: pair {info["pair"]}: {n} parameter elements, {info["channels"]} channels, {info["tensors"]} tensors; loss read on '
             f'its output {info["output"]}; same buffers every launch (cache resident or not by size); medians of {FLOOR_REPEATS}')
        emit(f'  ssd_scales (ranges {us(rg):.2f} us + scales {us(sc):.2f} us) vs floor_copy of {4 * n / 1e6:.2f} MB {c[0]:.2f} us: ratio {(us(rg) + us(sc)) / c[0]:.2f}')
        emit(f'  ssd_apply {us(apl):.2f} us vs floor_copy of {20 * n / 1e6:.2f} MB {c[1]:.2f} us: ratio {us(apl) / c[1]:.2f}')
        emit(f'  fq_measure_rows {us(fq):.2f} us vs floor_copy of {8 * ny / 1e6:.2f} MB {c[2]:.2f} us: ratio {us(fq) / c[2]:.2f}')
    if args.out:
        with open(args.out, 'w') as f: f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
