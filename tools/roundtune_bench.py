"""RoundTuningPass on the YOLOv6-s-like graph (INT4 per-channel weights, block_size 5, first k blocks, N steps per block):
ms per training step for three arms, the launches per step, and the round-tuning kernel's bytes / time against a copy of the
same bytes.

  torch : the reference's torch-op delegator (algorithm/training.py:490-527, restated in tests/golden/roundtune_cases.py),
          one eager step at a time
  eager : the HIP kernel, one grouped launch per step, eager steps
  graph : the HIP kernel, one grouped launch per step, the step captured once and replayed (the default)
  torch_graph : the torch-op delegator with the step captured and replayed too -- what of the `graph` arm's gain is the
          replay's and what the kernel's

ms per step = device-synchronised wall time of the training loop (the pass's own phase timers) / steps; the arms are
alternated in ONE process, --runs times, and the median with the smallest and largest run is reported.  Launches per step and
the kernel's time come from children under `rocprofv3 --kernel-trace --stats` (kernel trace only; arm given by --child).  The
`floor` child launches, for each block, the block's real job table and then `floor_copy` (tools/floor) over the same number
of bytes (12 B per element: w, r read, out written), 20 times each on rotating buffers: the kernel's distance to the copy floor
at the sizes that occur.

    python tools/roundtune_bench.py [--blocks 6] [--steps 200] [--runs 5] [--out profiles/r10_roundtune.txt]"""
import argparse
import ast
import csv
import ctypes
import glob
import itertools
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
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
FLOOR_SO = os.path.join(ROOT, 'tools', 'floor', 'libfloor.so')
FLOOR_REPEATS = 20


def setup(seed=3):
    from ppq_amd import harness
    from ppq_amd.calibration import RuntimeCalibrationPass
    torch.manual_seed(0)
    graph = harness.yolov6s_graph(seed=seed)
    harness.quantize_graph(graph, 'minmax')
    for op in graph.operations.values():
        for cfg, var in op.config_with_variable:
            if var.is_parameter and cfg.state.value == 1: cfg.num_of_bits, cfg.quant_min, cfg.quant_max = 4, -8, 7
    ex = harness.TorchExecutor(graph, 'cuda')
    harness.ParameterQuantizePass().optimize(graph)
    g = torch.Generator().manual_seed(9)
    batches = [torch.rand(2, 3, 160, 160, generator=g).to('cuda') for _ in range(8)]
    RuntimeCalibrationPass().optimize(graph, dataloader=batches, executor=ex, calib_steps=8)
    return graph, ex, batches


def run_arm(arm: str, blocks: int, steps: int):
    import ppq_amd.roundtune as R
    graph, ex, batches = setup()
    saved = R.RoundTuningDelegator
    if arm.startswith('torch'):
        import roundtune_cases as RC

        class TorchOpDelegator(saved):                 # the reference's __call__: 7 torch kernels forward, none backward
            def __call__(self, tensor, config):
                axis = config.channel_axis if config.policy.has_property(R.P.PER_CHANNEL) else None
                return RC.forward(tensor, self.rounding, config.scale, config.offset, axis, config.quant_min, config.quant_max)
        R.RoundTuningDelegator = TorchOpDelegator
    try:
        p = R.RoundTuningPass(steps=steps, group_weights=not arm.startswith('torch'), use_hip_graph=arm.endswith('graph'))
        p.max_blocks, p.profile_phases = blocks, True
        t0 = time.perf_counter()
        p.optimize(graph, batches, ex)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        R.RoundTuningDelegator = saved
    ph = p.phase_ms
    if arm.endswith('graph'):
        train_ms, n = ph.get('graph_replays', 0.0), p.stats['graph_replays']
    else:
        train_ms, n = ph.get('eager_steps', 0.0), p.stats['eager_steps']
    return {'arm': arm, 'blocks': len(p.report), 'steps': n, 'ms_per_step': train_ms / max(n, 1), 'pass_s': wall,
            'roundtune_weights': p.stats['roundtune_weights'], 'graph_failures': p.stats['graph_failures'],
            'flipped': p.stats['flipped'], 'tuned_elements': p.stats['tuned_elements']}


def run_floor(blocks: int):
    """Per block: FLOOR_REPEATS launches of the block's job table, then FLOOR_REPEATS copies of the same bytes."""
    from ppq_amd.blocks import split_graph_into_blocks
    from ppq_amd.ffi import roundtune_forward_multi
    from ppq_amd.roundtune import ROUND_TUNING_OP
    fl = ctypes.CDLL(FLOOR_SO)
    fl.floor_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    graph, ex, batches = setup()
    sizes = []
    for block in split_graph_into_blocks(graph, graph.topological_sort(), 5)[:blocks]:
        sets = []
        for _ in range(4):                                 # rotating buffers: no launch re-reads what the last one left in L2
            items = []
            for op in block.rps:
                if hasattr(op, 'config') and op.type in ROUND_TUNING_OP and op.inputs[1].is_parameter:
                    c, w = op.config.input_quantization_config[1], op.inputs[1].value
                    items.append((w.detach().clone(), torch.rand_like(w), c.scale.detach(), c.offset.detach(), c.channel_axis,
                                  c.quant_min, c.quant_max))
            sets.append((items, [torch.empty_like(it[0]) for it in items]))
        n = sum(it[0].numel() for it in sets[0][0])
        if n == 0: continue
        m = (n * 3 // 2 + 3) // 4 * 4                      # floats whose copy moves the same 12 n bytes
        src = [torch.rand(m, device='cuda') for _ in range(4)]
        dst = [torch.empty(m, device='cuda') for _ in range(4)]
        torch.cuda.synchronize()
        for k in range(FLOOR_REPEATS): roundtune_forward_multi(sets[k % 4][0], outs=sets[k % 4][1])
        st = torch.cuda.current_stream().cuda_stream
        for k in range(FLOOR_REPEATS):
            if fl.floor_copy(src[k % 4].data_ptr(), dst[k % 4].data_ptr(), m, 256, 2, 0, st) != 0: raise RuntimeError('floor_copy failed')
        torch.cuda.synchronize()
        sizes.append((str(block), len(sets[0][0]), n))
    return {'arm': 'floor', 'sizes': sizes}


def traced(arm: str, blocks: int, steps: int):
    """Child under rocprofv3: (kernel trace rows, child stdout) or (None, reason)."""
    rocprof = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if rocprof is None: return None, 'rocprofv3 not found'
    out = tempfile.mkdtemp(prefix='roundtune_trace_')
    cmd = [rocprof, '--kernel-trace', '--stats', '-d', out, '-o', 'run', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--child', arm, '--blocks', str(blocks), '--steps', str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    traces = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
    if r.returncode != 0 or not traces: return None, f'rc={r.returncode}; stderr tail {(r.stderr or "")[-300:]!r}'
    rows = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r['Start_Timestamp']))
    shutil.rmtree(out, ignore_errors=True)
    return rows, r.stdout


def _ns(row) -> int:
    return int(row['End_Timestamp']) - int(row['Start_Timestamp'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=6)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--child', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        print(run_floor(args.blocks) if args.child == 'floor' else run_arm(args.child, args.blocks, args.steps))
        return
    lines = [f'# tools/roundtune_bench.py --blocks {args.blocks} --steps {args.steps} --runs {args.runs}: YOLOv6-s-like, INT4 '
             f'per-channel weights, block_size 5, first {args.blocks} blocks, {args.steps} steps per block, batch 2x3x160x160, lr 1e-4',
             f'# device: {torch.cuda.get_device_name(0)}']
    arms = ('torch', 'eager', 'graph', 'torch_graph')
    for arm in arms: run_arm(arm, 1, 3)                                # warm MIOpen / the allocator for every arm
    runs = {arm: [] for arm in arms}
    for _ in range(args.runs):                                         # alternated: drift of the box hits all arms alike
        for arm in arms: runs[arm].append(run_arm(arm, args.blocks, args.steps))
    med = {}
    for arm in arms:
        ms = [r['ms_per_step'] for r in runs[arm]]
        med[arm] = statistics.median(ms)
        last = runs[arm][-1]
        lines.append(f'{arm:11s} ms/step median {med[arm]:.4f} (min {min(ms):.4f}, max {max(ms):.4f}, {len(ms)} runs); pass '
                     f'{statistics.median(r["pass_s"] for r in runs[arm]):.3f} s; {last["blocks"]} blocks, {last["steps"]} timed steps, '
                     f'{last["roundtune_weights"]} weights, graph_failures {last["graph_failures"]}, '
                     f'flipped {last["flipped"]} of {last["tuned_elements"]}')
    lines.append(f'ratio of medians, torch-op delegator / arm: eager {med["torch"] / med["eager"]:.2f}x, graph {med["torch"] / med["graph"]:.2f}x; replayed arms, torch_graph / graph: '
                 f'{med["torch_graph"] / med["graph"]:.2f}x')
    tsteps, dispatches = 20, {}
    for arm in ('torch', 'eager'):
        rows, err = traced(arm, args.blocks, tsteps)
        if rows is None:
            lines.append(f'trace {arm}: not measured ({err})')
            break                                                      # a child that failed: nothing more is started on the GPU
        dispatches[arm] = len(rows)
        lines.append(f'trace {arm}: {len(rows)} kernel dispatches for the whole child pass ({args.blocks} blocks x {tsteps} steps, plus '
                     f'calibration, pre/post losses): the per-step share is in the difference of the two arms')
        mine = [_ns(r) for r in rows if 'roundtune' in r.get('Kernel_Name', '')]
        if mine: lines.append(f'  roundtune_fwd: {len(mine)} dispatches, median {statistics.median(mine) / 1e3:.2f} us, '
                              f'min {min(mine) / 1e3:.2f} us, max {max(mine) / 1e3:.2f} us')
    if len(dispatches) == 2:
        lines.append(f'dispatches saved per step: {(dispatches["torch"] - dispatches["eager"]) / (args.blocks * tsteps):.1f}')
    rows, out = traced('floor', args.blocks, 0) if len(dispatches) == 2 else (None, 'an earlier child failed')
    if rows is None:
        lines.append(f'floor: not measured ({out})')
    else:
        sizes = ast.literal_eval(out.strip().splitlines()[-1])['sizes']  # the child's own dict literal
        both = [r for r in rows if 'roundtune' in r.get('Kernel_Name', '') or 'floor_copy' in r.get('Kernel_Name', '')]
        groups = [(k, [_ns(r) for r in g]) for k, g in itertools.groupby(both, key=lambda r: 'roundtune' in r['Kernel_Name'])]
        lines.append(f'floor: per block, {FLOOR_REPEATS} launches of its job table, then {FLOOR_REPEATS} floor_copy launches of the same '
                     'bytes (kernel-trace medians, rotating buffers)')
        if len(groups) != 2 * len(sizes):
            lines.append(f'  trace does not split into {2 * len(sizes)} runs ({len(groups)}): not reported')
        else:
            for i, (name, jobs, n) in enumerate(sizes):
                k_us, c_us = statistics.median(groups[2 * i][1]) / 1e3, statistics.median(groups[2 * i + 1][1]) / 1e3
                lines.append(f'  {name}: {jobs} jobs, {n} elements, {12 * n / 1e6:.3f} MB: roundtune_fwd {k_us:.2f} us, '
                             f'floor_copy {c_us:.2f} us, ratio {k_us / c_us:.2f}')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f: f.write(text + '\n')


if __name__ == '__main__':
    main()
