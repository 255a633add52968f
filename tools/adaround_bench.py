"""AdaroundPass on the YOLOv6-s-like graph (INT4 per-channel weights, block_size 4, first k blocks, N steps per block):
ms per training step for three arms, the launches per step, and the two AdaRound kernels' bytes / time.

  torch : the reference's torch-op delegator (legacy.py:122-132, restated below), one eager step at a time
  eager : the HIP kernels, grouped launches, eager steps
  graph : the HIP kernels, grouped launches, the step captured once and replayed (the default)

ms per step = device-synchronised wall time of the training loop (the pass's own phase timers) / steps.  Launches per step and
the kernel statistics come from a child run under `rocprofv3 --kernel-trace --stats` (arm given by --child).

    python tools/adaround_bench.py [--blocks 6] [--steps 200] [--out profiles/r08_adaround.txt]"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


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
    import ppq_amd.adaround as A
    graph, ex, batches = setup()
    saved = A.AdaRoundDelegator
    if arm == 'torch':
        import adaround_cases as AC

        class TorchOpDelegator(saved):                 # the reference's __call__: ~11 torch kernels forward, 15-20 backward
            def __call__(self, tensor, config):
                axis = config.channel_axis if config.policy.has_property(A.P.PER_CHANNEL) else None
                return AC.forward(tensor, self.rounding, config.scale, config.offset, axis, config.quant_min, config.quant_max)
        A.AdaRoundDelegator = TorchOpDelegator
    try:
        p = A.AdaroundPass(steps=steps, tune_steps=0, group_weights=(arm != 'torch'), use_hip_graph=(arm == 'graph'))
        p.max_blocks, p.profile_phases = blocks, True
        t0 = time.perf_counter()
        p.optimize(graph, batches, ex)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        A.AdaRoundDelegator = saved
    ph = p.phase_ms
    if arm == 'graph':
        train_ms = ph.get('graph_replays', 0.0)
        n = p.stats['graph_replays']
    else:
        train_ms = ph.get('eager_steps', 0.0)
        n = p.stats['eager_steps']
    return {'arm': arm, 'blocks': len(p.report), 'steps': n, 'ms_per_step': train_ms / max(n, 1), 'pass_s': wall,
            'adaround_weights': p.stats['adaround_weights'], 'graph_failures': p.stats['graph_failures']}


def traced(arm: str, blocks: int, steps: int):
    """Child under rocprofv3: (kernel dispatches, adaround kernel rows) or (None, reason)."""
    rocprof = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if rocprof is None: return None, 'rocprofv3 not found'
    out = tempfile.mkdtemp(prefix='adaround_trace_')
    cmd = [rocprof, '--kernel-trace', '--stats', '-d', out, '-o', 'run', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--child', arm, '--blocks', str(blocks), '--steps', str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    traces = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
    if r.returncode != 0 or not traces: return None, f'rc={r.returncode}; stderr tail {(r.stderr or "")[-300:]!r}'
    rows = list(csv.DictReader(open(traces[0])))
    shutil.rmtree(out, ignore_errors=True)
    return rows, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=6)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--child', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.child:
        print(run_arm(args.child, args.blocks, args.steps))
        return
    lines = [f'# tools/adaround_bench.py --blocks {args.blocks} --steps {args.steps}: YOLOv6-s-like, INT4 per-channel weights, '
             f'block_size 4, first {args.blocks} blocks, {args.steps} steps per block, batch 2x3x160x160, scale tuning off',
             f'# device: {torch.cuda.get_device_name(0)}']
    res = {}
    for arm in ('torch', 'eager', 'graph'):
        run_arm(arm, 1, 3)                                       # warm MIOpen / the allocator for this arm
        res[arm] = run_arm(arm, args.blocks, args.steps)
        lines.append(f'{arm:6s} {res[arm]}')
    lines.append(f'speed-up per step: eager {res["torch"]["ms_per_step"] / res["eager"]["ms_per_step"]:.2f}x, '
                 f'graph {res["torch"]["ms_per_step"] / res["graph"]["ms_per_step"]:.2f}x over the torch-op delegator')
    tsteps = 20
    for arm in ('torch', 'eager'):
        rows, err = traced(arm, args.blocks, tsteps)
        if rows is None:
            lines.append(f'trace {arm}: not measured ({err})')
            continue
        total = len(rows)
        ada = {}
        for r in rows:
            name = r.get('Kernel_Name', '')
            if 'adaround' not in name: continue
            k = 'adaround_bwd' if 'bwd' in name else 'adaround_fwd'
            ns = int(r['End_Timestamp']) - int(r['Start_Timestamp'])
            a = ada.setdefault(k, [0, 0]); a[0] += 1; a[1] += ns
        steps_total = args.blocks * tsteps
        lines.append(f'trace {arm}: {total} kernel dispatches for the whole child pass ({args.blocks} blocks x {tsteps} steps, '
                     f'plus calibration, pre/post losses): the per-step share is in the difference of the two arms below')
        for k, (cnt, ns) in sorted(ada.items()):
            lines.append(f'  {k}: {cnt} dispatches, {ns / cnt / 1e3:.2f} us each')
        res[arm]['dispatches'] = total
    if 'dispatches' in res['torch'] and 'dispatches' in res['eager']:
        lines.append(f'dispatches saved per step: {(res["torch"]["dispatches"] - res["eager"]["dispatches"]) / (args.blocks * tsteps):.1f}')
    # the two kernels' algorithmic bytes / time through the library's own event brackets
    from ppq_amd import _lib
    graph, ex, batches = setup()
    import ppq_amd.adaround as A
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    p = A.AdaroundPass(steps=args.steps, tune_steps=0, use_hip_graph=False)
    p.max_blocks = args.blocks
    p.optimize(graph, batches, ex)
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 32)()
    n = _lib.lib.ppqhip_prof_collect(arr, 32)
    for i in range(n):
        e = arr[i]
        name = e.name.decode()
        if not name.startswith('adaround'): continue
        lines.append(f'prof {name}: {e.launches} launches, {e.total_ms / e.launches * 1e3:.2f} us/launch (event-bracketed), '
                     f'{e.total_bytes / e.launches / 1e6:.3f} MB/launch, {e.total_bytes / (e.total_ms * 1e-3) / 1e12:.3f} TB/s')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f: f.write(text + '\n')


if __name__ == '__main__':
    main()
