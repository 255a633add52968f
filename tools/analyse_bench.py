"""graphwise_error_analyse on the ResNet-50 harness graph (batch 32 x 3 x 224 x 224, KL-calibrated INT8, steps = 8: 9 batches
per phase, 54 analysed operations): wall time per analysis for three arms, what the analysis launches, and the whole-tensor
measure launch against the memory system.

  torch : use_kernels=False -- the reference's procedure: index_select, one copy to the CPU per operation and batch, the
          measure there in fp32 (its index tables are made once and kept, which the reference does not do: the arm is faster
          than the reference itself)
  hip   : the kernels, 4096 samples per batch element (the default)
  whole : the kernels, fetchs=None: every element of every analysed output

Wall time = host clock around one analysis that ends in a device synchronise, the arms ALTERNATED in one process (torch hip
torch hip ...).  Per-launch times and dispatch counts come from a child of its own under `rocprofv3 --kernel-trace --stats`
(arm given by --child).  The whole-tensor launch's bytes are computed from the shapes (8 B per element: p and r once).

    python tools/analyse_bench.py [--repeats 4] [--method snr] [--out profiles/r09_analyse.txt]"""
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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

STEPS = 8
KERNELS = ('fetch_rows_kernel', 'measure_rows_kernel', 'measure_fold_kernel', 'measure_finish_kernel')


def setup(batch=32, size=224):
    from ppq_amd import harness
    from ppq_amd.calibration import RuntimeCalibrationPass
    torch.manual_seed(0)
    graph = harness.resnet50_graph(seed=0)
    harness.quantize_graph(graph, 'kl', hist_bins=2048)
    ex = harness.TorchExecutor(graph, 'cuda')
    harness.ParameterQuantizePass().optimize(graph)
    g = torch.Generator().manual_seed(9)
    batches = [torch.rand(batch, 3, size, size, generator=g).to('cuda') for _ in range(STEPS + 1)]
    RuntimeCalibrationPass(method='kl').optimize(graph, dataloader=batches, executor=ex, calib_steps=STEPS)
    return graph, ex, batches


def analyse_once(arm, graph, ex, batches, method):
    from ppq_amd import analyse
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = analyse.graphwise_error_analyse(graph, 'cuda', batches, method=method, steps=STEPS, verbose=False,
                                          fetchs=None if arm == 'whole' else 4096, executor=ex, use_kernels=(arm != 'torch'))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res, dict(analyse.last_analysis_stats)


def traced(arm, method):
    rocprof = shutil.which('rocprofv3') or ('/opt/rocm/bin/rocprofv3' if os.path.exists('/opt/rocm/bin/rocprofv3') else None)
    if rocprof is None: return None, 'rocprofv3 not found'
    out = tempfile.mkdtemp(prefix='analyse_trace_')
    cmd = [rocprof, '--kernel-trace', '--stats', '-d', out, '-o', 'run', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--child', arm, '--method', method]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    traces = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
    if r.returncode != 0 or not traces: return None, f'rc={r.returncode}; stderr tail {(r.stderr or "")[-300:]!r}'
    rows = list(csv.DictReader(open(traces[0])))
    shutil.rmtree(out, ignore_errors=True)
    return rows, None


def spread(values): return (max(values) - min(values)) / statistics.median(values)


def reference_agreement():
    """The measures on the device against the reference's recorded values (tests/golden/analyse.npz): maxima, a record."""
    import analyse_cases as C
    from ppq_amd import measure
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'analyse.npz'))
    fn = {'snr': measure.torch_snr_error, 'mse': measure.torch_mean_square_error, 'cosine': measure.torch_cosine_similarity}
    lines = []
    for method in C.METHODS:
        worst = (0.0, None, 0)
        for k, (name, shape) in enumerate(C.MEASURE_CASES):
            pred, real = (t.cuda() for t in C.measure_tensors(k))
            ref = gold[f'measure_{name}_{method}_none']
            err = np.abs(fn[method](pred, real, 'none').cpu().numpy().astype(np.float64) - ref)
            ulps = float((err / (2.0 ** -23 if method == 'cosine' else np.spacing(np.abs(ref)))).max())
            count = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
            if ulps >= worst[0]: worst = (ulps, name, count)
        lines.append(f'device vs the reference\'s recorded fp32 values, {method}: at most {worst[0]:.2f} fp32 ulps'
                     f'{" (of 1.0)" if method == "cosine" else ""} over {len(C.MEASURE_CASES)} cases (case {worst[1]}, count {worst[2]})')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=4)
    ap.add_argument('--method', default='snr')
    ap.add_argument('--child', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    graph, ex, batches = setup()
    if args.child:
        analyse_once(args.child, graph, ex, batches[:2], args.method)                      # warm: index tables, scratch, MIOpen
        print(analyse_once(args.child, graph, ex, batches, args.method)[0])
        return
    from ppq_amd import harness
    ops = [op for op in graph.operations.values() if hasattr(op, 'config') and op.type in harness.COMPUTING_OP]
    lines = [f'# tools/analyse_bench.py --repeats {args.repeats} --method {args.method}: ResNet-50 harness graph, KL-calibrated INT8, '
             f'batch 32 x 3 x 224 x 224, steps = {STEPS} ({STEPS + 1} batches per phase), {len(ops)} analysed operations',
             f'# device: {torch.cuda.get_device_name(0)}']
    times = {'torch': [], 'hip': [], 'whole': []}
    results = {}
    for arm in times: analyse_once(arm, graph, ex, batches, args.method)                   # warm every arm once
    for _ in range(args.repeats):
        for arm in ('torch', 'hip', 'whole'):                                              # alternated
            t, results[arm], stats = analyse_once(arm, graph, ex, batches, args.method)
            times[arm].append(t)
            print(f'{arm} {t:.3f} s', file=sys.stderr, flush=True)
            results[arm + '_stats'] = stats
    for arm, ts in times.items():
        lines.append(f'{arm:6s} wall s per analysis: ' + ' '.join(f'{t:.3f}' for t in ts) +
                     f'   median {statistics.median(ts):.3f}  min {min(ts):.3f}  max {max(ts):.3f}  spread {spread(ts) * 100:.1f} %   {results[arm + "_stats"]}')
    mt, mh = statistics.median(times['torch']), statistics.median(times['hip'])
    lines.append(f'hip over torch: {mt / mh:.2f}x by the medians ({(mt - mh) * 1e3:.0f} ms less per analysis); slowest hip run {max(times["hip"]):.3f} s, '
                 f'fastest torch run {min(times["torch"]):.3f} s')
    fwd = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for b in batches: ex.forward(b)
        torch.cuda.synchronize(); fwd.append((time.perf_counter() - t0) / len(batches))
    lines.append(f'for scale: one quantised forward without hooks (epilogues fused) {statistics.median(fwd) * 1e3:.1f} ms; an analysis runs {2 * (STEPS + 1)}')
    worst = max(abs(results['hip'][k] - results['torch'][k]) / max(abs(results['torch'][k]), 1e-30) for k in results['torch'])
    lines.append(f'hip vs torch results ({args.method}, MIOpen convolutions do not repeat bit for bit between runs): largest relative difference {worst:.2e}')
    top = sorted(results['hip'].items(), key=lambda kv: -kv[1])[:3]
    lines.append('largest three (hip, sampled): ' + ', '.join(f'{k} {v:.5f}' for k, v in top) +
                 ';  whole tensors: ' + ', '.join(f'{k} {results["whole"][k]:.5f}' for k, _ in top))
    # bytes of the whole-tensor measure launch of one forward, from the shapes
    from ppq_amd import analyse
    hooks = {op.name: analyse.OutputKeeper(op) for op in ops}
    with torch.no_grad(): ex.forward(inputs=batches[0], hooks=hooks)
    elems = sum(h.kept.numel() for h in hooks.values())
    for h in hooks.values(): h.kept = None
    whole_bytes = 8.0 * elems
    lines.append(f'whole-tensor measure launch: {elems / 1e6:.1f} M elements in {len(ops)} jobs = {whole_bytes / 1e9:.3f} GB per forward (8 B per element)')
    for arm in ('torch', 'hip', 'whole'):
        print(f'tracing {arm} ...', file=sys.stderr, flush=True)
        rows, err = traced(arm, args.method)
        if rows is None:
            lines.append(f'trace {arm}: not measured ({err})')
            continue
        per = {}
        for r in rows:
            name = r.get('Kernel_Name', '')
            for k in KERNELS:
                if k in name: per.setdefault(k, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
        lines.append(f'trace {arm}: {len(rows)} kernel dispatches in the child (calibration, warm-up and one analysis)')
        for k, us in per.items():
            lines.append(f'  {k}: {len(us)} dispatches, median {statistics.median(us):.2f} us, min {min(us):.2f}, max {max(us):.2f}')
        if arm == 'whole' and 'measure_rows_kernel' in per:
            big = sorted(per['measure_rows_kernel'])[-(STEPS + 1):]                         # the full-batch launches of the timed analysis
            fold = statistics.median(sorted(per.get('measure_fold_kernel', [0.0]))[-(STEPS + 1):])
            med = statistics.median(big)
            lines.append(f'  whole-tensor measure_rows_kernel: {whole_bytes / (med * 1e-6) / 1e12:.2f} TB/s = {whole_bytes / (med * 1e-6) / 8e12:.3f} of 8 TB/s '
                         f'(median {med:.1f} us); with its fold launch ({fold:.1f} us): {whole_bytes / ((med + fold) * 1e-6) / 8e12:.3f}')
    lines += reference_agreement()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f: f.write(text + '\n')


if __name__ == '__main__':
    main()
