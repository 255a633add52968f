"""MX fake quant (ppq_amd/mx.py) on the GPU: per element format and per kernel path the time of one launch against the copy floor,
the existing FP8 fake quant and the torch arm, and one end-to-end line per graph.

  paths   rows     [8192, 4096] along the last axis (a Gemm activation): eight lanes per 128-B block       134 MB in, 134 MB out
          strided  [32, 256, 56, 56] along axis 1 (an NCHW conv activation): lanes along H*W               103 MB in, 103 MB out
          weight3  [512, 512, 3, 3] along axis 1 (a 3x3 conv weight, inner = 9)                              9 MB in,   9 MB out
  arms    hip      CUDA.MXQuantize, one launch                       floor  tools/floor floor_copy on the same bytes
          fp8      CUDA.FloatingQuantize_T (per tensor, E4M3) at the same size
          torch    mx_fake_quant(use_kernels=False) on the same device: about fifteen launches and several temporaries

Inputs and outputs ROTATE over 4 buffers each for the two large paths, so that a launch finds none of its lines in the 256 MiB
Infinity Cache (8 x 134 MB resp. 8 x 103 MB in play); weight3 rotates over 8 (151 MB: it DOES fit, as a graph's weights do).  A
sample is the device-event time of `--launches` back-to-back launches divided by their number; `--repeats` samples per arm, arms
ALTERNATED; medians and (max - min) / median are reported.  GB/s = 8 bytes per element (one read, one write) over the median.
End to end: ResNet-50 (batch 32) and ViT-B/16 (batch 8) forwards with quantize_graph_mx (MXFP4 weights, MXFP8-E4M3 activations),
host clock around a forward that ends in a synchronise, both arms alternated.  The last line printed is one JSON object.

    python tools/mx_bench.py [--repeats 5] [--launches 20] [--out profiles/mx.txt] [--skip-graphs]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PATHS = [('rows', (8192, 4096), -1, 4), ('strided', (32, 256, 56, 56), 1, 4), ('weight3', (512, 512, 3, 3), 1, 8)]
FORMATS = ['MXFP8_E4M3', 'MXFP8_E5M2', 'MXFP6_E3M2', 'MXFP6_E2M3', 'MXFP4_E2M1', 'MXINT8']


def spread(values): return (max(values) - min(values)) / statistics.median(values)


def sample(fn, launches):
    """Milliseconds per launch of `launches` back-to-back calls of fn(i), by one device-event pair."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(launches): fn(i)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / launches


def bench_path(name, shape, axis, rotate, args, lines, summary):
    from north_star import load_floor
    from ppq_amd import CUDA, mx_fake_quant
    from ppq_amd._lib import lib
    from ppq_amd.ffi import _mx_geometry, _stream
    fl = load_floor()
    g = torch.Generator(device='cuda').manual_seed(7)
    xs = [torch.randn(*shape, device='cuda', generator=g) for _ in range(rotate)]
    outs = [torch.empty_like(x) for x in xs]
    n = xs[0].numel()
    outer, length, inner, _ = _mx_geometry(xs[0], axis % len(shape))
    one, zero = torch.ones(1, device='cuda'), torch.zeros(1, device='cuda')

    def hip(fmt_id): return lambda i: lib.ppqhip_mx_fq(xs[i % rotate].data_ptr(), outs[i % rotate].data_ptr(), 0, outer, length, inner, fmt_id, _stream())
    arms = {'floor_copy': (lambda i: fl.floor_copy(xs[i % rotate].data_ptr(), outs[i % rotate].data_ptr(), n, 256, 2, 0, _stream()), args.launches),
            'fp8 FloatingQuantize_T': (lambda i: CUDA.FloatingQuantize_T(xs[i % rotate], one, zero), args.launches)}
    for k, fmt in enumerate(FORMATS):
        arms[f'hip {fmt}'] = (hip(k), args.launches)
        arms[f'torch {fmt}'] = ((lambda f: lambda i: mx_fake_quant(xs[i % rotate], f, axis, use_kernels=False))(fmt), max(2, args.launches // 10))
    times = {arm: [] for arm in arms}
    for arm, (fn, launches) in arms.items(): sample(fn, 2)                              # warm every arm
    for _ in range(args.repeats):
        for arm, (fn, launches) in arms.items():                                         # alternated
            times[arm].append(sample(fn, launches))
    lines.append(f'{name}: {list(shape)} along axis {axis} = [outer {outer}, axis_len {length}, inner {inner}], {n * 4 / 1e6:.0f} MB, rotating over {rotate} inputs and {rotate} outputs')
    floor = statistics.median(times['floor_copy'])
    summary[name] = {}
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:24s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{8 * n / med / 1e6:.0f} GB/s   {floor / med:.2f} of the copy floor')
        summary[name][arm] = {'ms': med, 'GBps': 8 * n / med / 1e6, 'spread': spread(ts), 'of_copy_floor': floor / med}
    del xs, outs
    torch.cuda.empty_cache()


def bench_graph(kind, args, lines, summary):
    from ppq_amd import harness, quantize_graph_mx
    batch, size = (32, 224) if kind == 'resnet50' else (8, 224)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(batch, 3, size, size, generator=g).to('cuda')
    execs = {}
    for arm, use_kernels in (('hip', True), ('torch', False)):
        graph = harness.resnet50_graph(seed=0) if kind == 'resnet50' else harness.vit_graph(seed=0)
        ex = harness.TorchExecutor(graph, 'cuda')
        quantize_graph_mx(graph, ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=use_kernels)
        execs[arm] = ex
    times = {arm: [] for arm in execs}
    outs = {}
    for arm, ex in execs.items(): outs[arm] = ex.forward(x)[0]                           # warm
    for _ in range(args.repeats):
        for arm, ex in execs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ex.forward(x)
            torch.cuda.synchronize(); times[arm].append((time.perf_counter() - t0) * 1e3)
    same = bool(torch.equal(outs['hip'].view(torch.int32), outs['torch'].view(torch.int32)))
    lines.append(f'{kind}: batch {batch}, MXFP4_E2M1 weights, MXFP8_E4M3 activations, one forward; outputs of the two arms identical: {same}')
    summary[kind] = {'identical': same}
    for arm, ts in times.items():
        lines.append(f'  {arm:6s} ms per forward: ' + ' '.join(f'{t:.2f}' for t in ts) + f'   median {statistics.median(ts):.2f}  spread {spread(ts) * 100:.1f} %')
        summary[kind][arm + '_ms'] = statistics.median(ts)
    del execs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-graphs', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    for name, shape, axis, rotate in PATHS: bench_path(name, shape, axis, rotate, args, lines, summary)
    if not args.skip_graphs:
        for kind in ('resnet50', 'vit'): bench_graph(kind, args, lines, summary)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
