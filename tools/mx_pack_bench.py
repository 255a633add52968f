"""Packed MX export (ppq_amd/mx.py mx_quantize / mx_dequantize) on the GPU: per element format and per kernel path the time of one
pack and one unpack launch against the copy floor over the same bytes, the MX fake quant of the same tensor and the torch arm, and
the weight export of ResNet-50.

  paths   rows     [8192, 4096] along the last axis: eight lanes per 128-B block, dword stores          134 MB of float32
          strided  [32, 256, 56, 56] along axis 1 (NCHW): one lane per block, 16-B / 8-B stores           103 MB of float32
  arms    pack     ppqhip_mx_pack, one launch        unpack  ppqhip_mx_unpack, one launch
          floor    tools/floor floor_copy moving the same number of bytes (4 n + blocks * (B + 1), half read, half written), one
                   per block size B = 32 / 24 / 16, and one moving the 8 n bytes of mx_fq
          mx_fq    ppqhip_mx_fq on the same tensor (8 n bytes)
          torch    mx_quantize / mx_dequantize (use_kernels=False) on the same device

Inputs and outputs ROTATE over 4 buffers each, so that a launch finds none of its lines in the 256 MiB Infinity Cache.  A sample
is the device-event time of `--launches` back-to-back launches divided by their number; `--repeats` samples per arm, arms
ALTERNATED; medians and (max - min) / median are reported.  GB/s = the arm's own algorithmic bytes over the median.
ResNet-50: the 54 MXFP4 weights of quantize_graph_mx through export_graph_mx -- the whole call by the host clock (it builds the plan
and its arena), and the launch alone (MXPackPlan.run) against MXQuantizePlan.run on the same weights, floor_copy over the same
bytes and the torch arm.  The last line printed is one JSON object.

    python tools/mx_pack_bench.py [--repeats 5] [--launches 20] [--out profiles/mx_pack.txt] [--skip-graph]"""
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

PATHS = [('rows', (8192, 4096), -1, 4), ('strided', (32, 256, 56, 56), 1, 4)]
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


def measure(arms, args):
    """arms: name -> (fn, launches, bytes).  Warm every arm, then `--repeats` rounds with the arms alternated."""
    times = {arm: [] for arm in arms}
    for fn, _, _ in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, (fn, launches, _) in arms.items(): times[arm].append(sample(fn, launches))
    return times


def report(times, arms, floor_of, lines, out):
    for arm, ts in times.items():
        med, nbytes = statistics.median(ts), arms[arm][2]
        floor = statistics.median(times[floor_of(arm)])
        lines.append(f'  {arm:28s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{nbytes / med / 1e6:.0f} GB/s   {floor / med:.2f} of the copy floor ({floor_of(arm)})')
        out[arm] = {'ms': med, 'GBps': nbytes / med / 1e6, 'spread': spread(ts), 'of_copy_floor': floor / med}


def bench_path(name, shape, axis, rotate, args, lines, summary):
    from north_star import load_floor
    from ppq_amd import MXTensor, mx_dequantize, mx_quantize
    from ppq_amd._lib import lib
    from ppq_amd.ffi import CUDA, _mx_geometry, _stream, mx_block_bytes
    fl = load_floor()
    g = torch.Generator(device='cuda').manual_seed(7)
    xs = [torch.randn(*shape, device='cuda', generator=g) for _ in range(rotate)]
    ys = [torch.empty_like(x) for x in xs]
    n = xs[0].numel()
    axis %= len(shape)
    outer, length, inner, _ = _mx_geometry(xs[0], axis)
    blocks = outer * inner * ((length + 31) // 32)
    packed = {fmt: [CUDA.MXPack(x, fmt, axis) for x in xs] for fmt in FORMATS}           # the unpack arms read these
    tensors = {fmt: [MXTensor(fmt, shape, axis, e, s) for e, s in packed[fmt]] for fmt in FORMATS}      # the torch unpack arm rotates too
    few = max(2, args.launches // 10)
    arms = {}
    for B in (32, 24, 16):
        nbytes = 4 * n + blocks * (B + 1)
        arms[f'floor_copy B={B}'] = ((lambda c: lambda i: fl.floor_copy(xs[i % rotate].data_ptr(), ys[i % rotate].data_ptr(), c, 256, 2, 0, _stream()))(nbytes // 8),
                                     args.launches, nbytes)
    arms['floor_copy 8n'] = (lambda i: fl.floor_copy(xs[i % rotate].data_ptr(), ys[i % rotate].data_ptr(), n, 256, 2, 0, _stream()), args.launches, 8 * n)
    for k, fmt in enumerate(FORMATS):
        nbytes = 4 * n + blocks * (mx_block_bytes(fmt) + 1)
        arms[f'pack {fmt}'] = ((lambda k, p: lambda i: lib.ppqhip_mx_pack(xs[i % rotate].data_ptr(), p[i % rotate][0].data_ptr(), p[i % rotate][1].data_ptr(),
                                                                          outer, length, inner, k, _stream()))(k, packed[fmt]), args.launches, nbytes)
        arms[f'unpack {fmt}'] = ((lambda k, p: lambda i: lib.ppqhip_mx_unpack(p[i % rotate][0].data_ptr(), p[i % rotate][1].data_ptr(), ys[i % rotate].data_ptr(),
                                                                              outer, length, inner, k, _stream()))(k, packed[fmt]), args.launches, nbytes)
        arms[f'mx_fq {fmt}'] = ((lambda k: lambda i: lib.ppqhip_mx_fq(xs[i % rotate].data_ptr(), ys[i % rotate].data_ptr(), 0, outer, length, inner, k, _stream()))(k),
                                args.launches, 8 * n)
        arms[f'torch pack {fmt}'] = ((lambda f: lambda i: mx_quantize(xs[i % rotate], f, axis, use_kernels=False))(fmt), few, nbytes)
        arms[f'torch unpack {fmt}'] = ((lambda t: lambda i: mx_dequantize(t[i % rotate], use_kernels=False))(tensors[fmt]), few, nbytes)
    times = measure(arms, args)

    def floor_of(arm):
        if arm.startswith('floor_copy'): return arm
        fmt = arm.split()[-1]
        return 'floor_copy 8n' if arm.startswith('mx_fq') else f'floor_copy B={mx_block_bytes(fmt)}'
    lines.append(f'{name}: {list(shape)} along axis {axis} = [outer {outer}, axis_len {length}, inner {inner}], {n * 4 / 1e6:.0f} MB of float32, '
                 f'{blocks} blocks, rotating over {rotate} inputs and {rotate} outputs')
    summary[name] = {}
    report(times, arms, floor_of, lines, summary[name])
    del xs, ys, packed, tensors
    torch.cuda.empty_cache()


def bench_graph(args, lines, summary):
    from north_star import load_floor
    from ppq_amd import export_graph_mx, harness, quantize_graph_mx
    from ppq_amd.ffi import MXPackPlan, MXQuantizePlan, _stream
    fl = load_floor()
    graph = harness.resnet50_graph(seed=0)
    ex = harness.TorchExecutor(graph, 'cuda')
    delegators = quantize_graph_mx(graph, ex, 'MXFP4_E2M1', 'MXFP8_E4M3')
    group = next(d.group for d in delegators.values() if d.group is not None)
    items = [(var.value, fmt, axis) for var, fmt, axis in group.members]
    pack, fq = MXPackPlan(items), MXQuantizePlan(items)
    n = sum(v.numel() for v, _, _ in items)
    src, dst = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
    whole = {'export_graph_mx hip': [], 'export_graph_mx torch': []}
    for arm in whole: export_graph_mx(graph, delegators, use_kernels=arm.endswith('hip'))               # warm
    for _ in range(args.repeats):
        for arm in whole:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            exported = export_graph_mx(graph, delegators, use_kernels=arm.endswith('hip'))
            torch.cuda.synchronize(); whole[arm].append((time.perf_counter() - t0) * 1e3)
    nbytes = sum(t.nbytes for t in exported.values())
    arms = {'floor_copy': (lambda i: fl.floor_copy(src.data_ptr(), dst.data_ptr(), pack.bytes // 8, 256, 2, 0, _stream()), args.launches, pack.bytes),
            'MXPackPlan.run': (lambda i: pack.run(), args.launches, pack.bytes),
            'MXQuantizePlan.run': (lambda i: fq.run(), args.launches, fq.bytes)}
    times = measure(arms, args)
    lines.append(f'resnet50: {len(items)} MXFP4_E2M1 weights, {n} elements = {4 * n / 1e6:.1f} MB of float32 -> {nbytes / 1e6:.1f} MB packed '
                 f'(they fit the Infinity Cache, as a graph\'s weights do: no rotation)')
    summary['resnet50'] = {'weights': len(items), 'elements': n, 'packed_bytes': nbytes}
    report(times, arms, lambda arm: 'floor_copy', lines, summary['resnet50'])
    for arm, ts in whole.items():
        lines.append(f'  {arm:28s} ms per call (host clock, plan and arena built per call): ' + ' '.join(f'{t:.2f}' for t in ts) +
                     f'   median {statistics.median(ts):.2f}  spread {spread(ts) * 100:.1f} %')
        summary['resnet50'][arm] = {'ms': statistics.median(ts), 'spread': spread(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-graph', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_pack_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_pack_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    for name, shape, axis, rotate in PATHS: bench_path(name, shape, axis, rotate, args, lines, summary)
    if not args.skip_graph: bench_graph(args, lines, summary)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
