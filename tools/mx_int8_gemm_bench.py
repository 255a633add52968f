"""GEMM on two MXINT8 tensors (ppq_amd/mx.py mx_int8_matmul) on the GPU: per shape the time of one product on
the int8 MFMA against the only way to multiply two MXINT8 tensors without it.

  shapes  4096 x 4096 x 4096;  a ViT-B/16 MLP Gemm at batch 8: M = 1576, N = 3072, K = 768
  arms    mx_int8_matmul  mx_int8_matmul(a, b) on the two MXTensors: one launch of ppqhip_mx_int8_gemm on the packed bytes
          torch fp32      torch.matmul in float32 on the dequantised operands (dequantised once, outside the timing)
          mx_matmul e4m3  for orientation: mx_matmul on the same values quantised to MXFP8_E4M3 x MXFP8_E4M3 (the block-scaled MFMA;
                          other numbers: another element grid and the hardware's accumulation order)

The operands of every arm ROTATE over 4 sets, so that a launch does not find its own lines of the last one in the 256 MiB Infinity
Cache.  A sample is the device-event time of `--launches` back-to-back calls divided by their number; `--repeats` samples per arm,
arms ALTERNATED; medians and (max - min) / median are reported.  TOP/s = 2 M N nb 32 over the median.  Per shape the tool also
prints how far mx_int8_matmul is from float64 on the same values next to the float32 torch.matmul.  The last line printed is one
JSON object.

    python tools/mx_int8_gemm_bench.py [--repeats 5] [--launches 20] [--out profiles/mx_int8_gemm.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [('4096^3', 4096, 4096, 4096), ('ViT-B/16 MLP, batch 8', 1576, 3072, 768)]
ROTATE = 4


def spread(values): return (max(values) - min(values)) / statistics.median(values)


def sample(fn, launches):
    """Milliseconds per call of `launches` back-to-back calls of fn(i), by one device-event pair."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(launches): fn(i)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / launches


def bench(name, m, n, k, args, lines, summary):
    from ppq_amd import mx_dequantize, mx_int8_matmul, mx_matmul, mx_quantize
    g = torch.Generator(device='cuda').manual_seed(11)
    xs = [torch.randn(m, k, device='cuda', generator=g) for _ in range(ROTATE)]
    ws = [torch.randn(n, k, device='cuda', generator=g) * 0.05 for _ in range(ROTATE)]
    a, b = [mx_quantize(x, 'MXINT8', -1) for x in xs], [mx_quantize(w, 'MXINT8', -1) for w in ws]
    a32, b32 = [mx_dequantize(t) for t in a], [mx_dequantize(t) for t in b]
    a8, b8 = [mx_quantize(x, 'MXFP8_E4M3', -1) for x in xs], [mx_quantize(w, 'MXFP8_E4M3', -1) for w in ws]
    arms = {'mx_int8_matmul': lambda i: mx_int8_matmul(a[i % ROTATE], b[i % ROTATE]),
            'torch fp32': lambda i: torch.matmul(a32[i % ROTATE], b32[i % ROTATE].t()),
            'mx_matmul e4m3': lambda i: mx_matmul(a8[i % ROTATE], b8[i % ROTATE])}
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    ops = 2.0 * m * n * ((k + 31) // 32) * 32
    lines.append(f'{name}: M = {m}, N = {n}, K = {k}, MXINT8 x MXINT8, {ops / 1e9:.1f} GOP, operands rotating over {ROTATE} sets')
    summary[name] = {}
    base = statistics.median(times['torch fp32'])
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:14s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{ops / med / 1e9:.1f} TOP/s   {base / med:.2f} x torch fp32   [{min(ts):.4f}, {max(ts):.4f}]')
        summary[name][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts), 'TOPs': ops / med / 1e9}
    ref = a32[0].double() @ b32[0].double().t()
    dev_k, dev_t = float((mx_int8_matmul(a[0], b[0]).double() - ref).abs().max()), float((torch.matmul(a32[0], b32[0].t()).double() - ref).abs().max())
    lines.append(f'  against float64 on the same values, max |difference|: mx_int8_matmul {dev_k:.3e}, float32 torch.matmul {dev_t:.3e} '
                 f'at max |output| {float(ref.abs().max()):.3e}')
    summary[name]['vs_f64'] = {'mx_int8_matmul': dev_k, 'torch_fp32': dev_t, 'max_output': float(ref.abs().max())}
    del xs, ws, a, b, a32, b32, a8, b8
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_int8_gemm_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_int8_gemm_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    for name, m, n, k in SHAPES: bench(name, m, n, k, args, lines, summary)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
