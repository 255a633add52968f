"""GEMM on packed MX tensors (ppq_amd/mx.py mx_matmul / mx_linear) on the GPU: per shape and format pair the
time of one product on the block-scaled MFMA against the only way to multiply two MX tensors without it.

  shapes  4096 x 4096 x 4096;  a ViT-B/16 MLP Gemm at batch 8: M = 1576, N = 3072, K = 768
  pairs   MXFP4 x MXFP4, MXFP8 (E4M3) x MXFP4, MXFP8 x MXFP8        (activation x weight)
  arms    mx_matmul     mx_matmul(a, b) on the two MXTensors: one launch of ppqhip_mx_gemm on the packed bytes
          torch fp32    torch.matmul in float32 on the dequantised operands (dequantised once, outside the timing)
          torch bf16    torch.matmul in bfloat16 on the same values, for orientation (not the same numbers: bf16 rounds the scaled
                        FP8 / FP6 values only where a value needs more than 8 bits, but it accumulates differently)

The operands of every arm ROTATE over 4 sets, so that a launch does not find its own lines of the last one in the 256 MiB Infinity
Cache.  A sample is the device-event time of `--launches` back-to-back calls divided by their number; `--repeats` samples per arm,
arms ALTERNATED; medians and (max - min) / median are reported.  TFLOP/s = 2 M N nb 32 over the median.
Per pair the tool also prints how far mx_linear is from the simulated path -- mx_fake_quant of both operands, then a float32
torch.matmul -- which is the prediction every MX error report of this package computes.  The last line printed is one JSON object.

    python tools/mx_gemm_bench.py [--repeats 5] [--launches 20] [--out profiles/mx_gemm.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [('4096^3', 4096, 4096, 4096), ('ViT-B/16 MLP, batch 8', 1576, 3072, 768)]
PAIRS = [('MXFP4_E2M1', 'MXFP4_E2M1'), ('MXFP8_E4M3', 'MXFP4_E2M1'), ('MXFP8_E4M3', 'MXFP8_E4M3')]
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


def bench(name, m, n, k, fa, fb, args, lines, summary):
    from ppq_amd import mx_dequantize, mx_fake_quant, mx_linear, mx_matmul, mx_quantize
    g = torch.Generator(device='cuda').manual_seed(11)
    xs = [torch.randn(m, k, device='cuda', generator=g) for _ in range(ROTATE)]
    ws = [torch.randn(n, k, device='cuda', generator=g) * 0.05 for _ in range(ROTATE)]
    a = [mx_quantize(x, fa, -1) for x in xs]
    b = [mx_quantize(w, fb, -1) for w in ws]
    a32, b32 = [mx_dequantize(t) for t in a], [mx_dequantize(t) for t in b]
    a16, b16 = [t.to(torch.bfloat16) for t in a32], [t.to(torch.bfloat16) for t in b32]
    arms = {'mx_matmul': lambda i: mx_matmul(a[i % ROTATE], b[i % ROTATE]),
            'torch fp32': lambda i: torch.matmul(a32[i % ROTATE], b32[i % ROTATE].t()),
            'torch bf16': lambda i: torch.matmul(a16[i % ROTATE], b16[i % ROTATE].t())}
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    flops = 2.0 * m * n * ((k + 31) // 32) * 32
    key = f'{name} {fa} x {fb}'
    lines.append(f'{name}: M = {m}, N = {n}, K = {k}, {fa} x {fb}, {flops / 1e9:.1f} GFLOP, operands rotating over {ROTATE} sets')
    summary[key] = {}
    base = statistics.median(times['torch fp32'])
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:12s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{flops / med / 1e9:.1f} TFLOP/s   {base / med:.2f} x torch fp32   [{min(ts):.4f}, {max(ts):.4f}]')
        summary[key][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts), 'TFLOPs': flops / med / 1e9}
    # how far the deployed layer is from the simulation
    bias = torch.linspace(-1.0, 1.0, n, device='cuda')
    y = mx_linear(xs[0], b[0], fa, bias)
    sim = torch.matmul(mx_fake_quant(xs[0], fa, -1), mx_fake_quant(ws[0], fb, -1).t()) + bias
    ref = (a32[0].double() @ b32[0].double().t() + bias.double())
    dev_sim, dev_k, dev_s = float((y - sim).abs().max()), float((y.double() - ref).abs().max()), float((sim.double() - ref).abs().max())
    top = float(ref.abs().max())
    lines.append(f'  mx_linear against the simulated path (mx_fake_quant of both, float32 torch.matmul): max |difference| {dev_sim:.3e} '
                 f'at max |output| {top:.3e} ({dev_sim / top:.2e} of it); against float64 on the same values: mx_linear {dev_k:.3e}, simulated path {dev_s:.3e}')
    summary[key]['mx_linear_vs_simulated'] = {'max_abs': dev_sim, 'max_output': top, 'kernel_vs_f64': dev_k, 'simulated_vs_f64': dev_s}
    del xs, ws, a, b, a32, b32, a16, b16
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_gemm_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_gemm_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    for name, m, n, k in SHAPES:
        for fa, fb in PAIRS: bench(name, m, n, k, fa, fb, args, lines, summary)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
