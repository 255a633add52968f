"""INT4 weights on the linear INT8 kernels (ppq_amd/int8.py Int4Weight) on the GPU: per shape the time of one
layer with the weight packed two codes per byte against the same layer with the SAME codes stored as int8, in the same run.

  shapes  GEMM (M x N x K) 4096^3 -- compute-bound: does the unpack cost anything --, 16 x 4096 x 4096 and 64 x 11008 x 4096 --
          bound by reading the weight: does halving it show --; the ResNet-50 3x3 with C = 512 at 7 x 7, batch 32
  arms    int4    int8_matmul / int8_conv2d_packed with an Int4Weight: one launch of ppqhip_int4_gemm / ppqhip_int4_conv2d
          int8    the same call with int4_unpack of that weight: one launch of ppqhip_int8_gemm / ppqhip_int8_conv2d

Both arms give float32 output with a bias, and the tool checks once per shape that they give the same bits.  The operands of every arm
ROTATE over 4 sets, so that a launch does not find its own lines of the last one in the 256 MiB Infinity Cache.  A sample is the
device-event time of `--launches` back-to-back calls divided by their number; `--repeats` samples per arm, arms ALTERNATED; medians
and (max - min) / median are reported.  TOP/s = 2 M N Kp over the median; GB/s of weight = the weight's bytes over the median.  The last
line printed is one JSON object.

    python tools/int4_bench.py [--repeats 5] [--launches 20] [--out profiles/int4.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.int8_bench import ROTATE, sample, spread  # noqa: E402

BATCH = 32
GEMMS = [('GEMM 4096 x 4096 x 4096', 4096, 4096, 4096), ('GEMM 16 x 4096 x 4096', 16, 4096, 4096), ('GEMM 64 x 11008 x 4096', 64, 11008, 4096)]
CONVS = [('3x3, C = 512, 7 x 7', 512, 7, 512, 3, 1, 1)]        # name, C, H (= W), O, kernel, stride, pad


def configs(x, w):
    """An asymmetric 0 .. 255 activation config by min / max and a per-channel symmetric -8 .. 7 weight config by max."""
    from ppq_amd import LinearQuantizationConfig
    xc = LinearQuantizationConfig(symmetrical=False, quant_min=0, quant_max=255)
    xc.scale, xc.offset = ((x.max() - x.min()) / 255).reshape(()), torch.round(-x.min() / ((x.max() - x.min()) / 255)).reshape(())
    wc = LinearQuantizationConfig(channel_axis=0, quant_min=-8, quant_max=7)
    wc.scale, wc.offset = w.abs().amax(tuple(range(1, w.dim()))) / 7, torch.zeros(w.shape[0], device=w.device)
    return xc, wc


def bench(name, xs, ws, axis, call, ops, args, lines, summary):
    from ppq_amd import int4_quantize_weight, int4_unpack, int8_quantize
    bias = torch.randn(ws[0].shape[0], device='cuda')
    cfg = [configs(x, w) for x, w in zip(xs, ws)]
    X = [int8_quantize(x, c[0], axis) for x, c in zip(xs, cfg)]
    W4 = [int4_quantize_weight(w, c[1], 1) for w, c in zip(ws, cfg)]
    W8 = [int4_unpack(w) for w in W4]
    r = lambda i: i % ROTATE
    arms = {'int4': lambda i: call(X[r(i)], W4[r(i)], bias), 'int8': lambda i: call(X[r(i)], W8[r(i)], bias)}
    same = all(torch.equal(arms['int4'](i).contiguous().view(torch.int32), arms['int8'](i).contiguous().view(torch.int32)) for i in range(ROTATE))
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2 * ROTATE)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    lines.append(f'{name}: {ops / 1e9:.1f} GOP on the instruction, operands rotating over {ROTATE} sets; the two arms give the same bits: {same}')
    summary[name] = {'same_bits': same}
    base = statistics.median(times['int8'])
    for (arm, ts), w in zip(times.items(), (W4[0], W8[0])):
        med, wbytes = statistics.median(ts), w.values.numel()
        lines.append(f'  {arm:5s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{ops / med / 1e9:.1f} TOP/s   weight {wbytes / 2 ** 20:.1f} MiB, {wbytes / med / 1e6:.0f} GB/s   {base / med:.2f} x int8   [{min(ts):.4f}, {max(ts):.4f}]')
        summary[name][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts), 'TOPs': ops / med / 1e9, 'weight_bytes': wbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/int4_bench.py measures on the GPU; none is visible')
    from ppq_amd import int8_conv2d_packed, int8_matmul
    lines = [f'# tools/int4_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    g = torch.Generator(device='cuda').manual_seed(11)
    for name, m, n, k in GEMMS:
        xs = [torch.randn(m, k, device='cuda', generator=g) for _ in range(ROTATE)]
        ws = [torch.randn(n, k, device='cuda', generator=g) * 0.05 for _ in range(ROTATE)]
        bench(name, xs, ws, -1, int8_matmul, 2.0 * m * n * ((k + 31) // 32 * 32), args, lines, summary)
        del xs, ws
        torch.cuda.empty_cache()
    for name, c, hw, o, k, stride, pad in CONVS:
        xs = [torch.randn(BATCH, c, hw, hw, device='cuda', generator=g).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
        ws = [(torch.randn(o, c, k, k, device='cuda', generator=g) * 0.05).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
        oh = (hw + 2 * pad - k) // stride + 1
        bench(f'{name}, batch {BATCH}', xs, ws, 1, lambda x, w, b: int8_conv2d_packed(x, w, b, stride, pad), 2.0 * BATCH * oh * oh * o * k * k * ((c + 31) // 32 * 32),
              args, lines, summary)
        del xs, ws
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
