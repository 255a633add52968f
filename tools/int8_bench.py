"""Linear INT8 layers on the int8 MFMA (ppq_amd/int8.py) on the GPU: per shape the time of one layer with the
chained int32 accumulator against the two other ways this repository computes it, in the same run.

  shapes  GEMM 4096^3 and 1576 x 3072 x 768 (M x N x K); ResNet-50 at batch 32: 3x3 with C = 64 at 56 x 56, 1x1 from 256 to 64 at
          56 x 56, 3x3 with C = 512 at 7 x 7, and the 7x7 / 2 stem (C = 3)
  arms    int8             int8_matmul / int8_conv2d_packed on two Int8Tensors, float32 output, bias
          int8 fused       the same launch with ReLU and the result re-quantised to int8 codes only (out_config, out_float=False)
          mx_int8          mx_int8_matmul / mx_int8_conv2d_packed on the same values as MXINT8, float32 output, bias
          mx_int8 fused    the same with ReLU and the result packed as MXINT8 only
          simulated        the simulated layer: LinearQuantize_T on the activation, LinearQuantize_C on the weight, then a float32
                           matmul / F.conv2d with the bias

The operands of every arm ROTATE over 4 sets, so that a launch does not find its own lines of the last one in the 256 MiB Infinity
Cache.  A sample is the device-event time of `--launches` back-to-back calls divided by their number; `--repeats` samples per arm,
arms ALTERNATED; medians and (max - min) / median are reported.  TOP/s = 2 M N Kp over the median.  Per shape the tool also states how
far the int8 arm is from the simulated layer.  The last line printed is one JSON object.

    python tools/int8_bench.py [--repeats 5] [--launches 20] [--out profiles/int8.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 32
GEMMS = [('GEMM 4096 x 4096 x 4096', 4096, 4096, 4096), ('GEMM 1576 x 3072 x 768', 1576, 3072, 768)]
# name, C, H (= W), O, kernel, stride, pad
CONVS = [('3x3, C = 64, 56 x 56', 64, 56, 64, 3, 1, 1), ('1x1, 256 -> 64, 56 x 56', 256, 56, 64, 1, 1, 0), ('3x3, C = 512, 7 x 7', 512, 7, 512, 3, 1, 1),
         ('stem 7x7/2, C = 3, 224 x 224', 3, 224, 64, 7, 2, 3)]
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


def configs(x, w):
    """An asymmetric 0 .. 255 activation config and a per-channel symmetric weight config by min / max, and the output's."""
    from ppq_amd import LinearQuantizationConfig
    xc = LinearQuantizationConfig(symmetrical=False, quant_min=0, quant_max=255)
    xc.scale, xc.offset = ((x.max() - x.min()) / 255).reshape(()), torch.round(-x.min() / ((x.max() - x.min()) / 255)).reshape(())
    wc = LinearQuantizationConfig(channel_axis=0, quant_min=-127, quant_max=127)
    wc.scale, wc.offset = w.abs().amax(tuple(range(1, w.dim()))) / 127, torch.zeros(w.shape[0], device=w.device)
    oc = LinearQuantizationConfig(symmetrical=False, quant_min=0, quant_max=255)
    oc.scale, oc.offset = torch.tensor(0.05), torch.tensor(0.)     # host tensors: the launch takes the output grid as scalars, and reading them
    return xc, wc, oc                                               # from device memory would cost a synchronisation per call


def bench(name, conv, xs, ws, axis, call, mx_call, sim_call, ops, args, lines, summary):
    from ppq_amd import CUDA, int8_quantize, mx_quantize
    bias = torch.randn(ws[0].shape[0], device='cuda')
    cfg = [configs(x, w) for x, w in zip(xs, ws)]
    X, W = [int8_quantize(x, c[0], axis) for x, c in zip(xs, cfg)], [int8_quantize(w, c[1], 1, weight=True) for w, c in zip(ws, cfg)]
    MX, MW = [mx_quantize(x, 'MXINT8', axis) for x in xs], [mx_quantize(w, 'MXINT8', 1) for w in ws]
    fq = lambda t, c, ch: (CUDA.LinearQuantize_C(t, c.scale, c.offset, 0, c.quant_min, c.quant_max) if ch else
                           CUDA.LinearQuantize_T(t, c.scale.reshape(1), c.offset.reshape(1), c.quant_min, c.quant_max))
    r = lambda i: i % ROTATE
    arms = {'int8': lambda i: call(X[r(i)], W[r(i)], bias),
            'int8 fused': lambda i: call(X[r(i)], W[r(i)], bias, relu=True, out_config=cfg[r(i)][2], out_float=False),
            'mx_int8': lambda i: mx_call(MX[r(i)], MW[r(i)], bias),
            'mx_int8 fused': lambda i: mx_call(MX[r(i)], MW[r(i)], bias, relu=True, out_format='MXINT8', out_float=False),
            'simulated': lambda i: sim_call(fq(xs[r(i)], cfg[r(i)][0], False), fq(ws[r(i)], cfg[r(i)][1], True), bias)}
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    lines.append(f'{name}: {ops / 1e9:.1f} GOP on the instruction, operands rotating over {ROTATE} sets')
    summary[name] = {}
    base, mx = statistics.median(times['simulated']), statistics.median(times['mx_int8'])
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:14s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{ops / med / 1e9:.1f} TOP/s   {base / med:.2f} x simulated   {mx / med:.2f} x mx_int8   [{min(ts):.4f}, {max(ts):.4f}]')
        summary[name][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts), 'TOPs': ops / med / 1e9}
    y, sim = arms['int8'](0), arms['simulated'](0)
    diff, top = float((y - sim).abs().max()), float(sim.abs().max())
    lines.append(f'  int8 against the simulated layer on the same configs: max |difference| {diff:.3e} at max |output| {top:.3e}')
    summary[name]['checks'] = {'int8_vs_simulated': diff, 'max_output': top}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/int8_bench.py measures on the GPU; none is visible')
    from ppq_amd import int8_conv2d_packed, int8_matmul, mx_int8_conv2d_packed, mx_int8_matmul
    lines = [f'# tools/int8_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    g = torch.Generator(device='cuda').manual_seed(11)
    for name, m, n, k in GEMMS:
        xs = [torch.randn(m, k, device='cuda', generator=g) for _ in range(ROTATE)]
        ws = [torch.randn(n, k, device='cuda', generator=g) * 0.05 for _ in range(ROTATE)]
        bench(name, False, xs, ws, -1, int8_matmul, mx_int8_matmul, lambda x, w, b: torch.addmm(b, x, w.t()), 2.0 * m * n * ((k + 31) // 32 * 32), args, lines, summary)
        del xs, ws
        torch.cuda.empty_cache()
    for name, c, hw, o, k, stride, pad in CONVS:
        xs = [torch.randn(BATCH, c, hw, hw, device='cuda', generator=g).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
        ws = [(torch.randn(o, c, k, k, device='cuda', generator=g) * 0.05).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
        oh = (hw + 2 * pad - k) // stride + 1
        conv = lambda f: (lambda x, w, b, **kw: f(x, w, b, stride, pad, **kw))
        bench(f'{name}, batch {BATCH}', True, xs, ws, 1, conv(int8_conv2d_packed), conv(mx_int8_conv2d_packed), lambda x, w, b: F.conv2d(x, w, b, stride, pad),
              2.0 * BATCH * oh * oh * o * k * k * ((c + 31) // 32 * 32), args, lines, summary)
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
