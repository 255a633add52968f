"""The depthwise linear INT8 layer on v_dot4c_i32_i8 (ppq_amd/int8.py int8_depthwise_conv2d_packed) on the GPU:
per shape the time of one layer against the simulated layer the executor runs today, in the same run.

  shapes  the depthwise classes of MobileNetV2 at batch 32, C @ H (= W) and stride, 3 x 3 with padding 1: 32@112 s1, 96@112 s2,
          144@56 s1, 144@56 s2, 192@28 s1, 384@14 s1, 576@14 s2, 960@7 s1 -- and one 5 x 5 with padding 2: 240@28 s2
  arms    int8         int8_depthwise_conv2d_packed on an Int8Tensor and an Int8DepthwiseWeight, float32 output, bias
          int8 fused   the same launch with ReLU and the result re-quantised to int8 codes only (out_config, out_float=False)
          simulated    F.conv2d(groups=C) in float32 on the dequantised operands, channels-last, with the bias

The operands of every arm ROTATE over 4 sets, so that a launch does not find its own lines of the last one in the 256 MiB Infinity
Cache.  A sample is the device-event time of `--launches` back-to-back calls divided by their number; `--repeats` samples per arm,
arms ALTERNATED; medians, min / max and (max - min) / median are reported.  The bytes of an arm are what its algorithm needs, computed
here from the shapes: the operands once, the channel data and the output (the simulated arm: float32 x, w, bias and y); bytes over the
median is stated as a fraction of the 8 TB/s the HBM3E of an MI355X is specified at.  No counters are collected and nothing here
measures LDS bank conflicts.  The last line printed is one JSON object.

    python tools/int8_depthwise_bench.py [--repeats 5] [--launches 20] [--out profiles/int8_depthwise.txt]"""
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
HBM = 8e12
# C, H (= W), kernel, stride
SHAPES = [(32, 112, 3, 1), (96, 112, 3, 2), (144, 56, 3, 1), (144, 56, 3, 2), (192, 28, 3, 1), (384, 14, 3, 1), (576, 14, 3, 2), (960, 7, 3, 1), (240, 28, 5, 2)]
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
    wc.scale, wc.offset = w.abs().amax((1, 2, 3)) / 127, torch.zeros(w.shape[0], device=w.device)
    oc = LinearQuantizationConfig(symmetrical=False, quant_min=0, quant_max=255)
    oc.scale, oc.offset = torch.tensor(0.05), torch.tensor(0.)     # host tensors: the launch takes the output grid as scalars
    return xc, wc, oc


def bench(c, hw, k, stride, args, lines, summary, g):
    from ppq_amd import int8_depthwise_conv2d_packed, int8_depthwise_weight, int8_quantize
    pad, name = k // 2, f'{k}x{k} depthwise, {c}@{hw} s{stride}, batch {BATCH}'
    xs = [torch.randn(BATCH, c, hw, hw, device='cuda', generator=g).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
    ws = [torch.randn(c, 1, k, k, device='cuda', generator=g) * 0.2 for _ in range(ROTATE)]
    bias = torch.randn(c, device='cuda')
    cfg = [configs(x, w) for x, w in zip(xs, ws)]
    X, W = [int8_quantize(x, cf[0], 1) for x, cf in zip(xs, cfg)], [int8_depthwise_weight(w, cf[1]) for w, cf in zip(ws, cfg)]
    DX = [t.dequantize().contiguous(memory_format=torch.channels_last) for t in X]
    DW = [t.dequantize() for t in W]
    r = lambda i: i % ROTATE
    arms = {'int8': lambda i: int8_depthwise_conv2d_packed(X[r(i)], W[r(i)], bias, stride, pad),
            'int8 fused': lambda i: int8_depthwise_conv2d_packed(X[r(i)], W[r(i)], bias, stride, pad, relu=True, out_config=cfg[r(i)][2], out_float=False),
            'simulated': lambda i: F.conv2d(DX[r(i)], DW[r(i)], bias, stride, pad, groups=c)}
    oh, cp = (hw + 2 * pad - k) // stride + 1, (c + 31) // 32 * 32
    m, pixels = BATCH * oh * oh, BATCH * hw * hw
    moved = {'int8': pixels * cp + k * k * cp + 12 * c + 4 * m * c, 'int8 fused': pixels * cp + k * k * cp + 12 * c + m * cp,
             'simulated': 4 * (pixels * c + k * k * c + c + m * c)}
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    lines.append(f'{name}: operands rotating over {ROTATE} sets')
    summary[name] = {}
    base = statistics.median(times['simulated'])
    for arm, ts in times.items():
        med = statistics.median(ts)
        rate = moved[arm] / (med * 1e-3)
        lines.append(f'  {arm:11s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  [{min(ts):.4f}, {max(ts):.4f}]  spread {spread(ts) * 100:.1f} %   '
                     f'{moved[arm] / 1e6:.2f} MB, {rate / 1e12:.3f} TB/s = {rate / HBM:.3f} of 8 TB/s   {base / med:.2f} x simulated')
        summary[name][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts), 'bytes': moved[arm], 'of_hbm': rate / HBM, 'x_simulated': base / med}
    y, sim = arms['int8'](0), arms['simulated'](0)
    diff, top = float((y - sim).abs().max()), float(sim.abs().max())
    lines.append(f'  int8 against the simulated layer on the same codes: max |difference| {diff:.3e} at max |output| {top:.3e}')
    summary[name]['checks'] = {'int8_vs_simulated': diff, 'max_output': top}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/int8_depthwise_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/int8_depthwise_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    g = torch.Generator(device='cuda').manual_seed(11)
    for c, hw, k, stride in SHAPES:
        bench(c, hw, k, stride, args, lines, summary, g)
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
