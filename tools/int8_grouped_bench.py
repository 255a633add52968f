"""The grouped linear INT8 layer on the int8 MFMA (ppq_amd/int8.py int8_grouped_conv2d_packed) on the GPU: per
shape the time of one layer against the two ways such a layer could run before, in the same run.

  shapes  the four 3 x 3 classes of ResNeXt-50 32x4d at batch 32, C = O @ H (= W), groups 32, stride 1, padding 1:
          128@56, 256@28, 512@14, 1024@7
  arms    grouped      int8_grouped_conv2d_packed on an Int8Tensor and an Int8GroupedWeight, float32 output, bias
          dense        int8_conv2d_packed on the block-diagonal [O, C, 3, 3] weight with the same codes: the same bits, groups times
                       the MFMA work, the weight bytes and the gathers
          simulated    F.conv2d(groups=32) in float32 on the dequantised operands, channels-last, with the bias

The operands of every arm ROTATE over 4 sets, so that a launch does not find its own lines of the last one in the 256 MiB Infinity
Cache.  A sample is the device-event time of `--launches` back-to-back calls divided by their number; `--repeats` samples per arm,
arms ALTERNATED; medians, min / max and (max - min) / median are reported.  The integer arms are also stated as multiply-adds of the
layer itself (M O C_g kh kw, what the grouped layer needs; the dense arm executes groups times as many) over the median.  No counters
are collected and nothing here measures LDS bank conflicts or cache hits.  The last line printed is one JSON object.

    python tools/int8_grouped_bench.py [--repeats 5] [--launches 20] [--out profiles/int8_grouped.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.int8_depthwise_bench import configs, sample, spread  # noqa: E402  (the method and the configs of the depthwise measurement)

BATCH, GROUPS, K = 32, 32, 3
SHAPES = [(128, 56), (256, 28), (512, 14), (1024, 7)]                                    # C = O, H = W
ROTATE = 4


def bench(c, hw, args, lines, summary, g):
    from ppq_amd import Int8Tensor, int8_conv2d_packed, int8_grouped_conv2d_packed, int8_grouped_weight, int8_quantize
    cg, name = c // GROUPS, f'3x3 grouped, {c}@{hw}, {GROUPS} groups, batch {BATCH}'
    xs = [torch.randn(BATCH, c, hw, hw, device='cuda', generator=g).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
    ws = [torch.randn(c, cg, K, K, device='cuda', generator=g) * 0.2 for _ in range(ROTATE)]
    bias = torch.randn(c, device='cuda')
    cfg = [configs(x, w) for x, w in zip(xs, ws)]
    X, W = [int8_quantize(x, cf[0], 1) for x, cf in zip(xs, cfg)], [int8_grouped_weight(w, cf[1], GROUPS) for w, cf in zip(ws, cfg)]
    dense = []
    for t in W:                                                                          # the block-diagonal weight with the same codes
        codes = torch.zeros(c, K, K, c, dtype=torch.int8, device='cuda')
        for grp in range(GROUPS): codes[grp * cg:(grp + 1) * cg, :, :, grp * cg:(grp + 1) * cg] = t.codes()[grp * cg:(grp + 1) * cg]
        dense.append(Int8Tensor(codes, (c, c, K, K), 1, t.scale, 0, t.qmin, t.qmax, t.rounding, t.sums))
    DX = [t.dequantize().contiguous(memory_format=torch.channels_last) for t in X]
    DW = [t.dequantize() for t in W]
    r = lambda i: i % ROTATE
    arms = {'grouped': lambda i: int8_grouped_conv2d_packed(X[r(i)], W[r(i)], bias, 1, 1),
            'dense': lambda i: int8_conv2d_packed(X[r(i)], dense[r(i)], bias, 1, 1),
            'simulated': lambda i: F.conv2d(DX[r(i)], DW[r(i)], bias, 1, 1, groups=GROUPS)}
    macs = BATCH * hw * hw * c * cg * K * K
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    lines.append(f'{name}: operands rotating over {ROTATE} sets; nbs = {W[0].nbs}, {W[0].values[0].numel()} stored codes a row for {cg * K * K} live ones')
    summary[name] = {}
    med = {arm: statistics.median(ts) for arm, ts in times.items()}
    for arm, ts in times.items():
        lines.append(f'  {arm:10s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med[arm]:.4f}  [{min(ts):.4f}, {max(ts):.4f}]  '
                     f'spread {spread(ts) * 100:.1f} %   {macs / (med[arm] * 1e-3) / 1e12:.3f} T layer multiply-adds / s   '
                     f'{med["dense"] / med[arm]:.2f} x dense   {med["simulated"] / med[arm]:.2f} x simulated')
        summary[name][arm] = {'ms': med[arm], 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts), 'x_dense': med['dense'] / med[arm],
                              'x_simulated': med['simulated'] / med[arm]}
    y, yd, sim = arms['grouped'](0), arms['dense'](0), arms['simulated'](0)
    same, diff, top = bool(torch.equal(y, yd)), float((y - sim).abs().max()), float(sim.abs().max())
    lines.append(f'  grouped against dense: identical bits: {same}; against the simulated layer on the same codes: max |difference| {diff:.3e} at max |output| {top:.3e}')
    summary[name]['checks'] = {'grouped_equals_dense': same, 'grouped_vs_simulated': diff, 'max_output': top}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/int8_grouped_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/int8_grouped_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    g = torch.Generator(device='cuda').manual_seed(11)
    for c, hw in SHAPES:
        bench(c, hw, args, lines, summary, g)
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
