"""The fused epilogue of the MXINT8 convolution (ppq_amd/mx.py mx_int8_conv2d_packed(..., residual=, relu=, out_format='MXINT8');
DESIGN.md section 9.21) on the GPU: what ONE launch saves over the sequence it replaces.

  shapes  the ResNet-50 body shapes of tools/mx_int8_conv_bench.py at batch 32: 3x3 with C = 64 at 56 x 56, 1x1 from 256 to 64 at
          56 x 56, 3x3 with C = 512 at 7 x 7
  arms    fused     mx_int8_conv2d_packed(X, W, residual=R, relu=True, out_format='MXINT8'): packed in, packed out, ONE launch of
                    ppqhip_mx_int8_conv2d_fused, no float32 store
          sequence  the four launches it replaces: the plain int8 convolution, a torch add of the residual, a torch relu, then
                    mx_quantize of the float32 result to MXINT8 along the channels

The operands of every arm ROTATE over 4 sets, so that a launch does not find its own lines of the last one in the 256 MiB Infinity
Cache.  A sample is the device-event time of `--launches` back-to-back calls divided by their number; `--repeats` samples per arm,
arms ALTERNATED; medians and (max - min) / median are reported.  Per shape the tool also states whether the two arms leave the same
bytes.  Then a ResNet-50 forward at batch 32 with MXINT8 activations and weights: deploy_graph_mx(fuse=True, fuse_int8=True) against
the unfused deployment, both measured here, alternated.  No counters are read: nothing below says anything about the LDS bank
conflicts of the code gather.  The last line printed is one JSON object.

    python tools/mx_int8_fused_bench.py [--repeats 5] [--launches 20] [--out profiles/mx_int8_fused.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 32
# name, C, H (= W), O, kernel, stride, pad
SHAPES = [('3x3, C = 64, 56 x 56', 64, 56, 64, 3, 1, 1), ('1x1, 256 -> 64, 56 x 56', 256, 56, 64, 1, 1, 0), ('3x3, C = 512, 7 x 7', 512, 7, 512, 3, 1, 1)]
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


def report(times, unit, base_arm, lines, into):
    base = statistics.median(times[base_arm])
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:10s} ms per {unit}: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{base / med:.2f} x {base_arm}   [{min(ts):.4f}, {max(ts):.4f}]')
        into[arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts)}


def bench(name, c, hw, o, k, stride, pad, args, lines, summary):
    from ppq_amd import mx_int8_conv2d_packed, mx_quantize
    g = torch.Generator(device='cuda').manual_seed(11)
    oh = (hw + 2 * pad - k) // stride + 1
    X = [mx_quantize(torch.randn(BATCH, c, hw, hw, device='cuda', generator=g).contiguous(memory_format=torch.channels_last), 'MXINT8', 1) for _ in range(ROTATE)]
    W = [mx_quantize((torch.randn(o, c, k, k, device='cuda', generator=g) * 0.05).contiguous(memory_format=torch.channels_last), 'MXINT8', 1) for _ in range(ROTATE)]
    R = [torch.randn(BATCH, o, oh, oh, device='cuda', generator=g).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]

    def fused(i): return mx_int8_conv2d_packed(X[i % ROTATE], W[i % ROTATE], None, stride, pad, residual=R[i % ROTATE], relu=True, out_format='MXINT8')

    def sequence(i):
        y = mx_int8_conv2d_packed(X[i % ROTATE], W[i % ROTATE], None, stride, pad)
        return mx_quantize(torch.relu(y + R[i % ROTATE]), 'MXINT8', 1)

    arms = {'fused': fused, 'sequence': sequence}
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    m = BATCH * oh * oh
    lines.append(f'{name}, batch {BATCH}: M = {m}, O = {o}, nb\' = {k * k * ((c + 31) // 32)}, MXINT8 x MXINT8, residual + relu + MXINT8 out, '
                 f'operands rotating over {ROTATE} sets')
    summary[name] = {}
    report(times, 'call', 'sequence', lines, summary[name])
    a, b = fused(0), sequence(0)                      # torch.relu may leave -0 where the epilogue leaves +0: both pack code 0
    same = bool(torch.equal(a.elements, b.elements) and torch.equal(a.scales, b.scales))
    lines.append(f'  the two arms leave the same bytes: {same}')
    summary[name]['same_bytes'] = same
    del X, W, R
    torch.cuda.empty_cache()


def bench_resnet50(args, lines, summary):
    from ppq_amd import deploy_graph_mx, harness, quantize_graph_mx
    graph = harness.resnet50_graph(seed=0)
    ex = harness.TorchExecutor(graph, 'cuda').use_channels_last()
    delegators = quantize_graph_mx(graph, ex, 'MXINT8', 'MXINT8')
    g = torch.Generator(device='cuda').manual_seed(5)
    xs = [torch.randn(BATCH, 3, 224, 224, device='cuda', generator=g) for _ in range(ROTATE)]
    launches = max(1, args.launches // 4)
    run = lambda i: ex.forward(xs[i % ROTATE])
    modes = {'unfused': dict(fuse=False), 'fused': dict(fuse=True, fuse_int8=True)}
    times, logits, groups = {mode: [] for mode in modes}, {}, None
    for _ in range(args.repeats):
        for mode, kw in modes.items():
            dep = deploy_graph_mx(graph, ex, delegators, **kw)
            logits[mode] = ex.forward(xs[0])[0]
            times[mode].append(sample(run, launches))
            if kw['fuse']: groups = dep.groups
            dep.remove()
    key = 'ResNet-50 forward MXINT8 x MXINT8'
    packed = sum(1 for grp in groups.values() if grp.out_format is not None)
    lines.append(f'ResNet-50 forward, batch {BATCH}, channels-last executor, MXINT8 activations x MXINT8 weights; fused: {len(groups)} groups, '
                 f'{sum(1 for grp in groups.values() if grp.residual)} with a residual, {sum(1 for grp in groups.values() if grp.relu)} with a relu, '
                 f'{packed} hand their output over packed; {launches} forwards per sample')
    summary[key] = {'groups': len(groups), 'packed': packed}
    report(times, 'forward', 'unfused', lines, summary[key])
    same = bool(torch.equal(logits['fused'].view(torch.int32), logits['unfused'].view(torch.int32)))
    lines.append(f'  the logits of the two deployments have the same bits: {same}')
    summary[key]['same_logits'] = same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_int8_fused_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_int8_fused_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    for shape in SHAPES: bench(*shape, args, lines, summary)
    bench_resnet50(args, lines, summary)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
