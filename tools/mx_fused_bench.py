"""The fused epilogue of the MX convolution (residual, ReLU, MX re-quantisation of the result) on the GPU: what a
deployed layer costs when it takes packed activations in and gives packed activations out, against the unfused chain.

  shapes  ResNet-50 at batch 32, as tools/mx_conv_bench.py: the 7x7 / 2 stem (C = 3), 3x3 with C = 64 at 56 x 56, 1x1 from 256 to 64 at
          56 x 56, 3x3 with C = 512 at 7 x 7
  pairs   MXFP4 x MXFP4, MXFP8 (E4M3) x MXFP4        (activation x weight); the output is packed in the activation's format
  arms    fused         mx_conv2d_packed(X, W, relu=True, out_format=fmt): packed in, packed out, ONE launch of ppqhip_mx_conv2d_fused
          fused+float   the same with out_float=True: the float32 tensor is written as well (a residual or a float consumer needs it)
          unfused       mx_conv2d_packed(X, W), F.relu, mx_quantize on the plain kernel: three launches, two float32 round trips.
                        The issue words this arm as mx_conv2d + relu + mx_quantize; the input is taken packed here, as in the
                        fused arm, so that both arms do the same work and only the epilogue differs -- mx_conv2d would add the
                        quantisation of the input to this arm alone, which a fused chain pays once per graph input
          kernel        mx_conv2d_packed(X, W) alone: what the convolution itself costs

The operands ROTATE over 4 sets; a sample is the device-event time of `--launches` back-to-back calls divided by their number;
`--repeats` samples per arm, arms ALTERNATED; medians and ranges are reported.  Per pair the tool checks that the fused bytes are those
of the unfused chain.  Then a ResNet-50 forward at batch 32 under deploy_graph_mx(fuse=True) against fuse=False on the same graph.
The last line printed is one JSON object.

    python tools/mx_fused_bench.py [--repeats 5] [--launches 20] [--out profiles/mx_fused.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mx_conv_bench import BATCH, PAIRS, ROTATE, SHAPES, sample, spread  # noqa: E402


def bench(name, c, hw, o, k, stride, pad, fa, fb, args, lines, summary):
    from ppq_amd import mx_conv2d_packed, mx_quantize
    g = torch.Generator(device='cuda').manual_seed(11)
    xs = [torch.randn(BATCH, c, hw, hw, device='cuda', generator=g).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
    ws = [(torch.randn(o, c, k, k, device='cuda', generator=g) * 0.05).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
    X = [mx_quantize(x, fa, 1) for x in xs]
    W = [mx_quantize(w, fb, 1) for w in ws]
    del xs, ws
    arms = {'fused': lambda i: mx_conv2d_packed(X[i % ROTATE], W[i % ROTATE], None, stride, pad, relu=True, out_format=fa),
            'fused+float': lambda i: mx_conv2d_packed(X[i % ROTATE], W[i % ROTATE], None, stride, pad, relu=True, out_format=fa, out_float=True),
            'unfused': lambda i: mx_quantize(F.relu(mx_conv2d_packed(X[i % ROTATE], W[i % ROTATE], None, stride, pad)), fa, 1),
            'kernel': lambda i: mx_conv2d_packed(X[i % ROTATE], W[i % ROTATE], None, stride, pad)}
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    got, want = arms['fused'](0), arms['unfused'](0)
    same = bool(torch.equal(got.elements, want.elements) and torch.equal(got.scales, want.scales))
    m = got.scales.shape[0] * got.scales.shape[1] * got.scales.shape[2]
    key = f'{name} {fa} x {fb}'
    lines.append(f'{name}, batch {BATCH}: M = {m}, O = {o}, {fa} x {fb} -> {fa}, operands rotating over {ROTATE} sets; fused bytes == unfused bytes: {same}')
    summary[key] = {'identical_bytes': same}
    base = statistics.median(times['unfused'])
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:12s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{base / med:.2f} x unfused   [{min(ts):.4f}, {max(ts):.4f}]')
        summary[key][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts)}
    del X, W
    torch.cuda.empty_cache()


def bench_resnet50(fa, fb, args, lines, summary):
    from ppq_amd import deploy_graph_mx, harness, quantize_graph_mx
    graph = harness.resnet50_graph(seed=0)
    ex = harness.TorchExecutor(graph, 'cuda').use_channels_last()
    delegators = quantize_graph_mx(graph, ex, fb, fa)
    g = torch.Generator(device='cuda').manual_seed(5)
    xs = [torch.randn(BATCH, 3, 224, 224, device='cuda', generator=g) for _ in range(ROTATE)]
    launches = max(1, args.launches // 4)
    times = {'fuse=False': [], 'fuse=True': []}
    run = lambda i: ex.forward(xs[i % ROTATE])
    deps, logits = {}, {}
    for _ in range(args.repeats):
        for arm, fuse in (('fuse=False', False), ('fuse=True', True)):
            dep = deploy_graph_mx(graph, ex, delegators, fuse=fuse)
            logits[arm] = ex.forward(xs[0])[0]
            times[arm].append(sample(run, launches))
            deps[arm] = (len(dep.deployed), sum(len(grp.members) > 1 for grp in dep.groups.values()),
                         sum(grp.out_format is not None for grp in dep.groups.values()))
            dep.remove()
    _, tails, packed = deps['fuse=True']
    key = f'ResNet-50 forward {fa} x {fb}'
    lines.append(f'ResNet-50 forward, batch {BATCH}, channels-last executor, {fa} activations x {fb} weights: {deps["fuse=True"][0]} operations deployed, '
                 f'{tails} with a fused tail, {packed} hand their output over packed; {launches} forwards per sample')
    summary[key] = {'deployed': deps['fuse=True'][0], 'tails': tails, 'packed': packed}
    base = statistics.median(times['fuse=False'])
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:12s} ms per forward: ' + ' '.join(f'{t:.3f}' for t in ts) + f'   median {med:.3f}  spread {spread(ts) * 100:.1f} %   '
                     f'{base / med:.2f} x fuse=False   [{min(ts):.3f}, {max(ts):.3f}]')
        summary[key][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts)}
    same = bool(torch.equal(logits['fuse=True'], logits['fuse=False']))
    lines.append(f'  logits, fuse=True against fuse=False: torch.equal: {same}; max |difference| {float((logits["fuse=True"] - logits["fuse=False"]).abs().max()):.3e}')
    summary[key]['logits_equal'] = same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_fused_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_fused_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    for shape in SHAPES:
        for fa, fb in PAIRS: bench(*shape, fa, fb, args, lines, summary)
    for fa, fb in PAIRS: bench_resnet50(fa, fb, args, lines, summary)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
