"""Per-shape device time of ResNet-50's pointwise (1x1) convolutions: F.conv2d (MIOpen / rocBLAS with every helper launch it makes:
transposes, im2col, sub-tensor ops) against ffi.conv1x1 (ppqhip_conv1x1), on the distinct (Ci, Co, H, stride) classes of
harness.resnet50_graph at one or more batch sizes.

Method: profiler-free HIP-graph replay, as the `graph` mode of tools/north_star.py -- `iters` back-to-back calls captured into ONE
graph (operands rotate over `--rotate` buffer sets so that no call finds its input in cache from the call before), replayed
`--rounds` times, each replay timed with one event pair and divided by `iters`.  A launch-to-launch time inside a graph: an upper
bound of the kernel time that includes the inter-node gaps, which is what the vendor path pays for its helper launches too.
Reported per class and path: median, min and max over the rounds (the spread), TF/s at the median, and the verdict by the rule of
DESIGN.md section 2.9: native is enabled where its median is below the vendor's by more than the larger of the two spreads.

  python tools/pointwise_conv_bench.py --batches 1,8,32 --report profiles/r18_pointwise_conv_shapes.txt

`--fused`: per class and per ROLE the class has in ResNet-50's epilogue groups (P1: Conv -> Relu; P2: Conv -> Add(identity) -> Relu;
P2b: the last-executed convolution of Conv, Conv -> Add -> Relu, whose other convolution's raw output is the residual), the
calibration forward's two launches -- the convolution (F.conv2d, and ffi.conv1x1) followed by the sink epilogue launch with the
stores elided that the executor elides -- against the ONE launch of ffi.conv1x1_epilogue, with min/max sinks (phase 1) and with
2048-bin symmetric histogram sinks (phase 2) separately.  Verdict by the same rule on the sum of the two phases: fused where its
summed median is below the FASTER of the two two-launch paths by more than the larger min..max spread (so the verdict does not
depend on what harness.POINTWISE_KEEP_VENDOR holds when the tool runs; the last column shows which path it picks now).

  python tools/pointwise_conv_bench.py --fused --report profiles/r20_pointwise_epilogue_shapes.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path: sys.path.insert(0, ROOT)


def shape_classes():
    """[(Ci, Co, H, W, stride, count)] of the 1x1 convolutions of ResNet-50 at 224 x 224, from a meta-tensor walk of the graph."""
    import torch
    from ppq_amd import harness
    g = harness.resnet50_graph(seed=0)
    vals = {'input': torch.empty(1, 3, 224, 224, device='meta')}
    classes = {}
    for op in g.topological_sort():
        xs = [v.value.to('meta') if v.is_parameter else vals[v.name] for v in op.inputs]
        y = harness._forward(op, xs)
        if op.type == 'Conv' and tuple(xs[1].shape[2:]) == (1, 1):
            stride = harness._square(op.attributes.get('strides', 1))
            key = (int(xs[0].shape[1]), int(xs[1].shape[0]), int(xs[0].shape[2]), int(xs[0].shape[3]), stride)
            classes[key] = classes.get(key, 0) + 1
        vals[op.outputs[0].name] = y
    return [(*k, n) for k, n in classes.items()]


def time_graph(fn, sets, iters, rounds, warm=3):
    """Median / min / max microseconds per call of fn(set) over `rounds` replays of a graph of `iters` calls."""
    import torch
    for k in range(warm): fn(sets[k % len(sets)])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        for k in range(2): fn(sets[k % len(sets)])
    side.synchronize()
    with torch.cuda.graph(graph, stream=side):
        for k in range(iters): fn(sets[k % len(sets)])
    graph.replay(); torch.cuda.synchronize()
    per = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); graph.replay(); b.record(); b.synchronize()
        per.append(a.elapsed_time(b) * 1000.0 / iters)
    return statistics.median(per), min(per), max(per)


def roles():
    """{(Ci, Co, H, W, stride): {role: count}} of ResNet-50's pointwise convolutions, from the executor's own epilogue plan."""
    from ppq_amd import harness
    g = harness.resnet50_graph(seed=0)
    ops = g.topological_sort()
    shapes = {}
    for ci, co, h, w, stride, _ in shape_classes(): shapes.setdefault((ci, co, stride), []).append((ci, co, h, w, stride))
    import torch
    vals, cls = {'input': torch.empty(1, 3, 224, 224, device='meta')}, {}
    for op in ops:
        xs = [v.value.to('meta') if v.is_parameter else vals[v.name] for v in op.inputs]
        if op.type == 'Conv' and tuple(xs[1].shape[2:]) == (1, 1):
            cls[op.name] = (int(xs[0].shape[1]), int(xs[1].shape[0]), int(xs[0].shape[2]), int(xs[0].shape[3]),
                            harness._square(op.attributes.get('strides', 1)))
        vals[op.outputs[0].name] = harness._forward(op, xs)
    out = {}
    for grp in harness.plan_epilogues(ops, None, set(g.outputs)):
        last = grp.ops[len(grp.convs) - 1]                       # the last-executed convolution owns the fused launch
        if last.name not in cls or grp.pool is not None: continue
        role = 'P1' if grp.kind == 'P1' else ('P2b' if len(grp.convs) == 2 else 'P2')
        out.setdefault(cls[last.name], {}).setdefault(role, 0)
        out[cls[last.name]][role] += 1
    return out


def fused_main(args):
    import torch
    import torch.nn.functional as F
    from ppq_amd import CUDA, ffi, harness
    from ppq_amd.observer import _range_seed
    dev, batch = 'cuda:0', int(args.batches.split(',')[0])
    gen = torch.Generator().manual_seed(0)
    lines = ['# ci co h w stride role xcount sinks | vendor+ep us med (min..max) | native+ep | fused | today=V/N',
             f'# device: {torch.cuda.get_device_name(0)}; batch {batch}; iters {args.iters} x rounds {args.rounds}, {args.rotate} rotating operand sets']
    rows = lambda: torch.zeros(CUDA.hist_rows(), 2048, dtype=torch.int32, device=dev)
    slots = lambda: _range_seed(torch.device(dev))[1].clone()
    summary = []
    for key, by_role in sorted(roles().items()):
        ci, co, h, w, stride = key
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        sets = [(torch.randn(batch, ci, h, w, generator=gen).to(dev), (torch.randn(co, ci, 1, 1, generator=gen) * ci ** -0.5).to(dev),
                 torch.randn(batch, co, ho, wo, generator=gen).to(dev)) for _ in range(args.rotate)]
        ba, bb = (torch.randn(co, generator=gen) * 0.05).to(dev), (torch.randn(co, generator=gen) * 0.05).to(dev)
        today_native = key not in harness.POINTWISE_KEEP_VENDOR
        for role, count in sorted(by_role.items()):
            tot = {'vendor': [0.0, 0.0], 'native': [0.0, 0.0], 'fused': [0.0, 0.0]}
            for sink in ('minmax', 'hist'):
                mk = (lambda: ('minmax', slots())) if sink == 'minmax' else (lambda: ('hist_rows', rows(), False, 8.0 / 2048, 0.0, False))
                ja, jr, jo = mk(), mk(), mk()

                def today(s, conv):
                    y = conv(s)
                    if role == 'P1': return (ffi.bias_act_stats_ if sink == 'minmax' else ffi.bias_act_hist_)(y, ba, True, jo)
                    launch = ffi.bias_add_act_stats if sink == 'minmax' else ffi.bias_add_act_hist
                    if role == 'P2': return launch(y, ba, s[2], None, True, ja, None, jo, ffi.ELIDE_A)
                    return launch(y, ba, s[2], bb, True, ja, jr, jo, ffi.ELIDE_A | ffi.ELIDE_B)

                def fused(s):
                    if role == 'P1': return ffi.conv1x1_epilogue(s[0], s[1], stride, ba, None, None, True, None, None, jo)
                    if role == 'P2': return ffi.conv1x1_epilogue(s[0], s[1], stride, ba, s[2], None, True, ja, None, jo)
                    return ffi.conv1x1_epilogue(s[0], s[1], stride, ba, s[2], bb, True, ja, jr, jo)

                with torch.no_grad():
                    assert today(sets[0], lambda s: ffi.conv1x1(s[0], s[1], None, stride)) is not None and fused(sets[0]) is not None
                    res = {'vendor': time_graph(lambda s: today(s, lambda s: F.conv2d(s[0], s[1], None, stride=stride)), sets, args.iters, args.rounds),
                           'native': time_graph(lambda s: today(s, lambda s: ffi.conv1x1(s[0], s[1], None, stride)), sets, args.iters, args.rounds),
                           'fused': time_graph(fused, sets, args.iters, args.rounds)}
                row = f'{ci:5d} {co:5d} {h:3d} {w:3d} {stride} {role:3s} x{count} {sink:6s} |' + ' |'.join(
                    f' {res[k][0]:7.1f} ({res[k][1]:.1f}..{res[k][2]:.1f})' for k in ('vendor', 'native', 'fused')) + f' | {"N" if today_native else "V"}'
                lines.append(row); print(row, flush=True)
                for k in tot: tot[k][0] += res[k][0]; tot[k][1] = max(tot[k][1], res[k][2] - res[k][1])
            now = min(tot['native'], tot['vendor'])
            gain, spread = now[0] - tot['fused'][0], max(now[1], tot['fused'][1])
            row = (f'# {key} {role} x{count}: both phases, best two-launch path {now[0]:.1f} us, fused {tot["fused"][0]:.1f} us, gain {gain:.1f} us, '
                   f'larger spread {spread:.1f} us -> {"FUSE" if gain > spread else "keep"}; vendor+ep {tot["vendor"][0]:.1f}, native+ep {tot["native"][0]:.1f}')
            summary.append(row); print(row, flush=True)
        del sets
    lines += summary
    if args.report:
        with open(args.report, 'w') as f: f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fused', action='store_true')
    ap.add_argument('--batches', default='32')
    ap.add_argument('--iters', type=int, default=24)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--rotate', type=int, default=4)
    ap.add_argument('--report', default=None)
    args = ap.parse_args()
    if args.fused: return fused_main(args)
    import torch
    import torch.nn.functional as F
    from ppq_amd import ffi
    native = getattr(ffi, 'conv1x1', None)          # absent in a tree from before the kernel: the vendor column alone
    dev = 'cuda:0'
    lines = ['# ci co h w stride count batch | vendor us med (min..max) TF | native us med (min..max) TF | ratio verdict',
             f'# device: {torch.cuda.get_device_name(0)}; iters {args.iters} x rounds {args.rounds}, {args.rotate} rotating operand sets']
    totals = {}
    gen = torch.Generator().manual_seed(0)
    for batch in [int(b) for b in args.batches.split(',')]:
        tot_v = tot_n = tot_best = 0.0
        for ci, co, h, w, stride, count in shape_classes():
            sets = [(torch.randn(batch, ci, h, w, generator=gen).to(dev), (torch.randn(co, ci, 1, 1, generator=gen) * ci ** -0.5).to(dev))
                    for _ in range(args.rotate)]
            flops = 2.0 * batch * co * ci * ((h - 1) // stride + 1) * ((w - 1) // stride + 1)
            with torch.no_grad():
                v = time_graph(lambda s: F.conv2d(s[0], s[1], None, stride=stride), sets, args.iters, args.rounds)
                n = time_graph(lambda s: native(s[0], s[1], None, stride), sets, args.iters, args.rounds) if native else None
            row = f'{ci:5d} {co:5d} {h:3d} {w:3d} {stride} x{count} b{batch:<3d} | {v[0]:8.1f} ({v[1]:.1f}..{v[2]:.1f}) {flops / v[0] / 1e6:6.1f}'
            tot_v += count * v[0]
            if n is not None:
                spread = max(v[2] - v[1], n[2] - n[1])
                wins = v[0] - n[0] > spread
                row += (f' | {n[0]:8.1f} ({n[1]:.1f}..{n[2]:.1f}) {flops / n[0] / 1e6:6.1f} | {n[0] / v[0]:.2f} '
                        f'{"native" if wins else "VENDOR"}  flops {flops:.3g}')
                tot_n += count * n[0]
                tot_best += count * (n[0] if wins else v[0])
            lines.append(row)
            print(row, flush=True)
            del sets
        totals[batch] = (tot_v, tot_n, tot_best)
        row = f'# batch {batch}: all 36 pointwise convolutions per forward: vendor {tot_v:.0f} us, native {tot_n:.0f} us, per-class best {tot_best:.0f} us'
        lines.append(row)
        print(row, flush=True)
    if args.report:
        with open(args.report, 'w') as f: f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
