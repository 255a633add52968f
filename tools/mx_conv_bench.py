"""Convolution on packed MX tensors (ppq_amd/mx.py mx_conv2d / mx_conv2d_packed) on the GPU: per shape and
format pair the time of one MX convolution on the block-scaled MFMA against the ways to compute it without the implicit-GEMM kernel.

  shapes  ResNet-50 at batch 32: the 7x7 / 2 stem (C = 3), 3x3 with C = 64 at 56 x 56, 1x1 from 256 to 64 at 56 x 56, 3x3 with C = 512
          at 7 x 7
  pairs   MXFP4 x MXFP4, MXFP8 (E4M3) x MXFP4        (activation x weight)
  arms    mx_conv2d     mx_conv2d(x, W, fmt): mx_quantize of the float32 activation plus the kernel -- the deployed layer, two launches
          kernel        mx_conv2d_packed on the activation packed beforehand: one launch of ppqhip_mx_conv2d
          gather+matmul the packed im2col operand [M, kh kw nbc] gathered from the packed activation with torch indexing (pixel table
                        built beforehand), then mx_matmul: the only way onto the instruction before this kernel
          simulated     mx_fake_quant of the activation and of the weight, then a float32 F.conv2d: the simulated layer

The operands of every arm ROTATE over 4 sets, so that a launch does not find its own lines of the last one in the 256 MiB Infinity
Cache.  A sample is the device-event time of `--launches` back-to-back calls divided by their number; `--repeats` samples per arm,
arms ALTERNATED; medians and (max - min) / median are reported.  TFLOP/s = 2 M O nb' 32 over the median.
Per pair the tool also prints how far mx_conv2d is from the simulated layer and how far both are from float64 on the same values
(first two images).  Then a ResNet-50 forward at batch 32 under deploy_graph_mx against the simulated forward of the same
quantize_graph_mx graph.  The last line printed is one JSON object.

    python tools/mx_conv_bench.py [--repeats 5] [--launches 20] [--out profiles/mx_conv.txt]"""
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
# name, C, H (= W), O, kernel, stride, pad
SHAPES = [('stem 7x7/2, C = 3, 224 x 224', 3, 224, 64, 7, 2, 3), ('3x3, C = 64, 56 x 56', 64, 56, 64, 3, 1, 1),
          ('1x1, 256 -> 64, 56 x 56', 256, 56, 64, 1, 1, 0), ('3x3, C = 512, 7 x 7', 512, 7, 512, 3, 1, 1)]
PAIRS = [('MXFP4_E2M1', 'MXFP4_E2M1'), ('MXFP8_E4M3', 'MXFP4_E2M1')]
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


def pixel_table(n, h, w, k, stride, pad):
    """int64 [M, k * k] on the GPU: the flat pixel behind every tap of every output pixel; n * h * w (a row of zeros) in the padding."""
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    img = torch.arange(n, device='cuda').view(n, 1, 1, 1, 1)
    iy = (torch.arange(oh, device='cuda') * stride - pad).view(1, oh, 1, 1, 1) + torch.arange(k, device='cuda').view(1, 1, 1, k, 1)
    ix = (torch.arange(ow, device='cuda') * stride - pad).view(1, 1, ow, 1, 1) + torch.arange(k, device='cuda').view(1, 1, 1, 1, k)
    inside = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    return torch.where(inside, (img * h + iy) * w + ix, torch.full_like(img, n * h * w)).reshape(n * oh * ow, k * k), oh, ow


def gather_matmul(X, W, table, m, nb):
    """mx_matmul on the im2col operand gathered from the packed activation X: a zero pixel under scale 127 stands for the padding."""
    from ppq_amd import MXTensor, mx_matmul
    e, s = X.elements.reshape(-1, X.elements.shape[-1]), X.scales.reshape(-1, X.scales.shape[-1])
    e = torch.cat([e, torch.zeros_like(e[:1])])
    s = torch.cat([s, torch.full_like(s[:1], 127)])
    a = MXTensor(X.format, (m, nb * 32), 1, e[table].reshape(m, -1), s[table].reshape(m, -1))
    o = W.shape[0]
    b = MXTensor(W.format, (o, nb * 32), 1, W.elements.reshape(o, -1), W.scales.reshape(o, -1))
    return mx_matmul(a, b)


def bench(name, c, hw, o, k, stride, pad, fa, fb, args, lines, summary):
    from ppq_amd import mx_conv2d, mx_conv2d_packed, mx_dequantize, mx_fake_quant, mx_quantize
    g = torch.Generator(device='cuda').manual_seed(11)
    xs = [torch.randn(BATCH, c, hw, hw, device='cuda', generator=g).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
    ws = [(torch.randn(o, c, k, k, device='cuda', generator=g) * 0.05).contiguous(memory_format=torch.channels_last) for _ in range(ROTATE)]
    X = [mx_quantize(x, fa, 1) for x in xs]
    W = [mx_quantize(w, fb, 1) for w in ws]
    table, oh, ow = pixel_table(BATCH, hw, hw, k, stride, pad)
    m, nbc = BATCH * oh * ow, (c + 31) // 32
    nb = k * k * nbc
    arms = {'mx_conv2d': lambda i: mx_conv2d(xs[i % ROTATE], W[i % ROTATE], fa, None, stride, pad),
            'kernel': lambda i: mx_conv2d_packed(X[i % ROTATE], W[i % ROTATE], None, stride, pad),
            'gather+matmul': lambda i: gather_matmul(X[i % ROTATE], W[i % ROTATE], table, m, nb),
            'simulated': lambda i: F.conv2d(mx_fake_quant(xs[i % ROTATE], fa, 1), mx_fake_quant(ws[i % ROTATE], fb, 1), None, stride, pad)}
    times = {arm: [] for arm in arms}
    for fn in arms.values(): sample(fn, 2)
    for _ in range(args.repeats):
        for arm, fn in arms.items(): times[arm].append(sample(fn, args.launches))
    flops = 2.0 * m * o * nb * 32
    key = f'{name} {fa} x {fb}'
    lines.append(f'{name}, batch {BATCH}: M = {m}, O = {o}, nb\' = {nb} (nbc = {nbc}), {fa} x {fb}, {flops / 1e9:.1f} GFLOP on the instruction, '
                 f'operands rotating over {ROTATE} sets')
    summary[key] = {}
    base = statistics.median(times['simulated'])
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:14s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{flops / med / 1e9:.1f} TFLOP/s   {base / med:.2f} x simulated   [{min(ts):.4f}, {max(ts):.4f}]')
        summary[key][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts), 'TFLOPs': flops / med / 1e9}
    # how far the deployed layer is from the simulation
    y = mx_conv2d(xs[0], W[0], fa, None, stride, pad)
    tie = bool(torch.equal(y, gather_matmul(X[0], W[0], table, m, nb).reshape(BATCH, oh, ow, o).permute(0, 3, 1, 2)))
    sim = arms['simulated'](0)
    ref = F.conv2d(mx_dequantize(X[0])[:2].cpu().double(), mx_dequantize(W[0]).cpu().double(), None, stride, pad)
    dev_sim, same = float((y - sim).abs().max()), bool(torch.equal(y.contiguous().view(torch.int32), sim.contiguous().view(torch.int32)))
    dev_k, dev_s = float((y[:2].cpu().double() - ref).abs().max()), float((sim[:2].cpu().double() - ref).abs().max())
    top = float(ref.abs().max())
    lines.append(f'  mx_conv2d has the bits of gather+matmul: {tie}')
    lines.append(f'  mx_conv2d against the simulated layer (mx_fake_quant of both, float32 F.conv2d): identical bits: {same}; max |difference| '
                 f'{dev_sim:.3e} at max |output| {top:.3e} ({dev_sim / top:.2e} of it); against float64 on the same values (two images): '
                 f'mx_conv2d {dev_k:.3e}, simulated layer {dev_s:.3e}')
    summary[key]['mx_conv2d_vs_simulated'] = {'ties_gather_matmul': tie, 'identical_bits': same, 'max_abs': dev_sim, 'max_output': top, 'kernel_vs_f64': dev_k, 'simulated_vs_f64': dev_s}
    del xs, ws, X, W, table
    torch.cuda.empty_cache()


def bench_resnet50(fa, fb, args, lines, summary):
    from ppq_amd import deploy_graph_mx, harness, quantize_graph_mx
    graph = harness.resnet50_graph(seed=0)
    ex = harness.TorchExecutor(graph, 'cuda').use_channels_last()
    delegators = quantize_graph_mx(graph, ex, fb, fa)
    g = torch.Generator(device='cuda').manual_seed(5)
    xs = [torch.randn(BATCH, 3, 224, 224, device='cuda', generator=g) for _ in range(ROTATE)]
    launches = max(1, args.launches // 4)
    times = {'simulated': [], 'deployed': []}
    simulated = ex.forward(xs[0])[0]
    dep = deploy_graph_mx(graph, ex, delegators)
    deployed = ex.forward(xs[0])[0]
    run = lambda i: ex.forward(xs[i % ROTATE])
    for _ in range(args.repeats):
        dep.remove()
        sample(run, 1)
        times['simulated'].append(sample(run, launches))
        dep.refresh()
        sample(run, 1)
        times['deployed'].append(sample(run, launches))
    key = f'ResNet-50 forward {fa} x {fb}'
    lines.append(f'ResNet-50 forward, batch {BATCH}, channels-last executor, {fa} activations x {fb} weights: {len(dep.deployed)} operations deployed '
                 f'({sum(graph.operations[n].type == "Conv" for n in dep.deployed)} Conv), {len(dep.skipped)} skipped; {launches} forwards per sample')
    summary[key] = {'deployed': len(dep.deployed), 'skipped': dep.skipped}
    base = statistics.median(times['simulated'])
    for arm, ts in times.items():
        med = statistics.median(ts)
        lines.append(f'  {arm:14s} ms per forward: ' + ' '.join(f'{t:.3f}' for t in ts) + f'   median {med:.3f}  spread {spread(ts) * 100:.1f} %   '
                     f'{base / med:.2f} x simulated   [{min(ts):.3f}, {max(ts):.3f}]')
        summary[key][arm] = {'ms': med, 'min_ms': min(ts), 'max_ms': max(ts), 'spread': spread(ts)}
    diff, top = float((deployed - simulated).abs().max()), float(simulated.abs().max())
    lines.append(f'  logits, deployed against simulated: max |difference| {diff:.3e} at max |logit| {top:.3e} ({diff / top:.2e} of it); '
                 f'top-1 agrees on {int((deployed.argmax(1) == simulated.argmax(1)).sum())} of {BATCH} images')
    summary[key]['logits'] = {'max_abs': diff, 'max_logit': top}
    dep.remove()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_conv_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_conv_bench.py --repeats {args.repeats} --launches {args.launches}', f'# device: {torch.cuda.get_device_name(0)}']
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
