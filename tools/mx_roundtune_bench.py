"""MX round tuning on the GPU: what a training step costs with the delegators on the torch restatement, on the
HIP kernel and replayed from a HIP graph, what the forward kernel costs next to a copy of the same bytes, and what the pass does to the
block losses.

  steps    MXRoundTuningPass on the first `--blocks` blocks of harness.yolov6s_graph (8 batches of [2, 3, 160, 160]) and of
           harness.resnet50_graph (4 batches of [8, 3, 224, 224]) under quantize_graph_mx(MXFP4_E2M1 weights, MXFP8_E4M3
           activations), `--steps` steps per block at `--lr`.  Three arms, ALTERNATED `--repeats` times in this one process, every
           parameter put back before each run:
             torch   the delegators on the torch restatement (use_kernels=False), one forward per weight, eager steps
             kernel  ppqhip_mx_round_fwd_multi, every weight of a block in one launch, eager steps
             graph   the same, the step captured once per block and replayed
           ms per step = the synchronised wall time of the eager steps resp. of the replays of all blocks over their number (the
           pass's own phase clock); the activations' MXDelegator runs its kernel in all three.  Medians and (max - min) / median.
           Of each arm's last run: the block losses before and after and the share of elements that left round-to-nearest.
  forward  ppqhip_mx_round_fwd_multi on one MXFP4 tensor (12 bytes + 1/32 byte per element) next to tools/floor floor_copy of the same
           bytes (1.5 floats copied per element) and ppqhip_roundtune_fwd_multi per tensor at the same size (12 bytes per element),
           rotating over 4 sets of tensors; a sample is the device-event time of `--launches` back-to-back launches over their
           number, the arms alternated.
The last line printed is one JSON object.

    python tools/mx_roundtune_bench.py [--blocks 3] [--steps 60] [--lr 1e-3] [--repeats 3] [--launches 50] [--out profiles/mx_roundtune.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from mx_bench import sample, spread  # noqa: E402

MODELS = {'yolov6s': ('yolov6s_graph', (2, 3, 160, 160), 8), 'resnet50': ('resnet50_graph', (8, 3, 224, 224), 4)}
ARMS = {'torch': dict(use_kernels=False, group_weights=False, use_hip_graph=False),
        'kernel': dict(use_kernels=True, group_weights=True, use_hip_graph=False),
        'graph': dict(use_kernels=True, group_weights=True, use_hip_graph=True)}
FORWARD_SHAPES = [(512, 4608), (4096, 4096)]          # the largest ResNet-50 conv weight as [O, C kh kw]; a 4096 x 4096 Gemm weight


class Model:
    def __init__(self, name: str, device: str = 'cuda'):
        from ppq_amd import harness, quantize_graph_mx
        builder, shape, count = MODELS[name]
        self.name = name
        self.graph = getattr(harness, builder)(seed=0)
        self.ex = harness.TorchExecutor(self.graph, device)
        quantize_graph_mx(self.graph, self.ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=(device != 'cpu'))
        g = torch.Generator().manual_seed(9)
        self.batches = [torch.rand(*shape, generator=g).to(device) for _ in range(count)]
        self.parameters = [(v, v.value.detach().clone()) for op in self.graph.operations.values() for v in op.inputs
                           if v.is_parameter and isinstance(v.value, torch.Tensor)]

    def restore(self) -> None:
        for v, saved in self.parameters: v.value = saved.clone()

    def run(self, arm: str, blocks: int, steps: int, lr: float) -> dict:
        from ppq_amd import MXRoundTuningPass
        self.restore()
        p = MXRoundTuningPass(steps=steps, lr=lr, **ARMS[arm])
        p.max_blocks, p.profile_phases = blocks, True
        p.optimize(self.graph, self.batches, self.ex)
        replayed = arm == 'graph' and p.stats['graph_replays'] > 0
        ms, n = (p.phase_ms.get('graph_replays', 0.0), p.stats['graph_replays']) if replayed else (p.phase_ms.get('eager_steps', 0.0), p.stats['eager_steps'])
        return {'ms_per_step': ms / max(n, 1), 'steps': n, 'report': p.report, 'stats': dict(p.stats), 'skipped': len(p.skipped)}


def bench_steps(name: str, args, lines, summary, device: str = 'cuda'):
    model = Model(name, device)
    arms = [a for a in ARMS if device != 'cpu' or a == 'torch']
    runs = {arm: [] for arm in arms}
    for arm in arms: model.run(arm, 1, 3, args.lr)                                       # warm every arm
    for _ in range(args.repeats):
        for arm in arms: runs[arm].append(model.run(arm, args.blocks, args.steps, args.lr))      # alternated
    builder, shape, count = MODELS[name]
    lines.append(f'{name}: harness.{builder}, MXFP4_E2M1 weights, MXFP8_E4M3 activations, {count} batches of {list(shape)}, first {args.blocks} blocks, '
                 f'{args.steps} steps per block, lr {args.lr:g}')
    summary[name] = {}
    base = statistics.median(r['ms_per_step'] for r in runs[arms[0]])
    for arm in arms:
        ts = [r['ms_per_step'] for r in runs[arm]]
        last = runs[arm][-1]
        med = statistics.median(ts)
        st = last['stats']
        lines.append(f'  {arm:7s} ms per step: ' + ' '.join(f'{t:.3f}' for t in ts) + f'   median {med:.3f}  spread {spread(ts) * 100:.1f} %   {base / med:.2f} x the torch arm'
                     f'   ({last["steps"]} timed steps; {st["mx_weights"]} weights, {st["grouped_weights"]} grouped, {st["graph_blocks"]} blocks replayed, '
                     f'{st["graph_failures"]} capture failures)')
        for block, pre, post in last['report']:
            lines.append(f'          {block}: loss {pre:.6e} -> {post:.6e} ({"kept" if not post > pre else "withdrawn"})')
        share = st['flipped'] / max(st['tuned_elements'], 1)
        lines.append(f'          {st["flipped"]} of {st["tuned_elements"]} elements of the kept blocks left round-to-nearest ({share * 100:.2f} %)')
        summary[name][arm] = {'ms_per_step': med, 'samples': ts, 'spread': spread(ts), 'x_torch': base / med, 'report': last['report'],
                              'flipped': st['flipped'], 'tuned_elements': st['tuned_elements'], 'graph_blocks': st['graph_blocks'],
                              'graph_failures': st['graph_failures']}
    del model
    if device != 'cpu': torch.cuda.empty_cache()


def bench_forward(shape, args, lines, summary, rotate: int = 4):
    from north_star import load_floor
    from ppq_amd import ffi
    from ppq_amd.ffi import _stream
    fl = load_floor()
    g = torch.Generator(device='cuda').manual_seed(7)
    n = shape[0] * shape[1]
    ws = [torch.randn(*shape, device='cuda', generator=g) for _ in range(rotate)]
    splits = ffi.mx_round_split_multi([(w, 'MXFP4_E2M1', -1) for w in ws])
    outs = [torch.empty_like(w) for w in ws]
    items = [[(f, r, c, 'MXFP4_E2M1', 1)] for f, r, c in splits]
    jobs = [ffi.mx_round_forward_jobs(it, [o]) for it, o in zip(items, outs)]
    scale, offset = torch.full((1,), 0.05, device='cuda'), torch.zeros(1, device='cuda')
    linear = [[(w, r, scale, offset, None, -8, 7)] for w, (_, r, _) in zip(ws, splits)]
    m = n * 3 // 2
    src, dst = [torch.randn(m, device='cuda', generator=g) for _ in range(rotate)], [torch.empty(m, device='cuda') for _ in range(rotate)]
    arms = {'copy of 12 n bytes': (lambda i: fl.floor_copy(src[i % rotate].data_ptr(), dst[i % rotate].data_ptr(), m, 256, 2, 0, _stream()), 12.0),
            'mx_round_fwd': (lambda i: ffi.mx_round_forward_multi(items[i % rotate], outs=[outs[i % rotate]], jobs=jobs[i % rotate]), 12.0 + 1 / 32),
            'roundtune_fwd': (lambda i: ffi.roundtune_forward_multi(linear[i % rotate], outs=[outs[i % rotate]]), 12.0)}
    times = {arm: [] for arm in arms}
    for arm, (fn, _) in arms.items(): sample(fn, 4)
    for _ in range(args.forward_repeats):
        for arm, (fn, _) in arms.items(): times[arm].append(sample(fn, args.launches))
    lines.append(f'forward: one MXFP4_E2M1 tensor {list(shape)} along its last axis, {n * 4 / 1e6:.1f} MB, rotating over {rotate} sets; calls through ppq_amd.ffi')
    copy = statistics.median(times['copy of 12 n bytes'])
    key = f'forward {shape[0]}x{shape[1]}'
    summary[key] = {}
    for arm, ts in times.items():
        med, per = statistics.median(ts), arms[arm][1]
        lines.append(f'  {arm:20s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{per * n / med / 1e6:.0f} GB/s   {med / copy:.2f} x the copy')
        summary[key][arm] = {'ms': med, 'spread': spread(ts), 'GBps': per * n / med / 1e6, 'x_copy': med / copy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--forward-repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--models', nargs='+', default=list(MODELS))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mx_roundtune.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_roundtune_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_roundtune_bench.py --blocks {args.blocks} --steps {args.steps} --lr {args.lr:g} --repeats {args.repeats} '
             f'--forward-repeats {args.forward_repeats} --launches {args.launches} --models {" ".join(args.models)}',
             f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    for name in args.models: bench_steps(name, args, lines, summary)
    for shape in FORWARD_SHAPES: bench_forward(shape, args, lines, summary)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
