"""int8_bmm (ppq_amd/int8.py) against what a user had before it, on attention's two MatMuls, on the GPU, in one
process.

  arms    bmm     int8_bmm: one launch of ppqhip_int8_bmm for all batches
          float   torch.matmul on the DEQUANTISED float32 operands, the dequantisation included: what serves these MatMuls without it
          loop    (a . b^T only) int8_matmul once per batch, b as a weight with sums: the family's kernel, `batch` launches
  shapes  ViT-B/16 at 8 images (96 heads): Q.K^T 197 x 197 x 64 and P.V 197 x 64 x 197; and 96 x 1024 x 1024 x 64 (a . b^T)

Per-call times are device-event times of `--launches` back-to-back calls divided by their number, `--repeats` samples per arm, arms
ALTERNATED; near the host's floor of some 0.03 ms a launch they say little about a kernel.  Kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats -d DIR -o bmm --output-format csv -- python tools/int8_bmm_bench.py --trace
    python tools/int8_bmm_bench.py --from-trace DIR/.../bmm_kernel_trace.csv [--out profiles/int8_bmm.txt]

`--trace` issues per shape `--launches` calls of each arm in the order bmm, float, loop, the bmm and loop arms through their bindings
with `mul` made beforehand, so that every dispatch between the last q8_bmm_kernel of a shape and the next q8_gemm_kernel / q8_bmm_kernel
belongs to the float arm.  `--from-trace` (no GPU needed) sums each arm's dispatches per call, drops the first two calls as warm-up and
reports the median.  The last line printed is one JSON object.

    python tools/int8_bmm_bench.py [--repeats 5] [--launches 40] [--out profiles/int8_bmm.txt]"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, transpose_b, batch, M, N, K, za, zb): a softmax output is unsigned, stored re-centred with zero point -128
SHAPES = [('ViT-B/16 Q.K^T', True, 96, 197, 197, 64, 3, 0), ('ViT-B/16 P.V', False, 96, 197, 64, 197, -128, 4), ('1024 x 1024 x 64', True, 96, 1024, 1024, 64, 3, 0)]
WARM = 2
label = lambda name, tb, batch, m, n, k, za, zb: f'{name}: {batch} x {m} x {n} x {k}, {"a . b^T" if tb else "a . b"}, za = {za}, zb = {zb}'
arms_of = lambda tb: ('bmm', 'float', 'loop') if tb else ('bmm', 'float')


def operands(case, g):
    """The two activations of random codes, and b's batches as weights with sums for the loop arm."""
    import torch
    from ppq_amd import Int8Tensor
    _, tb, batch, m, n, k, za, zb = case
    def codes(rows, cols, pad):
        v = torch.randint(-128, 128, (batch, rows, cols), device='cuda', generator=g, dtype=torch.int8)
        return torch.nn.functional.pad(v, (0, -cols % 32), value=pad)
    A = Int8Tensor(codes(m, k, za), (batch, m, k), 2, torch.tensor(0.02, device='cuda'), za, -128, 127, 0)
    B = Int8Tensor(codes(n, k, zb) if tb else codes(k, n, zb), (batch, n, k) if tb else (batch, k, n), 2, torch.tensor(0.015, device='cuda'), zb, -128, 127, 0)
    As = [Int8Tensor(A.values[i], (m, k), 1, A.scale, za, -128, 127, 0) for i in range(batch)] if tb else None
    Ws = [Int8Tensor(B.values[i], (n, k), 1, B.scale, 0, -128, 127, 0, B.values[i].sum(1, dtype=torch.int32)) for i in range(batch)] if tb else None
    return A, B, As, Ws


def arms(case, A, B, As, Ws, bindings):
    import torch
    from ppq_amd import CUDA, int8_bmm, int8_matmul
    _, tb, batch, m, n, k, za, zb = case
    f = {'float': lambda: torch.matmul(A.dequantize(), B.dequantize().transpose(1, 2) if tb else B.dequantize())}
    if bindings:
        mul = A.scale.reshape(1) * B.scale.reshape(1)
        muln = mul.expand(n).contiguous()
        f['bmm'] = lambda: CUDA.Int8Bmm(A.values, B.values, tb, za, zb, mul, n)
        if tb: f['loop'] = lambda: [CUDA.Int8Matmul(x.values, w.values, w.sums, za, muln) for x, w in zip(As, Ws)]
    else:
        f['bmm'] = lambda: int8_bmm(A, B, tb)
        if tb: f['loop'] = lambda: [int8_matmul(x, w) for x, w in zip(As, Ws)]
    return {arm: f[arm] for arm in arms_of(tb)}


def measure(args):
    import torch
    from tools.int8_bench import sample
    if not torch.cuda.is_available(): raise SystemExit('tools/int8_bmm_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/int8_bmm_bench.py --repeats {args.repeats} --launches {args.launches}' + (' --trace' if args.trace else ''),
             f'# device: {torch.cuda.get_device_name(0)}; ms per CALL by device events (the host floor included), median [min, max]']
    summary, g = {'device': torch.cuda.get_device_name(0)}, torch.Generator(device='cuda').manual_seed(11)
    prepared = [(case, arms(case, *operands(case, g), args.trace)) for case in SHAPES]    # every operand exists before the first traced call
    torch.cuda.synchronize()
    for case, fs in prepared:
        if args.trace:
            for fn in fs.values():
                for _ in range(args.launches): fn()
            torch.cuda.synchronize()
            continue
        same = torch.equal(fs['bmm']().view(torch.int32), torch.stack(fs['loop']()).view(torch.int32)) if case[1] else None
        err = float((fs['bmm']() - fs['float']()).abs().max() / fs['float']().abs().max())
        times = {arm: [] for arm in fs}
        for fn in fs.values(): sample(lambda i: fn(), 4)
        for _ in range(args.repeats):
            for arm, fn in fs.items(): times[arm].append(sample(lambda i: fn(), args.launches))
        med = {arm: statistics.median(ts) for arm, ts in times.items()}
        lines.append(f'{label(*case)}; bits of the loop arm: {same}; max |bmm - float| / max |float| = {err:.2e}')
        for arm, ts in times.items(): lines.append(f'  {arm:6s} {med[arm]:.4f} [{min(ts):.4f}, {max(ts):.4f}] ms per call   {med[arm] / med["bmm"]:.2f} x bmm')
        summary[label(*case)] = {'same_bits_as_loop': same, 'rel_err_vs_float': err, **{arm: {'ms': med[arm], 'min_ms': min(ts), 'max_ms': max(ts)} for arm, ts in times.items()}}
    torch.cuda.synchronize()
    return lines, summary


def from_trace(args):
    """Kernel time per call and arm of a --trace run: the dispatches in start order, cut as the module docstring says."""
    with open(args.from_trace, newline='') as f: rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    us = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    first = next(i for i, r in enumerate(rows) if 'q8_bmm_kernel' in r['Kernel_Name'])
    rows, at = rows[first:], 0
    lines = [f'# kernel times: rocprofv3 --kernel-trace --stats of tools/int8_bmm_bench.py --trace --launches {args.launches}, a run of its own;',
             f'# microseconds of kernel time per CALL (all of a call\'s dispatches summed), median [min, max] of the {args.launches - WARM} calls after {WARM} of warm-up']
    summary = {}
    for case in SHAPES:
        lines.append(label(*case))
        for arm in arms_of(case[1]):
            if arm == 'float':                                                           # up to the next kernel of this family
                end = next((i for i in range(at, len(rows)) if 'q8_gemm_kernel' in rows[i]['Kernel_Name'] or 'q8_bmm_kernel' in rows[i]['Kernel_Name']), len(rows))
            else: end = at + args.launches * (case[2] if arm == 'loop' else 1)
            group, per = rows[at:end], (end - at) // args.launches
            want = {'bmm': 'q8_bmm_kernel', 'loop': 'q8_gemm_kernel'}.get(arm)
            if arm == 'float' and group:                                                 # a call ends with the matmul's own kernel, the segment's last;
                ends = [i + 1 for i, r in enumerate(group) if r['Kernel_Name'] == group[-1]['Kernel_Name']]     # what the first call adds is warm-up
                split = [group[a:b] for a, b in zip([0] + ends, ends)]
            else: split = [group[j * per:(j + 1) * per] for j in range(args.launches)] if per * args.launches == len(group) else []
            if len(split) != args.launches or per == 0 or (want and any(want not in r['Kernel_Name'] for r in group)):
                raise SystemExit(f'the trace does not follow the tool\'s order at {label(*case)}, {arm}: {len(group)} dispatches')
            calls = [sum(us(r) for r in rs) for rs in split[WARM:]]
            med, at = statistics.median(calls), end
            lines.append(f'  {arm:6s} {med:9.2f} [{min(calls):.2f}, {max(calls):.2f}] us per call in {per} dispatch(es)')
            summary.setdefault(label(*case), {})[arm] = {'kernel_us': med, 'min_us': min(calls), 'max_us': max(calls), 'dispatches': per}
    return lines, summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--trace', action='store_true', help='only issue the launches, for a run under rocprofv3 --kernel-trace')
    ap.add_argument('--from-trace', default=None, help='the kernel trace (csv) of a --trace run: report kernel times from it')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines, summary = from_trace(args) if args.from_trace else measure(args)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a' if args.from_trace else 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
