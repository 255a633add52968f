"""The skinny linear INT8 GEMM (ppq_amd/int8.py int8_matmul(..., skinny=True)) against the tile kernel on the
layers it was written for, on the GPU, in the same process.

  arms    skinny  int8_matmul(..., skinny=True): one launch of ppqhip_int8_gemm_skinny / ppqhip_int4_gemm_skinny
          tile    the same call with skinny=False: one launch of ppqhip_int8_gemm / ppqhip_int4_gemm, the 64 x 64 tile kernel
  codecs  int8 and packed INT4 weights, the same codes (-8 .. 7) in both
  shapes  M in 1, 16, 64; (N, K) = (1000, 2048) ResNet-50's head, (3072, 768) and (768, 3072) ViT-B's MLP, (4096, 4096)

The layer is bound by reading its weight, so the weights ROTATE over as many sets as together exceed the 256 MiB Infinity Cache in
the SMALLER codec (int4), and the rotation goes on across arms and cases: no launch finds its weight in a cache.  The tool checks on four sets that the arms give the same bits, then
takes `--repeats` samples per arm, arms ALTERNATED; a sample is the device-event time of `--launches` back-to-back calls divided by their
number.  That is a time per CALL: where it sits at the host's floor of some 0.03 ms it says nothing about the kernel.  Kernel times
come from a run of their own under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -o skinny --output-format csv -- python tools/int8_skinny_bench.py --trace
    python tools/int8_skinny_bench.py --from-trace DIR/.../skinny_kernel_trace.csv [--out profiles/int8_skinny.txt]

`--trace` issues exactly `--launches` calls per shape, codec and arm and nothing else on these kernels; `--from-trace` (no GPU needed)
cuts the trace's dispatches of the two kernels, in start order, into those groups, drops the first two of each as warm-up and reports
the median kernel time and the algorithmic weight bytes over it as a fraction of 8 TB/s.  The last line printed is one JSON object.

    python tools/int8_skinny_bench.py [--repeats 5] [--launches 40] [--out profiles/int8_skinny.txt]"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLC_BYTES = 256 * 2 ** 20
PEAK_BYTES_PER_S = 8e12
MS = (1, 16, 64)
SHAPES = [('ResNet-50 head', 1000, 2048), ('ViT-B MLP up', 3072, 768), ('ViT-B MLP down', 768, 3072), ('4096 x 4096', 4096, 4096)]
CODECS = ('int8', 'int4')
ARMS = ('skinny', 'tile')
WARM = 2
cases = lambda: [(name, n, k, m, codec) for name, n, k in SHAPES for m in MS for codec in CODECS]
label = lambda name, n, k, m, codec: f'{name}: M = {m}, N = {n}, K = {k}, {codec} weight'
weight_bytes = lambda n, k, codec: n * ((k + 31) // 32 * 32) // (2 if codec == 'int4' else 1)
sets_of = lambda n, k: LLC_BYTES // weight_bytes(n, k, 'int4') + 2


def operands(n, k, g):
    """One activation per M and `sets_of(n, k)` weights of random codes in -8 .. 7, as int8 and packed."""
    import torch
    from ppq_amd import Int8Tensor, int4_pack
    scale, kp = torch.tensor(0.02, device='cuda'), (k + 31) // 32 * 32
    code = lambda rows, lo, hi: torch.nn.functional.pad(torch.randint(lo, hi, (rows, k), device='cuda', generator=g, dtype=torch.int8), (0, kp - k))
    xs = {m: Int8Tensor(code(m, -128, 128), (m, k), 1, scale, 0, -128, 127, 0) for m in MS}
    w8 = []
    for _ in range(sets_of(n, k)):
        v = code(n, -8, 8)
        w8.append(Int8Tensor(v, (n, k), 1, torch.full((n,), 0.01, device='cuda'), 0, -8, 7, 0, v.sum(1, dtype=torch.int32)))
    return xs, {'int8': w8, 'int4': [int4_pack(w) for w in w8]}


def measure(args):
    import torch
    from ppq_amd import int8_matmul
    from tools.int8_bench import sample
    if not torch.cuda.is_available(): raise SystemExit('tools/int8_skinny_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/int8_skinny_bench.py --repeats {args.repeats} --launches {args.launches}' + (' --trace' if args.trace else ''),
             f'# device: {torch.cuda.get_device_name(0)}; ms per CALL by device events (the host floor included), median [min, max]']
    summary, g = {'device': torch.cuda.get_device_name(0)}, torch.Generator(device='cuda').manual_seed(11)
    count = [0]                                                                          # launches so far: the rotation goes on across arms and cases

    def run(fn, launches, timed=True):
        first, count[0] = count[0], count[0] + launches
        if timed: return sample(lambda i: fn(first + i), launches)
        for i in range(launches): fn(first + i)
    for name, n, k in SHAPES:
        xs, ws = operands(n, k, g)
        bias, sets = torch.randn(n, device='cuda', generator=g), sets_of(n, k)
        for m in MS:
            for codec in CODECS:
                arms = {arm: (lambda i, s=arm == 'skinny': int8_matmul(xs[m], ws[codec][i % sets], bias, skinny=s)) for arm in ARMS}
                if args.trace:
                    for fn in arms.values(): run(fn, args.launches, timed=False)
                    continue
                same = all(torch.equal(arms['skinny'](i).view(torch.int32), arms['tile'](i).view(torch.int32)) for i in range(4))
                times = {arm: [] for arm in ARMS}
                for fn in arms.values(): run(fn, 8)
                for _ in range(args.repeats):
                    for arm, fn in arms.items(): times[arm].append(run(fn, args.launches))
                med = {arm: statistics.median(ts) for arm, ts in times.items()}
                lines.append(f'{label(name, n, k, m, codec)}; {sets} weight sets of {weight_bytes(n, k, codec) / 2 ** 20:.2f} MiB; same bits: {same}')
                for arm, ts in times.items():
                    lines.append(f'  {arm:6s} {med[arm]:.4f} [{min(ts):.4f}, {max(ts):.4f}] ms per call   {med["tile"] / med[arm]:.2f} x tile')
                summary[label(name, n, k, m, codec)] = {'same_bits': same, **{arm: {'ms': med[arm], 'min_ms': min(ts), 'max_ms': max(ts)} for arm, ts in times.items()}}
        del xs, ws
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    return lines, summary


def from_trace(args):
    """Kernel times of a --trace run: the dispatches of the two GEMM kernels in start order, `--launches` per case and arm."""
    with open(args.from_trace, newline='') as f: rows = [r for r in csv.DictReader(f) if 'q8_skinny_kernel' in r['Kernel_Name'] or 'q8_gemm_kernel' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    groups = [(c, arm) for c in cases() for arm in ARMS]
    if len(rows) != len(groups) * args.launches: raise SystemExit(f'{len(rows)} dispatches in the trace, expected {len(groups)} x {args.launches}')
    lines = [f'# kernel times: rocprofv3 --kernel-trace --stats of tools/int8_skinny_bench.py --trace --launches {args.launches}, a run of its own;',
             f'# median [min, max] in microseconds of the {args.launches - WARM} dispatches after {WARM} of warm-up; weight GB/s = the weight\'s bytes over the median, and its share of 8 TB/s']
    summary = {}
    for j, (c, arm) in enumerate(groups):
        group = rows[j * args.launches:(j + 1) * args.launches]
        want = 'q8_skinny_kernel' if arm == 'skinny' else 'q8_gemm_kernel'
        if any(want not in r['Kernel_Name'] for r in group): raise SystemExit(f'the trace does not follow the tool\'s order at {label(*c)}, {arm}')
        us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in group[WARM:]]
        med, wb = statistics.median(us), weight_bytes(c[1], c[2], c[4])
        if arm == ARMS[0]: lines.append(label(*c))
        lines.append(f'  {arm:6s} {med:8.2f} [{min(us):.2f}, {max(us):.2f}] us   weight {wb / med / 1e3:7.0f} GB/s = {wb / (med * 1e-6) / PEAK_BYTES_PER_S * 100:4.1f} % of 8 TB/s')
        summary.setdefault(label(*c), {})[arm] = {'kernel_us': med, 'min_us': min(us), 'max_us': max(us), 'weight_bytes': wb}
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
