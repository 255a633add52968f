"""The MX scale rules on the GPU: what FLOOR, CEIL, EVEN and MSE cost in the fake-quant and the pack
kernels next to the copy floor, and what they buy in squared error.

  tensors  rows     [8192, 4096] along the last axis (a Gemm activation): the rows4 body                   134 MB in
           strided  [32, 256, 56, 56] along axis 1 (an NCHW conv activation): the strided body             103 MB in
           -- the two large tensors of tools/mx_bench.py, rotating over 4 inputs and 4 outputs as there
  arms     copy     tools/floor floor_copy on the same floats (8 bytes per element)
           fq       ppqhip_mx_fq under each rule, `format | rule << 8`             8 bytes per element
           pack     ppqhip_mx_pack under each rule into preallocated outputs       4 bytes + the packed bytes per element
           for `--formats` (default MXFP8_E4M3 and MXFP4_E2M1: the widest and the narrowest packed element)
A sample is the device-event time of `--launches` back-to-back launches divided by their number; `--repeats` samples per arm, arms
ALTERNATED; medians and (max - min) / median are reported, and each arm's share of the copy of its own tensor.
Error: sum (y - x)^2 / sum x^2 of mx_fake_quant on one fixed tensor -- [4096, 1024] Gaussian times a log-normal factor per block of
32 -- for the six formats and the four rules, each rule also as a fraction of FLOOR.  The last line printed is one JSON object.

    python tools/mx_scale_bench.py [--repeats 7] [--launches 20] [--out profiles/mx_scale.txt]"""
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

TENSORS = [('rows', (8192, 4096), -1, 4), ('strided', (32, 256, 56, 56), 1, 4)]
FORMATS = ['MXFP8_E4M3', 'MXFP8_E5M2', 'MXFP6_E3M2', 'MXFP6_E2M3', 'MXFP4_E2M1', 'MXINT8']
RULES = ['FLOOR', 'CEIL', 'EVEN', 'MSE']


def bench_tensor(name, shape, axis, rotate, args, lines, summary):
    from north_star import load_floor
    from ppq_amd._lib import lib
    from ppq_amd.ffi import _mx_geometry, _stream, mx_format_arg, mx_packed_shapes
    fl = load_floor()
    g = torch.Generator(device='cuda').manual_seed(7)
    xs = [torch.randn(*shape, device='cuda', generator=g) for _ in range(rotate)]
    outs = [torch.empty_like(x) for x in xs]
    n = xs[0].numel()
    outer, length, inner, _ = _mx_geometry(xs[0], axis % len(shape))
    arms = {'copy': (lambda i: fl.floor_copy(xs[i % rotate].data_ptr(), outs[i % rotate].data_ptr(), n, 256, 2, 0, _stream()), 8.0)}
    keep = []
    for fmt in args.formats:
        eshape, sshape = mx_packed_shapes(shape, axis % len(shape), fmt)
        es = [torch.empty(eshape, dtype=torch.uint8, device='cuda') for _ in range(rotate)]
        ss = [torch.empty(sshape, dtype=torch.uint8, device='cuda') for _ in range(rotate)]
        keep.append((es, ss))
        packed_bytes = 4.0 + (es[0].numel() + ss[0].numel()) / n
        for rule in RULES:
            arg = mx_format_arg(fmt, rule)
            arms[f'fq {fmt} {rule}'] = ((lambda a: lambda i: lib.ppqhip_mx_fq(xs[i % rotate].data_ptr(), outs[i % rotate].data_ptr(), 0, outer, length, inner, a, _stream()))(arg), 8.0)
            arms[f'pack {fmt} {rule}'] = ((lambda a, es, ss: lambda i: lib.ppqhip_mx_pack(xs[i % rotate].data_ptr(), es[i % rotate].data_ptr(), ss[i % rotate].data_ptr(),
                                                                                          outer, length, inner, a, _stream()))(arg, es, ss), packed_bytes)
    times = {arm: [] for arm in arms}
    for arm, (fn, _) in arms.items(): sample(fn, 2)                                      # warm every arm
    for _ in range(args.repeats):
        for arm, (fn, _) in arms.items(): times[arm].append(sample(fn, args.launches))   # alternated
    lines.append(f'{name}: {list(shape)} along axis {axis} = [outer {outer}, axis_len {length}, inner {inner}], {n * 4 / 1e6:.0f} MB, rotating over {rotate} inputs and {rotate} outputs')
    copy = statistics.median(times['copy'])
    summary[name] = {}
    for arm, ts in times.items():
        med, per = statistics.median(ts), arms[arm][1]
        lines.append(f'  {arm:24s} ms per call: ' + ' '.join(f'{t:.4f}' for t in ts) + f'   median {med:.4f}  min {min(ts):.4f}  max {max(ts):.4f}  spread {spread(ts) * 100:.1f} %   '
                     f'{per * n / med / 1e6:.0f} GB/s   {med / copy:.2f} x the copy')
        summary[name][arm] = {'ms': med, 'min': min(ts), 'max': max(ts), 'spread': spread(ts), 'GBps': per * n / med / 1e6, 'x_copy': med / copy}
    del xs, outs, keep
    torch.cuda.empty_cache()


def error_table(lines, summary):
    from ppq_amd import mx_fake_quant
    g = torch.Generator(device='cuda').manual_seed(11)
    x = torch.randn(4096, 32, 32, device='cuda', generator=g) * torch.exp(torch.randn(4096, 32, 1, device='cuda', generator=g) * 2.0)
    x = x.reshape(4096, 1024)
    power = float((x.double() ** 2).sum())
    lines.append('relative squared error sum (y - x)^2 / sum x^2 of mx_fake_quant, [4096, 1024] Gaussian times exp(2 N(0, 1)) per block of 32')
    lines.append(f'  {"format":12s} ' + ' '.join(f'{r:>22s}' for r in RULES) + '    blocks moved off the floor code: CEIL / EVEN / MSE')
    summary['error'] = {}
    for fmt in FORMATS:
        codes = {r: torch.zeros(4096, 32, dtype=torch.uint8, device='cuda') for r in RULES}
        err = {r: float(((mx_fake_quant(x, fmt, scale_codes=codes[r], scale_rule=r) - x).double() ** 2).sum()) / power for r in RULES}
        moved = [float((codes[r] != codes['FLOOR']).double().mean()) for r in RULES[1:]]
        lines.append(f'  {fmt:12s} ' + ' '.join(f'{err[r]:12.5e} ({err[r] / err["FLOOR"]:6.4f}x)' for r in RULES) + '    ' + ' / '.join(f'{m * 100:.1f} %' for m in moved))
        summary['error'][fmt] = {r: err[r] for r in RULES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--formats', nargs='+', default=['MXFP8_E4M3', 'MXFP4_E2M1'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available(): raise SystemExit('tools/mx_scale_bench.py measures on the GPU; none is visible')
    lines = [f'# tools/mx_scale_bench.py --repeats {args.repeats} --launches {args.launches} --formats {" ".join(args.formats)}',
             f'# device: {torch.cuda.get_device_name(0)}']
    summary = {'device': torch.cuda.get_device_name(0)}
    for name, shape, axis, rotate in TENSORS: bench_tensor(name, shape, axis, rotate, args, lines, summary)
    error_table(lines, summary)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f: f.write(text + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
