"""Host time per call of the per-step job-table builders of ``ppq_amd.ffi``, on the tree given as argv[1] (default: this one).

    python tools/ffi_tables_bench.py [TREE]

Tiny tensors: the launches cost the GPU microseconds, so the loop measures the host.  Prints one JSON line,
``{builder: [median us, min us, max us]}`` over REPEATS repeats of CALLS calls.  To compare two trees run it on each in turn, several
times, alternating (a fresh process each time) and compare the medians of the process medians; a builder counts as slower when that
difference exceeds max - min of the parent's process medians (profiles/ffi_tables.txt)."""
import json
import os
import statistics
import sys
import time

tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, tree)
import torch  # noqa: E402

from ppq_amd import ffi  # noqa: E402
from ppq_amd.ffi import CUDA  # noqa: E402

assert os.path.abspath(ffi.__file__).startswith(tree), ffi.__file__
DEV = 'cuda:0'
CALLS, REPEATS = 200, 15


def f(*shape): return torch.rand(*shape, device=DEV) + 0.5


def timed(fn):
    for _ in range(20): fn()
    out = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS): fn()
        out.append((time.perf_counter() - t0) / CALLS * 1e6)
        torch.cuda.synchronize()
    return [round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)]


def weight_items(n):
    items = []
    for k in range(n):
        w = f(16, 8, 3, 3)
        items.append((w, f(16, 8, 3, 3), f(16) * 0.01, torch.zeros(16, device=DEV), 0, -8, 7))
    return items, [torch.empty_like(it[0]) for it in items]


res = {}
for n in (4, 16):                      # weights of one block (tools/roundtune_bench.py: 2 .. 4 convolutions; 16: a wide block)
    items, outs = weight_items(n)
    dys = [f(16, 8, 3, 3) for _ in range(n)]
    reg = torch.tensor([0.01, 10.0, 9.0], device=DEV)
    res[f'adaround_forward_multi[{n}]'] = timed(lambda: ffi.adaround_forward_multi(items, outs))
    res[f'adaround_backward_multi[{n}]'] = timed(lambda: ffi.adaround_backward_multi(items, dys, reg, outs))
    res[f'roundtune_forward_multi[{n}]'] = timed(lambda: ffi.roundtune_forward_multi(items, outs))
    split = ffi.mx_round_split_multi([(f(16, 64), 'MXFP4_E2M1', -1) for _ in range(n)])
    mitems = [(fl, torch.rand_like(fl), c, 'MXFP4_E2M1', -1) for fl, _, c in split]
    mouts = [torch.empty_like(it[0]) for it in mitems]
    res[f'mx_round_forward_multi[{n}]'] = timed(lambda: ffi.mx_round_forward_multi(mitems, mouts))
    jobs = ffi.mx_round_forward_jobs(mitems, mouts)
    res[f'mx_round_forward_multi[{n}, jobs=]'] = timed(lambda: ffi.mx_round_forward_multi(mitems, mouts, jobs))

for n in (8, 54):                      # activations observed per forward (ResNet-50: 54 convolutions)
    xs = [f(2, 16, 8, 8) for _ in range(n)]
    slots = [torch.tensor([float('inf'), float('-inf')], device=DEV).repeat(CUDA.minmax_slots(), 1).contiguous() for _ in range(n)]
    res[f'MinMax_T_Slots_Multi[{n}]'] = timed(lambda: CUDA.MinMax_T_Slots_Multi(xs, slots))
    rows = [torch.zeros(CUDA.hist_rows(), 2048, dtype=torch.int32, device=DEV) for _ in range(n)]
    scales = [0.001] * n
    res[f'Histogram_T_Rows_Multi[{n}]'] = timed(lambda: CUDA.Histogram_T_Rows_Multi(xs, rows, scales))
    mins, maxs = [0.0] * n, [2.0] * n
    res[f'Histogram_Asymmetric_T_Rows_Multi[{n}]'] = timed(lambda: CUDA.Histogram_Asymmetric_T_Rows_Multi(mins, maxs, xs, rows))
    dests = [torch.empty(2, device=DEV) for _ in range(n)]
    hints = [ffi.quantile_hint(torch.device(DEV)) for _ in range(n)]
    res[f'Quantile_Multi[{n}]'] = timed(lambda: CUDA.Quantile_Multi(xs, 0.999, dests, hints))
    ys = [f(4, 16, 8, 8) for _ in range(n)]
    rs = [f(4, 16, 8, 8) for _ in range(n)]
    sums = [torch.empty(4, 4, dtype=torch.float64, device=DEV) for _ in range(n)]
    fq = [(y, r, f(16) * 0.01, torch.zeros(16, device=DEV), 1, -128, 127, 0) for y, r in zip(ys, rs)]
    res[f'fq_measure_rows_multi[{n}]'] = timed(lambda: ffi.fq_measure_rows_multi(fq, sums))
    ms = [(y, r, None) for y, r in zip(ys, rs)]
    res[f'measure_rows_multi[{n}]'] = timed(lambda: ffi.measure_rows_multi(ms, sums))
    accs = [torch.zeros(2, dtype=torch.float64, device=DEV) for _ in range(n)]
    fin = [(s, 1024, a, None) for s, a in zip(sums, accs)]
    res[f'measure_finish_multi[{n}]'] = timed(lambda: ffi.measure_finish_multi(fin, 'snr'))

y, b = f(2, 16, 8, 8), f(16)
res['bias_act_'] = timed(lambda: ffi.bias_act_(y, b, True))
a2, b2 = f(2, 16, 8, 8), f(2, 16, 8, 8)
res['bias_add_act'] = timed(lambda: ffi.bias_add_act(a2, b, b2, None, True))
torch.cuda.synchronize()
print(json.dumps({'tree': tree, 'us_per_call': res}))
