"""Record what the REFERENCE's ChannelwiseSplitPass (ppq/quantization/optim/equalization.py:577-650) does on the CPU to the
case graphs of channel_split_cases.py.

Run where the reference is importable (oracle/reference_import.find_reference); no test imports the reference:

    python tests/golden/make_channel_split.py

Writes tests/golden/channel_split.npz -- per case k the initial parameters (``c{k}_init_<var>``), the mask of every split pair
in every iteration (``c{k}_mask_it{n}_p{p}``, n from 1, p the index in the pair list), every parameter after every iteration
(``c{k}_it{n}_<var>``), for the cases with ``including_act`` the per-channel activation maxima the reference collected at the
start of every iteration (``c{k}_act_it{n}_<var>``) and, for the executable cases, one input batch with the reference's graph
outputs before and after the pass (``c{k}_x``, ``c{k}_before_<var>``, ``c{k}_after_<var>``) -- and
tests/golden/channel_split.json: per case the pair list, the pairs skipped as grouped and ``drift = max |after - before| / max
|before|`` of the reference's own outputs, and the pass constructor's parameters [name, default, required].  The conditions
the tests rely on (check_conditions) are asserted before anything is written.  The archive is written with fixed time stamps:
two runs give the same bytes.  The import shims and the graph builder are make_equalization.py's."""
import contextlib
import inspect
import io
import json
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_equalization import pair_names, reference_graph  # noqa: E402  (sets up the shims and imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppq import TorchExecutor  # noqa: E402
from ppq.quantization.algorithm.equalization import ChannelSplitHelper, EqualizationPair  # noqa: E402
from ppq.quantization.optim.equalization import EQUALIZATION_OPERATION_TYPE, ChannelwiseSplitPass  # noqa: E402

import channel_split_cases as CC  # noqa: E402
import equalization_cases as EC  # noqa: E402


def make_pass(case: dict, **kw):
    kw = dict(dict(including_bias=case['including_bias'], including_act=case['including_act']), **kw)
    return ChannelwiseSplitPass(iterations=case['iterations'], threshold=case['threshold'], **kw)


def run_case(k: int, out: dict) -> dict:
    case = CC.CASES[k]
    params = CC.case_parameters(k)
    g = reference_graph(CC.base_index(k), params)
    p = make_pass(case)
    interested = [op for op in g.operations.values() if op.type in EQUALIZATION_OPERATION_TYPE]
    found = p.find_equalization_pair(g, interested)
    pairs = pair_names(g, found)
    skipped = [q for q, pair in enumerate(found)
               if any(op.type == 'Conv' and op.attributes.get('group', 1) != 1 for op in pair.upstream_layers + pair.downstream_layers)]
    active = [q for q in range(len(pairs)) if q not in skipped]
    masks, snaps, acts, keys, seen = [], [], [], [], []
    inner_split, inner_up, inner_collect, inner_reduce = (EqualizationPair.channel_split, ChannelSplitHelper.channel_split_upstream,
                                                          ChannelwiseSplitPass.collect_activations, EqualizationPair.reduce_by_axis)

    def channel_split(self, *a, **kw):
        seen.clear()
        inner_split(self, *a, **kw)
        masks.append(seen[0].detach().clone())
        snaps.append({v.name: v.value.detach().clone() for v in g.variables.values() if v.is_parameter})

    def channel_split_upstream(op, mask, scale_factor):
        seen.append(mask)
        return inner_up(op=op, mask=mask, scale_factor=scale_factor)

    def reduce_by_axis(self, *a, **kw):
        r = inner_reduce(self, *a, **kw)
        keys.append(r.detach().clone())
        return r

    def collect_activations(self, *a, **kw):
        r = inner_collect(self, *a, **kw)
        acts.append({n: t.amax(dim=-1).detach().clone() for n, t in r.items()})
        return r
    ex = TorchExecutor(g, device='cpu')
    x = CC.case_batches(k)[0]
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        before = [y.detach().clone() for y in ex.forward(x)] if case['executable'] else None
    EqualizationPair.channel_split, EqualizationPair.reduce_by_axis = channel_split, reduce_by_axis
    ChannelSplitHelper.channel_split_upstream = staticmethod(channel_split_upstream)
    ChannelwiseSplitPass.collect_activations = collect_activations
    try:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            p.optimize(graph=g, dataloader=CC.case_batches(k), executor=ex, collate_fn=None)
    finally:
        EqualizationPair.channel_split, EqualizationPair.reduce_by_axis = inner_split, inner_reduce
        ChannelSplitHelper.channel_split_upstream = staticmethod(inner_up)
        ChannelwiseSplitPass.collect_activations = inner_collect
    A = len(active)
    assert len(masks) == len(snaps) == A * case['iterations'] and len(keys) == 2 * len(masks), (case['name'], len(masks), A)
    assert len(acts) == (case['iterations'] if case['including_act'] else 0)
    pre = f'c{k}_'
    for name, t in params.items(): out[pre + 'init_' + name] = t.numpy()
    for it in range(case['iterations']):
        for n, q in enumerate(active): out[f'{pre}mask_it{it + 1}_p{q}'] = masks[it * A + n].numpy().astype(np.uint8)
        snap = snaps[(it + 1) * A - 1] if A else params
        for name, t in snap.items(): out[f'{pre}it{it + 1}_{name}'] = t.contiguous().numpy()
        if case['including_act']:
            for name, t in acts[it].items(): out[f'{pre}act_it{it + 1}_{name}'] = t.numpy()
    info = dict(pairs=pairs, skipped=skipped, drift=None)
    if case['executable']:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            after = [y.detach().clone() for y in ex.forward(x)]
        out[pre + 'x'] = x.numpy()
        drift = 0.0
        for name, y0, y1 in zip(EC.CASES[CC.base_index(k)]['outputs'], before, after):
            out[f'{pre}before_{name}'], out[f'{pre}after_{name}'] = y0.numpy(), y1.numpy()
            drift = max(drift, float((y1 - y0).abs().max() / y0.abs().max()))
        info['drift'] = drift
    # what check_conditions needs and the archive does not hold: the keys of the first iteration's pairs
    info['_keys'] = [(keys[2 * n], keys[2 * n + 1]) for n in range(len(masks))]
    return info


def check_conditions(out: dict, book: dict) -> None:
    """The conditions without which the tests would pass vacuously."""
    names = [c['name'] for c in CC.CASES]
    first = {k: np.concatenate([v for n, v in out.items() if n.startswith(f'c{k}_mask_it1_')] or [np.zeros(0, np.uint8)]) for k in range(len(names))}
    for name in ('chain', 'add_pair', 'gemm', 'zero_act'):                # every growing case: masked and unmasked channels
        m = first[names.index(name)]
        assert 0 < m.sum() < m.size, (name, m)
    later = [n for n, v in out.items() if '_mask_it' in n and '_mask_it1_' not in n and v.any()]
    assert later, 'no case splits in iteration 2 or later'
    k = names.index('grouped')
    assert book[names[k]]['skipped'] == list(range(len(book[names[k]]['pairs']))) and first[k].size == 0, 'grouped is not skipped whole'
    on, off = names.index('zero_act'), names.index('zero_act_off')
    assert not np.array_equal(first[on], first[off]) and (first[on] >= first[off]).all(), 'activations do not change a mask'
    k = names.index('nan_key')
    up, down = book['nan_key']['_keys'][0]
    c = int(torch.isnan(up).nonzero()[0])
    assert float(down[c]) >= CC.CASES[k]['threshold'] and not out[f'c{k}_mask_it1_p0'][c] and out[f'c{k}_mask_it1_p0'].any(), 'nan_key'
    assert any(len(up) > 1 and len(down) > 1 for up, down in book['add_pair']['pairs']), 'no pair with two upstream and two downstream layers'
    assert not first[names.index('no_split')].any() and first[names.index('no_split')].size, 'no level in which nothing splits'
    for k, case in enumerate(CC.CASES):
        for n, v in out.items():
            if n.startswith(f'c{k}_mask_it1_'): assert 4 <= v.size <= 16, (n, v.size)                 # the cases hold 4 to 16 channels
            elif n.startswith(f'c{k}_mask_'): assert 4 <= v.size <= 32, (n, v.size)                   # and at most double per iteration


def write_npz(path: str, arrays: dict) -> None:
    """numpy's .npz layout with fixed time stamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    out, book = {}, {}
    for k, case in enumerate(CC.CASES):
        book[case['name']] = run_case(k, out)
        m = {n[len(f'c{k}_mask_'):]: v.tolist() for n, v in out.items() if n.startswith(f'c{k}_mask_')}
        print(case['name'], 'drift', book[case['name']]['drift'], m)
    check_conditions(out, book)
    for info in book.values(): del info['_keys']
    sig = inspect.signature(ChannelwiseSplitPass.__init__)
    constructor = [[n, None if q.default is inspect.Parameter.empty else q.default, q.default is inspect.Parameter.empty]
                   for n, q in sig.parameters.items() if n != 'self']          # [name, default, required]
    write_npz(os.path.join(HERE, 'channel_split.npz'), out)
    with open(os.path.join(HERE, 'channel_split.json'), 'w') as f:
        json.dump({'cases': book, 'constructor': constructor}, f, indent=1, sort_keys=True)
    print('channel_split.npz', len(CC.CASES), 'cases', os.path.getsize(os.path.join(HERE, 'channel_split.npz')), 'bytes')


if __name__ == '__main__':
    main()
