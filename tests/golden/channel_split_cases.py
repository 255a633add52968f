"""Channelwise-split cases shared by tests/golden/make_channel_split.py (which records what the reference's
ChannelwiseSplitPass does to them on the CPU) and the channel-split tests.

A case is one of the topologies of equalization_cases.py (``base``: its name there; parameters and batches are the ones of that
case, seeded there) plus the pass settings.  ``input_scale`` multiplies the calibration batches: the activation maxima of
``zero_act`` are made large enough that ``0.5 * act`` lifts upstream keys over the threshold which the weights alone leave under
it -- ``zero_act_off`` is the same case without activations, so the two record different masks.  ``no_split`` has a threshold
nothing reaches: a level in which nothing splits.  ``nan_key``: the NaN upstream key meets a downstream key over the threshold
and must stay single.

``executable``: the harness can run the graph and its outputs are finite (see equalization_cases.py)."""
from math import sqrt

import numpy as np
import torch

import equalization_cases as EC

_BASE = {c['name']: k for k, c in enumerate(EC.CASES)}

CASES = [
    dict(name='chain', base='chain', threshold=0.5, iterations=3, including_bias=False, including_act=False),
    dict(name='add_pair', base='add_pair', threshold=0.5, iterations=2, including_bias=True, including_act=False),
    dict(name='grouped', base='grouped', threshold=0.5, iterations=2, including_bias=False, including_act=False),
    dict(name='gemm', base='gemm', threshold=0.5, iterations=2, including_bias=True, including_act=False),
    dict(name='zero_act', base='zero_act', threshold=1.0, iterations=2, including_bias=True, including_act=True, input_scale=4.0),
    dict(name='zero_act_off', base='zero_act', threshold=1.0, iterations=2, including_bias=True, including_act=False, input_scale=4.0),
    dict(name='nan_key', base='nan_key', threshold=0.05, iterations=1, including_bias=False, including_act=False),
    dict(name='no_split', base='chain', threshold=1000.0, iterations=1, including_bias=False, including_act=False),
]
for _c in CASES: _c['executable'] = EC.CASES[_BASE[_c['base']]]['executable']


def base_index(k: int) -> int:
    return _BASE[CASES[k]['base']]


def case_parameters(k: int) -> dict:
    return EC.case_parameters(base_index(k))


def case_batches(k: int) -> list:
    return [x * CASES[k].get('input_scale', 1.0) for x in EC.case_batches(base_index(k))]


def harness_graph(k: int, parameters: dict = None):
    """Case k as a ``ppq_amd.harness`` graph; ``parameters`` may hold split tensors (any channel counts that agree)."""
    return EC.harness_graph(base_index(k), case_parameters(k) if parameters is None else parameters)


def split_map(mask) -> np.ndarray:
    """The plan of a mask, as ppqhip_split_plan_job describes it: entry d holds the channel it copies, bit 31 set on both halves
    of a split channel.  int32, mask.sum() + len(mask) entries."""
    out = []
    for c, m in enumerate(np.asarray(mask).astype(bool).tolist()):
        out += [c | 0x80000000] * 2 if m else [c]
    return np.array(out, dtype=np.uint32).view(np.int32)


def split_reference(x: torch.Tensor, plan: np.ndarray, axis: int) -> torch.Tensor:
    """``x`` gathered along ``axis`` by a plan, on the CPU: index_select, then ONE float32 multiply of the split channels."""
    plan = torch.from_numpy(np.asarray(plan).view(np.uint32).astype(np.int64))
    out = torch.index_select(x, axis, plan & 0x7fffffff).clone()
    halves = (plan >> 31).bool()
    idx = [slice(None)] * x.ndim
    idx[axis] = halves
    out[tuple(idx)] = out[tuple(idx)] * (1 / sqrt(2))
    return out
