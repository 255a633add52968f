"""Channelwise split -- the reference's ``ChannelwiseSplitPass`` (``setting.channel_split`` of its pre-quantisation pipeline).

Mirror of ppq/quantization/optim/equalization.py:577-650 (the pass) and of ppq/quantization/algorithm/equalization.py:200-290,
361-393 (``ChannelSplitHelper``, ``EqualizationPair.channel_split``).  Per pair and iteration the reference computes the keys of
layerwise equalization,

    up[c] = max |upstream rows of channel c|     down[c] = max |downstream slices of channel c|
    mask[c] = up[c] >= threshold and down[c] >= threshold

and replaces every masked channel of the upstream weights, their biases and the downstream weights by TWO channels holding
``row * (1 / sqrt(2))`` each: two channels of half the energy, whose contributions a downstream layer adds up to what the one
channel gave.  It does so with ``mask.tolist()`` -- a synchronisation -- and one torch operation per channel of every tensor.

Here a LEVEL of pairs that share no operation (``build_schedule``) is the plan launch pair of csrc/split.hip (keys, mask and
prefix sum of all its pairs), ONE copy of the level's new channel counts to the host -- the new tensors have to be allocated,
and their size is the count -- and ONE gather launch for all its tensors.  ``use_kernels=False`` is the torch arm: the reference
restated op for op, the only path on CPU tensors and the comparison arm on the device.

What is reproduced as it is and what is not followed is listed in INTEGRATION.md section 10."""
from math import prod, sqrt
from typing import Callable, Dict, Iterable, List, Sequence, Union

import torch

from .equalization import (_LINEAR_TYPES, EqualizationPair, LayerwiseEqualizationPass, _check_endpoint, _has_bias, _trans_b,
                           build_schedule, channel_axis, key_value_from_downstream, key_value_from_upstream, pair_jobs,
                           parameters_on_device, reduce_by_axis)

SPLIT_FACTOR = 1 / sqrt(2)              # channel_split hands this Python float to torch: float32 0.70710677 on a float32 tensor


# ------------------------------------------------------------------------------------ the torch arm
def split_by_mask(mask: torch.Tensor, tensor: torch.Tensor, axis: int, scale_factor: float) -> torch.Tensor:
    """``tensor`` with every masked channel of ``axis`` replaced by two channels of ``channel * scale_factor``.  The operations
    are ChannelSplitHelper.split_by_mask's (algorithm/equalization.py:203-220), because they are what the reference costs: the
    mask comes to the host (a synchronisation on the device), every resulting channel is one one-row tensor -- a product for a
    half, a view for an unsplit channel -- and ONE concatenation joins the C to 2 C of them."""
    flags = mask.tolist()
    if tensor.shape[axis] != len(flags):
        raise ValueError(f'split_by_mask: axis {axis} of a tensor shaped {tuple(tensor.shape)} holds {tensor.shape[axis]} channels, '
                         f'the mask {len(flags)}')
    channels_first = tensor.transpose(axis, 0)
    rows = []
    for c, split in enumerate(flags):
        if split: rows.extend(channels_first[c].unsqueeze(0) * scale_factor for _ in range(2))
        else: rows.append(channels_first[c].unsqueeze(0))
    return torch.cat(rows, dim=0).transpose(0, axis)


def channel_split_upstream(op, mask: torch.Tensor, scale_factor: float) -> None:
    """The OUTPUT channels of ``op`` split by ``mask``: its weight and, where it has one, its bias are rebound to the grown
    tensors (algorithm/equalization.py:222-260; a ConvTranspose raises as everywhere in this package)."""
    _check_endpoint(op)
    weight, bias = op.inputs[1], (op.inputs[-1] if _has_bias(op) else None)
    if bias is not None and not bias.is_parameter: raise ValueError(f'Bias of Op {op.name} is non-static.')
    stored_in_out = op.type in _LINEAR_TYPES and _trans_b(op) == 0        # [in, out]: the channels are the columns
    w = torch.transpose(weight.value, 1, 0) if stored_in_out else weight.value
    w = split_by_mask(mask, w, 0, scale_factor)
    if stored_in_out: w = torch.transpose(w, 1, 0)
    b = split_by_mask(mask, bias.value, 0, scale_factor) if bias is not None else None
    weight.value = w
    if bias is not None: bias.value = b


def channel_split_downstream(op, mask: torch.Tensor, scale_factor: float) -> None:
    """The INPUT channels of ``op`` split by ``mask`` (algorithm/equalization.py:262-289).  A Conv weight [O, I / G, k...] is
    brought to one row per input channel in (group, cin_local) order -- [G, O / G, I / G, k...], axes 1 and 2 exchanged, the
    first two merged --, split, and taken back the same way; the pass never gets here with G > 1 (is_group_conv)."""
    _check_endpoint(op)
    weight = op.inputs[1]
    w = weight.value
    if op.type == 'Conv':
        G = op.attributes.get('group', 1)
        per_group = torch.reshape(w, (G, w.shape[0] // G) + w.shape[1:])
        input_major = torch.transpose(per_group, 1, 2)
        rows = split_by_mask(mask, torch.reshape(input_major, (-1,) + input_major.shape[2:]), 0, scale_factor)
        input_major = torch.reshape(rows, (G, -1) + rows.shape[1:])
        per_group = torch.transpose(input_major, 1, 2)
        w = torch.reshape(per_group, (G * per_group.shape[1],) + per_group.shape[2:])
    else:
        stored_out_in = _trans_b(op) != 0                                 # [out, in]: the channels are the columns
        if stored_out_in: w = torch.transpose(w, 1, 0)
        w = split_by_mask(mask, w, 0, scale_factor)
        if stored_out_in: w = torch.transpose(w, 1, 0)
    weight.value = w


def channel_split(pair: EqualizationPair, value_threshold: float = 2, including_act: bool = False, act_multiplier: float = 0.5,
                  including_bias: bool = False, bias_multiplier: float = 0.5,
                  activations: Dict[str, torch.Tensor] = None) -> torch.Tensor:
    """EqualizationPair.channel_split (algorithm/equalization.py:361-393) with torch operations in the reference's order:
    equalization's keys, the mask, then every upstream and every downstream layer split by it; returns the mask.
    ``activations``: {output variable name: [channels, batches] absolute maxima}."""
    activations = activations or {}
    up = reduce_by_axis([key_value_from_upstream(op, including_bias=including_bias, including_act=including_act,
                                                 bias_multiplier=bias_multiplier, act_multiplier=act_multiplier,
                                                 activation=activations.get(op.outputs[0].name)) for op in pair.upstream_layers])
    down = reduce_by_axis([key_value_from_downstream(op) for op in pair.downstream_layers])
    mask = torch.logical_and(up >= value_threshold, down >= value_threshold)
    for op in pair.upstream_layers: channel_split_upstream(op, mask, SPLIT_FACTOR)
    for op in pair.downstream_layers: channel_split_downstream(op, mask, SPLIT_FACTOR)
    return mask


def is_group_conv(pair: EqualizationPair) -> bool:
    """optim/equalization.py:631-638: a pair with ANY grouped Conv endpoint is not split at all."""
    return any(op.type in {'Conv', 'ConvTranspose'} and op.attributes.get('group', 1) != 1 for op in pair.operations)


# ------------------------------------------------------------------------------------ the kernel arm
def split_tensors(pair: EqualizationPair) -> List[tuple]:
    """(variable, channel axis) of every tensor a split of this (ungrouped) pair replaces."""
    out = []
    for op in pair.upstream_layers:
        out.append((op.inputs[1], channel_axis(op, False)))
        if _has_bias(op): out.append((op.inputs[-1], 0))
    for op in pair.downstream_layers: out.append((op.inputs[1], channel_axis(op, True)))
    return out


def mask_of_plan(src_of: torch.Tensor, num_channel: int) -> torch.Tensor:
    """The mask a plan ``src_of[:count]`` came from."""
    mask = torch.zeros(num_channel, dtype=torch.bool, device=src_of.device)
    mask[(src_of[src_of < 0] & 0x7fffffff).long()] = True
    return mask


class ChannelwiseSplitPass(LayerwiseEqualizationPass):
    """optim/equalization.py:577-650.  The first nine arguments are the reference's (names, order, defaults).

    ``use_kernels``: float32 CUDA parameters are split by the HIP kernels, a LEVEL of independent pairs per plan launch pair,
    copy and gather launch (``schedule='levelled'``; ``'sequential'`` is the reference's order, one pair at a time, and exists
    for the tests).  CPU parameters, and everything when ``use_kernels`` is off, take the torch arm over the same schedule.

    ``stats``: ``pairs``, ``skipped_pairs`` (grouped), ``levels``, ``launches`` (device kernels: two per plan chunk, one per
    gather chunk -- a chunk holds 32 jobs / 72 segments), ``copies`` (device-to-host: one per level on the kernel arm; the torch
    arm's ``tolist()`` per tensor are not counted), ``channels_before`` / ``channels_after`` (summed over the pairs),
    ``split_channels`` (one entry per iteration) and ``collect_launches``.  ``keep_masks = True`` keeps every mask in
    ``masks[(iteration, pair index)]`` (an inspection aid)."""
    PASS_NAME = 'PPQ Channelwise Split Pass'

    def __init__(self, iterations: int, threshold: float = 2, including_bias: bool = False, bias_multiplier: float = 0.5,
                 including_act: bool = False, act_multiplier: float = 0.5, interested_layers: List[str] = None,
                 optimize_level: int = 2, verbose: bool = False, use_kernels: bool = True, schedule: str = 'levelled') -> None:
        super().__init__(iterations=iterations, value_threshold=threshold, including_bias=including_bias, bias_multiplier=bias_multiplier,
                         including_act=including_act, act_multiplier=act_multiplier, interested_layers=interested_layers,
                         optimize_level=optimize_level, verbose=verbose, use_kernels=use_kernels, schedule=schedule)
        self.keep_masks = False
        self.masks: Dict[tuple, torch.Tensor] = {}          # ``activations`` holds the LAST iteration's maxima here
        self.stats: Dict[str, object] = {}

    def optimize(self, graph, dataloader: Iterable = None, executor=None, collate_fn: Callable = None,
                 activations: Union[Dict[str, torch.Tensor], Sequence[Dict[str, torch.Tensor]]] = None, **kwargs) -> None:
        """``activations`` (not in the reference): per-channel maxima to use instead of collecting them -- one
        {output variable name: [channels]} per iteration (the channel counts change), or a single one for ``iterations == 1``."""
        interested = self.interested_operations(graph)
        pairs = self.pairs = self.find_equalization_pair(graph=graph, interested_operations=interested)
        active = [p for p, pair in enumerate(pairs) if not is_group_conv(pair)]
        for p in active:
            for op in pairs[p].operations: _check_endpoint(op)
        params = [v.value for p in active for op in pairs[p].operations for v in op.inputs[1:] if v.is_parameter]
        on_device = parameters_on_device(params, self.use_kernels, 'ChannelwiseSplitPass')
        if isinstance(activations, dict): activations = [activations]
        if self.including_act and activations is not None and len(activations) < self.iterations:
            raise ValueError(f'ChannelwiseSplitPass: {self.iterations} iterations need as many activation records, {len(activations)} given')
        self.stats = dict(pairs=len(pairs), skipped_pairs=len(pairs) - len(active), levels=0, launches=0, copies=0,
                          channels_before=sum(pair.num_channel() for pair in pairs), channels_after=0,
                          split_channels=[0] * self.iterations, collect_launches=0)
        self.masks, self.activations = {}, {}
        if self.verbose: print(f'{len(pairs)} equalization pair(s) was found, ready to run optimization.')
        run = self._run_kernels if on_device else self._run_torch
        active_pairs = [pairs[p] for p in active]
        with torch.no_grad():
            if self.including_act:                          # the maxima of the graph AS IT THEN IS, every iteration (:621-627)
                for it in range(self.iterations):
                    if activations is not None: acts = activations[it]
                    else: acts = self.collect_activations(graph, executor, dataloader, collate_fn, interested, on_device=on_device)
                    self.activations = {n: a.detach().reshape(-1).contiguous() for n, a in acts.items()}
                    for level in build_schedule(active_pairs, 1, self.schedule):
                        run(pairs, [(it, active[q]) for _, q in level])
            else:
                for level in build_schedule(active_pairs, self.iterations, self.schedule):
                    run(pairs, [(it, active[q]) for it, q in level])
        self.stats['channels_after'] = sum(pair.num_channel() for pair in pairs)

        # channel split changes the fp32 value of the weights: store it for the procedures that follow (:646-650)
        for op in graph.operations.values():
            if hasattr(op, 'store_parameter_value'): op.store_parameter_value()

    def _run_torch(self, pairs, level) -> None:
        self.stats['levels'] += 1
        acts = {n: a.unsqueeze(-1) for n, a in self.activations.items()}
        for it, p in level:
            before = pairs[p].num_channel()
            mask = channel_split(pairs[p], value_threshold=self.value_threshold, including_bias=self.including_bias,
                                 including_act=self.including_act, bias_multiplier=self.bias_multiplier,
                                 act_multiplier=self.act_multiplier, activations=acts)
            self.stats['split_channels'][it] += pairs[p].num_channel() - before
            if self.keep_masks: self.masks[(it, p)] = mask

    def plan_items(self, pair: EqualizationPair, src_of: torch.Tensor, count: torch.Tensor) -> tuple:
        """One pair's item of ``ffi.split_plan_table``: the key segments are the ones equalization reads."""
        (_, _, segments), _ = pair_jobs(pair, None, self.value_threshold, self.including_bias, self.including_act, self.bias_multiplier,
                                        self.act_multiplier, self.activations, num_channel=src_of.numel() // 2)
        return (src_of, count, self.value_threshold, segments)

    def _run_kernels(self, pairs, level) -> None:
        """One level: the plans of its pairs, ONE copy of their counts, the gather of every tensor of the pairs that grow.  The
        tables are built per level: the split before replaced the tensors they would point to."""
        from . import ffi
        self.stats['levels'] += 1
        device = pairs[level[0][1]].upstream_layers[0].inputs[1].value.device
        sizes = [pairs[p].num_channel() for _, p in level]
        plans = list(torch.split(torch.empty(2 * sum(sizes), dtype=torch.int32, device=device), [2 * C for C in sizes]))
        counts = torch.empty(len(level), dtype=torch.int32, device=device)
        items = [self.plan_items(pairs[p], plans[k], counts[k:k + 1]) for k, (_, p) in enumerate(level)]
        ffi.split_plan_multi(items)
        self.stats['launches'] += ffi.split_plan_launches(items)
        new_sizes = counts.tolist()                                        # the one copy: the new tensors are allocated by it
        self.stats['copies'] += 1
        gathers, rebind = [], []
        for (it, p), C, count, src_of in zip(level, sizes, new_sizes, plans):
            if self.keep_masks: self.masks[(it, p)] = mask_of_plan(src_of[:count], C)
            self.stats['split_channels'][it] += count - C
            if count == C: continue                                        # nothing splits: the pair's tensors stay the same objects
            for var, axis in split_tensors(pairs[p]):
                x = var.value
                if x.shape[axis] != C: raise ValueError(f'ChannelwiseSplitPass: {var.name} has {x.shape[axis]} channels, its pair has {C}')
                out = torch.empty(x.shape[:axis] + (count,) + x.shape[axis + 1:], dtype=torch.float32, device=device)
                gathers.append((x, out, src_of, C, count, prod(x.shape[axis + 1:])))
                rebind.append((var, out))
        if not gathers: return
        ffi.split_apply_multi(gathers)
        self.stats['launches'] += ffi.split_apply_launches(gathers)
        for var, out in rebind: var.value = out
