"""Layerwise equalization -- the reference's most used pre-quantisation pass (``LayerwiseEqualizationPass``).

Mirror of ppq/quantization/optim/equalization.py:214-575 (the pass, its pair search and its activation collection) and of
ppq/quantization/algorithm/equalization.py:27-198, 292-360, 419-451 (``EqualizationHelper``, ``EqualizationPair.equalize``,
``calculate_scale``, ``reduce_by_axis``).  Per pair the reference computes

    up[c] = max |upstream rows of channel c|     down[c] = max |downstream slices of channel c|
    s = clamp(1 / sqrt(up / down), 0.1, 10);  s = 1 where up + down < value_threshold
    upstream weight and bias *= s                downstream weight /= s

as ~20 small torch launches, ``iterations`` times.  Here pairs that share no operation are gathered into LEVELS and a level is
TWO launches (csrc/equalize.hip): the scales of all its pairs, then their application.  ``use_kernels=False`` is the torch arm:
the reference restated op for op -- the only path on CPU tensors and the comparison arm on the device.

What is reproduced as it is and what is not followed is listed in INTEGRATION.md section 7."""
from typing import Callable, Dict, Iterable, List, Optional

import torch

from .calibration import QuantizationOptimizationPass

OPTIMIZATION_LAYERTYPE_CONFIG = {                                       # optim/equalization.py:16-19
    1: {'Relu', 'MaxPool', 'GlobalMaxPool', 'PRelu', 'AveragePool', 'GlobalAveragePool', 'LeakyRelu', 'Identity'},
    2: {'Relu', 'MaxPool', 'GlobalMaxPool', 'Add', 'Sub', 'PRelu', 'AveragePool', 'GlobalAveragePool', 'LeakyRelu', 'Identity'},
}
EQUALIZATION_OPERATION_TYPE = {'Conv', 'Gemm', 'ConvTranspose'}         # optim/equalization.py:20
_LINEAR_TYPES = {'Gemm', 'MatMul'}
COLLECT_STEPS = 16                                                      # collect_activations(steps=16): `if idx > steps: break`


def _unsupported(op) -> TypeError:
    return TypeError(f'Unsupported Op type {op.name}({op.type}) for Equalization Optimization.')


def _check_endpoint(op) -> None:
    if op.type == 'ConvTranspose':
        raise TypeError(f'Unsupported Op type {op.name}({op.type}) for Equalization Optimization. '
                        'ConvTranspose is not executable by this harness')
    if op.type not in _LINEAR_TYPES | {'Conv'}: raise _unsupported(op)
    if not op.inputs[1].is_parameter: raise ValueError(f'Parameter of Op {op.name} is non-static.')


def _trans_b(op) -> int:
    """Gemm follows ``transB``.  The harness's own Gemm is ``F.linear`` (weight [out, in]), so a Gemm without the attribute is
    ``transB = 1`` here; its MatMul multiplies by [in, out]."""
    return int(op.attributes.get('transB', 1 if op.type == 'Gemm' else 0))


def _has_bias(op) -> bool:
    return len(op.inputs) == 3


# ------------------------------------------------------------------------------------ the torch arm
def key_value_from_upstream(op, including_bias: bool = False, including_act: bool = False, bias_multiplier: float = 0.5,
                            act_multiplier: float = 0.5, activation: Optional[torch.Tensor] = None) -> torch.Tensor:
    """algorithm/equalization.py:29-94 with ``including_weight = True`` and ``weight_multiplier = 1.0`` (what ``equalize``
    hands it whatever the pass was given): [channels, *] -- one row per output channel."""
    _check_endpoint(op)
    w = op.inputs[1].value * 1.0
    if op.type in _LINEAR_TYPES:
        assert w.ndim == 2, f'Unexpected Error, Parameter of MatMul {op.name} should be 2-d.'
        if _trans_b(op) == 0: w = torch.transpose(w, 1, 0)
    else: w = torch.reshape(w, (w.shape[0], -1))
    buffer = [w]
    if including_bias and _has_bias(op) and op.inputs[-1].is_parameter:
        buffer.append(torch.reshape(op.inputs[-1].value * bias_multiplier, (w.shape[0], 1)))
    if including_act and activation is not None:
        buffer.append(activation * act_multiplier)
    return torch.cat(buffer, dim=-1)


def key_value_from_downstream(op) -> torch.Tensor:
    """algorithm/equalization.py:96-136: one row per input channel.  For a grouped Conv the rows come out in (cin_local, group)
    order -- ``permute(2, 0, 1, ...)`` of [G, O / G, I / G, k...] -- which is NOT the order ``scale_to_downstream`` applies the
    scale in; reproduced as it is."""
    _check_endpoint(op)
    w = op.inputs[1].value * 1.0
    if op.type in _LINEAR_TYPES:
        assert w.ndim == 2, f'Unexpected Error, Parameter of MatMul {op.name} should be 2-d.'
        return torch.transpose(w, 1, 0) if _trans_b(op) != 0 else w
    groups = op.attributes.get('group', 1)
    if w.ndim not in (3, 4, 5): raise ValueError(f'Unexpected dimension of weight of {op.name}.')
    w = torch.reshape(w, (groups, w.shape[0] // groups) + w.shape[1:])
    w = torch.permute(w, (2, 0, 1) + tuple(range(3, w.ndim)))
    return torch.reshape(w, (w.shape[0] * w.shape[1], -1))


def scale_to_upstream(op, scale_factor: torch.Tensor) -> None:
    """algorithm/equalization.py:138-171, in place."""
    _check_endpoint(op)
    w = op.inputs[1].value
    if _has_bias(op) and not op.inputs[-1].is_parameter: raise ValueError(f'Bias of Op {op.name} is non-static.')
    with torch.no_grad():
        if op.type == 'Conv': w *= torch.reshape(scale_factor, [-1] + [1] * (w.ndim - 1))
        elif _trans_b(op) == 0: torch.transpose(w, 1, 0).mul_(torch.reshape(scale_factor, (-1, 1)))
        else: w *= torch.reshape(scale_factor, (-1, 1))
        if _has_bias(op): op.inputs[-1].value *= scale_factor


def scale_to_downstream(op, scale_factor: torch.Tensor) -> None:
    """algorithm/equalization.py:173-197, in place: [G, O / G, I / G, k...] /= scale as [G, 1, I / G, 1...]."""
    _check_endpoint(op)
    w = op.inputs[1].value
    with torch.no_grad():
        if op.type == 'Conv':
            groups = op.attributes.get('group', 1)
            v = torch.reshape(w, (groups, w.shape[0] // groups) + w.shape[1:])
            v /= torch.reshape(scale_factor, [groups, 1, -1] + [1] * (v.ndim - 3))
        elif _trans_b(op) != 0: torch.transpose(w, 1, 0).div_(torch.reshape(scale_factor, (-1, 1)))
        else: w /= torch.reshape(scale_factor, (-1, 1))


def calculate_scale(upstream_key_values: torch.Tensor, downstream_key_values: torch.Tensor, value_threshold: float,
                    scale_clip_value: float = 10) -> torch.Tensor:
    """algorithm/equalization.py:419-426."""
    scale = 1 / torch.sqrt(upstream_key_values / downstream_key_values)
    scale = torch.clamp(scale, 1 / scale_clip_value, scale_clip_value)
    scale[(upstream_key_values + downstream_key_values) < value_threshold] = 1
    return scale


def reduce_by_axis(params: List[torch.Tensor], axis: int = 1) -> torch.Tensor:
    """algorithm/equalization.py:428-436, ABSOLUTE_MAX (the only method the pass can reach)."""
    return torch.max(torch.abs(torch.cat(params, dim=axis)), dim=axis)[0]


class EqualizationPair:
    """algorithm/equalization.py:292-360: the operations whose output channels are scaled (``upstream_layers``) and the ones
    whose input channels take the inverse (``downstream_layers``)."""
    def __init__(self, upstream_layers: list, downstream_layers: list):
        self.upstream_layers = upstream_layers
        self.downstream_layers = downstream_layers

    @ property
    def operations(self) -> list:
        return list(self.upstream_layers) + list(self.downstream_layers)

    def num_channel(self) -> int:
        op = self.upstream_layers[0]
        return int(op.inputs[1].value.shape[channel_axis(op, False)])

    def equalize(self, value_threshold: float, including_weight: bool = True, weight_multiplier: float = 1.0,
                 including_act: bool = False, act_multiplier: float = 0.5, including_bias: bool = False,
                 bias_multiplier: float = 0.5, activations: Dict[str, torch.Tensor] = None) -> torch.Tensor:
        """One equalization of this pair with torch operations, the reference's sequence op for op; returns the scale.
        ``including_weight`` / ``weight_multiplier`` are accepted and NOT used, as in the reference (:335-338 does not forward
        them).  ``activations``: {output variable name: [channels, batches] absolute maxima} for ``including_act``."""
        activations = activations or {}
        ups = [key_value_from_upstream(op, including_bias=including_bias, including_act=including_act,
                                       bias_multiplier=bias_multiplier, act_multiplier=act_multiplier,
                                       activation=activations.get(op.outputs[0].name)) for op in self.upstream_layers]
        downs = [key_value_from_downstream(op) for op in self.downstream_layers]
        scale = calculate_scale(reduce_by_axis(ups), reduce_by_axis(downs), value_threshold=value_threshold)
        for op in self.upstream_layers: scale_to_upstream(op, scale)
        for op in self.downstream_layers: scale_to_downstream(op, scale)
        return scale

    def __repr__(self) -> str:
        return f'EqualizationPair({[op.name for op in self.upstream_layers]} -> {[op.name for op in self.downstream_layers]})'


# ------------------------------------------------------------------------------------ pair discovery
def _endpoints(start, relay: set, direction: str, memo: dict) -> list:
    """The last operation of every path the reference's TraversalCommand finds from ``start`` (ppq/IR/search.py:428-458 with
    ``rp_expr = type in relay``, ``ep_expr = type not in relay``): walk through relay types, stop at the first other type.  A
    path that runs out of operations inside the relay types (a graph output behind a Relu) matches nothing."""
    if start.name in memo: return memo[start.name]
    if direction == 'up': following = [v.source_op for v in start.inputs if v.source_op is not None]
    else: following = [d for v in start.outputs for d in v.dest_ops]
    found = []
    for op in following:
        for end in ([op] if op.type not in relay else _endpoints(op, relay, direction, memo)):
            if all(end is not f for f in found): found.append(end)
    memo[start.name] = found
    return found


def find_equalization_pair(graph, interested_operations: list, optimize_level: int = 2) -> List[EqualizationPair]:
    """optim/equalization.py:430-486: per interested operation ONE search down to the first non-relay operations and ONE
    search up from all of those (no closure); only the upstream set is marked visited; a pair with an endpoint that is not
    Conv / Gemm / ConvTranspose is dropped.  The layers of a pair are listed in graph order (the reference lists a set)."""
    relay = OPTIMIZATION_LAYERTYPE_CONFIG[optimize_level]
    order = {name: k for k, name in enumerate(graph.operations)}
    visited, pairs = set(), []
    for operation in interested_operations:
        if operation.name in visited: continue
        if operation.type not in EQUALIZATION_OPERATION_TYPE: continue
        downstream = _endpoints(operation, relay, 'down', {})
        memo, upstream = {}, []
        for op in downstream:
            for end in _endpoints(op, relay, 'up', memo):
                if all(end is not u for u in upstream): upstream.append(end)
        visited.update(op.name for op in upstream)
        if any(op.type not in EQUALIZATION_OPERATION_TYPE for op in upstream + downstream): continue
        if upstream and downstream:
            pairs.append(EqualizationPair(upstream_layers=sorted(upstream, key=lambda op: order[op.name]),
                                          downstream_layers=sorted(downstream, key=lambda op: order[op.name])))
    return pairs


# ------------------------------------------------------------------------------------ schedule
def build_schedule(pairs: List[EqualizationPair], iterations: int, schedule: str = 'levelled') -> List[List[tuple]]:
    """Levels of (iteration, pair index) over the reference's sequence ``for iteration: for pair``.  Pairs that share no
    operation touch disjoint memory and commute bit for bit, so an instance goes one level after the latest EARLIER instance
    that shares an operation (or a parameter) with it.  ``'sequential'``: one level per instance, the reference's order."""
    if schedule not in {'levelled', 'sequential'}: raise ValueError(f'schedule is levelled or sequential, {schedule} was given.')
    instances = [(it, p) for it in range(iterations) for p in range(len(pairs))]
    if schedule == 'sequential': return [[inst] for inst in instances]
    touched = []
    for pair in pairs:
        keys = set()
        for op in pair.operations:
            keys.add(('op', op.name))
            keys.update(('var', v.name) for v in op.inputs if v.is_parameter)
        touched.append(keys)
    last, levels = {}, []
    for it, p in instances:
        level = 1 + max((last.get(k, -1) for k in touched[p]), default=-1)
        if level == len(levels): levels.append([])
        levels[level].append((it, p))
        for k in touched[p]: last[k] = level
    return levels


# ------------------------------------------------------------------------------------ the kernel arm
def _weight(op) -> torch.Tensor:
    w = op.inputs[1].value
    if not (isinstance(w, torch.Tensor) and w.dtype == torch.float32 and w.is_contiguous()):
        raise TypeError(f'LayerwiseEqualizationPass: the weight of {op.name} must be a contiguous float32 tensor for the kernels '
                        '(use_kernels=False equalizes anything torch can)')
    return w


def channel_axis(op, downstream: bool) -> int:
    """Which axis of the weight of ``op`` is the pair's channel: the OUTPUT channels of an upstream operation, the INPUT channels
    of a downstream one.  A Conv stores [out, in / groups, k...], a Gemm [out, in] (``transB``) or [in, out], a MatMul [in, out]."""
    if op.type in _LINEAR_TYPES: return int((_trans_b(op) != 0) == downstream)
    return int(downstream)


def endpoint_layout(op, downstream: bool, reference_key_order: bool = True) -> tuple:
    """How the kernels address the weight of one endpoint of a pair: (weight variable, channel axis, the pair's channel count
    as this weight tells it, key segment, apply geometry) with the segment (div, a, b, outer, stride, run) of
    ``ppqhip_equalize_segment`` -- the elements the key of channel c is taken over -- and (run, inner, group_out) of
    ``ppqhip_equalize_apply_job`` -- the scale every element takes.  The scale of a grouped downstream Conv is applied in the
    natural (group, cin_local) order; ``reference_key_order`` lists its KEY rows in the reference's (cin_local, group) order
    (what equalization and the channel split reproduce; SSD reads the natural order)."""
    var = op.inputs[1]
    w = var.value
    if downstream and op.type not in _LINEAR_TYPES:                                # [G * og, ipg, k...]: channel g * ipg + i reads
        G = int(op.attributes.get('group', 1))                                     # w[g * og : (g + 1) * og, i]
        og, ipg, K = w.shape[0] // G, w.shape[1], w.numel() // (w.shape[0] * w.shape[1])
        # the reference's key row of that channel is r = i * G + g, the natural one r = g * ipg + i
        segment = (G, K, og * ipg * K, og, ipg * K, K) if reference_key_order else (ipg, og * ipg * K, K, og, ipg * K, K)
        return var, 1, G * ipg, segment, (K, ipg, og)
    if channel_axis(op, downstream) == 1:                                          # [rows, C]: channel c is column c
        rows, C = w.shape
        return var, 1, C, (1, 1, 0, rows, C, 1), (1, C, 0)
    C = w.shape[0]                                                                 # [C, ...]: channel c is row c
    epc = w.numel() // C
    return var, 0, C, (1, epc, 0, 1, 0, epc), (epc, C, 0)


def parameters_on_device(params: list, use_kernels: bool, who: str) -> bool:
    """The kernel arm runs when it is wanted and every parameter is on the GPU; CPU parameters take the torch arm; a mixture is
    refused."""
    cuda = [isinstance(t, torch.Tensor) and t.is_cuda for t in params]
    if not use_kernels or not any(cuda): return False
    if not all(cuda): raise TypeError(f'{who}: the parameters of the pairs are partly on the GPU and partly not')
    return True


def pair_jobs(pair: EqualizationPair, scale: torch.Tensor, value_threshold: float, including_bias: bool, including_act: bool,
              bias_multiplier: float, act_multiplier: float, activations: Dict[str, torch.Tensor], num_channel: int = None):
    """(scale item, apply items) of one pair for ``ffi.equalize_scale_table`` / ``ffi.equalize_apply_table``.  ``num_channel``:
    the pair's channel count where no ``scale`` is there to tell it (channel_split.py wants the key segments alone)."""
    C = scale.numel() if num_channel is None else int(num_channel)
    segments, applies = [], []

    def need(count, op):
        if count != C: raise ValueError(f'LayerwiseEqualizationPass: {op.name} has {count} channels, its pair has {C}')

    for op in pair.upstream_layers:
        _check_endpoint(op)
        w = _weight(op)
        _, _, count, segment, apply = endpoint_layout(op, False)
        need(count, op)
        segments.append((w, *segment, 1.0, False))
        applies.append((w, scale, *apply, False))
        if _has_bias(op):
            if not op.inputs[-1].is_parameter: raise ValueError(f'Bias of Op {op.name} is non-static.')
            b = op.inputs[-1].value
            need(b.numel(), op)
            if including_bias: segments.append((b, 1, 1, 0, 1, 0, 1, bias_multiplier, False))
            applies.append((b, scale, 1, C, 0, False))
        act = activations.get(op.outputs[0].name) if including_act else None
        if act is not None:
            need(act.numel(), op)
            segments.append((act, 1, 1, 0, 1, 0, 1, act_multiplier, False))
    for op in pair.downstream_layers:
        _check_endpoint(op)
        w = _weight(op)
        if op.type in _LINEAR_TYPES:
            if w.ndim != 2: raise ValueError(f'Unexpected Error, Parameter of MatMul {op.name} should be 2-d.')
        elif w.ndim not in (3, 4, 5): raise ValueError(f'Unexpected dimension of weight of {op.name}.')
        _, _, count, segment, apply = endpoint_layout(op, True)
        need(count, op)
        segments.append((w, *segment, 1.0, True))
        applies.append((w, scale, *apply, True))
    return (scale, value_threshold, segments), applies


class LayerwiseEqualizationPass(QuantizationOptimizationPass):
    """optim/equalization.py:214-575.  The first eleven arguments are the reference's (names, order, defaults);
    ``including_weight`` and ``weight_multiplier`` are stored and -- as there -- never reach the key computation.

    ``use_kernels``: float32 CUDA parameters are equalized by the two HIP kernels, a LEVEL of independent pair instances per
    pair of launches (``schedule='levelled'``; ``'sequential'`` issues the reference's order one instance at a time and exists
    for the tests).  CPU parameters, and everything when ``use_kernels`` is off, take the torch arm over the same schedule.

    ``stats``: ``pairs``, ``levels``, ``launches`` (entry-point calls: two per level, a level of more than 32 pairs or 72
    segments is chunked inside the library), ``channels``, and -- counted on the device over the LAST iteration's scales, one copy
    at the end -- ``scaled_channels`` (s != 1) and ``clipped_channels`` (s at 0.1 or 10).  ``keep_scales = True`` keeps a copy of
    every scale in ``scales[(iteration, pair index)]`` (an inspection aid: one device copy per pair instance)."""
    PASS_NAME = 'PPQ Layerwise Equalization Pass'

    def __init__(self, iterations: int, value_threshold: float = 0.5, including_weight: bool = True,
                 weight_multiplier: float = 1.0, including_bias: bool = False, including_act: bool = False,
                 bias_multiplier: float = 0.5, act_multiplier: float = 0.5, interested_layers: List[str] = None,
                 optimize_level: int = 2, verbose: bool = False, use_kernels: bool = True, schedule: str = 'levelled') -> None:
        if schedule not in {'levelled', 'sequential'}: raise ValueError(f'schedule is levelled or sequential, {schedule} was given.')
        self.optimize_level = optimize_level
        self.iterations = iterations
        self.value_threshold = value_threshold
        self.including_weight = including_weight
        self.weight_multiplier = weight_multiplier
        self.including_bias = including_bias
        self.bias_multiplier = bias_multiplier
        self.including_act = including_act
        self.act_multiplier = act_multiplier
        self.interested_layers = interested_layers
        self.verbose = verbose
        self.use_kernels = use_kernels
        self.schedule = schedule
        self.keep_scales = False
        self.scales: Dict[tuple, torch.Tensor] = {}
        self.pairs: List[EqualizationPair] = []
        self.activations: Dict[str, torch.Tensor] = {}      # {output variable name: per-channel |max|}, owned by the pass
        self.stats: Dict[str, int] = {}
        super().__init__(name=self.PASS_NAME)

    def find_equalization_pair(self, graph, interested_operations: list) -> List[EqualizationPair]:
        return find_equalization_pair(graph, interested_operations, self.optimize_level)

    # ---- activations ------------------------------------------------------------------------------
    @ staticmethod
    def aggregate(op, tensor: torch.Tensor) -> torch.Tensor:
        """optim/equalization.py:493-502: per-channel max |x| of one output."""
        if op.type in {'Conv', 'ConvTranspose'}:
            tensor = tensor.transpose(0, 1).reshape(shape=[tensor.shape[1], -1])
            tensor = torch.max(tensor.abs(), dim=-1, keepdim=False)[0]
        elif op.type in {'MatMul', 'Gemm'}:
            tensor = torch.max(tensor.transpose(0, 1).abs(), dim=-1, keepdim=False)[0]
        return tensor

    def collect_activations(self, graph, executor, dataloader: Iterable, collate_fn: Callable, operations: list,
                            steps: int = COLLECT_STEPS, on_device: bool = True) -> Dict[str, torch.Tensor]:
        """optim/equalization.py:488-526: {output variable name: per-channel max |x|} over the first batches of the dataloader
        (the loop leaves at ``idx > steps``, so up to ``steps + 2`` batches are visited).  On the device every collected forward
        is ONE per-channel min/max launch for all observed outputs (``ppqhip_minmax_c_multi``, accumulating) and max(|min|,
        |max|) -- exactly max |x| -- is folded once at the end; the torch arm aggregates output by output as the reference
        does.  The maxima stay with the pass: nothing is written into ``graph.variables``."""
        names = []
        for op in operations:
            assert len(op.outputs) == 1, f'Num of output of layer {op.name} is supposed to be 1'
            names.append(op.outputs[0].name)
        if not names: return {}
        lo = hi = sizes = None
        collected: Dict[str, list] = {n: [] for n in names}
        for idx, batch in enumerate(dataloader):
            data = collate_fn(batch) if collate_fn is not None else batch
            outputs = executor.forward(data, output_names=names)
            if on_device:
                from .ffi import CUDA
                if lo is None:
                    sizes = [int(y.shape[1]) for y in outputs]
                    lo = torch.full((sum(sizes),), float('inf'), dtype=torch.float32, device=outputs[0].device)
                    hi = -lo
                CUDA.MinMax_C_Multi(list(outputs), [1] * len(outputs), list(torch.split(lo, sizes)), list(torch.split(hi, sizes)))
                self.stats['collect_launches'] = self.stats.get('collect_launches', 0) + 1
            else:
                for name, op, y in zip(names, operations, outputs): collected[name].append(self.aggregate(op, y).unsqueeze(-1))
            if idx > steps: break
        if on_device:
            if lo is None: return {}
            return dict(zip(names, torch.split(torch.maximum(lo.abs(), hi.abs()), sizes)))
        return {n: torch.cat(v, dim=-1).amax(dim=-1) for n, v in collected.items() if v}

    # ---- the pass ---------------------------------------------------------------------------------
    def interested_operations(self, graph) -> list:
        if self.interested_layers is None:
            return [op for op in graph.operations.values() if op.type in EQUALIZATION_OPERATION_TYPE]
        return [graph.operations[name] for name in self.interested_layers if name in graph.operations]

    def optimize(self, graph, dataloader: Iterable = None, executor=None, collate_fn: Callable = None,
                 activations: Dict[str, torch.Tensor] = None, **kwargs) -> None:
        """``activations`` (not in the reference): per-channel maxima to use instead of collecting them, {output variable
        name: [channels]}."""
        interested = self.interested_operations(graph)
        pairs = self.pairs = self.find_equalization_pair(graph=graph, interested_operations=interested)
        for pair in pairs:
            for op in pair.operations: _check_endpoint(op)
        params = [v.value for pair in pairs for op in pair.operations for v in op.inputs[1:] if v.is_parameter]
        on_device = parameters_on_device(params, self.use_kernels, 'LayerwiseEqualizationPass')
        self.stats = dict(pairs=len(pairs), levels=0, launches=0, channels=0, scaled_channels=0, clipped_channels=0)
        self.scales = {}

        if self.including_act:
            if activations is None:
                activations = self.collect_activations(graph, executor, dataloader, collate_fn, interested, on_device=on_device)
            self.activations = {n: a.detach().reshape(-1).contiguous() for n, a in activations.items()}
        else: self.activations = {}

        if self.verbose: print(f'{len(pairs)} equalization pair(s) was found, ready to run optimization.')
        levels = build_schedule(pairs, self.iterations, self.schedule)
        self.stats['levels'] = len(levels)
        self.stats['channels'] = sum(pair.num_channel() for pair in pairs)
        with torch.no_grad():
            last = self._run_kernels(pairs, levels) if on_device else self._run_torch(pairs, levels)
        if last:
            s = torch.cat([t.reshape(-1) for t in last])
            clipped = ((s == s.new_tensor(0.1)) | (s == 10)) & (s != 1)
            counts = torch.stack([(s != 1).sum(), clipped.sum()]).tolist()         # the one copy
            self.stats['scaled_channels'], self.stats['clipped_channels'] = int(counts[0]), int(counts[1])

        # equalization changes the fp32 value of the weights: store it for the procedures that follow (:570-574)
        for op in graph.operations.values():
            if hasattr(op, 'store_parameter_value'): op.store_parameter_value()

    def _run_torch(self, pairs, levels) -> List[torch.Tensor]:
        acts = {n: a.unsqueeze(-1) for n, a in self.activations.items()}
        last: Dict[int, torch.Tensor] = {}
        for level in levels:
            for it, p in level:
                s = pairs[p].equalize(value_threshold=self.value_threshold, including_weight=self.including_weight,
                                      weight_multiplier=self.weight_multiplier, including_bias=self.including_bias,
                                      including_act=self.including_act, bias_multiplier=self.bias_multiplier,
                                      act_multiplier=self.act_multiplier, activations=acts)
                last[p] = s
                if self.keep_scales: self.scales[(it, p)] = s.detach().clone()
        return [last[p] for p in sorted(last)]

    def _run_kernels(self, pairs, levels) -> List[torch.Tensor]:
        from . import ffi
        if not pairs or not levels: return []
        device = pairs[0].upstream_layers[0].inputs[1].value.device
        sizes = [pair.num_channel() for pair in pairs]
        buffers = list(torch.split(torch.empty(sum(sizes), dtype=torch.float32, device=device), sizes))
        jobs = [pair_jobs(pair, buffers[p], self.value_threshold, self.including_bias, self.including_act, self.bias_multiplier,
                          self.act_multiplier, self.activations) for p, pair in enumerate(pairs)]
        tables = {}                                         # a level's tables depend on its set of pairs alone
        for level in levels:
            key = tuple(p for _, p in level)
            if key not in tables:
                tables[key] = (ffi.equalize_scale_table([jobs[p][0] for p in key]),
                               ffi.equalize_apply_table([item for p in key for item in jobs[p][1]]))
            scale_table, apply_table = tables[key]
            ffi.equalize_scale_multi(scale_table)
            ffi.equalize_apply_multi(apply_table)
            self.stats['launches'] += 2
            if self.keep_scales:
                for it, p in level: self.scales[(it, p)] = buffers[p].clone()
        return buffers
