"""SSD equalization -- the reference's loss-checked pre-quantisation pass (``SSDEqualizationPass``).

Mirror of ppq/quantization/optim/ssd.py:30-573.  Per pair (Conv / Gemm -> relay operations -> Conv / Gemm) and iteration the
reference tries four scales -- the DFQ one and three activation-aware ones (``one_step_equalization``, :288-320) -- measures
the quantization loss of the pair for each (``test_ssd_loss``, :431-472: a min/max calibration, a histogram calibration and a
loss pass over the pair) and keeps a candidate only if its loss is below ``loss_threshold`` x the loss before.  Every one of
those sixteen passes per calibration batch re-runs the graph from its input to the pair, although nothing upstream changes.

``use_kernels=False`` is the torch arm: that sequence with this package's primitives, one ``executor.forward`` wherever the
reference has one.  ``use_kernels=True`` does the same work with

* ONE prefix forward per distinct batch per (iteration, pair): the pair's inputs stay on the device and serve the range
  collection and all five evaluations; the unquantised run of the pair made by the min/max phase is the FP32 target of the
  loss phase (nothing of the pair is quantised in either -- the same launches on the same bits);
* three launches (csrc/ssd.hip): the four scales of the pair, all four candidate parameter sets out of place (recovering the
  originals costs nothing) and the loss read with the last fake-quant done in registers.

What is reproduced as it is and what is not followed is listed in INTEGRATION.md section 8."""
from math import ceil
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch
import torch.nn.functional as F

from .calibration import QuantizationOptimizationPass
from .core import QuantizationProperty as P
from .core import QuantizationStates, rounding_value, state_value
from .equalization import _check_endpoint, _trans_b, endpoint_layout, parameters_on_device
from .qfunction import PPQLinearQuantFunction

OPTIMIZATION_LAYERTYPE_CONFIG = {                                       # optim/ssd.py:24-26
    1: {'Relu', 'MaxPool', 'GlobalMaxPool', 'PRelu', 'AveragePool', 'GlobalAveragePool'},
}
EQUALIZATION_OPERATION_TYPE = {'Conv', 'Gemm', 'ConvTranspose'}         # optim/ssd.py:27
MAX_LOSS_IMAGES = 200                                                   # optim/ssd.py:528


def _quantable(op) -> bool:
    return hasattr(op, 'config')


def _downstream(op) -> list:
    return [d for v in op.outputs for d in v.dest_ops]


def _activated(config) -> bool:
    return state_value(config.state) in (QuantizationStates.ACTIVATED.value, QuantizationStates.PASSIVE.value)


def clamp_calib_steps(calib_steps: int, dataloader: Iterable, collate_fn: Callable = None) -> int:
    """optim/ssd.py:509-528: at most ceil(200 / batchsize) steps; the batch size is read from the first batch -- a tensor, the
    first tensor of a list / tuple, the first tensor value of a dict (1 when there is none)."""
    batchsize = 1
    for data in dataloader:
        if collate_fn is not None: data = collate_fn(data)
        if isinstance(data, torch.Tensor): batchsize = data.shape[0]
        elif isinstance(data, (list, tuple)):
            for value in data:
                if isinstance(value, torch.Tensor):
                    batchsize = value.shape[0]
                    break
        elif isinstance(data, dict):
            for value in data.values():
                if isinstance(value, torch.Tensor):
                    batchsize = value.shape[0]
                    break
        break
    return min(calib_steps, ceil(MAX_LOSS_IMAGES / batchsize))


def lift_activation_range(op_range: torch.Tensor, channel_ratio: float) -> torch.Tensor:
    """optim/ssd.py:133-137: every channel below ``channel_ratio`` x the largest one is lifted to it."""
    op_range_max = op_range.max()
    return torch.where(op_range < op_range_max * channel_ratio, op_range_max * channel_ratio, op_range)


def calculate_scale(first_weight_range: torch.Tensor, last_weight_range: torch.Tensor, act_range: Optional[torch.Tensor],
                    algo_type: int, channel_ratio: float, ssd_min_scale: float = 8, ssd_max_scale: float = 2,
                    dfq_min_scale: float = 0.1, dfq_max_scale: float = 10, eps: float = 1e-8) -> torch.Tensor:
    """The scale of optim/ssd.py:290-320, operation for operation."""
    if algo_type == 0:
        scale = torch.sqrt(last_weight_range / (first_weight_range + eps))
        return torch.clamp(scale, dfq_min_scale, dfq_max_scale)
    first_weight_range = torch.where(first_weight_range < first_weight_range.max() * channel_ratio,
                                     first_weight_range.max() * channel_ratio, first_weight_range)
    last_weight_range = torch.where(last_weight_range < last_weight_range.max() * channel_ratio,
                                    last_weight_range.max() * channel_ratio, last_weight_range)
    kernel_scale = first_weight_range.max() / (first_weight_range + eps)
    next_kernel_scale = last_weight_range.max() / (last_weight_range + eps)
    act_range = torch.where(act_range < 0.01, torch.tensor(0.01, device=act_range.device, dtype=torch.float32), act_range)
    act_scale = act_range.max() / (act_range + eps)
    if algo_type == 1: return torch.min(kernel_scale, act_scale)
    if algo_type == 2:
        kernel_scale = kernel_scale / next_kernel_scale
        act_scale = act_scale / next_kernel_scale
        scale = torch.min(kernel_scale, act_scale)
        scale = torch.min(scale, torch.tensor(ssd_min_scale, dtype=torch.float32, device=scale.device))
        scale = scale / scale.min()
        return torch.clamp(scale, 1.0, ssd_max_scale)
    kernel_scale = (kernel_scale / next_kernel_scale).sqrt()
    scale = (act_scale * kernel_scale).sqrt()
    return torch.clamp(scale, 1.0, ssd_max_scale)


def pair_geometry(pair: list):
    """The pair's tensors as the kernels address them: (C, first segment, last segment, apply items) with an apply item
    (variable, run, inner, group_out, divide) per tensor; segments are (tensor, div, a, b, outer, stride, run) of
    ``ppqhip_equalize_segment``.  None for a Gemm behind a flattened Conv (the reshape branches of :190-204 / :245-259), which
    the torch arm's expressions handle."""
    first, last = pair[0], pair[-1]
    w1, _, C, seg1, apply1 = endpoint_layout(first, False)
    w2, _, count, seg2, apply2 = endpoint_layout(last, True, reference_key_order=False)
    applies = [(w1, *apply1, False)]
    if len(first.parameters) > 1: applies.append((first.parameters[1], 1, C, 0, False))
    if count != C:
        if last.type == 'Gemm': return None
        raise ValueError(f'SSDEqualizationPass: {last.name} has {count} input channels, its pair has {C}')
    applies.append((w2, *apply2, True))
    return C, (w1.value, *seg1), (w2.value, *seg2), applies


class SSDEqualizationPass(QuantizationOptimizationPass):
    """optim/ssd.py:30-573.  The first six arguments are the reference's (names, order, defaults).

    ``use_kernels``: float32 contiguous CUDA parameters take the kernel arm (see the module docstring); CPU parameters, and
    everything when ``use_kernels`` is off, take the torch arm.  Both arms compute the same bits on the device as long as the
    graph's forward is reproducible from one run to the next.

    ``stats``: ``pairs``, ``accepted`` ({algo index: count}, -1 = nothing accepted), ``prefix_forwards`` (``executor.forward``
    calls), ``pair_forwards`` (runs of a pair), ``launches`` (calls of the loss-read, scale and apply entry points of the
    library made by the pass itself).  ``history[(iteration, pair index)] = {basic, losses[4], best_idx}``.  ``verbose`` prints
    what the reference logs."""
    def __init__(self, optimize_level: int = 1, channel_ratio: float = 0.5, loss_threshold: float = 0.8, layer_norm: bool = False,
                 quant_func: Callable = PPQLinearQuantFunction, iteration: int = 3, use_kernels: bool = True,
                 verbose: bool = False):
        self.channel_ratio = channel_ratio
        self.loss_threshold = loss_threshold
        self.layer_norm = layer_norm
        self.quant_func = quant_func
        self.start_op_types = EQUALIZATION_OPERATION_TYPE
        self.relay_op_types = OPTIMIZATION_LAYERTYPE_CONFIG[optimize_level]
        self.end_op_types = EQUALIZATION_OPERATION_TYPE
        self.iteration = iteration
        self.use_kernels = use_kernels
        self.verbose = verbose
        self.stats: Dict[str, object] = {}
        self.history: Dict[tuple, dict] = {}
        self.pairs: List[list] = []
        self._graph = None
        self._cache: Optional[dict] = None          # kernel arm: what one prefix forward per batch left for this (iteration, pair)
        super().__init__(name='SSD Equalization Pass')

    # ---- pairs ------------------------------------------------------------------------------------
    def collect_all_pairs(self, graph) -> List[list]:
        """optim/ssd.py:77-90 over the search of ppq/IR/search.py:428-458, 546-556: from every start operation in graph
        order, depth first through the relay types to the first Conv / Gemm / ConvTranspose; a path is kept when every
        operation on it but the last has exactly one downstream operation."""
        memo: Dict[str, list] = {}

        def paths_from(start) -> list:
            if start.name in memo: return memo[start.name]
            found = []
            for op in _downstream(start):
                if op.type in self.end_op_types: found.append([start, op])
                elif op.type in self.relay_op_types: found.extend([start] + path for path in paths_from(op))
            memo[start.name] = found
            return found

        pairs = []
        for op in graph.operations.values():
            if op.type in self.start_op_types: pairs.extend(paths_from(op))
        return [path for path in pairs if all(len(_downstream(op)) == 1 for op in path[:-1])]

    # ---- batches ----------------------------------------------------------------------------------
    @ staticmethod
    def _calib_batches(data_loader: Iterable, collate_fn: Callable, calib_steps: int):
        """(position in the loader, batch) as the calibration loops of :115-129 / :342-351 visit them."""
        calib_step = 0
        for _ in range(ceil(calib_steps / len(data_loader))):
            for index, data in enumerate(data_loader):
                yield index, (collate_fn(data) if collate_fn is not None else data)
                calib_step += 1
                if calib_step >= calib_steps: break

    @ staticmethod
    def _loss_batches(data_loader: Iterable, collate_fn: Callable, calib_steps: int):
        """The loss loop of :458-471 has no ``break``: every batch of the loader, ceil(calib_steps / len) times."""
        for _ in range(ceil(calib_steps / len(data_loader))):
            for index, data in enumerate(data_loader):
                yield index, (collate_fn(data) if collate_fn is not None else data)

    def _graph_input(self, name: str, data, like: torch.Tensor) -> torch.Tensor:
        """The value of graph input ``name`` in a batch (the harness's executor hands back nothing for an input)."""
        names = list(self._graph.inputs) if self._graph is not None else [name]
        if isinstance(data, dict): value = data[name]
        elif isinstance(data, (list, tuple)): value = data[names.index(name)]
        else: value = data
        return value.to(like.device)

    def _forward(self, executor, data, names: List[str], like: torch.Tensor) -> List[torch.Tensor]:
        outs = executor.forward(data, output_names=names)
        self.stats['prefix_forwards'] = self.stats.get('prefix_forwards', 0) + 1
        return [self._graph_input(n, data, like) if o is None else o for n, o in zip(names, outs)]

    def _pair_inputs(self, pair: list, executor, index: int, data) -> List[torch.Tensor]:
        """The input of the pair's first operation for one batch: the kept tensor in the kernel arm, else one forward."""
        if self._cache is not None: return [self._cache['inputs'][index]]
        return self._forward(executor, data, [pair[0].inputs[0].name], pair[0].parameters[0].value)

    def _fill_cache(self, pair: list, executor, data_loader: Iterable, collate_fn: Callable, calib_steps: int) -> None:
        """Kernel arm: ONE forward per distinct batch gives the pair's input and -- for the first ``calib_steps`` visits -- the
        per-channel max(relu(y)) of its first output (one per-channel min/max launch)."""
        from .ffi import CUDA
        names = [pair[0].inputs[0].name, pair[0].outputs[0].name]
        like = pair[0].parameters[0].value
        inputs, ranges, total = {}, {}, None
        visits = [index for index, _ in self._calib_batches(_Indices(len(data_loader)), None, calib_steps)]
        for index, data in enumerate(data_loader):
            if collate_fn is not None: data = collate_fn(data)
            x, y = self._forward(executor, data, names, like)
            inputs[index] = x
            if index in visits:
                lo = torch.full((y.shape[1],), float('inf'), dtype=torch.float32, device=y.device)
                hi = -lo
                CUDA.MinMax_C_Multi([y], [1], [lo], [hi])
                self.stats['launches'] += 1
                ranges[index] = F.relu(hi)
        for index in visits:                                               # the order (and the repeats) of the reference's sum
            total = ranges[index] if total is None else total + ranges[index]
        self._cache = dict(inputs=inputs, act_sum=total, fp={})

    # ---- ranges -----------------------------------------------------------------------------------
    def collect_activation_range(self, pair: list, executor, data_loader: Iterable, collate_fn: Callable,
                                 calib_steps: int) -> Dict[object, torch.Tensor]:
        """optim/ssd.py:92-138 for the pair's FIRST operation (the reference collects the last one's too and never reads it):
        the mean over ``calib_steps`` batches of the per-channel max(relu(y)), lifted to ``channel_ratio`` x its maximum."""
        op = pair[0]
        if self._cache is not None: total = self._cache['act_sum']
        else:
            total = 0.0
            for _, data in self._calib_batches(data_loader, collate_fn, calib_steps):
                y = self._forward(executor, data, [op.outputs[0].name], op.parameters[0].value)[0]
                y = F.relu(y)
                y = y.permute(1, 0, *(range(y.ndim)[2:])).contiguous()
                total = total + y.reshape((y.shape[0], -1)).max(1)[0]
        return {op: lift_activation_range(total / calib_steps, self.channel_ratio)}

    def layer_weight_norm(self, pairs: List[list]) -> None:
        """optim/ssd.py:140-150."""
        for pair in pairs:
            first, last = pair[0].parameters[0], pair[-1].parameters[0]
            scale = (last.value.abs().max() / first.value.abs().max()).sqrt()
            first.value = first.value * scale
            if len(pair[0].parameters) > 1: pair[0].parameters[1].value = pair[0].parameters[1].value * scale
            last.value = last.value / scale

    def prepare_weight_for_equalization(self, pair: list) -> Tuple[torch.Tensor, torch.Tensor]:
        """optim/ssd.py:152-210: max |w| per output channel of the first weight and per input channel of the last one -- for a
        grouped Conv in the natural (group, cin_local) order."""
        _check_endpoint(pair[0]); _check_endpoint(pair[-1])
        w1, w2 = pair[0].parameters[0].value, pair[-1].parameters[0].value
        if pair[0].type == 'Conv': first_weight_range = w1.reshape(w1.shape[0], -1).abs().max(dim=1)[0]
        elif _trans_b(pair[0]): first_weight_range = w1.abs().max(dim=1)[0]                      # [C_out, C_in]
        else: first_weight_range = w1.abs().max(dim=0)[0]                                        # [C_in, C_out]
        if pair[-1].type == 'Conv':
            G = pair[-1].attributes.get('group', 1)
            v = w2.reshape(G, w2.shape[0] // G, w2.shape[1], -1).permute(0, 2, 1, 3).contiguous()
            last_weight_range = v.reshape(G * w2.shape[1], -1).abs().max(dim=1)[0]
        else:
            C_out = first_weight_range.shape[0]
            if _trans_b(pair[-1]):
                if C_out != w2.shape[1]:                                                         # behind a flattened Conv
                    v = w2.reshape(w2.shape[0], C_out, -1).permute(1, 0, 2).contiguous().reshape(C_out, -1)
                    last_weight_range = v.abs().max(dim=1)[0]
                else: last_weight_range = w2.abs().max(dim=0)[0]
            else:
                if C_out != w2.shape[0]: last_weight_range = w2.reshape(C_out, -1).abs().max(dim=1)[0]
                else: last_weight_range = w2.abs().max(dim=1)[0]
        return first_weight_range, last_weight_range

    def write_back(self, pair: list, scale: torch.Tensor) -> None:
        """optim/ssd.py:212-262: new tensors, the old ones are not written."""
        _check_endpoint(pair[0]); _check_endpoint(pair[-1])
        first, last = pair[0].parameters[0], pair[-1].parameters[0]
        w1, w2 = first.value, last.value
        if pair[0].type == 'Conv': first.value = w1 * scale.reshape([-1] + [1] * (w1.ndim - 1))
        elif _trans_b(pair[0]): first.value = w1 * scale.reshape(-1, 1)
        else: first.value = w1 * scale.reshape(1, -1)
        if len(pair[0].parameters) > 1: pair[0].parameters[1].value = pair[0].parameters[1].value * scale
        if pair[-1].type == 'Conv':
            G = pair[-1].attributes.get('group', 1)
            v = w2.reshape((G, w2.shape[0] // G) + tuple(w2.shape[1:]))
            v = v / scale.reshape([G, 1, -1] + [1] * (w2.ndim - 2))
            last.value = v.reshape(w2.shape)
        elif _trans_b(pair[-1]):
            if scale.numel() != w2.shape[1]:
                v = w2.reshape(w2.shape[0], scale.numel(), -1) / scale.reshape(1, -1, 1)
                last.value = v.reshape(w2.shape[0], -1)
            else: last.value = w2 / scale.reshape(1, -1)
        else:
            if scale.numel() != w2.shape[0]:
                v = w2.reshape(scale.numel(), -1, w2.shape[-1]) / scale.reshape(-1, 1, 1)
                last.value = v.reshape(-1, w2.shape[-1])
            else: last.value = w2 / scale.reshape(-1, 1)

    def one_step_equalization(self, pair: list, op_act_channel_range: Dict[object, torch.Tensor] = {}, algo_type: int = 2,
                              ssd_min_scale: float = 8, ssd_max_scale: float = 2, dfq_min_scale: float = 0.1,
                              dfq_max_scale: float = 10, eps: float = 1e-8) -> torch.Tensor:
        """optim/ssd.py:264-322 with torch operations: algo 0 is the DFQ scale, 1-3 the activation-aware ones.  Returns the
        scale it wrote back."""
        first_weight_range, last_weight_range = self.prepare_weight_for_equalization(pair)
        scale = calculate_scale(first_weight_range, last_weight_range, op_act_channel_range.get(pair[0]) if algo_type else None,
                                algo_type, self.channel_ratio, ssd_min_scale, ssd_max_scale, dfq_min_scale, dfq_max_scale, eps)
        self.write_back(pair, scale)
        return scale

    def candidates(self, pair: list, act_range: torch.Tensor) -> Optional[dict]:
        """Kernel arm: the four scales (one call) and the four candidate parameter sets (one launch), out of place.  Returns
        {scales [4, C], ranges [2, C], params: {variable: [4, *shape]}}; None when the torch arm has to take the pair."""
        from . import ffi
        _check_endpoint(pair[0]); _check_endpoint(pair[-1])
        geometry = pair_geometry(pair)
        if geometry is None: return None
        C, seg1, seg2, applies = geometry
        dev = seg1[0].device
        scales = torch.empty((4, C), dtype=torch.float32, device=dev)
        ranges = torch.empty((2, C), dtype=torch.float32, device=dev)
        ffi.ssd_scales_multi([(seg1, seg2, act_range.contiguous(), self.channel_ratio, scales, ranges)])
        outs = {var: torch.empty((4,) + tuple(var.value.shape), dtype=torch.float32, device=dev) for var, *_ in applies}
        ffi.ssd_apply_multi([(var.value, outs[var], scales, run, inner, og, divide) for var, run, inner, og, divide in applies])
        self.stats['launches'] += 2
        return dict(scales=scales, ranges=ranges, params=outs)

    # ---- loss -------------------------------------------------------------------------------------
    def build_observer_pair(self, pair: list) -> dict:
        from .observer import OperationObserver
        return {op: OperationObserver(operation=op) for op in pair if _quantable(op)}

    def run_pair(self, pair: list, inputs: List[torch.Tensor], hooks: dict = {}, defer_last: bool = False):
        """optim/ssd.py:392-421.  ``defer_last``: hand back the last operation's outputs BEFORE their fake-quant, with their
        configs (the kernel arm's loss read quantises them in registers)."""
        from .harness import _forward
        self.stats['pair_forwards'] = self.stats.get('pair_forwards', 0) + 1
        for op in pair:
            inputs = inputs + [param.value for param in op.parameters]
            if _quantable(op):
                input_configs = list(op.config.input_quantization_config)
                assert len(inputs) == len(input_configs)
                inputs_quant = [self.quant_func(value, config) for value, config in zip(inputs, input_configs)]
                hook = hooks.get(op, None)
                if hook is not None: hook.pre_forward_hook(inputs, inputs_quant, input_configs)
            else: inputs_quant = inputs
            outputs = _forward(op, inputs_quant)
            outputs = list(outputs) if isinstance(outputs, (list, tuple)) else [outputs]
            if _quantable(op):
                output_configs = list(op.config.output_quantization_config)
                if defer_last and op is pair[-1]: return outputs, output_configs
                outputs_quant = [self.quant_func(value, config) for value, config in zip(outputs, output_configs)]
                hook = hooks.get(op, None)
                if hook is not None: hook.post_forward_hook(outputs, outputs_quant, output_configs)
                inputs = outputs_quant
            else: inputs = outputs
        return (inputs, [None] * len(inputs)) if defer_last else inputs

    def calibrate(self, pair: list, data_loader: Iterable, executor, hooks: dict, collate_fn: Callable, calib_steps: int,
                  keep_fp: bool = False) -> None:
        """optim/ssd.py:332-351.  ``keep_fp`` (kernel arm, nothing of the pair quantised yet): the outputs are the FP32 targets
        of the loss phase and are kept per batch."""
        for index, data in self._calib_batches(data_loader, collate_fn, calib_steps):
            outputs = self.run_pair(pair, self._pair_inputs(pair, executor, index, data), hooks)
            if keep_fp: self._cache['fp'][index] = outputs

    def calibration_passive_param(self, pair: list, scale_multiplier: float = 1.0) -> None:
        """optim/ssd.py:353-371: a PASSIVE_INIT bias takes weight scale x input scale."""
        for op in pair:
            if not _quantable(op): continue
            if op.type in {'Conv', 'ConvTranspose', 'Gemm'} and len(op.inputs) == 3:
                input_config, weight_config, bias_config = op.config.input_quantization_config
                if state_value(bias_config.state) != QuantizationStates.PASSIVE_INIT.value: continue
                bias_config.scale = weight_config.dominated_by.scale * input_config.dominated_by.scale * scale_multiplier
                bias_config.state = QuantizationStates.PASSIVE
                bias_config.offset = torch.zeros_like(bias_config.scale, dtype=torch.float)
                assert not bias_config.policy.has_property(P.ASYMMETRICAL), (
                    'Negative parameter does not support ASYMMETRICAL quantization')

    def initiate_pair_state(self, pair: list) -> None:
        """optim/ssd.py:373-380."""
        for op in pair:
            if not _quantable(op): continue
            for config in op.config.input_quantization_config + op.config.output_quantization_config:
                if state_value(config.state) == QuantizationStates.ACTIVATED.value: config.state = QuantizationStates.INITIAL
                elif state_value(config.state) == QuantizationStates.PASSIVE.value: config.state = QuantizationStates.PASSIVE_INIT

    def dequantize_pair(self, pair: list) -> None:
        for op in pair:
            if _quantable(op): op.dequantize()

    def restore_quantize_state(self, pair: list) -> None:
        for op in pair:
            if _quantable(op): op.restore_quantize_state()

    def calculate_mse(self, fp_res: List[torch.Tensor], quant_res: List[torch.Tensor]) -> torch.Tensor:
        """optim/ssd.py:424-428."""
        from .measure import torch_mean_square_error
        if fp_res and fp_res[0].is_cuda: self.stats['launches'] += 2 * len(fp_res)
        return torch.stack([torch_mean_square_error(fp, q) for fp, q in zip(fp_res, quant_res)]).mean()

    def _fused_mse(self, fp_res: List[torch.Tensor], raw: List[torch.Tensor], configs: list) -> torch.Tensor:
        """``calculate_mse(fp_res, [quant_func(y, config)])`` with the fake-quant of an activated linear config done inside
        the loss read (``ppqhip_fq_measure_rows_multi``): the same bits, no quantised output written."""
        from . import ffi
        from .measure import kernel_path
        losses = []
        for fp, y, config in zip(fp_res, raw, configs):
            pol = getattr(config, 'policy', None)
            fusable = (config is not None and _activated(config) and pol.has_property(P.LINEAR) and not pol.has_property(P.DYNAMIC)
                       and kernel_path(fp, y) and fp.ndim >= 2
                       and (pol.has_property(P.PER_TENSOR) or (pol.has_property(P.PER_CHANNEL) and config.channel_axis % y.ndim == 1)))
            if not fusable:
                losses.append(self.calculate_mse([fp], [y if config is None else self.quant_func(y, config)]))
                continue
            axis = None if pol.has_property(P.PER_TENSOR) else 1
            scale = config.scale.reshape(-1).to(y.device).contiguous()
            offset = config.offset.reshape(-1).to(y.device).contiguous()
            sums = ffi.fq_measure_rows_multi([(y, fp, scale, offset, axis, config.quant_min, config.quant_max,
                                               rounding_value(config.rounding))])[0]
            rows = torch.empty(y.shape[0], dtype=torch.float32, device=y.device)
            ffi.measure_finish_multi([(sums, y.numel() // y.shape[0], None, rows)], 'mse')
            self.stats['launches'] += 2
            losses.append(torch.mean(rows))
        return torch.stack(losses).mean()

    @ torch.no_grad()
    def test_ssd_loss(self, pair: list, executor, data_loader: Iterable, collate_fn: Callable, calib_steps: int) -> float:
        """optim/ssd.py:431-472: calibrate the INITIAL configs of the pair (min/max pass, then a histogram pass for the
        operations that have a histogram observer), derive the passive bias scales, then the mean over every batch of the
        loader of the MSE between the pair run dequantized and restored."""
        from .observer import TorchHistObserver, render_observers
        observers = self.build_observer_pair(pair)
        hooks = {op: observers[op].hook for op in observers}
        # kernel arm: while nothing of the pair is quantised the calibration run IS the dequantized run of the loss phase
        share = self._cache is not None and not any(_activated(c) for op in pair if _quantable(op)
                                                    for c in op.config.input_quantization_config + op.config.output_quantization_config)
        if self._cache is not None: self._cache['fp'] = {}
        self.calibrate(pair, data_loader, executor, hooks, collate_fn, calib_steps, keep_fp=share)
        render_observers([ob for observer in observers.values() for ob in observer.observers()])
        for op in [op for op, observer in observers.items() if all(type(ob) is not TorchHistObserver for ob in observer.observers())]:
            observers.pop(op); hooks.pop(op)
        if len(hooks) > 0:
            self.calibrate(pair, data_loader, executor, hooks, collate_fn, calib_steps)
            render_observers([ob for observer in observers.values() for ob in observer.observers()])
        self.calibration_passive_param(pair)
        loss = []
        for index, data in self._loss_batches(data_loader, collate_fn, calib_steps):
            inputs = self._pair_inputs(pair, executor, index, data)
            fp_output = self._cache['fp'].get(index) if share else None
            if fp_output is None:
                self.dequantize_pair(pair)
                fp_output = self.run_pair(pair, inputs)
                self.restore_quantize_state(pair)
                if share: self._cache['fp'][index] = fp_output
            if self._cache is not None:
                raw, configs = self.run_pair(pair, inputs, defer_last=True)
                loss.append(self._fused_mse(fp_output, raw, configs))
            else: loss.append(self.calculate_mse(fp_output, self.run_pair(pair, inputs)))
        if self._cache is not None: self._cache['fp'] = {}
        return torch.stack(loss).mean().item()

    # ---- parameters -------------------------------------------------------------------------------
    def collect_original_parameter(self, pair: list) -> Dict[object, torch.Tensor]:
        """optim/ssd.py:475-481.  Nothing here writes a parameter in place, so the kernel arm keeps the tensors themselves."""
        clone = self._cache is None
        return {var: (var.value.clone() if clone else var.value) for op in pair for var in op.inputs + op.outputs if var.is_parameter}

    def store_parameter(self, pair: list) -> None:
        for op in pair:
            if _quantable(op): op.store_parameter_value()

    def recover_original_parameter(self, pair: list, original_weights: Dict[object, torch.Tensor]) -> None:
        for op in pair:
            for var in op.inputs + op.outputs:
                if var.is_parameter: var.value = original_weights[var]
        self.store_parameter(pair)

    def _on_device(self, pairs: List[list]) -> bool:
        params = [var.value for pair in pairs for op in (pair[0], pair[-1]) for var in op.parameters]
        if not parameters_on_device(params, self.use_kernels, 'SSDEqualizationPass'): return False
        for pair in pairs:
            for op in (pair[0], pair[-1]):
                for var in op.parameters:
                    if var.value.dtype != torch.float32 or not var.value.is_contiguous():
                        raise TypeError(f'SSDEqualizationPass: {var.name} must be a contiguous float32 tensor for the kernels '
                                        '(use_kernels=False equalizes anything torch can)')
        return True

    # ---- the pass ---------------------------------------------------------------------------------
    def optimize(self, graph, dataloader: Iterable, executor, collate_fn: Callable = None, calib_steps: int = 32, **kwargs) -> None:
        """optim/ssd.py:500-573."""
        self._graph = graph
        calib_steps = clamp_calib_steps(calib_steps, dataloader, collate_fn)
        all_pairs = self.pairs = self.collect_all_pairs(graph)
        for pair in all_pairs: _check_endpoint(pair[0]); _check_endpoint(pair[-1])
        kernels = self._on_device(all_pairs)
        self.stats = dict(pairs=len(all_pairs), accepted={}, prefix_forwards=0, pair_forwards=0, launches=0, calib_steps=calib_steps)
        self.history = {}
        if self.layer_norm: self.layer_weight_norm(all_pairs)
        try:
            for i in range(self.iteration):
                if self.verbose: print(f'DFQ/SSD Equalization Iteration {i + 1}/{self.iteration}')
                for p, pair in enumerate(all_pairs):
                    if self.verbose: print(f"Now Processing Pair {p + 1}/{len(all_pairs)}: {'--'.join(op.name for op in pair)}")
                    self.store_parameter(pair)
                    self._cache = None
                    if kernels: self._fill_cache(pair, executor, dataloader, collate_fn, calib_steps)
                    op_act_range = self.collect_activation_range(pair, executor, dataloader, collate_fn, calib_steps)
                    original_weights = self.collect_original_parameter(pair)
                    basic_loss = self.test_ssd_loss(pair, executor, dataloader, collate_fn, calib_steps)
                    best_loss, best_idx, losses = basic_loss, -1, []
                    made = self.candidates(pair, op_act_range[pair[0]]) if kernels else None
                    for algo in range(0, 4):
                        if made is None: self.one_step_equalization(pair, op_act_range, algo)
                        else:
                            for var, out in made['params'].items(): var.value = out[algo]
                        self.store_parameter(pair)
                        self.initiate_pair_state(pair)
                        loss = self.test_ssd_loss(pair, executor, dataloader, collate_fn, calib_steps)
                        losses.append(loss)
                        if self.verbose:
                            print(f"{'DFQ Step' if algo == 0 else f'SSD Algo {algo}'}, Loss Before Equalization {basic_loss} || "
                                  f'Loss After Equalization {loss}')
                        if loss < basic_loss * self.loss_threshold and loss < best_loss: best_idx, best_loss = algo, loss
                        self.recover_original_parameter(pair, original_weights)
                    if best_idx >= 0:
                        if made is None: self.one_step_equalization(pair, op_act_range, best_idx)
                        else:
                            for var, out in made['params'].items(): var.value = out[best_idx].clone()
                        self.store_parameter(pair)
                    if self.verbose:
                        print('SSD and DFQ Deactivated' if best_idx < 0 else
                              f"{'DFQ Step' if best_idx == 0 else f'SSD Algo {best_idx}'} Activated, Loss Before Equalization "
                              f'{basic_loss} || Loss After Equalization {best_loss}')
                    self.initiate_pair_state(pair)
                    self.stats['accepted'][best_idx] = self.stats['accepted'].get(best_idx, 0) + 1
                    self.history[(i, p)] = dict(basic=basic_loss, losses=losses, best_idx=best_idx)
        finally:
            self._cache = None


class _Indices:
    """A stand-in loader of ``n`` batches (the visiting order of the calibration loop without touching the data)."""
    def __init__(self, n: int): self.n = n
    def __len__(self) -> int: return self.n
    def __iter__(self): return iter(range(self.n))
