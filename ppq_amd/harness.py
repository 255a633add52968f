"""Measurement harness: the smallest caller that can drive the calibration hot path end to end
when PPQ itself is not importable (the GPU box has no /root/reference).

NOT a re-implementation of PPQ's graph IR / executor / quantizers (all out of scope, SURVEY
section 2): it offers just the slice of their interfaces that ``RuntimeCalibrationPass`` and the
observers touch, with the reference's names and call protocol --

* ``Variable`` / ``Operation`` / ``QuantableOperation`` / ``BaseGraph``   ppq/IR/base/graph.py:15-260,
                                                                           ppq/IR/quantize.py:15-140
* ``TorchExecutor.forward(inputs, output_names, hooks)``                   ppq/executor/torch.py:365-577
  (quantize inputs -> pre_forward_hook -> op -> quantize outputs -> post_forward_hook)
* a TensorRT-style INT8 policy (``quantize_graph``)                        quantizer/TensorRTQuantizer.py
  + the state edits of QuantizeFusionPass / QuantizeSimplifyPass           optim/refine.py
* ``ParameterQuantizePass`` / ``ParameterBakingPass``                      now ppq_amd/parameters.py (re-exported here)
* ``resnet50_graph`` -- the ResNet-50 topology (53 Conv + 1 Gemm, BN pre-folded) with seeded
  He-initialised weights, standing in for the ONNX model that cannot be loaded here (no `onnx`).

The dense math (conv / gemm) is PyTorch-ROCm (MIOpen / rocBLAS), exactly as in the reference; only
the quantization simulation goes through this package's kernels.
"""
import contextlib
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

from .core import LinearQuantizationConfig, QuantizationStates, TensorQuantizationConfig, is_initial
from .core import QuantizationProperty as P
from .qfunction import PPQuantFunction

PASSIVE_OPERATIONS = {'MaxPool', 'GlobalMaxPool', 'Reshape', 'Flatten', 'Identity', 'Dropout', 'Slice', 'Pad', 'Resize',
                      'Split', 'Transpose', 'Interp', 'Squeeze', 'Unsqueeze'}        # ppq/core/common.py:50-53
COMPUTING_OP = {'Conv', 'Gemm', 'ConvTranspose', 'MatMul'}


class Variable:
    def __init__(self, name: str, value: torch.Tensor = None, is_parameter: bool = False):
        self.name = name
        self.value = value
        self.stored_value = None         # QuantableVariable.stored_value, IR/quantize.py:183-205 (set when its op is quantised)
        self.is_parameter = is_parameter
        self.dest_ops: List['Operation'] = []
        self.source_op: Optional['Operation'] = None

    def __hash__(self): return hash(self.name)
    def __eq__(self, o): return isinstance(o, Variable) and o.name == self.name


class OperationQuantizationConfig:
    """ppq/core/quant.py:952-1013."""
    def __init__(self, input_quantization_configs, output_quantization_configs):
        self.input_quantization_config: List[TensorQuantizationConfig] = input_quantization_configs
        self.output_quantization_config: List[TensorQuantizationConfig] = output_quantization_configs


class Operation:
    def __init__(self, name: str, op_type: str, attributes: dict = None, inputs=None, outputs=None):
        self.name, self.type = name, op_type
        self.attributes = attributes or {}
        self.inputs: List[Variable] = inputs or []
        self.outputs: List[Variable] = outputs or []

    @ property
    def parameters(self) -> List[Variable]:
        return [v for v in self.inputs if v.is_parameter]

    def __str__(self): return f'{self.name}({self.type})'


class QuantableOperation(Operation):
    """ppq/IR/quantize.py:15-140."""
    def __init__(self, op: Operation, config: OperationQuantizationConfig):
        super().__init__(op.name, op.type, op.attributes, op.inputs, op.outputs)
        self.config = config
        self.store_parameter_value()

    def store_parameter_value(self):
        """IR/quantize.py:113-122: keep a copy of every parameter as it is when the operation is quantised."""
        for var in self.inputs:
            if var.is_parameter and isinstance(var.value, torch.Tensor): var.stored_value = var.value.detach().clone()
        return self

    def _swap_parameters(self) -> None:
        for var in self.inputs:
            if var.is_parameter and isinstance(var.value, torch.Tensor) and var.stored_value is not None:
                parked = var.value
                var.value = var.stored_value.to(parked.device)
                var.stored_value = parked

    @ property
    def config_with_variable(self):
        return list(zip(self.config.input_quantization_config, self.inputs)) + \
            list(zip(self.config.output_quantization_config, self.outputs))

    def dequantize(self):
        """ppq/IR/quantize.py:124-141: park every config in FP32, remembering its state, AND swap every parameter with
        its stored value -- a dequantised operation computes with the parameters it had when it was quantised (the
        current, possibly finetuned / bias-corrected / baked ones wait in stored_value).  This is what makes the FP32
        targets of the training based passes independent of what earlier blocks did to the parameters."""
        if getattr(self, '_dequantized', False): return self
        for cfg, _ in self.config_with_variable:
            cfg.detail['Stored State'] = cfg.state
            cfg.state = QuantizationStates.FP32
        self._swap_parameters()
        self._dequantized = True
        return self

    def restore_quantize_state(self):
        """ppq/IR/quantize.py:143-160: the states and the current parameters come back."""
        if not getattr(self, '_dequantized', False): return self
        for cfg, _ in self.config_with_variable:
            if 'Stored State' in cfg.detail: cfg.state = cfg.detail.pop('Stored State')
        self._swap_parameters()
        self._dequantized = False
        return self

    def baking_parameters(self, quant_func: Callable):
        """IR/quantize.py:98-111."""
        for config, var in self.config_with_variable:
            if var.is_parameter and QuantizationStates.is_activated(config.state):
                var.value = quant_func(var.value, config)
                config.state = (QuantizationStates.BAKED if config.state == QuantizationStates.ACTIVATED
                                else QuantizationStates.PASSIVE_BAKED)


class BaseGraph:
    def __init__(self, name: str):
        self.name = name
        self.operations: Dict[str, Operation] = {}
        self.variables: Dict[str, Variable] = {}
        self.inputs: Dict[str, Variable] = {}
        self.outputs: Dict[str, Variable] = {}

    def create_variable(self, name: str, value=None, is_parameter=False) -> Variable:
        v = Variable(name, value, is_parameter)
        self.variables[name] = v
        return v

    def create_operation(self, op_type: str, name: str, inputs: List[Variable], attributes: dict = None) -> Variable:
        out = self.create_variable(name + '_out')
        op = Operation(name, op_type, attributes, list(inputs), [out])
        out.source_op = op
        for v in inputs: v.dest_ops.append(op)
        self.operations[name] = op
        return out

    def topological_sort(self) -> List[Operation]:
        return list(self.operations.values())        # operations are created in execution order


# ------------------------------------------------------------------------------------ native pointwise convolution
# Where ffi.conv1x1 (ppqhip_conv1x1) runs a Conv in place of F.conv2d.  Both constants are FROZEN from the
# per-shape measurement of tools/pointwise_conv_bench.py (profiles/r18_pointwise_conv.txt), not tuned at run time:
POINTWISE_MIN_WORK = 3.2e9        # FLOPs (2 N Co Ci Ho Wo) of one call from which the native kernel is used: every class enabled below was
#                                   measured faster at 3.29e9 and above (ResNet-50 at batch 32); at a quarter of it only the stride-2 ones still are
POINTWISE_KEEP_VENDOR = frozenset({   # (Ci, Co, H, W, stride) classes that stay on F.conv2d: measured NOT faster natively by more than the
    (64, 64, 56, 56, 1), (256, 64, 56, 56, 1), (256, 128, 56, 56, 1), (1024, 256, 14, 14, 1), (2048, 512, 7, 7, 1)})   # spread, plain (r18) AND fused (r20)
#   native in ResNet-50 as a plain GEMM (profiles/r18_pointwise_conv.txt): (256, 1024, 14, 14, 1) x 6 layers, (512, 128, 28, 28, 1) x 3 and
#   the down convolutions (256, 512, 56, 56, 2), (512, 1024, 28, 28, 2).  Native because the calibration forward's ONE fused launch
#   (ffi.conv1x1_epilogue) beats F.conv2d + the sink epilogue launch by more than the spread, summed over the two phases
#   (profiles/r20_pointwise_epilogue.txt): (64, 256, 56, 56, 1) x 4, (128, 512, 28, 28, 1) x 4, (512, 2048, 7, 7, 1) x 3,
#   (512, 256, 28, 28, 1), (1024, 512, 14, 14, 1) and the down convolution (1024, 2048, 14, 14, 2).  These pay their r18 deficit
#   (2 .. 9 us per layer) in forwards without sinks and as the non-owning convolution of a two-conv group; the calibration
#   pass has no forward without sinks.  ((64, 64, 56, 56, 1) also measured faster fused, but lies below POINTWISE_MIN_WORK at batch 32,
#   where it was measured: it stays.  (256, 128, 56, 56, 1) cleared the rule by 1 us in one run and 4 us in the other: it stays too.)
POINTWISE_KEEP_UNFUSED = frozenset({   # (Ci, Co, H, W, stride, role) measured NOT faster as ONE ffi.conv1x1_epilogue launch than as
    (512, 1024, 28, 28, 2, 'P2b')})    # ffi.conv1x1 + the sink epilogue launch, summed over the two calibration phases (r20)


def _square(v):
    """The one value of an ONNX per-axis attribute given as an int or as a list of equal ints; None when the axes differ."""
    if isinstance(v, (list, tuple)):
        return int(v[0]) if len(v) > 0 and all(int(e) == int(v[0]) for e in v) else None
    return int(v)


def pointwise_eligible(x, w, attributes: dict, min_work: float) -> bool:
    """Whether ``Conv(x, w[, bias])`` with `attributes` is one the native pointwise kernel takes: a 1x1 kernel, no padding, no
    dilation, one group, a square stride of 1 or 2, float32 contiguous-NCHW operands on the GPU, no autograd, at least
    `min_work` FLOPs and a shape class that is not in POINTWISE_KEEP_VENDOR.  Shapes, layout and attributes only: the bias plays no
    part, so the fused path (convolution without bias, the epilogue adds it) and the unfused one (with bias) decide alike."""
    a = attributes or {}
    if not (isinstance(x, torch.Tensor) and isinstance(w, torch.Tensor) and x.dim() == 4 and w.dim() == 4): return False
    if tuple(w.shape[2:]) != (1, 1) or w.shape[1] != x.shape[1]: return False
    if _square(a.get('pads', 0)) != 0 or _square(a.get('dilations', 1)) != 1 or a.get('group', 1) != 1: return False
    stride = _square(a.get('strides', 1))
    if stride not in (1, 2): return False
    if not (x.is_cuda and w.is_cuda and x.dtype is torch.float32 and w.dtype is torch.float32): return False
    if not (x.is_contiguous() and w.is_contiguous()) or x.numel() == 0: return False
    if torch.is_grad_enabled() or x.requires_grad or w.requires_grad: return False
    n, c, h, wd = (int(v) for v in x.shape)
    o = int(w.shape[0])
    if (c, o, h, wd, stride) in POINTWISE_KEEP_VENDOR: return False
    return 2.0 * n * o * c * ((h - 1) // stride + 1) * ((wd - 1) // stride + 1) >= min_work


def _conv(x, w, bias, a: dict, native_min_work=None):
    """The executor's convolution: ffi.conv1x1 where ``pointwise_eligible`` (`native_min_work` None: never), else F.conv2d."""
    if native_min_work is not None and pointwise_eligible(x, w, a, native_min_work):
        from .ffi import conv1x1
        y = conv1x1(x, w, bias, _square(a.get('strides', 1)))
        if y is not None: return y                    # (None: PPQHIP_NOT_FUSED, the kernel has no path for these pointers)
    return F.conv2d(x, w, bias, stride=a.get('strides', 1), padding=a.get('pads', 0), groups=a.get('group', 1))


# ------------------------------------------------------------------------------------ op library
def _forward(op: Operation, x: List[torch.Tensor], native_min_work=None):
    t, a = op.type, op.attributes
    if t == 'Conv': return _conv(x[0], x[1], x[2] if len(x) > 2 else None, a, native_min_work)
    if t == 'Gemm': return F.linear(x[0], x[1], x[2] if len(x) > 2 else None)
    if t == 'MatMul': return torch.matmul(x[0], x[1])
    if t == 'Relu': return F.relu(x[0])
    if t == 'Gelu': return F.gelu(x[0])
    if t == 'Add': return x[0] + x[1]
    if t == 'MaxPool': return F.max_pool2d(x[0], a['kernel_shape'], a.get('strides', 1), a.get('pads', 0))
    if t == 'GlobalAveragePool': return F.adaptive_avg_pool2d(x[0], 1)
    if t == 'Flatten': return torch.flatten(x[0], 1)
    if t == 'LayerNormalization': return F.layer_norm(x[0], x[0].shape[-1:], x[1], x[2])
    if t == 'Softmax': return F.softmax(x[0], dim=a.get('axis', -1))
    if t == 'Mul': return x[0] * (x[1] if len(x) > 1 else a['value'])
    if t == 'Reshape': return x[0].reshape(a['shape'])
    if t == 'Transpose': return x[0].permute(a['perm'])
    if t == 'Concat': return torch.cat([v.expand(x[-1].shape[0], *v.shape[1:]) if v.shape[0] == 1 else v for v in x],
                                       dim=a.get('axis', 1))
    if t == 'Slice': return x[0].narrow(a['axis'], a['start'], a['length'])
    if t == 'Resize': return F.interpolate(x[0], scale_factor=a.get('scale', 2), mode=a.get('mode', 'nearest'))
    raise NotImplementedError(f'Graph op: {op.name}({op.type}) has no backend implementation')


# ------------------------------------------------------------------------------------ convolution epilogues
class EpilogueGroup:
    """Consecutive operations whose elementwise tail runs as ONE epilogue launch (ffi.bias_act_ / ffi.bias_add_act):
    ``P1``  Conv(bias) -> Relu [-> MaxPool: the pooled form, ffi.bias_act_(pool=...)];
    ``P2``  Conv_a(bias) [, Conv_b(bias)] -> Add(a, b) -> Relu.
    ``ops``: the members in execution order; ``convs``: the convolutions, Add input 0's producer first; ``add`` / ``relu``;
    ``keep``: the variable names the planner was told to keep (graph outputs, requested outputs); ``pool``: the MaxPool of a
    pooled P1, else None."""
    __slots__ = ('kind', 'ops', 'convs', 'add', 'relu', 'keep', 'pool')

    def __init__(self, kind, ops, convs, add, relu, keep=(), pool=None):
        self.kind, self.ops, self.convs, self.add, self.relu, self.keep = kind, ops, convs, add, relu, frozenset(keep)
        self.pool = pool

    def __repr__(self): return f'{self.kind}({", ".join(op.name for op in self.ops)})'


def pool_window(op: Operation) -> Optional[tuple]:
    """``(kernel, stride, pad)`` of a MaxPool the epilogue launch can take in (what ``_forward`` hands to F.max_pool2d), or None:
    every attribute an int or a pair of equal ints, ``dilations`` / ``ceil_mode`` absent or at their defaults.  Whether the
    kernel has a path for the window (kernel <= 3, ...) is decided at the launch."""
    a = op.attributes

    def square(value):
        if isinstance(value, (list, tuple)):
            if not 1 <= len(value) <= 2 or any(v != value[0] for v in value): return None
            value = value[0]
        return value if isinstance(value, int) and not isinstance(value, bool) else None
    if 'kernel_shape' not in a or square(a.get('dilations', 1)) != 1 or a.get('ceil_mode', 0) not in (0, False): return None
    window = tuple(square(v) for v in (a['kernel_shape'], a.get('strides', 1), a.get('pads', 0)))
    return None if any(v is None for v in window) else window


def _in_cfg(op, i):
    return op.config.input_quantization_config[i] if isinstance(op, QuantableOperation) else None


def _out_cfg(op, i):
    return op.config.output_quantization_config[i] if isinstance(op, QuantableOperation) else None


def plan_epilogues(operations: List[Operation], hooks: Dict[str, object] = None, keep=(), passes_through: Callable = None,
                   grad_enabled: bool = False) -> List[EpilogueGroup]:
    """The epilogue groups of `operations` (in execution order).  No device, no tensor values: graph, configs and hooks.

    A group is formed only when (1) its members are consecutive in `operations`; (2) every intermediate tensor has its
    group successor as only consumer and is not in `keep` (graph outputs, requested outputs); (3) every config of a tensor
    the kernel does NOT write -- P1: the conv output, P2: the Add output, as producer output and as consumer input --
    passes through (`passes_through(cfg)`: not activated, not delegated), and so do the configs between a conv and the
    Add (the Add must see the biased conv output itself); (4) the hooks of the members are absent or plain
    ``observer.CalibrationHook``s that observe none of the configs of (3); (5) autograd is off.
    A P1 group takes in the MaxPool behind its Relu (the pooled form) under the same rules: consecutive; the Relu output
    feeds only the pool and is not kept; the window is one ``pool_window`` accepts; the Relu output config and the pool's input
    config pass through (the pool must see the Relu output itself, not a fake-quantised copy); the pool's hook is absent or
    a plain ``CalibrationHook`` that does not observe the pool's input.  Otherwise the group is the plain P1 and the pool
    runs on its own."""
    if grad_enabled: return []
    from .observer import CalibrationHook
    hooks = hooks or {}
    keep = set(keep)
    if passes_through is None:
        def passes_through(c): return not QuantizationStates.is_activated(c.state)

    def through(*cfgs): return all(c is None or passes_through(c) for c in cfgs)

    def hooks_ok(members, unwritten):
        for op in members:
            h = hooks.get(op.name)
            if h is None: continue
            if type(h) is not CalibrationHook: return False
            if any(c is not None and c in h._observer_table for c in unwritten): return False
        return True

    def conv_ok(op):
        return (op.type == 'Conv' and len(op.inputs) == 3 and op.inputs[2].is_parameter and len(op.outputs) == 1
                and op.outputs[0].name not in keep)

    def only_feeds(v, op): return len(v.dest_ops) == 1 and v.dest_ops[0] is op

    def relu_after(op, i):
        if i >= len(operations): return None
        r = operations[i]
        out = op.outputs[0]
        if r.type != 'Relu' or len(r.inputs) != 1 or r.inputs[0] is not out or not only_feeds(out, r) or out.name in keep:
            return None
        return r

    def pool_after(relu, i):
        if i >= len(operations): return None
        m, out = operations[i], relu.outputs[0]
        if (m.type != 'MaxPool' or len(m.inputs) != 1 or len(m.outputs) != 1 or m.inputs[0] is not out or not only_feeds(out, m)
                or out.name in keep or pool_window(m) is None): return None
        between = (_out_cfg(relu, 0), _in_cfg(m, 0))
        if not through(*between) or not hooks_ok([m], between[1:]): return None
        return m

    def try_p2(i):
        for n_conv in (2, 1):
            j = i + n_conv
            if j + 1 >= len(operations): continue
            add, convs = operations[j], operations[i:j]
            if add.type != 'Add' or len(add.inputs) != 2 or len(add.outputs) != 1 or not all(conv_ok(c) for c in convs): continue
            by_out = {c.outputs[0].name: c for c in convs}
            x0, x1 = add.inputs
            if x0.name not in by_out or x0 is x1: continue
            if n_conv == 2 and x1.name not in by_out: continue
            ordered = [by_out[x0.name]] + ([by_out[x1.name]] if n_conv == 2 else [])
            if not all(only_feeds(c.outputs[0], add) for c in convs): continue
            relu = relu_after(add, j + 1)
            if relu is None: continue
            unwritten = (_out_cfg(add, 0), _in_cfg(relu, 0))
            between = [_out_cfg(c, 0) for c in convs] + [_in_cfg(add, 0), _in_cfg(add, 1)]
            if not through(*unwritten, *between): return None
            members = list(operations[i:j + 2])
            if not hooks_ok(members, unwritten): return None
            return EpilogueGroup('P2', members, ordered, add, relu, keep)
        return None

    def try_p1(i):
        conv = operations[i]
        if not conv_ok(conv): return None
        relu = relu_after(conv, i + 1)
        if relu is None: return None
        unwritten = (_out_cfg(conv, 0), _in_cfg(relu, 0))
        if not through(*unwritten) or not hooks_ok([conv, relu], unwritten): return None
        pool = pool_after(relu, i + 2)
        return EpilogueGroup('P1', [conv, relu] + ([pool] if pool is not None else []), [conv], None, relu, keep, pool)

    groups, i = [], 0
    while i < len(operations):
        g = try_p2(i) if operations[i].type == 'Conv' else None
        if g is None and operations[i].type == 'Conv': g = try_p1(i)
        if g is None:
            i += 1
            continue
        groups.append(g)
        i += len(g.ops)
    return groups


def elidable_stores(grp: EpilogueGroup, hooks, jobs: Dict[str, tuple], recorder=None) -> set:
    """The convolutions of a P2 group whose biased output ``a`` / ``b`` the epilogue launch need not STORE in this
    calibration forward (ffi.ELIDE_A / ELIDE_B): the tensor then has no reader left.  Its graph consumer is the group's Add,
    which happens inside the launch; its observer takes its statistic inside the launch too.  So a store stays unless
    all of these hold: (1) the Add is the variable's only consumer; (2) it is no graph output and was not requested
    (``grp.keep``); (3) its observer got a sink in this launch (``jobs``: member name -> job) and touches the tensor
    through that job only (``reads_only_its_job``: not a subclass, not a replaced ``observe``); (4) nothing records the
    tensors of this forward (``recorder``: ``ObservationQueue.recorder`` of ``reuse_activations``); (5) no other hook of
    the group observes the variable (the Add's input side).
    The Relu of a pooled P1 group stands to its MaxPool as a convolution of a P2 group stands to the Add: the pool happens
    inside the launch (``store=False`` of ffi.bias_act_stats_ / bias_act_hist_), and the same five conditions decide."""
    if recorder is not None or not hooks: return set()
    if grp.kind == 'P2': producers, reader = grp.convs, grp.add
    elif grp.pool is not None: producers, reader = [grp.relu], grp.pool
    else: return set()
    reader_hook = hooks.get(reader.name)
    out = set()
    for op in producers:
        v, hook = op.outputs[0], hooks.get(op.name)
        if len(v.dest_ops) != 1 or v.dest_ops[0] is not reader or v.name in grp.keep: continue
        if op.name not in jobs or hook is None or not isinstance(op, QuantableOperation): continue
        obs = [hook._observer_table.get(c) for c in op.config.output_quantization_config]
        if len(obs) != 1 or obs[0] is None or not obs[0].reads_only_its_job(): continue
        if reader_hook is not None and isinstance(reader, QuantableOperation) and any(
                c in reader_hook._observer_table for x, c in zip(reader.inputs, reader.config.input_quantization_config) if x is v):
            continue
        out.add(op.name)
    return out


class TorchExecutor:
    """The forward loop of ppq/executor/torch.py:457-577 (hook protocol of executor/base.py:44-102)."""
    def __init__(self, graph: BaseGraph, device: str = 'cuda'):
        self._graph = graph
        self._device = device
        self._default_quant_fn = PPQuantFunction
        self.cache_parameter_quantization = False     # opt-in: see _quantize_parameter
        self._param_cache: Dict[str, tuple] = {}
        self.fuse_parameter_quantization = True       # all weights of a forward in ONE launch: _fused_parameters
        self._plans: list = []
        self._plan_signature = None
        self._plan_cache: Dict[tuple, list] = {}
        self._fused: Dict[tuple, torch.Tensor] = {}
        self._delegates: Dict[object, Callable] = {}
        self._overrides: Dict[str, Callable] = {}     # operation name -> fn(op, raw inputs): register_operation_override
        self._takes_packed: set = set()               # ... whose fn takes input 0 in the packed form a group override handed over
        self._group_overrides: Dict[str, tuple] = {}  # first member's name -> (member names, fn): register_group_override
        self.fuse_epilogues = True                    # conv bias [+ residual Add] + Relu [+ MaxPool] in ONE launch: plan_epilogues
        self._epilogue_cache: Dict[tuple, dict] = {}
        self.channels_last = False                    # see use_channels_last()
        self.native_pointwise_conv = True             # eligible 1x1 convolutions on ffi.conv1x1 (pointwise_eligible); else F.conv2d
        self.pointwise_min_work = POINTWISE_MIN_WORK  # FLOPs per call from which they are
        self.fuse_pointwise_epilogue = True           # ... and, in a forward with sinks, take their epilogue group into the GEMM's store: _pointwise_epilogue
        for v in graph.variables.values():
            if v.is_parameter and v.value is not None: v.value = v.value.to(device)

    def use_channels_last(self) -> 'TorchExecutor':
        """Keep 4-D activations and conv weights in channels-last memory format: MIOpen's FP32 convolutions
        are ~8 % faster in NHWC on MI355X (tools/conv_format_probe.py) and the per-tensor statistics /
        fake-quant kernels stream any dense layout in storage order (ffi._dense), so no layout copy appears
        anywhere on the calibration path.  Values are those of the NCHW run up to the convolution
        algorithm's own rounding."""
        self.channels_last = True
        for v in self._graph.variables.values():
            if v.is_parameter and isinstance(v.value, torch.Tensor) and v.value.dim() == 4:
                v.value = v.value.contiguous(memory_format=torch.channels_last)
        return self

    def _native_min_work(self):
        """What ``_conv`` takes as `native_min_work`: None (F.conv2d throughout) with the flag off or in channels-last."""
        return self.pointwise_min_work if self.native_pointwise_conv and not self.channels_last else None

    def _place(self, value: torch.Tensor) -> torch.Tensor:
        value = value.to(self._device)
        if self.channels_last and value.dim() == 4: value = value.contiguous(memory_format=torch.channels_last)
        return value

    def register_quantize_delegate(self, config, delegator: Callable) -> None:
        """ppq/executor/torch.py:296-323: a delegator takes over the quantisation of one config."""
        self._delegates[config] = delegator

    def remove_quantize_delegate(self, config) -> None:
        self._delegates.pop(config, None)

    def register_operation_override(self, op_name: str, fn: Callable, takes_packed: bool = False) -> None:
        """Run operation ``op_name`` as ``fn(op, raw_inputs)`` -- a tensor or a list of tensors, one per output -- in place of the
        quantisation of its inputs and its torch forward (a deployed kernel that does both: ``mx.deploy_graph_mx``).  The output
        configs are applied as usual.  A forward that hooks the operation runs the simulated path for it, so calibration and the
        analysis passes see what they see without the override; an overridden operation joins no epilogue group.
        ``takes_packed``: ``fn`` also accepts, as ``raw_inputs[0]``, the packed form of that input where a group override
        (``register_group_override``) produced one; it is then never asked to quantise it again."""
        if op_name not in self._graph.operations: raise KeyError(f'register_operation_override: the graph has no operation {op_name!r}')
        if not callable(fn): raise TypeError(f'register_operation_override: fn must be callable, got {type(fn)}')
        self._overrides[op_name] = fn
        if takes_packed: self._takes_packed.add(op_name)
        else: self._takes_packed.discard(op_name)

    def remove_operation_override(self, op_name: str) -> None:
        self._overrides.pop(op_name, None)
        self._takes_packed.discard(op_name)

    def register_group_override(self, op_names: List[str], fn: Callable) -> None:
        """Run the operations ``op_names`` -- a chain in execution order: every member's output feeds only the next member --
        as ONE call ``fn(ops, inputs, need_float) -> (values, packed)`` at the position of the first (a deployed kernel with a
        fused tail: ``mx.deploy_graph_mx(fuse=True)``).  ``inputs[k]`` are the raw inputs of member k (None where the input is
        another member's output); input 0 of the first member arrives packed when a group handed it over packed and the member's
        own override ``takes_packed``.  ``values``: variable name -> float tensor; ``packed``: variable name -> packed form.  Every
        member's output must be in one of them, and every name in ``need_float`` in ``values``: the last output's name is in
        ``need_float`` whenever anything but an override that ``takes_packed`` reads it in this forward -- a graph output, a
        requested output, a consumer without such an override or with a hook.  The other outputs may alias the last one, as
        the unwritten tensors of an epilogue group do.  No output config of a member is applied: the caller registers only
        groups whose configs pass through.
        A forward in which a member is hooked, an output other than the last is a graph output or requested, or a member is
        missing from the operations that run, does not use the group: its operations run one by one, through their own
        overrides or the simulated path.  ``forward_cached`` and ``partial_graph_forward`` ask for every group's last output as
        float (a group may still hand its packed form to the next group's first member within the call); ``forward_cached`` caches
        only that last output, so a later request for another member's output recomputes it."""
        if not op_names: raise ValueError('register_group_override: no operations')
        for name in op_names:
            if name not in self._graph.operations: raise KeyError(f'register_group_override: the graph has no operation {name!r}')
        if not callable(fn): raise TypeError(f'register_group_override: fn must be callable, got {type(fn)}')
        self._group_overrides[op_names[0]] = (tuple(op_names), fn)

    def remove_group_override(self, first_name: str) -> None:
        self._group_overrides.pop(first_name, None)

    def _group_plan(self, operations: List[Operation], hooks, output_names, all_float: bool) -> Dict[str, tuple]:
        """First member's name -> (member ops, fn, need_float) for the group overrides this forward uses."""
        if not self._group_overrides: return {}
        hooks = hooks or {}
        keep = set(self._graph.outputs) | set(output_names or ())
        at = {op.name: i for i, op in enumerate(operations)}
        plan = {}
        for first, (names, fn) in self._group_overrides.items():
            if any(n not in at or n in hooks for n in names): continue
            if any(at[a] >= at[b] for a, b in zip(names, names[1:])): continue
            ops = [operations[at[n]] for n in names]
            if any(v.name in keep for m in ops[:-1] for v in m.outputs): continue
            need = set()
            for v in ops[-1].outputs:
                handed = [d.name in self._takes_packed and d.name in self._overrides and d.name not in hooks and d.name in at
                          and d.inputs[0] is v and sum(1 for x in d.inputs if x is v) == 1 for d in v.dest_ops]
                if all_float or v.name in keep or not handed or not all(handed): need.add(v.name)
            plan[first] = (ops, fn, need)
        return plan

    def _run_group(self, entry: tuple, raw_of: Callable, packed: Dict[str, object]) -> Dict[str, object]:
        """Run one group override; returns variable name -> value for every member's output.  A tensor that left the launch
        packed only is represented by its packed form, which no code that expects a float tensor can mistake for one."""
        ops, fn, need = entry
        inside = {v.name for m in ops for v in m.outputs}
        inputs = [[None if v.name in inside else raw_of(v) for v in m.inputs] for m in ops]
        head = ops[0]
        if head.name in self._takes_packed and head.inputs[0].name in packed: inputs[0][0] = packed[head.inputs[0].name]
        if any(x is None for k, m in enumerate(ops) for x, v in zip(inputs[k], m.inputs) if v.name not in inside):
            raise ValueError(f'group override of {head.name}: an input was not computed')
        values, handed = fn(ops, inputs, need)
        out = {}
        for m in ops:
            for v in m.outputs:
                if v.name in values: out[v.name] = values[v.name]
                elif v.name in handed and v.name not in need: out[v.name] = handed[v.name]
                else: raise RuntimeError(f'group override of {head.name}: no {"float " if v.name in need else ""}value for {v.name}')
        packed.update(handed)
        return out

    def _override_inputs(self, op: Operation, raw_in: list, packed: Dict[str, object]) -> list:
        """The raw inputs an operation override gets: input 0 in its packed form where a group handed one over and the override
        takes it."""
        if packed and op.name in self._takes_packed and op.inputs[0].name in packed:
            raw_in = list(raw_in)
            raw_in[0] = packed[op.inputs[0].name]
        return raw_in

    def quantize_function(self, tensor: torch.Tensor, config=None) -> torch.Tensor:
        if self._delegates and config in self._delegates:          # torch.py:610-613
            return self._delegates[config](tensor, config)
        return self._default_quant_fn(tensor, config)

    def _input_side(self, op: Operation, raw_in: list, hook) -> list:
        """Quantise the inputs of `op`, then ``pre_forward_hook``: what ``_forward`` computes with."""
        qin, cfgs = raw_in, None
        if isinstance(op, QuantableOperation):
            cfgs = list(op.config.input_quantization_config)
            qin = [self._quantize_parameter(v, c) if v.is_parameter else self.quantize_function(x, c)
                   for v, x, c in zip(op.inputs, raw_in, cfgs)]
        if hook is not None: qin = hook.pre_forward_hook(inputs=raw_in, quant_inputs=qin, quant_configs=cfgs)
        return qin

    def _output_side(self, op: Operation, outs, hook) -> list:
        """What `op` computed as a list, quantised, then ``post_forward_hook``: the values of its output variables."""
        fp_outs = outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
        cfgs = None
        if isinstance(op, QuantableOperation):
            cfgs = list(op.config.output_quantization_config)
            outs = [self.quantize_function(y, c) for y, c in zip(outs, cfgs)]
        if hook is not None: outs = hook.post_forward_hook(outputs=fp_outs, quant_outputs=outs, quant_configs=cfgs)
        return outs

    def _step(self, op: Operation, raw_in: list, hook, packed: Optional[Dict[str, object]]) -> list:
        """Run one operation (torch.py:499-563): its override, or input side -> ``_forward``; then the output side.  `packed`:
        what the group overrides of this forward handed over, where an override may take it (``_override_inputs``)."""
        override = self._overrides.get(op.name) if hook is None else None        # a hooked operation runs the simulation
        if override is not None: outs = override(op, self._override_inputs(op, raw_in, packed))
        else:
            qin, native = self._input_side(op, raw_in, hook), self._native_min_work()
            # (the flag travels only with a convolution that takes it: everything else calls _forward as it always did)
            if native is not None and op.type == 'Conv' and pointwise_eligible(qin[0], qin[1], op.attributes, native): outs = _forward(op, qin, native)
            else: outs = _forward(op, qin)
        return self._output_side(op, outs, hook)

    def _walk(self, operations: List[Operation], hooks, output_names: List[str], read: Callable, write: Callable,
              hand_packed: bool = False, write_aliases: bool = True, done: Callable = None, unfed: str = None) -> None:
        """Run `operations` (in execution order) on the caller's store -- ``read(variable)``, ``write(op, outputs)`` -- each as part
        of its group override, of its epilogue group, or through ``_step``.
        ``hand_packed``: a group override may leave its last output packed only, and an operation override reads it so.
        ``write_aliases``: also write the outputs a fused unit never materialised on their own -- all but the last of a group
        override, the input of an epilogue group's Relu.  ``done()``: asked after every unit, true ends the walk.  ``unfed``:
        the caller's name, to refuse an operation with an input nobody fed or computed."""
        groups, packed = self._group_plan(operations, hooks, output_names, not hand_packed), {}
        plan = self._epilogue_plan(operations, hooks, output_names, [m.name for e in groups.values() for m in e[0]])
        fused_done = set()
        for op in operations:
            if op.name in fused_done: continue
            vals = None
            if op.name in groups:
                members = groups[op.name][0]
                vals, aliases = self._run_group(groups[op.name], read, packed), members[:-1]
            elif op.name in plan:
                grp = plan[op.name]
                vals, members, aliases = self._run_epilogue(grp, read, hooks), grp.ops, (grp.add or grp.convs[0],)
            if vals is None:
                raw_in = [read(v) for v in op.inputs]
                if unfed and any(x is None for x in raw_in): raise ValueError(f'{unfed}: input of {op.name} was not fed')
                write(op, self._step(op, raw_in, hooks.get(op.name) if hooks else None, packed if hand_packed else None))
            else:
                for m in members:                     # a fused unit ran: its members are done
                    fused_done.add(m.name)
                    if write_aliases or m not in aliases: write(m, [vals[v.name] for v in m.outputs])
            if done is not None and done(): break

    def forward_with_gradient(self, inputs, output_names: List[str] = None, hooks=None):
        """torch.py:412-455: the same walk with autograd enabled (finetuning passes)."""
        return TorchExecutor.forward.__wrapped__(self, inputs, output_names, hooks)

    def partial_graph_forward(self, operations: List[Operation], feed_dict: Dict[str, torch.Tensor],
                              output_names: List[str], with_gradient: bool = False) -> List[torch.Tensor]:
        """ppq/executor/torch.py:654-682: run only `operations` (already in execution order) on the
        given feeds -- the block forward of the training based passes.  Like ``forward`` it records no autograd
        graph unless ``with_gradient`` (the finetuning passes' training step) asks for one."""
        g = self._graph
        results = [None] * len(output_names)

        def write(op, outs):
            for v, y in zip(op.outputs, outs):
                v.value = y
                if v.name in output_names: results[output_names.index(v.name)] = y
        with contextlib.nullcontext() if with_gradient else torch.no_grad():
            for name, value in feed_dict.items(): g.variables[name].value = self._place(value)
            self._fused_parameters(operations)            # the multi-tensor plan covers the parameters of THESE operations only
            self._walk(operations, None, output_names, lambda v: v.value, write, unfed='partial_graph_forward')
        for v in g.variables.values():
            if not v.is_parameter: v.value = None
        return results

    def _fused_parameters(self, operations=None) -> None:
        """Fake-quantise every parameter whose config is an activated, non-delegated LINEAR one with a
        single multi-tensor launch (ffi.LinearQuantizePlan -> ppqhip_fq_linear_multi) instead of one
        launch per weight; same per-forward work as the reference executor (torch.py:516-518), same
        values as PPQLinearQuantFunction.  The device job table holds POINTERS, so in-place updates of
        weights / scales need no rebuild; replaced tensors or edited configs do (signature check)."""
        self._fused = {}
        if not self.fuse_parameter_quantization or self._default_quant_fn is not PPQuantFunction: return
        from .ffi import FloatingQuantizePlan, LinearQuantizePlan
        todo, sig = [], []
        for op in (self._graph.operations.values() if operations is None else operations):
            if not isinstance(op, QuantableOperation): continue
            for v, c in zip(op.inputs, op.config.input_quantization_config):
                if not (v.is_parameter and isinstance(v.value, torch.Tensor) and v.value.is_cuda): continue
                if not QuantizationStates.is_activated(c.state) or c in self._delegates: continue
                pol = c.policy
                floating = pol.has_property(P.FLOATING)
                if not (pol.has_property(P.LINEAR) or floating) or pol.has_property(P.DYNAMIC): continue
                if v.value.dtype != torch.float32 or v.value.requires_grad or v.value.numel() == 0: continue
                if not (isinstance(c.scale, torch.Tensor) and isinstance(c.offset, torch.Tensor)): continue
                axis = c.channel_axis if pol.has_property(P.PER_CHANNEL) else None
                if not LinearQuantizePlan.accepts(v.value, c.scale, c.offset, axis): continue   # per-tensor launch instead
                rnd = int(getattr(c.rounding, 'value', c.rounding))
                todo.append((v, c, axis, rnd, floating))
                sig.append((v.name, id(c), v.value.data_ptr(), c.scale.data_ptr(), c.offset.data_ptr(), tuple(v.value.shape), c.scale.numel(),
                            axis, c.quant_min, c.quant_max, rnd, floating,
                            (c.exponent_bits, c.mantissa_bits) if floating else None))
        if not todo:
            self._plans, self._plan_signature = [], None
            return
        cached = self._plan_cache.get(tuple(sig))
        if cached is not None:
            self._plan_cache[tuple(sig)] = self._plan_cache.pop(tuple(sig))          # most recently used last
            self._plans, self._plan_signature = cached, sig
        if sig != self._plan_signature:
            groups: Dict[tuple, list] = {}
            for item in todo: groups.setdefault((item[3], item[4]), []).append(item)
            self._plans = []
            for (rnd, floating), items in groups.items():
                if floating:        # TRT_FP8 policy: per-channel FP8 weights (one launch for all of them too)
                    plan = FloatingQuantizePlan([(v.value, c.scale, c.offset, axis, c.exponent_bits, c.mantissa_bits,
                                                  c.quant_min, c.quant_max) for v, c, axis, _, _ in items], rounding=rnd)
                else:
                    plan = LinearQuantizePlan([(v.value, c.scale, c.offset, axis, c.quant_min, c.quant_max)
                                               for v, c, axis, _, _ in items], rounding=rnd)
                self._plans.append((plan, [(v.name, id(c)) for v, c, _, _, _ in items]))
            self._plan_signature = sig
            if len(self._plan_cache) >= 8: self._plan_cache.pop(next(iter(self._plan_cache)))   # block / whole-graph plans alternate
            self._plan_cache[tuple(sig)] = self._plans
        for plan, keys in self._plans:
            for key, out in zip(keys, plan.run()): self._fused[key] = out

    def _epilogue_plan(self, operations: List[Operation], hooks, output_names, grouped=()) -> Dict[str, EpilogueGroup]:
        """First member name -> group, for a forward over `operations` (plan_epilogues), cached per (operations, hooks,
        requested outputs, delegates, config states) signature like the parameter plans."""
        if not self.fuse_epilogues or torch.is_grad_enabled() or self._default_quant_fn is not PPQuantFunction: return {}
        states = tuple(c.state for op in operations if isinstance(op, QuantableOperation)
                       for c in (*op.config.input_quantization_config, *op.config.output_quantization_config))
        sig = (tuple(op.name for op in operations), tuple((k, id(h)) for k, h in hooks.items()) if hooks else (),
               tuple(output_names or ()), tuple(id(c) for c in self._delegates), states, tuple(sorted(self._overrides)), tuple(sorted(grouped)))
        plan = self._epilogue_cache.get(sig)
        if plan is None:
            delegates = self._delegates

            def passes_through(c): return not QuantizationStates.is_activated(c.state) and c not in delegates
            groups = plan_epilogues(operations, hooks, set(self._graph.outputs) | set(output_names or ()), passes_through)
            if self._overrides:                       # an operation that runs its override is a member of no group
                groups = [g for g in groups if not any(m.name in self._overrides and not (hooks and m.name in hooks) for m in g.ops)]
            if grouped:                               # nor is a member of a group override that this forward uses
                groups = [g for g in groups if not any(m.name in grouped for m in g.ops)]
            plan = {g.ops[0].name: g for g in groups}
            if len(self._epilogue_cache) >= 8: self._epilogue_cache.pop(next(iter(self._epilogue_cache)))
            self._epilogue_cache[sig] = plan
        return plan

    def _run_epilogue(self, grp: EpilogueGroup, raw_of: Callable, hooks) -> Optional[Dict[str, torch.Tensor]]:
        """Run one planned group: every conv without bias, ONE epilogue launch, then -- member by member, in op order --
        the quantize_function calls and hooks of the unfused loop on the tensors the kernel wrote (the planner guarantees
        that the configs of the tensors it did not write pass through and are not observed).  Returns variable name ->
        value for the outputs of every member, or None before anything ran when the operands' layout does not qualify."""
        from .ffi import (ELIDE_A, ELIDE_B, bias_act_, bias_act_hist_, bias_act_stats_, bias_add_act, bias_add_act_hist,
                          bias_add_act_stats)
        for conv in grp.convs:                       # conv output layout follows x / w: both dense, both in one format
            x, w = raw_of(conv.inputs[0]), conv.inputs[1].value
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                    and isinstance(w, torch.Tensor) and w.dim() == 4): return None
            fmt = torch.channels_last if self.channels_last else torch.contiguous_format
            if not (x.is_contiguous(memory_format=fmt) and w.is_contiguous(memory_format=fmt)): return None
        if grp.add is not None:
            b_var = grp.add.inputs[1]
            if b_var.source_op not in grp.convs:
                b = raw_of(b_var)
                if not (isinstance(b, torch.Tensor) and b.is_cuda and b.dtype == torch.float32): return None
        hooks = hooks or {}
        ys, biases = {}, {}
        for conv in grp.ops[:len(grp.convs)]:        # the convolutions, in execution order
            qin = self._input_side(conv, [raw_of(v) for v in conv.inputs], hooks.get(conv.name))
            a = conv.attributes
            biases[conv.name] = qin[2]
            if conv is grp.ops[len(grp.convs) - 1]:  # the last one may take the whole group into its store
                done = self._pointwise_epilogue(grp, conv, qin, ys, biases, raw_of, hooks)
                if done is not None: return self._group_values(grp, hooks, raw_of, *done)
            ys[conv.name] = _conv(qin[0], qin[1], None, a, self._native_min_work())
        if grp.kind == 'P1':
            conv = grp.convs[0]
            y = ys[conv.name]
            stored = {grp.relu.name: y}                  # member -> the tensor the launch stores as that member's output
            fed = self._epilogue_sinks(grp, hooks, stored, y)
            # the pooled form (contiguous NCHW only): sink launch, then plain pooled launch, then the group without its pool
            window = pool_window(grp.pool) if grp.pool is not None and not self.channels_last else None
            pooled, elided = None, set()
            if fed is not None:
                job = fed[0].get(grp.relu.name)
                launch = bias_act_hist_ if job is not None and job[0] == 'hist_rows' else bias_act_stats_
                if window is not None:
                    elided = elidable_stores(grp, hooks, fed[0], fed[1].recorder)
                    pooled = launch(y, biases[conv.name], True, job, pool=window, store=not elided)
                    if pooled is None: elided = set()
                if pooled is None and not launch(y, biases[conv.name], True, job): fed = None
            if fed is None:
                if window is not None: pooled = bias_act_(y, biases[conv.name], relu=True, pool=window)
                if pooled is None and not bias_act_(y, biases[conv.name], relu=True):
                    y.add_(biases[conv.name].view(1, -1, 1, 1)).relu_()      # PyTorch's own conv-bias step, then F.relu
            tail = {conv.name: y, grp.relu.name: y}
            if grp.pool is not None: tail[grp.pool.name] = pooled    # (None: the loop below runs the pool itself)
        else:
            conv_a = grp.convs[0]
            a = ys[conv_a.name]
            conv_b = grp.convs[1] if len(grp.convs) > 1 else None
            b = ys[conv_b.name] if conv_b is not None else raw_of(grp.add.inputs[1])
            bias_b = biases[conv_b.name] if conv_b is not None else None
            stored = {conv_a.name: a, grp.relu.name: None}                    # (out does not exist yet)
            if conv_b is not None: stored[conv_b.name] = b
            fed, out, elided = self._epilogue_sinks(grp, hooks, stored, a), None, set()
            if fed is not None:
                jobs = fed[0]
                elided = elidable_stores(grp, hooks, jobs, fed[1].recorder)
                mask = (ELIDE_A if conv_a.name in elided else 0) | (ELIDE_B if conv_b is not None and conv_b.name in elided else 0)
                launch = bias_add_act_hist if next(iter(jobs.values()))[0] == 'hist_rows' else bias_add_act_stats
                out = launch(a, biases[conv_a.name], b, bias_b, True, jobs.get(conv_a.name),
                             jobs.get(conv_b.name) if conv_b is not None else None, jobs.get(grp.relu.name), mask)
                if out is None: fed, elided = None, set()
                else: stored[grp.relu.name] = out
            if out is None: out = bias_add_act(a, biases[conv_a.name], b, bias_b, relu=True)
            if out is None:
                a.add_(biases[conv_a.name].view(1, -1, 1, 1))
                if conv_b is not None: b.add_(biases[conv_b.name].view(1, -1, 1, 1))
                out = F.relu(a + b)
            tail = {conv_a.name: a, grp.add.name: out, grp.relu.name: out}
            if conv_b is not None: tail[conv_b.name] = b
        return self._group_values(grp, hooks, raw_of, tail, stored, fed, elided)

    def _pointwise_epilogue(self, grp: EpilogueGroup, conv: Operation, qin: list, ys: dict, biases: dict, raw_of: Callable, hooks):
        """The fused form of a group whose LAST-EXECUTED convolution `conv` is one the native pointwise kernel takes:
        ffi.conv1x1_epilogue runs the GEMM, the bias(es), the Add, the Relu and the sinks of the group's observers as one launch,
        and the convolution's raw output never exists.  (tail, stored, fed, elided) as ``_run_epilogue`` builds them, or None --
        nothing ran, the caller goes on as if this had not been tried -- unless: the flag is on, the layout is contiguous NCHW,
        `conv` is ``pointwise_eligible`` (so the fused and the unfused forward run it on the same kernel) and its (class, role) is
        not in POINTWISE_KEEP_UNFUSED; the forward has sinks and records nothing; in a P2 group every tensor the launch does not
        store -- `conv`'s biased output and, with two convolutions, the other's -- is in ``elidable_stores``.  The other
        convolution of a two-conv group has run already, without bias: its raw output is the residual, and as float addition
        commutes bit for bit it does not matter which of the two owns the Add."""
        native = self._native_min_work()
        if not self.fuse_pointwise_epilogue or native is None or grp.pool is not None: return None
        x, w = qin[0], qin[1]
        if not pointwise_eligible(x, w, conv.attributes, native): return None
        stride = _square(conv.attributes.get('strides', 1))
        role = 'P1' if grp.kind == 'P1' else ('P2b' if len(grp.convs) == 2 else 'P2')
        if (int(x.shape[1]), int(w.shape[0]), int(x.shape[2]), int(x.shape[3]), stride, role) in POINTWISE_KEEP_UNFUSED: return None
        from .ffi import conv1x1_epilogue
        stored = {grp.relu.name: None}
        if grp.kind == 'P2': stored.update({c.name: None for c in grp.convs})
        fed = self._epilogue_sinks(grp, hooks, stored, x)
        if fed is None or fed[1].recorder is not None: return None
        jobs = fed[0]
        if grp.kind == 'P1':
            out = conv1x1_epilogue(x, w, stride, biases[conv.name], None, None, True, None, None, jobs.get(grp.relu.name))
            if out is None: return None
            return {conv.name: out, grp.relu.name: out}, {grp.relu.name: out}, fed, set()
        others = [c for c in grp.convs if c is not conv]
        if elidable_stores(grp, hooks, jobs, fed[1].recorder) != {c.name for c in grp.convs}: return None
        other = others[0] if others else None
        resid = ys[other.name] if other is not None else raw_of(next(v for v in grp.add.inputs if v.source_op is not conv))
        out = conv1x1_epilogue(x, w, stride, biases[conv.name], resid, biases[other.name] if other is not None else None, True,
                               jobs.get(conv.name), jobs.get(other.name) if other is not None else None, jobs.get(grp.relu.name))
        if out is None: return None
        # `conv`'s own output never exists, yet it has a name in the hook walk: an uninitialised tensor of its shape (no kernel, no
        # traffic) that its observer claims as prepaid without reading, and that nobody can read afterwards (`elided`)
        stored = {conv.name: torch.empty_like(out), grp.relu.name: out}
        if other is not None: stored[other.name] = resid
        tail = {conv.name: stored[conv.name], grp.add.name: out, grp.relu.name: out}
        if other is not None: tail[other.name] = resid
        return tail, stored, fed, {c.name for c in grp.convs}

    def _group_values(self, grp: EpilogueGroup, hooks, raw_of: Callable, tail: dict, stored: dict, fed, elided: set):
        """What follows a group's launch: member by member, in op order, the quantize_function calls and hooks of the unfused loop."""
        if fed is not None:                              # only after a launch that took place
            for name, job in fed[0].items(): fed[1].prepay(stored[name], job[1])
        values: Dict[str, torch.Tensor] = {}
        for op in grp.ops:
            hook = hooks.get(op.name)
            if op.type != 'Conv':                   # Add / Relu / MaxPool: their input side (the launch has computed them already)
                qin = self._input_side(op, [values[v.name] if v.name in values else raw_of(v) for v in op.inputs], hook)
                if tail[op.name] is None: tail[op.name] = _forward(op, qin)      # the MaxPool no launch took in: F.max_pool2d
            for v, y in zip(op.outputs, self._output_side(op, tail[op.name], hook)): values[v.name] = y
        # a tensor the launch did not store still holds the convolution WITHOUT its bias.  The loop above handed it on all the
        # same: to quantize_function, whose config is INITIAL (stat_job hands out jobs for INITIAL configs only) so that it
        # passes the tensor through, and whose result is discarded here; and to the hook, whose observer claimed the prepaid
        # pair without reading it (reads_only_its_job).  Nobody gets to read it afterwards -- the variable has no value
        for name in elided:
            for v in next(m for m in grp.ops if m.name == name).outputs: values[v.name] = None
        return values

    @ staticmethod
    def _epilogue_sinks(grp: EpilogueGroup, hooks, stored: Dict[str, torch.Tensor], like: torch.Tensor):
        """Calibration forwards: ``({member name: job}, queue)`` when the statistic every observer of the group's stored
        outputs is about to queue can ride the epilogue launch instead -- the running range in the min/max phase
        (``('minmax', slots)``: ffi.bias_act_stats_ / bias_add_act_stats), the histogram rows in the histogram phase
        (``('hist_rows', ...)``: ffi.bias_act_hist_ / bias_add_act_hist).  Each such observer has a job (``stat_job``),
        one queue, no side stream, and all jobs of the group are of one kind; None otherwise (no hooks, nothing observed,
        any observer without a job, mixed kinds: today's path).  ``stored``: the members whose output the launch stores;
        ``like``: a tensor on the launch's device."""
        jobs, queue = {}, None
        for op in grp.ops:
            hook = hooks.get(op.name)
            if hook is None or not isinstance(op, QuantableOperation): continue
            for cfg in op.config.output_quantization_config:
                ob = hook._observer_table.get(cfg)
                if ob is None: continue
                if op.name not in stored or op.name in jobs or hook.stream is not None or ob.queue is None: return None
                if queue is not None and ob.queue is not queue: return None
                job = ob.stat_job(like)
                if job is None: return None
                jobs[op.name], queue = job, ob.queue
        if len({job[0] for job in jobs.values()}) > 1: return None
        return (jobs, queue) if jobs else None

    def _quantize_parameter(self, var: Variable, config) -> torch.Tensor:
        """A parameter and its scale do not change between calibration forwards, so its fake-quantised
        value is computed once and kept resident (the reference recomputes it every forward until
        ParameterBakingPass; same values, ppq/executor/torch.py:516-518).  The cache entry is keyed on
        the identity + version of value, scale and offset and on the config state."""
        hit = self._fused.get((var.name, id(config)))
        if hit is not None: return hit
        if not self.cache_parameter_quantization or not QuantizationStates.is_activated(config.state):
            return self.quantize_function(var.value, config)
        key = (var.value.data_ptr(), var.value._version, id(config.scale), config.scale._version,
               id(config.offset), config.offset._version, int(getattr(config.state, 'value', config.state)))
        hit = self._param_cache.get(var.name)
        if hit is not None and hit[0] == key: return hit[1]
        q = self.quantize_function(var.value, config)
        self._param_cache[var.name] = (key, q)
        return q

    @ torch.no_grad()
    def forward_cached(self, inputs, output_names: List[str], cache: Dict[str, torch.Tensor]) -> List[torch.Tensor]:
        """``forward(inputs, output_names)`` that REUSES the quantised activations in ``cache`` (variable name -> tensor) and
        adds every tensor it computes: only the operations between what is cached and what is asked for run.  The values are
        those of ``forward`` as long as the owner drops the entries that depend on parameters / scales it changed
        (blocks.PrefixCache does).  A block-wise pass asks for the inputs of block after block: with the cache the quantised
        prefix of the graph is walked once per batch overall instead of once per block."""
        g = self._graph
        if isinstance(inputs, torch.Tensor): inputs = {next(iter(g.inputs)): inputs}
        elif isinstance(inputs, (list, tuple)): inputs = {k: v for k, v in zip(g.inputs, inputs)}
        for name, value in inputs.items():
            if name not in cache: cache[name] = self._place(value)
        need, stack = set(), [g.variables[n] for n in output_names]
        while stack:
            v = stack.pop()
            if v.name in cache or v.is_parameter: continue
            op = v.source_op
            if op is None: raise ValueError(f'forward_cached: graph input {v.name} was not fed')
            if op.name in need: continue
            need.add(op.name)
            stack.extend(op.inputs)
        ops = [op for op in g.topological_sort() if op.name in need]

        def write(op, outs):
            for v, y in zip(op.outputs, outs): cache[v.name] = y
        if ops:
            self._fused_parameters(ops)
            # what a fused unit never materialised on its own is not cached: it aliases another tensor; a later request recomputes it
            self._walk(ops, None, output_names, lambda v: v.value if v.is_parameter else cache[v.name], write, write_aliases=False)
        return [cache[n] for n in output_names]

    @ torch.no_grad()
    def forward(self, inputs, output_names: List[str] = None, hooks: Dict[str, object] = None) -> List[torch.Tensor]:
        g = self._graph
        if isinstance(inputs, torch.Tensor): inputs = {next(iter(g.inputs)): inputs}
        elif isinstance(inputs, (list, tuple)): inputs = {k: v for k, v in zip(g.inputs, inputs)}
        for name, value in inputs.items(): g.variables[name].value = self._place(value)
        # explicit output names and no hooks: the walk ends with the last requested tensor (a block's quantised inputs need
        # the graph only up to the block; the reference walks on to the end, torch.py:499-570 -- same values)
        stop_early = output_names is not None and not hooks
        if output_names is None: output_names = list(g.outputs)
        results = [None] * len(output_names)
        visited = set()
        self._fused_parameters()

        def finish(op, outs):
            for v, y in zip(op.outputs, outs):
                v.value = y
                if v.name in output_names: results[output_names.index(v.name)] = y
            visited.add(op.name)
            for v in op.inputs:                      # runtime clear, torch.py:564-568
                if not v.is_parameter and all(d.name in visited for d in v.dest_ops): v.value = None
        self._walk(g.topological_sort(), hooks, output_names, lambda v: v.value, finish, hand_packed=True,
                   done=(lambda: all(r is not None for r in results)) if stop_early else None)      # nothing downstream was asked for
        for v in g.variables.values():
            if not v.is_parameter: v.value = None
        return results


# ------------------------------------------------------------------------------------ quantizer
def quantize_graph(graph: BaseGraph, activation_algorithm: str = 'kl', per_channel_weight: bool = True,
                   symmetrical: bool = True, weight_symmetrical: bool = True, num_of_bits: int = 8,
                   hist_bins: int = None, fp8: bool = False, passive_bias: bool = False) -> None:
    """TensorRT-style INT8 policy (TensorRTQuantizer.py:12-107): per-tensor activations on every
    operation, per-channel `minmax` weights on axis 0, FP32 bias; then the state edits of
    QuantizeFusionPass (computing op -> activation, passive ops) and QuantizeSimplifyPass."""
    qmin, qmax = (-(2 ** (num_of_bits - 1)), 2 ** (num_of_bits - 1) - 1) if symmetrical else (0, 2 ** num_of_bits - 1)
    wmin, wmax = (-(2 ** (num_of_bits - 1)), 2 ** (num_of_bits - 1) - 1) if weight_symmetrical else (0, 2 ** num_of_bits - 1)

    def act_cfg():
        if fp8:
            from .core import FloatingQuantizationConfig
            return FloatingQuantizationConfig(calibration='floating')
        c = LinearQuantizationConfig(symmetrical=symmetrical, quant_min=qmin, quant_max=qmax, num_of_bits=num_of_bits,
                                     calibration=activation_algorithm)
        if hist_bins is not None: c.detail['OBSERVER_KL_HIST_BINS_MANUL_OVERRIDE'] = hist_bins
        return c

    for name, op in list(graph.operations.items()):
        in_cfgs = []
        for i, v in enumerate(op.inputs):
            if v.is_parameter and op.type in COMPUTING_OP and i == 1:
                in_cfgs.append(LinearQuantizationConfig(symmetrical=weight_symmetrical, quant_min=wmin, quant_max=wmax,
                                                        num_of_bits=num_of_bits, calibration='minmax',
                                                        channel_axis=0 if per_channel_weight else None))
            elif v.is_parameter and passive_bias and not fp8 and op.type in COMPUTING_OP and i == 2:
                # the integer platforms' policy (PPLQuantizer.py:54-66): a 32-bit symmetric bias whose scale is NOT observed but
                # derived -- input scale x weight scale -- by PassiveParameterQuantizePass once both are calibrated
                in_cfgs.append(LinearQuantizationConfig(symmetrical=True, quant_min=-(2 ** 31 - 1), quant_max=2 ** 31 - 1, num_of_bits=32,
                                                        calibration=None, channel_axis=0 if per_channel_weight else None))
                in_cfgs[-1].state = QuantizationStates.PASSIVE_INIT
            elif v.is_parameter:
                c = act_cfg(); c.state = QuantizationStates.FP32      # bias / norm parameters stay FP32
                in_cfgs.append(c)
            else:
                in_cfgs.append(act_cfg())
        qop = QuantableOperation(op, OperationQuantizationConfig(in_cfgs, [act_cfg() for _ in op.outputs]))
        for v in qop.inputs: v.dest_ops[v.dest_ops.index(op)] = qop
        for v in qop.outputs: v.source_op = qop
        graph.operations[name] = qop
    ops = list(graph.operations.values())
    # The states AND the dominance links the reference's refine passes leave (TensorQuantizationConfig.dominated_by: an
    # OVERLAPPED config reads its root's scale / offset, which is what PassiveParameterQuantizePass multiplies):
    # QuantizeSimplifyPass (optim/refine.py): an input produced by a quantable op is already quantised by its producer
    for op in ops:
        for v, c in zip(op.inputs, op.config.input_quantization_config):
            if v.source_op is not None and is_initial(c):
                src = v.source_op
                c.dominated_by = src.config.output_quantization_config[src.outputs.index(v)]        # -> OVERLAPPED
    # QuantizeFusionPass: computing op followed by a single activation -> the conv output is not quantised on its own (the
    # activation's output config rules it); passive operations share their input's quantisation
    for op in ops:
        out = op.outputs[0]
        if op.type in COMPUTING_OP | {'Add'} and len(out.dest_ops) == 1 and out.dest_ops[0].type in {'Relu', 'Gelu'}:
            op.config.output_quantization_config[0].dominated_by = out.dest_ops[0].config.output_quantization_config[0]
        if op.type in PASSIVE_OPERATIONS:
            first = op.config.input_quantization_config[0]
            if first.dominated_by is not op.config.output_quantization_config[0].dominated_by:
                op.config.output_quantization_config[0].dominated_by = first
            else: op.config.output_quantization_config[0].state = QuantizationStates.OVERLAPPED


from .parameters import ParameterBakingPass, ParameterQuantizePass  # noqa: E402,F401  (kept under their old names here)


# ------------------------------------------------------------------------------------ topologies
def _he(shape, gen) -> torch.Tensor:
    fan_in = shape[1] * (shape[2] * shape[3] if len(shape) == 4 else 1)
    return torch.randn(shape, generator=gen) * (2.0 / fan_in) ** 0.5


def resnet50_graph(seed: int = 0, num_classes: int = 1000) -> BaseGraph:
    """ResNet-50 v1.5 topology, BatchNorm folded into the convolutions (PPQ's FORMATTER_FUSE_BN,
    ppq/core/common.py:40), seeded He-initialised weights, small random biases."""
    gen = torch.Generator().manual_seed(seed)
    g = BaseGraph('resnet50')
    x = g.create_variable('input')
    g.inputs['input'] = x
    n = [0]

    def conv(inp, cin, cout, k, stride=1, pad=0, relu=True, tag='conv'):
        n[0] += 1
        w = g.create_variable(f'{tag}{n[0]}_w', _he([cout, cin, k, k], gen), True)
        b = g.create_variable(f'{tag}{n[0]}_b', torch.randn(cout, generator=gen) * 0.05, True)
        y = g.create_operation('Conv', f'{tag}{n[0]}', [inp, w, b], {'strides': stride, 'pads': pad})
        if relu: y = g.create_operation('Relu', f'relu{n[0]}', [y])
        return y

    y = conv(x, 3, 64, 7, 2, 3)
    y = g.create_operation('MaxPool', 'maxpool', [y], {'kernel_shape': 3, 'strides': 2, 'pads': 1})
    cin = 64
    for stage, (blocks, width) in enumerate(zip([3, 4, 6, 3], [64, 128, 256, 512])):
        for blk in range(blocks):
            stride = 2 if (blk == 0 and stage > 0) else 1
            identity = y
            z = conv(y, cin, width, 1)
            z = conv(z, width, width, 3, stride, 1)
            z = conv(z, width, width * 4, 1, relu=False)
            if blk == 0:
                identity = conv(y, cin, width * 4, 1, stride, 0, relu=False, tag='down')
            n[0] += 1
            z = g.create_operation('Add', f'add{n[0]}', [z, identity])
            y = g.create_operation('Relu', f'relu{n[0]}', [z])
            cin = width * 4
    y = g.create_operation('GlobalAveragePool', 'gap', [y])
    y = g.create_operation('Flatten', 'flatten', [y])
    w = g.create_variable('fc_w', torch.randn([num_classes, 2048], generator=gen) * (1.0 / 2048) ** 0.5, True)
    b = g.create_variable('fc_b', torch.zeros(num_classes), True)
    y = g.create_operation('Gemm', 'fc', [y, w, b])
    g.outputs[y.name] = y
    return g


def yolov6s_graph(seed: int = 0, num_classes: int = 80) -> BaseGraph:
    """A YOLOv6-s-like detector (BASELINE config 5), deploy form: EfficientRep backbone (RepVGG blocks
    re-parameterised to 3x3 Conv + Relu, widths 32-64-128-256-512, repeats 1-2-4-6-2, SPPF-style pooling
    tail), Rep-PAN neck (1x1 reduce, nearest x2 Resize, Concat, Rep blocks; 3x3 stride-2 down path) and a
    decoupled head per scale (1x1 stem, 3x3 + 1x1 class branch, 3x3 + 1x1 box branch): 6 outputs at strides
    8 / 16 / 32.  Seeded He-initialised weights, BatchNorm folded.  Stands in for the ONNX model that cannot be
    loaded here (no `onnx`); what matters to this package is the operator mix the finetuning passes walk:
    plain conv chains, fan-outs that close at a Concat, Resize / MaxPool passive ops, multiple outputs."""
    gen = torch.Generator().manual_seed(seed)
    g = BaseGraph('yolov6s')
    x = g.create_variable('input')
    g.inputs['input'] = x
    n = [0]

    def conv(inp, cin, cout, k=3, stride=1, relu=True, tag='conv'):
        n[0] += 1
        # He-UNIFORM weights: every output channel spreads over its whole per-channel range, so INT4 (16 levels)
        # keeps information in nearly every weight -- like a trained, quantisation-aware detector, and unlike a
        # raw re-parameterised RepVGG kernel whose identity tap would own the range and round the rest to zero
        a = (6.0 / (cin * k * k)) ** 0.5
        w = g.create_variable(f'{tag}{n[0]}_w', (torch.rand([cout, cin, k, k], generator=gen) * 2 - 1) * a, True)
        b = g.create_variable(f'{tag}{n[0]}_b', torch.randn(cout, generator=gen) * 0.05, True)
        y = g.create_operation('Conv', f'{tag}{n[0]}', [inp, w, b], {'strides': stride, 'pads': k // 2})
        if relu: y = g.create_operation('Relu', f'relu{n[0]}', [y])
        return y

    def rep(inp, c, repeats):
        for _ in range(repeats): inp = conv(inp, c, c, 3, tag='rep')
        return inp

    def cat(name, vs): return g.create_operation('Concat', name, vs, {'axis': 1})

    y = conv(x, 3, 32, 3, 2, tag='stem')                         # stride 2
    feats, cin = [], 32
    for stage, (c, r) in enumerate(zip([64, 128, 256, 512], [2, 4, 6, 2])):
        y = conv(y, cin, c, 3, 2, tag=f's{stage}_down')
        y = rep(y, c, r)
        cin = c
        feats.append(y)                                          # strides 4, 8, 16, 32
    # SPPF-style tail on the stride-32 feature
    p = conv(feats[3], 512, 256, 1, tag='sppf_in')
    m1 = g.create_operation('MaxPool', 'sppf_pool1', [p], {'kernel_shape': 5, 'strides': 1, 'pads': 2})
    m2 = g.create_operation('MaxPool', 'sppf_pool2', [m1], {'kernel_shape': 5, 'strides': 1, 'pads': 2})
    m3 = g.create_operation('MaxPool', 'sppf_pool3', [m2], {'kernel_shape': 5, 'strides': 1, 'pads': 2})
    c5 = conv(cat('sppf_cat', [p, m1, m2, m3]), 1024, 512, 1, tag='sppf_out')
    c3, c4 = feats[1], feats[2]                                  # 128 @ s8, 256 @ s16
    # Rep-PAN: top-down
    r5 = conv(c5, 512, 128, 1, tag='reduce5')
    u5 = g.create_operation('Resize', 'up5', [r5], {'scale': 2})
    p4 = rep(conv(cat('cat_p4', [u5, c4]), 128 + 256, 128, 3, tag='p4_in'), 128, 3)
    r4 = conv(p4, 128, 64, 1, tag='reduce4')
    u4 = g.create_operation('Resize', 'up4', [r4], {'scale': 2})
    p3 = rep(conv(cat('cat_p3', [u4, c3]), 64 + 128, 64, 3, tag='p3_in'), 64, 3)          # out @ s8
    # bottom-up
    d3 = conv(p3, 64, 64, 3, 2, tag='down3')
    n4 = rep(conv(cat('cat_n4', [d3, r4]), 64 + 64, 128, 3, tag='n4_in'), 128, 3)         # out @ s16
    d4 = conv(n4, 128, 128, 3, 2, tag='down4')
    n5 = rep(conv(cat('cat_n5', [d4, r5]), 128 + 128, 256, 3, tag='n5_in'), 256, 3)       # out @ s32
    for name, f, c in (('s8', p3, 64), ('s16', n4, 128), ('s32', n5, 256)):
        stem = conv(f, c, c, 1, tag=f'head_{name}_stem')
        cls = conv(conv(stem, c, c, 3, tag=f'head_{name}_cls'), c, num_classes, 1, relu=False, tag=f'head_{name}_cls_out')
        box = conv(conv(stem, c, c, 3, tag=f'head_{name}_box'), c, 4, 1, relu=False, tag=f'head_{name}_box_out')
        g.outputs[cls.name] = cls
        g.outputs[box.name] = box
    _unit_variance_init(g, torch.rand(2, 3, 96, 96, generator=gen))
    return g


@ torch.no_grad()
def _unit_variance_init(g: BaseGraph, sample: torch.Tensor) -> None:
    """Layer-sequential unit-variance rescaling of the seeded weights (a trained, BatchNorm-folded detector has
    O(1) activations everywhere; 56 unnormalised He-initialised convolutions in a row do not: the positive mean
    of ReLU outputs compounds to 1e10).  One CPU forward on a seeded sample; every Conv's weight and bias are
    divided by the standard deviation of its output.  Deterministic in `seed`."""
    values = {next(iter(g.inputs)): sample}
    for op in g.operations.values():
        xs = [v.value if v.is_parameter else values[v.name] for v in op.inputs]
        y = _forward(op, xs)
        if op.type == 'Conv':
            std = float(y.std())
            if std > 0:
                op.inputs[1].value = op.inputs[1].value / std
                if len(op.inputs) > 2: op.inputs[2].value = op.inputs[2].value / std
                y = y / std
        values[op.outputs[0].name] = y


def small_cnn_graph(seed: int = 0, width: int = 16) -> BaseGraph:
    """Conv-Relu-Conv-Add-Relu-GAP-Gemm: a tiny graph for smoke / parity tests."""
    gen = torch.Generator().manual_seed(seed)
    g = BaseGraph('small_cnn')
    x = g.create_variable('input'); g.inputs['input'] = x

    def conv(inp, cin, cout, name, relu):
        w = g.create_variable(name + '_w', _he([cout, cin, 3, 3], gen), True)
        b = g.create_variable(name + '_b', torch.randn(cout, generator=gen) * 0.1, True)
        y = g.create_operation('Conv', name, [inp, w, b], {'strides': 1, 'pads': 1})
        return g.create_operation('Relu', name + '_relu', [y]) if relu else y

    a = conv(x, 3, width, 'c1', True)
    b_ = conv(a, width, width, 'c2', False)
    s = g.create_operation('Add', 'add', [b_, a])
    s = g.create_operation('Relu', 'add_relu', [s])
    p = g.create_operation('GlobalAveragePool', 'gap', [s])
    f = g.create_operation('Flatten', 'flatten', [p])
    w = g.create_variable('fc_w', torch.randn([10, width], generator=gen) * 0.3, True)
    bb = g.create_variable('fc_b', torch.zeros(10), True)
    y = g.create_operation('Gemm', 'fc', [f, w, bb])
    g.outputs[y.name] = y
    return g


def transformer_mlp_graph(seed: int = 0, dim: int = 64, hidden: int = 256) -> BaseGraph:
    """LayerNorm -> Gemm -> Gelu -> Gemm -> Add(residual): the MLP half of a ViT block, the operator
    mix BASELINE config 4 (ViT-B/16, FP8 E4M3) exercises."""
    gen = torch.Generator().manual_seed(seed)
    g = BaseGraph('transformer_mlp')
    x = g.create_variable('input'); g.inputs['input'] = x
    gamma = g.create_variable('ln_w', torch.ones(dim) + torch.randn(dim, generator=gen) * 0.05, True)
    beta = g.create_variable('ln_b', torch.randn(dim, generator=gen) * 0.05, True)
    h = g.create_operation('LayerNormalization', 'ln', [x, gamma, beta])
    w1 = g.create_variable('fc1_w', torch.randn([hidden, dim], generator=gen) * (1.0 / dim) ** 0.5, True)
    b1 = g.create_variable('fc1_b', torch.zeros(hidden), True)
    h = g.create_operation('Gemm', 'fc1', [h, w1, b1])
    h = g.create_operation('Gelu', 'gelu', [h])
    w2 = g.create_variable('fc2_w', torch.randn([dim, hidden], generator=gen) * (1.0 / hidden) ** 0.5, True)
    b2 = g.create_variable('fc2_b', torch.zeros(dim), True)
    h = g.create_operation('Gemm', 'fc2', [h, w2, b2])
    y = g.create_operation('Add', 'residual', [h, x])
    g.outputs[y.name] = y
    return g


def vit_graph(seed: int = 0, depth: int = 12, dim: int = 768, heads: int = 12, mlp_dim: int = 3072, patch: int = 16,
              image: int = 224, num_classes: int = 1000) -> BaseGraph:
    """ViT-B/16 topology (BASELINE config 4): patch-embedding Conv, class token + position embedding,
    `depth` pre-norm blocks (LayerNorm -> QKV Gemm -> scaled-dot-product attention with two MatMul ->
    projection Gemm -> residual; LayerNorm -> Gemm -> Gelu -> Gemm -> residual), final LayerNorm, head.
    Seeded random weights (no onnx / checkpoints in the image)."""
    gen = torch.Generator().manual_seed(seed)
    g = BaseGraph('vit')
    tokens, hd = (image // patch) ** 2 + 1, dim // heads

    def param(name, *shape, std=None, ones=False):
        if ones: val = torch.ones(*shape)
        elif std == 0: val = torch.zeros(*shape)
        else: val = torch.randn(*shape, generator=gen) * (std if std is not None else (1.0 / shape[-1]) ** 0.5)
        return g.create_variable(name, val, True)

    def gemm(inp, name, cin, cout):
        return g.create_operation('Gemm', name, [inp, param(name + '_w', cout, cin), param(name + '_b', cout, std=0)])

    def layer_norm(inp, name):
        return g.create_operation('LayerNormalization', name, [inp, param(name + '_w', dim, ones=True), param(name + '_b', dim, std=0)])
    x = g.create_variable('input'); g.inputs['input'] = x
    h = g.create_operation('Conv', 'patch_embed', [x, param('patch_w', dim, 3, patch, patch, std=(1.0 / (3 * patch * patch)) ** 0.5),
                                                  param('patch_b', dim, std=0)], {'strides': patch})
    h = g.create_operation('Reshape', 'patch_flat', [h], {'shape': (-1, dim, tokens - 1)})
    h = g.create_operation('Transpose', 'patch_tokens', [h], {'perm': (0, 2, 1)})
    h = g.create_operation('Concat', 'cat_cls', [param('cls_token', 1, 1, dim, std=0.02), h], {'axis': 1})
    h = g.create_operation('Add', 'add_pos', [h, param('pos_embed', 1, tokens, dim, std=0.02)])
    for i in range(depth):
        p = f'blk{i}_'
        a = layer_norm(h, p + 'ln1')
        qkv = gemm(a, p + 'qkv', dim, 3 * dim)
        parts = []
        for k, nm in enumerate('qkv'):
            t = g.create_operation('Slice', p + nm + '_slice', [qkv], {'axis': 2, 'start': k * dim, 'length': dim})
            t = g.create_operation('Reshape', p + nm + '_heads', [t], {'shape': (-1, tokens, heads, hd)})
            parts.append(g.create_operation('Transpose', p + nm + '_t', [t], {'perm': (0, 2, 3, 1) if nm == 'k' else (0, 2, 1, 3)}))
        att = g.create_operation('MatMul', p + 'qk', [parts[0], parts[1]])
        att = g.create_operation('Mul', p + 'scale', [att], {'value': hd ** -0.5})
        att = g.create_operation('Softmax', p + 'softmax', [att], {'axis': -1})
        ctx = g.create_operation('MatMul', p + 'av', [att, parts[2]])
        ctx = g.create_operation('Transpose', p + 'ctx_t', [ctx], {'perm': (0, 2, 1, 3)})
        ctx = g.create_operation('Reshape', p + 'ctx', [ctx], {'shape': (-1, tokens, dim)})
        h = g.create_operation('Add', p + 'res1', [gemm(ctx, p + 'proj', dim, dim), h])
        m = layer_norm(h, p + 'ln2')
        m = g.create_operation('Gelu', p + 'gelu', [gemm(m, p + 'fc1', dim, mlp_dim)])
        h = g.create_operation('Add', p + 'res2', [gemm(m, p + 'fc2', mlp_dim, dim), h])
    h = layer_norm(h, 'ln_f')
    h = g.create_operation('Slice', 'cls_out', [h], {'axis': 1, 'start': 0, 'length': 1})
    h = g.create_operation('Reshape', 'cls_flat', [h], {'shape': (-1, dim)})
    y = gemm(h, 'head', dim, num_classes)
    g.outputs[y.name] = y
    return g


def quantize_graph_fp8(graph: BaseGraph, exponent: int = 4, mantissa: int = 3, operations=None) -> None:
    """TRT_FP8-style policy (quantizer/FP8Quantizer.py:107-200): only the inputs of Conv / Gemm / MatMul
    are quantised -- activations per tensor with the power-of-2 'floating' observer, weights per
    channel (axis 0) with the same observer; everything else stays FP32.  `operations`: names of the
    operations a dispatcher chose to quantise (default: all; the reference's 'conservative' dispatcher
    leaves everything downstream of a non-quantable type such as Add on the FP32 platform)."""
    from .core import FloatingQuantizationConfig
    qmax = 448.0 if (exponent, mantissa) == (4, 3) else 57344.0
    for name, op in list(graph.operations.items()):
        if operations is not None and name not in operations: continue
        in_cfgs = []
        for i, v in enumerate(op.inputs):
            c = FloatingQuantizationConfig(exponent=exponent, mantissa=mantissa, quant_min=-qmax, quant_max=qmax,
                                           calibration='floating',
                                           channel_axis=0 if (v.is_parameter and i == 1) else None)
            if op.type not in COMPUTING_OP or (v.is_parameter and i != 1): c.state = QuantizationStates.FP32
            in_cfgs.append(c)
        outs = []
        for _ in op.outputs:
            c = FloatingQuantizationConfig(exponent=exponent, mantissa=mantissa, quant_min=-qmax, quant_max=qmax)
            c.state = QuantizationStates.FP32
            outs.append(c)
        qop = QuantableOperation(op, OperationQuantizationConfig(in_cfgs, outs))
        for v in qop.inputs: v.dest_ops[v.dest_ops.index(op)] = qop
        for v in qop.outputs: v.source_op = qop
        graph.operations[name] = qop
