"""Round tuning -- the reference's current weight-rounding finetune (``RoundTuningPass``).

Mirror of ppq/quantization/algorithm/training.py:490-590 (``TensorwiseRoundTuningImpl`` / ``ChannelwiseRoundTuningImpl``,
``RoundTruningDelegator`` -- the reference's spelling, exported here too) and of ppq/quantization/optim/training.py:866-1034
(``RoundTuningPass``).  The delegator's forward is ONE HIP kernel (csrc/roundtune.hip) for every round-tuned weight of a block
(:class:`RoundTuningGroup`), where the reference's torch delegator issues 7 elementwise kernels per weight; its backward is
the identity, so there is no backward launch: autograd hands ``dy`` to R as it is.  The one-time expressions (R, the floored
weight, ``finalize``) stay the reference's torch code.  HIP path only: a CPU tensor raises.

The decisions taken where the reference is unusable are listed in INTEGRATION.md section 6."""
from typing import Any, List

import torch
from torch.autograd import Function

from .blocks import compute_block_loss, torch_mean_square_error
from .core import QuantizationProperty as P
from .core import QuantizationStates, state_value
from .ffi import roundtune_forward_multi
from .lsq import BlockTraining, LaunchGroup, LearnedStepSizePass, _channel_axis

ROUND_TUNING_OP = {'Gemm', 'MatMul', 'ConvTranspose', 'PPQBiasFusedMatMul', 'Conv'}           # optim/training.py:929


class _RoundTuneFunction(Function):
    """One weight, one job of the kernel: forward = RoundTruningDelegator.__call__, backward = training.py:502-504 (``dy`` for
    the tensor and ``dy`` for R, nothing else)."""
    @ staticmethod
    def forward(ctx, tensor, rounding, scale, offset, axis, quant_min: int, quant_max: int) -> torch.Tensor:
        item = (tensor.detach(), rounding.detach(), scale.detach(), offset.detach(), axis, quant_min, quant_max)
        return roundtune_forward_multi([item])[0]

    @ staticmethod
    def backward(ctx, dy: torch.Tensor):
        return dy, dy, None, None, None, None, None


class _GroupedRound(Function):
    """A member of a :class:`RoundTuningGroup` or an ``MXRoundTuningGroup``: forward hands out what the group's ONE launch
    wrote, backward is the same identity -- autograd installs ``dy`` as the rounding's ``.grad`` and sums when one weight is read
    twice in a forward."""
    @ staticmethod
    def forward(ctx, tensor, rounding, group, slot: int) -> torch.Tensor:
        return group.outputs[slot].detach()

    @ staticmethod
    def backward(ctx, dy: torch.Tensor):
        return dy, dy, None, None


class RoundTuningGroup(LaunchGroup):
    """The round-tuning delegators of one block as ONE ``ppqhip_roundtune_fwd_multi`` launch per step (:meth:`prepare`).
    Outputs are allocated once, so a captured HIP graph of the step finds them at fixed addresses.  dR = dy exactly, so there
    is no backward launch."""
    def __init__(self, members):
        super().__init__(members)
        self.outs = [torch.empty_like(v.value) for _, _, v in members]

    @ staticmethod
    def eligible(delegator, config, var) -> bool:
        w = var.value
        return (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
                and isinstance(config.scale, torch.Tensor) and isinstance(config.offset, torch.Tensor)
                and config.scale.is_contiguous() and config.offset.is_contiguous())

    def prepare(self) -> None:
        """Start of a step: the delegator's forward of every member (ONE launch)."""
        items = [(v.value.detach(), d.rounding.detach(), c.scale.detach(), c.offset.detach(), _channel_axis(c), c.quant_min,
                  c.quant_max) for d, c, v in self.members]
        self.outputs = roundtune_forward_multi(items, outs=self.outs)
        self.launches += 1


class RoundTuningDelegator:
    """training.py:529-590 (the TorchQuantizeDelegator protocol: ``__call__(tensor, config)``).  Construction REPLACES
    ``var.value`` by the floored weight ``floor(W / s) * s`` and keeps the original for :meth:`withdraw`."""
    def __init__(self, var, config) -> None:
        self.config = config
        self.var = var
        self.is_parameter = self.var.is_parameter

        if config.policy.has_property(P.FLOATING):
            raise TypeError('Incorrect Quantization Property. Except Linear Quantization Policy.')
        if config.policy.has_property(P.DYNAMIC):
            raise TypeError('Incorrect Quantization Property. Except Static Quantization Policy.')
        if not self.var.is_parameter:
            raise TypeError(f'Variable {self.var.name} is not a parameter!')
        if self.var.value is None or not isinstance(self.var.value, torch.Tensor):
            raise ValueError(f'Unexpected value type of {self.var.name}')
        if self.config.scale is None:
            raise ValueError('Quantization Scale has not been correctly set.')

        self._param_backup = self.var.value.detach().clone()
        with torch.no_grad():
            scale = config.scale
            if config.policy.has_property(P.PER_CHANNEL):
                shape = [1 if axis != config.channel_axis else -1 for axis in range(self.var.value.ndim)]
                scale = scale.view(shape)
            rounding = (self.var.value / scale) - (self.var.value / scale).floor()
            self.var.value = (self.var.value / scale).floor() * scale
            self._scale = scale
            self._initial_up = rounding > .5                # for RoundTuningPass.stats['flipped']
        self._rounding = rounding
        self._rounding.requires_grad = True
        self.group, self.slot = None, None                  # set by RoundTuningGroup: this weight rides the block's launch

    @ property
    def rounding(self) -> torch.Tensor:
        return self._rounding

    def trainable_tensors(self) -> List[torch.Tensor]:
        return [self._rounding]

    def flipped(self) -> torch.Tensor:
        """How many elements are on the other side of .5 than their initial R (a device scalar)."""
        with torch.no_grad():
            return ((self._rounding > .5) != self._initial_up).sum()

    def finalize(self) -> None:
        with torch.no_grad():
            self.var.value += (self._rounding > .5) * self._scale

    def withdraw(self) -> None:
        with torch.no_grad():
            self.var.value.copy_(self._param_backup)

    def __call__(self, tensor: torch.Tensor, config) -> torch.Tensor:
        if self.group is not None and self.group.outputs is not None and tensor is self.var.value:
            return _GroupedRound.apply(tensor, self._rounding, self.group, self.slot)
        if not tensor.is_contiguous(): tensor = tensor.contiguous()
        return _RoundTuneFunction.apply(tensor, self._rounding, config.scale, config.offset, _channel_axis(config),
                                        config.quant_min, config.quant_max)


RoundTruningDelegator = RoundTuningDelegator                # the reference's spelling (training.py:529)


def _train_bias(op, job: BlockTraining) -> None:
    """The bias of a three-input op is trained as it is (optim/training.py:944-947).  The reference keeps no backup of it (b);
    the frame does: it is a trained tensor no delegator answers for."""
    if len(op.inputs) != 3: return
    bias = op.inputs[-1]
    if bias.is_parameter and isinstance(bias.value, torch.Tensor) and bias.value.is_floating_point():
        bias.value.requires_grad = True
        job.tensors.append(bias.value)


class RoundTuningPass(LearnedStepSizePass):
    """optim/training.py:866-1034: block-wise round tuning (``block_size`` = the reference's depth limit, default 5) on
    ``LearnedStepSizePass.finetune``'s frame.  What is this pass's own:

    * the pre-loss is ``torch_mean_square_error``, the step loss and the post-loss the sum of ``torch.nn.MSELoss()`` over the
      block outputs;
    * a :class:`RoundTuningDelegator` on the weight of every Conv / ConvTranspose / Gemm / MatMul / PPQBiasFusedMatMul whose
      config is ACTIVATED with a tensor scale; the bias of a three-input op is trained as it is;
    * a block that ended worse gets its weights AND biases back bit for bit, any other block is finalised:
      ``W = floor(W / s) * s + (R > .5) * s``.

    ``group_weights``: the block's weights in ONE launch per step.  ``stats['flipped']`` of ``stats['tuned_elements']`` weight elements of the kept blocks ended on the other side of .5 than
    they started: with the default lr and steps R moves by a few hundredths at most, so this is what tells whether the pass
    did anything."""
    def __init__(self, interested_layers: List[str] = [], steps: int = 500, lr: float = 1e-4, block_size: int = 5,
                 expire_device: str = 'cpu', collecting_device: str = 'cuda', optimizer: Any = None, *,
                 group_weights: bool = True, use_hip_graph: bool = True, fused_adam: bool = True):
        super().__init__(name='PPQ Rounding Tuning Pass', interested_layers=list(interested_layers or []), steps=steps, lr=lr,
                         block_size=block_size, expire_device=expire_device, collecting_device=collecting_device,
                         optimizer=optimizer, group_weights=group_weights, use_hip_graph=use_hip_graph, fused_adam=fused_adam)
        self.expire_device, self.collecting_device = expire_device, collecting_device
        self.loss_fn = torch.nn.MSELoss()
        self.stats.update(roundtune_weights=0, skipped_weights=0, flipped=0, tuned_elements=0)
        self.keep_roundings = False                 # an inspection aid: True keeps every trained R (weight name -> tensor) in
        self.roundings = {}                         # `roundings`, taken before the block finalises or withdraws

    def optimize(self, graph, dataloader, executor, collate_fn=None, **kwargs):
        self.roundings = {}
        return super().optimize(graph, dataloader, executor, collate_fn=collate_fn, **kwargs)

    def _check_block(self, block) -> None:
        if self._world() != 1:
            raise ValueError('RoundTuningPass runs in one process: data-parallel round tuning is not supported')

    def _delegate(self, block, executor, job: BlockTraining) -> None:
        """optim/training.py:926-947."""
        for op in block.rps:
            if not hasattr(op, 'config') or op.type not in ROUND_TUNING_OP: continue
            if len(op.inputs) > 1 and op.inputs[1].is_parameter:
                cfg, var = op.config.input_quantization_config[1], op.inputs[1]
                if cfg.policy.has_property(P.FLOATING) or cfg.policy.has_property(P.DYNAMIC):
                    RoundTuningDelegator(config=cfg, var=var)          # raises the reference's TypeError, touches nothing
                if not isinstance(cfg.scale, torch.Tensor) or state_value(cfg.state) != QuantizationStates.ACTIVATED.value:
                    self.stats['skipped_weights'] += 1                 # (d): never floored, never delegated
                elif cfg not in job.delegators:
                    if not (isinstance(var.value, torch.Tensor) and var.value.is_cuda):
                        raise TypeError(f'RoundTuningPass: {var.name} is not a CUDA tensor (ppq_amd has no CPU path)')
                    job.register(executor, cfg, RoundTuningDelegator(config=cfg, var=var))
            _train_bias(op, job)

    # The hooks from here to _settle are MXRoundTuningPass's too (it takes them as they are): what differs is named by
    # _group_class, _weights_stat and _keep.
    _group_class, _weights_stat = RoundTuningGroup, 'roundtune_weights'

    def _pre_loss(self, block, qt_inputs, fp_outputs, executor) -> float:
        return compute_block_loss(block, qt_inputs, fp_outputs, executor, torch_mean_square_error)

    def _post_loss(self, block, qt_inputs, fp_outputs, executor) -> float:
        return compute_block_loss(block, qt_inputs, fp_outputs, executor, self.loss_fn)      # training.py:982-984

    def _build_groups(self, block, job: BlockTraining, uniq) -> None:
        every = [(d, cfg, d.var) for cfg, d in job.delegators.items()]
        self.stats[self._weights_stat] += len(every)
        members = [m for m in every if self._group_class.eligible(*m)] if self.group_weights else []
        if members: job.groups = [self._group_class(members)]

    def _step_loss(self, block, names, outs, fp_output):
        loss = 0.0
        for n, y in zip(names, outs): loss += self.loss_fn(y, fp_output[n])
        return loss

    def _settle(self, job: BlockTraining, worse: bool) -> None:
        """A block that ended worse gets its weights back (the frame: its biases), any other is finalised -- (a): a withdrawn
        block is NOT finalised -- and counted in ``stats``."""
        if self.keep_roundings: self.roundings.update({d.var.name: d.rounding.detach().clone() for d in job.delegators.values()})
        flipped = []
        for d in job.delegators.values():
            if worse: d.withdraw(); continue
            flipped.append(self._keep(d))
            self.stats['tuned_elements'] += d.rounding.numel()
        if flipped: self.stats['flipped'] += int(torch.stack(flipped).sum())

    @ staticmethod
    def _keep(delegator) -> torch.Tensor:
        """Finalise ``delegator``; returns its ``flipped()``."""
        delegator.finalize()
        return delegator.flipped()
