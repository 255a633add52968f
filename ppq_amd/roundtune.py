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

from .blocks import block_forward, compute_block_loss, torch_mean_square_error
from .core import QuantizationProperty as P
from .core import QuantizationStates, state_value
from .ffi import roundtune_forward_multi
from .lsq import LearnedStepSizePass

ROUND_TUNING_OP = {'Gemm', 'MatMul', 'ConvTranspose', 'PPQBiasFusedMatMul', 'Conv'}           # optim/training.py:929


def _channel_axis(config):
    return config.channel_axis if config.policy.has_property(P.PER_CHANNEL) else None


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


class _GroupedRoundTune(Function):
    """A member of a :class:`RoundTuningGroup`: forward hands out what the group's ONE launch wrote, backward is the same
    identity -- autograd installs ``dy`` as R's ``.grad`` and sums when one weight is read twice in a forward."""
    @ staticmethod
    def forward(ctx, tensor, rounding, group, slot: int) -> torch.Tensor:
        return group.outputs[slot].detach()

    @ staticmethod
    def backward(ctx, dy: torch.Tensor):
        return dy, dy, None, None


class RoundTuningGroup:
    """The round-tuning delegators of one block as ONE ``ppqhip_roundtune_fwd_multi`` launch per step (:meth:`prepare`).
    Outputs are allocated once, so a captured HIP graph of the step finds them at fixed addresses.  dR = dy exactly, so
    :meth:`flush` has nothing to launch (it is there for the group protocol of the block-wise passes)."""
    def __init__(self, members):
        self.members = members                              # [(delegator, config, var)]
        self.outs = [torch.empty_like(v.value) for _, _, v in members]
        self.outputs = None
        self.launches = 0
        for k, (d, _, _) in enumerate(members): d.group, d.slot = self, k

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

    def flush(self) -> None:
        """End of the backward sweep: nothing to do, every R already holds its ``dy``."""

    def release(self) -> None:
        for d, _, _ in self.members: d.group, d.slot = None, None


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
            return _GroupedRoundTune.apply(tensor, self._rounding, self.group, self.slot)
        if not tensor.is_contiguous(): tensor = tensor.contiguous()
        return _RoundTuneFunction.apply(tensor, self._rounding, config.scale, config.offset, _channel_axis(config),
                                        config.quant_min, config.quant_max)


RoundTruningDelegator = RoundTuningDelegator                # the reference's spelling (training.py:529)


class RoundTuningPass(LearnedStepSizePass):
    """optim/training.py:866-1034: block-wise round tuning.  Per block (``block_size`` = the reference's depth limit, default 5):

    1. ``pre_loss`` (``torch_mean_square_error``), before any delegator exists;
    2. a :class:`RoundTuningDelegator` on the weight of every Conv / ConvTranspose / Gemm / MatMul / PPQBiasFusedMatMul whose
       config is ACTIVATED with a tensor scale; the bias of a three-input op is trained as it is;
    3. ``steps`` of Adam(lr) (or the user's optimizer class) on the sum of ``torch.nn.MSELoss()`` over the block outputs;
    4. ``post_loss`` (``MSELoss``) with the delegators still registered; a block that ended worse gets its weights AND biases
       back bit for bit, any other block is finalised: ``W = floor(W / s) * s + (R > .5) * s``.

    The MI355X-side execution choices are LearnedStepSizePass's: the block's weights in ONE launch per step
    (``group_weights``), the step captured once as a HIP graph with the capturable Adam and replayed (``use_hip_graph``;
    ``use_hip_graph=False`` is the reference's optimizer).  ``report`` = [(block, pre_loss, post_loss)];
    ``stats['flipped']`` of ``stats['tuned_elements']`` weight elements of the kept blocks ended on the other side of .5 than
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

    def finetune(self, block, executor, qt_inputs, fp_outputs):
        """optim/training.py:910-999 for one block."""
        self._check_block(block)
        if len(qt_inputs) == 0: raise ValueError('Dataset is empty.')
        self.enable_block_gradient(block)
        with self._phase('pre_loss'):
            pre_loss = compute_block_loss(block, qt_inputs, fp_outputs, executor, torch_mean_square_error)

        delegators, tensors, biases = {}, [], []
        try:
            for op in block.rps:
                if not hasattr(op, 'config') or op.type not in ROUND_TUNING_OP: continue
                if len(op.inputs) > 1 and op.inputs[1].is_parameter:
                    cfg, var = op.config.input_quantization_config[1], op.inputs[1]
                    if cfg.policy.has_property(P.FLOATING) or cfg.policy.has_property(P.DYNAMIC):
                        RoundTuningDelegator(config=cfg, var=var)          # raises the reference's TypeError, touches nothing
                    if not isinstance(cfg.scale, torch.Tensor) or state_value(cfg.state) != QuantizationStates.ACTIVATED.value:
                        self.stats['skipped_weights'] += 1                 # (d): never floored, never delegated
                    elif cfg not in delegators:
                        if not (isinstance(var.value, torch.Tensor) and var.value.is_cuda):
                            raise TypeError(f'RoundTuningPass: {var.name} is not a CUDA tensor (ppq_amd has no CPU path)')
                        d = RoundTuningDelegator(config=cfg, var=var)
                        tensors.append(d.rounding)
                        executor.register_quantize_delegate(cfg, d)
                        delegators[cfg] = d
                if len(op.inputs) == 3 and op.inputs[-1].is_parameter and isinstance(op.inputs[-1].value, torch.Tensor) \
                        and op.inputs[-1].value.is_floating_point():
                    op.inputs[-1].value.requires_grad = True
                    tensors.append(op.inputs[-1].value)
                    biases.append(op.inputs[-1].value)
        except Exception:                                  # (c): a refusal half-way leaves the block as it was found
            for cfg, d in delegators.items():
                d.withdraw(); executor.remove_quantize_delegate(cfg)
            self.disable_block_gradient(block)
            raise
        uniq, seen = [], set()
        for t in tensors:
            if t.requires_grad and id(t) not in seen: seen.add(id(t)); uniq.append(t)
        if not uniq:                                       # (c): nothing stays requires_grad on the early exit
            for cfg in delegators: executor.remove_quantize_delegate(cfg)
            self.disable_block_gradient(block)
            return 0.0, 0.0
        loose = [(t, t.detach().clone()) for t in uniq if any(t is b for b in biases)]     # (b): the reference has no backup

        names = [v.name for v in block.ep.outputs]
        every = [(d, cfg, d.var) for cfg, d in delegators.items()]
        members = [m for m in every if RoundTuningGroup.eligible(*m)] if self.group_weights else []
        group = RoundTuningGroup(members) if members else None
        self.stats['blocks'] += 1
        self.stats['roundtune_weights'] += len(every)
        self.stats['grouped_weights'] += len(members)
        graphable = self._graphable(qt_inputs, fp_outputs, uniq)
        opt = self._make_optimizer(uniq, graphable)

        def train_step(qt_input, fp_output) -> None:
            opt.zero_grad()
            if group is not None: group.prepare()
            with torch.enable_grad():
                outs = block_forward(executor, block.rps, qt_input, names, with_gradient=True)
                loss = 0.0
                for n, y in zip(names, outs): loss += self.loss_fn(y, fp_output[n])
            loss.backward()
            if group is not None: group.flush()
            opt.step()

        try:
            done = self._train_with_graph(train_step, qt_inputs, fp_outputs) if graphable else 0
            with self._phase('eager_steps'):
                for step in range(done, self.steps):
                    train_step(qt_inputs[step % len(qt_inputs)], fp_outputs[step % len(qt_inputs)])
                    self.stats['eager_steps'] += 1
        finally:
            if group is not None: group.outputs = None  # stale after the last optimizer step: one job per weight from here
        with self._phase('post_loss'):                 # measured with the delegators still registered (training.py:982-984)
            post_loss = compute_block_loss(block, qt_inputs, fp_outputs, executor, self.loss_fn)
        if group is not None: group.release()
        if self.keep_roundings: self.roundings.update({d.var.name: d.rounding.detach().clone() for d, _, _ in every})
        keep = not post_loss > pre_loss
        flipped = []
        for cfg, d in delegators.items():
            if keep:
                d.finalize()                               # (a): a withdrawn block is NOT finalised
                flipped.append(d.flipped())
                self.stats['tuned_elements'] += d.rounding.numel()
            else: d.withdraw()
            executor.remove_quantize_delegate(cfg)
            d.rounding.grad = None
        if flipped: self.stats['flipped'] += int(torch.stack(flipped).sum())
        if not keep:
            with torch.no_grad():
                for t, backup in loose: t.copy_(backup)
        self.disable_block_gradient(block)
        return pre_loss, post_loss
