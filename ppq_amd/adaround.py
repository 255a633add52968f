"""AdaRound -- block-wise reconstruction with learned weight rounding (the reference's ``blockwise_reconstruction`` setting).

Mirror of ppq/quantization/optim/legacy.py: ``TimeDecay`` (:22-33), ``AdaroundRegTerm`` (:36-64), ``AdaRoundDelegator``
(:67-136) and ``AdaroundPass`` (:139-297).  The delegator's forward (soft-rounded fake quant of a weight) and the gradient of V
through it, with the regulariser's gradient fused in, are two HIP kernels (csrc/adaround.hip): every AdaRound weight of a block
in ONE forward and ONE backward launch per step (:class:`AdaroundGroup`), where the reference's torch delegator issues about 11
elementwise kernels forward and 15-20 backward per weight.  The one-time expressions (``initiate_rounding``, ``finalize``) stay
the reference's torch code.  HIP path only: a CPU tensor raises.

The quirks of the reference that are reproduced, and the decisions taken where it is unusable, are listed in INTEGRATION.md
section 6."""
from typing import List

import numpy as np
import torch
from torch.autograd import Function

from .blocks import COMPUTING_OP, torch_mean_square_error
from .core import QuantizationProperty as P
from .core import QuantizationStates, rounding_value, state_value
from .ffi import adaround_backward_multi, adaround_forward_multi
from .lsq import (BlockTraining, LaunchGroup, LearnedStepSizePass, LSQActivationGroup, LSQDelegator, LSQWeightGroup, _channel_axis,
                  _unique)


class TimeDecay:
    """legacy.py:22-33 (float64, numpy's cosine)."""
    def __init__(self, t_max: int, decay: float = 0.2, beta_start: float = 20, beta_end: float = 2):
        self.t_max = t_max
        self.start_decay = decay * t_max
        self.start_b = beta_start
        self.end_b = beta_end

    def __call__(self, t):
        rel_t = (t - self.start_decay) / (self.t_max - self.start_decay)
        return self.end_b + 0.5 * (self.start_b - self.end_b) * (1 + np.cos(rel_t * np.pi))


class AdaroundRegTerm(torch.nn.Module):
    """legacy.py:36-64.  ``forward`` is the reference's torch expression (for callers that build their own loss);
    :class:`AdaroundPass` does not call it: the gradient of the term is fused into the backward launch (:meth:`host_values`)."""
    def __init__(self, max_iter: int = 20000, zeta: float = 1.1, gamma: float = -0.1, alpha: float = 0.01, beta: float = 20,
                 warm_ratio: float = 0.2):
        self.max_iter = max_iter
        self.zeta = zeta
        self.gamma = gamma
        self.alpha = alpha
        self.beta = beta
        self.warm_ratio = warm_ratio
        self.temp_anneal = TimeDecay(self.max_iter, self.warm_ratio)
        super().__init__()

    def rectified_sigmoid(self, r: torch.Tensor) -> torch.Tensor:
        return ((self.zeta - self.gamma) * torch.sigmoid(r) + self.gamma).clamp(0, 1)

    def forward(self, r: torch.Tensor, iter: int) -> torch.Tensor:
        if iter < self.max_iter * self.warm_ratio:
            round_loss = 0
        else:
            self.beta = self.temp_anneal(iter)
            round_loss = self.alpha * (1 - torch.pow((self.rectified_sigmoid(r) - 0.5).abs() * 2, self.beta)).sum()
        return round_loss

    def host_values(self, iter: int, scale: float) -> np.ndarray:
        """{k, beta, beta - 1} of ``forward(r, iter) * scale`` as the backward kernel reads them: k = 0 where the term is the
        integer 0; else k = float32(scale) * float32(alpha) rounded to float32 (the two scalar multiplications autograd does),
        beta the annealed exponent and beta - 1 formed in double (pow_backward), both then cast to float32."""
        if iter < self.max_iter * self.warm_ratio: return np.zeros(3, dtype=np.float32)
        beta = float(self.temp_anneal(iter))
        k = np.float32(np.float32(scale) * np.float32(self.alpha))
        return np.array([k, np.float32(beta), np.float32(beta - 1.0)], dtype=np.float32)


class _AdaRoundFunction(Function):
    """One weight, one job of each kernel: forward = AdaRoundDelegator.__call__, backward = dV (plus the regulariser's
    gradient when ``reg[0]`` != 0).  W, the scale and the offset receive no gradient (they are in no optimizer)."""
    @ staticmethod
    def forward(ctx, tensor, rounding, scale, offset, axis, quant_min: int, quant_max: int, reg) -> torch.Tensor:
        item = (tensor.detach(), rounding.detach(), scale.detach(), offset.detach(), axis, quant_min, quant_max)
        ctx.item, ctx.reg = item, reg
        return adaround_forward_multi([item])[0]

    @ staticmethod
    def backward(ctx, dy: torch.Tensor):
        dv = adaround_backward_multi([ctx.item], [dy.contiguous()], ctx.reg)[0]
        return None, dv, None, None, None, None, None, None


class _GroupedAdaRound(Function):
    """A member of an :class:`AdaroundGroup`: forward hands out what the group's ONE forward launch wrote, backward stashes
    ``dy`` -- V is an autograd leaf, :meth:`AdaroundGroup.flush` computes every member's dV in ONE launch after the sweep."""
    @ staticmethod
    def forward(ctx, tensor, rounding, group, slot: int) -> torch.Tensor:
        ctx.group, ctx.slot = group, slot
        return group.outputs[slot].detach()

    @ staticmethod
    def backward(ctx, dy: torch.Tensor):
        prev = ctx.group.dys[ctx.slot]              # a weight read twice in one forward: dV is linear in dy, sum the two
        ctx.group.dys[ctx.slot] = dy.contiguous() if prev is None else prev + dy
        return None, None, None, None


class AdaroundGroup(LaunchGroup):
    """The AdaRound delegators of one block as ONE ``ppqhip_adaround_fwd_multi`` launch (:meth:`prepare`, start of a step) and
    ONE ``ppqhip_adaround_bwd_multi`` launch (:meth:`flush`, end of the backward sweep).  Outputs and dV buffers are allocated
    once and dV is installed as V's ``.grad``, so a captured HIP graph of the step finds them at fixed addresses."""
    def __init__(self, members, reg: torch.Tensor):
        super().__init__(members)
        self.reg = reg
        self.outs = [torch.empty_like(v.value) for _, _, v in members]
        self.gv = [torch.empty_like(d.rounding) for d, _, _ in members]
        self.dys = [None] * len(members)

    @ staticmethod
    def eligible(delegator, config, var) -> bool:
        w = var.value
        return (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
                and isinstance(config.scale, torch.Tensor) and isinstance(config.offset, torch.Tensor)
                and config.scale.is_contiguous() and config.offset.is_contiguous())

    def _items(self, slots):
        m = self.members
        return [(m[k][2].value.detach(), m[k][0].rounding.detach(), m[k][1].scale.detach(), m[k][1].offset.detach(),
                 _channel_axis(m[k][1]), m[k][1].quant_min, m[k][1].quant_max) for k in slots]

    def prepare(self) -> None:
        """Start of a step: the soft-rounded fake quant of every member (ONE launch)."""
        self.outputs = adaround_forward_multi(self._items(range(len(self.members))), outs=self.outs)
        self.dys = [None] * len(self.members)
        self.launches += 1

    def flush(self) -> None:
        """End of the backward sweep: dV of every member that received a ``dy`` (ONE launch), installed as V's ``.grad``."""
        live = [k for k, dy in enumerate(self.dys) if dy is not None]
        if not live: return
        adaround_backward_multi(self._items(live), [self.dys[k] for k in live], self.reg, dvs=[self.gv[k] for k in live])
        self.launches += 1
        for k in live:
            leaf, g = self.members[k][0].rounding, self.gv[k]
            if leaf.grad is None: leaf.grad = g
            elif leaf.grad is not g: leaf.grad.add_(g)
        self.dys = [None] * len(self.members)


class AdaRoundDelegator:
    """legacy.py:67-136 (the TorchQuantizeDelegator protocol: ``__call__(tensor, config)``)."""
    def __init__(self, var, config, steps: int) -> None:
        self.reg = AdaroundRegTerm(max_iter=steps)
        self.config = config
        self.var = var
        self.is_parameter = self.var.is_parameter
        self.rounding = self.initiate_rounding(value=self.var.value, config=self.config, zeta=1.1, gamma=-0.1)

        if not self.var.is_parameter:
            raise TypeError(f'Can not create adaround delegator with variable {var.name}, '
                            'Adaround delegator works only with parameter.')
        if state_value(self.config.state) == QuantizationStates.PASSIVE.value:
            raise TypeError(f'Can not create adaround delegator with variable {var.name}, '
                            'Adaround delegator can not work with passive parameter.')
        if not config.policy.has_property(P.LINEAR) or config.policy.has_property(P.DYNAMIC):
            raise TypeError(f'Can not create adaround delegator with variable {var.name}: '
                            'AdaRound needs a static LINEAR (integer) quantization policy.')
        self.param_backup = None
        if self.is_parameter:
            self.param_backup = self.var.value.detach().clone()
        self.group, self.slot = None, None          # set by AdaroundGroup: this weight rides the block's multi-tensor launches
        self.reg_values = torch.zeros(3, dtype=torch.float32, device=self.rounding.device)     # {k, beta, beta - 1}: term off

    @ staticmethod
    def initiate_rounding(value: torch.Tensor, config, zeta: float, gamma: float) -> torch.Tensor:
        with torch.no_grad():
            scale, offset = config.scale, config.offset
            if config.policy.has_property(P.PER_CHANNEL):
                shape = [1 if axis != config.channel_axis else -1 for axis in range(value.ndim)]
                scale = scale.view(shape)

            rounding = (value / scale) - (value / scale).floor()
            rounding = - torch.log((zeta - gamma) / (rounding - gamma) - 1)
            rounding = torch.zeros_like(rounding).copy_(rounding)
            rounding.requires_grad = True
        return rounding

    def trainable_tensors(self) -> List[torch.Tensor]:
        tensors = [self.rounding]
        return tensors

    def finalize(self) -> None:
        # legacy.py:107-116 verbatim, under no_grad: the value is the same, and the new weight is a leaf that needs no gradient
        with torch.no_grad():
            weight, scale, offset = self.var.value, self.config.scale, self.config.offset
            if self.config.policy.has_property(P.PER_CHANNEL):
                shape = [1 if axis != self.config.channel_axis else -1 for axis in range(weight.ndim)]
                scale = scale.view(shape)
                offset = offset.view(shape)
            weight = (weight / scale).floor() + (self.rounding >= 0).float()
            weight = torch.clamp(weight + offset, self.config.quant_min, self.config.quant_max)
            weight = (weight - offset) * scale
        self.var.value = weight

    def withdraw(self) -> None:
        with torch.no_grad():
            self.var.value.copy_(self.param_backup)

    def __call__(self, tensor: torch.Tensor, config) -> torch.Tensor:
        if self.group is not None and self.group.outputs is not None and tensor is self.var.value:
            return _GroupedAdaRound.apply(tensor, self.rounding, self.group, self.slot)
        if not tensor.is_contiguous(): tensor = tensor.contiguous()
        return _AdaRoundFunction.apply(tensor, self.rounding, config.scale, config.offset, _channel_axis(config),
                                       config.quant_min, config.quant_max, self.reg_values)

    def regularization_loss(self, step: int) -> torch.Tensor:
        return self.reg.forward(r=self.rounding, iter=step)


class AdaroundPass(LearnedStepSizePass):
    """legacy.py:139-297: block-wise AdaRound (``block_size`` = the reference's depth limit, default 4) on
    ``LearnedStepSizePass.finetune``'s frame.  What is this pass's own:

    * between the pre-loss and the delegators, ``tune_block_weight_scale``: 900 steps of Adam(lr) + MultiStepLR([450, 600]) on
      MSE(Q(W), W) per computing-op weight through ``LSQDelegator(is_parameter_trainable=False)`` -- all weights of the block in
      ONE loop (Adam is elementwise and the losses are independent: the values of one loop per weight), each weight keeping its
      own withdraw decision.  A failure later in the block does not take it back;
    * an AdaRound delegator on every ACTIVATED, non-PASSIVE parameter config, an ``LSQDelegator(is_offset_trainable=False)`` on
      the other ACTIVATED / PASSIVE configs when ``is_scale_trainable``;
    * the step loss is the block MSE; ``gamma`` x the regulariser's gradient is added by the backward launch, from a device row
      ``before_step`` refreshes.  ``anneal_regularization=True`` evaluates the regulariser at the true step instead of the
      reference's shadowed index;
    * every delegator withdraws when the block ended worse, else finalises.

    ``group_weights``: the block's AdaRound weights in ONE forward and ONE backward launch per step."""
    def __init__(self, name: str = 'Block-wise Adaround Reconstruction', interested_layers: List[str] = [],
                 is_scale_trainable: bool = False, steps: int = 8000, lr: float = 1e-3, gamma: float = 1.0,
                 collecting_device: str = 'cuda', block_size: int = 4, *, anneal_regularization: bool = False,
                 group_weights: bool = True, use_hip_graph: bool = True, fused_adam: bool = True, tune_steps: int = 900):
        super().__init__(name=name, interested_layers=list(interested_layers or []), steps=steps, gamma=gamma,
                         is_scale_trainable=is_scale_trainable, lr=lr, block_size=block_size, collecting_device=collecting_device,
                         loss_fn=torch_mean_square_error, group_weights=group_weights, use_hip_graph=use_hip_graph,
                         fused_adam=fused_adam)
        self.collecting_device = collecting_device
        self.loss_fn = torch_mean_square_error
        self.anneal_regularization = anneal_regularization
        self.tune_steps = tune_steps                # the reference's fixed 900 (legacy.py:175)
        self.stats['adaround_weights'] = 0
        self.stats['tuned_weights'] = 0
        self.keep_roundings = False                 # an inspection aid: True keeps every trained V (weight name -> tensor) in
        self.roundings = {}                         # `roundings`, taken before the block finalises or withdraws

    def optimize(self, graph, dataloader, executor, collate_fn=None, **kwargs):
        self.roundings = {}
        return super().optimize(graph, dataloader, executor, collate_fn=collate_fn, **kwargs)

    def _block_loss(self, block, qt_inputs, fp_outputs, executor) -> float:
        """optim/training.py:300-335 as the reference returns it, a Python double: the keep / withdraw decision compares the
        same numbers (one process only, so there is nothing to average across ranks)."""
        from .blocks import compute_block_loss
        return compute_block_loss(block, qt_inputs, fp_outputs, executor, self._loss)

    # ---- step 2 ---------------------------------------------------------------------------------------------------------
    def tune_block_weight_scale(self, block, steps: int = None, loss_fn=torch_mean_square_error) -> None:
        """legacy.py:170-202 for every computing-op weight of the block in ONE loop (see the class docstring).  W is trained
        too and not restored (quirk (b)): ``trainable_tensors`` returns it and ``param_backup`` is None."""
        steps = self.tune_steps if steps is None else steps
        members = []
        for op in block.rps:
            if op.type in COMPUTING_OP and hasattr(op, 'config') and len(op.inputs) > 1:
                c, v = op.config.input_quantization_config[1], op.inputs[1]
                if not isinstance(c.scale, torch.Tensor): continue
                d = LSQDelegator(config=c, var=v, is_parameter_trainable=False)
                if len(d.trainable_tensors()) == 0: continue
                members.append((d, c, v))
        if not members: return
        params = _unique(t for d, _, _ in members for t in d.trainable_tensors())
        self.stats['tuned_weights'] += len(members)
        optimizer = torch.optim.Adam(params, lr=self.lr)
        scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, [int(steps / 2), int(steps * 2 / 3)])
        by_round = {}                                  # one LSQWeightGroup per rounding policy, as LSQWeightGroup.build groups
        for m in (members if self.group_weights else []):
            if LSQWeightGroup.eligible(*m): by_round.setdefault(rounding_value(m[1].rounding), []).append(m)
        groups = [LSQWeightGroup(g) for g in by_round.values()]

        def losses():
            return [loss_fn(d(v.value, c), v.value) for d, c, v in members]
        with torch.no_grad(): initial = torch.stack([l.reshape(()) for l in losses()]).tolist()
        try:
            for _ in range(steps):
                optimizer.zero_grad()
                for g in groups: g.prepare()
                with torch.enable_grad(): loss = sum(losses())
                loss.backward()
                for g in groups: g.flush()
                optimizer.step()
                scheduler.step()
        finally:
            for g in groups: g.outputs = None; g.release()
        with torch.no_grad(): post = torch.stack([l.reshape(()) for l in losses()]).tolist()
        for (d, _, _), a, b in zip(members, initial, post):
            if b > a: d.withdraw()

    # ---- per block --------------------------------------------------------------------------------------------------------
    def _reg_table(self, num_outputs: int, device) -> torch.Tensor:
        """{k, beta, beta - 1} per training step, built on the host with TimeDecay in double: the reference evaluates the term
        at ``idx``, which its output loop has shadowed to ``num_outputs - 1`` (quirk (a)); ``anneal_regularization`` uses the
        step."""
        if self.steps <= 0: return torch.zeros(1, 3, dtype=torch.float32, device=device)
        reg = AdaroundRegTerm(max_iter=self.steps)
        if not self.anneal_regularization:
            row = reg.host_values(num_outputs - 1, self.gamma)
            return torch.from_numpy(np.tile(row, (max(self.steps, 1), 1))).to(device)
        return torch.from_numpy(np.stack([reg.host_values(t, self.gamma) for t in range(self.steps)] or [np.zeros(3, np.float32)])).to(device)

    def _check_block(self, block) -> None:
        if self._world() != 1:
            raise ValueError('AdaroundPass runs in one process: data-parallel AdaRound is not supported')
        for op in block.rps:
            if not hasattr(op, 'config'): continue
            for cfg, var in op.config_with_variable:
                if var.is_parameter and state_value(cfg.state) == QuantizationStates.ACTIVATED.value:
                    if cfg.policy.has_property(P.FLOATING) or cfg.policy.has_property(P.DYNAMIC) or not cfg.policy.has_property(P.LINEAR):
                        raise TypeError(f'AdaroundPass: {op.name}.{var.name} has a FLOATING / DYNAMIC quantization policy; '
                                        'AdaRound rounds static integer grids only')
                    if not (isinstance(var.value, torch.Tensor) and var.value.is_cuda):
                        raise TypeError(f'AdaroundPass: {var.name} is not a CUDA tensor (ppq_amd has no CPU path)')

    def _before_delegators(self, block) -> None:
        with self._phase('tune_weight_scale'):
            self.tune_block_weight_scale(block)

    def _delegate(self, block, executor, job: BlockTraining) -> None:
        """legacy.py:222-240."""
        for op in block.rps:
            if not hasattr(op, 'config'): continue
            for cfg, var in op.config_with_variable:
                st = state_value(cfg.state)
                if st not in (QuantizationStates.ACTIVATED.value, QuantizationStates.PASSIVE.value): continue
                if var.is_parameter and st != QuantizationStates.PASSIVE.value:
                    job.register(executor, cfg, AdaRoundDelegator(config=cfg, var=var, steps=self.steps))
                elif self.is_scale_trainable:
                    job.register(executor, cfg, LSQDelegator(config=cfg, var=var, is_offset_trainable=False))

    @ staticmethod
    def _adaround_members(job: BlockTraining) -> list:
        return [(d, cfg, d.var) for cfg, d in job.delegators.items() if isinstance(d, AdaRoundDelegator)]

    def _build_groups(self, block, job: BlockTraining, uniq) -> None:
        table = self._reg_table(len(block.ep.outputs), uniq[0].device)
        reg = table[0].clone()                         # the device buffer every backward launch reads: the regulariser's
        ada = self._adaround_members(job)              # gradient is added there, the step loss is the block MSE alone
        for d, _, _ in ada: d.reg_values = reg
        self.stats['adaround_weights'] += len(ada)
        members = [m for m in ada if AdaroundGroup.eligible(*m)] if self.group_weights else []
        if members: job.groups = [AdaroundGroup(members, reg)]
        if self.group_activations and self.is_scale_trainable: job.act_groups = LSQActivationGroup.build(job.delegators)
        constant = not self.anneal_regularization

        def before_step(step: int) -> None:
            if step == 0 or not constant: reg.copy_(table[step])
        job.before_step = before_step

    def _step_loss(self, block, names, outs, fp_output):
        return sum(self._loss(y, fp_output[n]) for n, y in zip(names, outs))

    def _settle(self, job: BlockTraining, worse: bool) -> None:
        """legacy.py:286-293.  (The post-loss was measured with the soft rounding h(V) still delegated: quirk (c).)"""
        if self.keep_roundings:
            self.roundings.update({d.var.name: d.rounding.detach().clone() for d, _, _ in self._adaround_members(job)})
        for d in job.delegators.values():
            if worse: d.withdraw()
            else: d.finalize()
