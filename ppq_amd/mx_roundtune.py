"""Round tuning on the MX element grid: learned up / down rounding of MX weights.

``quantize_graph_mx`` rounds every weight element to the nearest element value of its block.  With eight magnitudes per MXFP4
element nearest is often not the best choice for the layer's output; ``MXRoundTuningPass`` learns, per element, whether to take the
element value just below or just above the weight on the block's own grid -- the block scale stays fixed -- with the block-wise
training machinery of ``RoundTuningPass``:

    split    (once per weight)  c = the block's E8M0 code under the config's scale rule, X = 2^(c - 127), u = v / X
             lo = the largest element magnitude <= |u|, hi = the next one (the largest normal stays)
             floored = (sign | lo) * X;  rounding = (|u| - lo) / (hi - lo) in [0, 1), 0 where hi == lo;  a NaN keeps its bits
    forward  (once per step)    out = rounding > .5 ? (sign | up(|floored / X|)) * X : floored;  backward: dy for both

Every step is exact in float32: the HIP kernels (``ppq_amd/csrc/mx_roundtune.hip``, ``use_kernels=True``) and the torch restatement
below (``use_kernels=False``, any device) give identical bits; ``tests/mx_round_reference.py`` restates the contract by tables.  The
tuned weight is an ordinary float32 tensor ON the MX grid: ``mx_fake_quant`` leaves it as it is (but for MXFP8_E4M3 under EVEN, which
the pass refuses), so ``export_graph_mx`` and ``deploy_graph_mx`` work on it unchanged."""
from typing import Any, Dict, List

import torch
from torch.autograd import Function

from .core import QuantizationStates, state_value
from .ffi import MX_BLOCK, mx_round_forward_jobs, mx_round_forward_multi, mx_round_split_multi
from .lsq import BlockTraining, LaunchGroup, LearnedStepSizePass
from .roundtune import RoundTuningPass, _GroupedRound, _train_bias
from .mx import (_SPEC, MX_OPERATIONS, MXDelegator, MXFormat, MXScaleRule, _activated, _bits_to_float, _check_codes, _check_input, _config_rule,
                 _mx_scale_code, _pow2, mx_block_axis)


# ---- the torch restatement ----------------------------------------------------------------------------------------------------------
def _grid(format: MXFormat):
    """(shift, sub_limit, sub_scale, sub_quantum, max_bits): ``MxFmt`` of mx_common.hpp -- MXINT8 is the fixed-point grid throughout."""
    _, m, emin, _, max_normal = _SPEC[format.name]
    max_bits = int(torch.tensor(max_normal, dtype=torch.float32).view(torch.int32))
    if not format.is_float: return 17, 0x7f800000, 64.0, 0.015625, max_bits
    return 23 - m, (emin + 127) << 23, 2.0 ** (m - emin), 2.0 ** (emin - m), max_bits


def _mx_floor(umag: torch.Tensor, format: MXFormat) -> torch.Tensor:
    """``mx_floor`` of mx_common.hpp: the pattern of the largest element magnitude <= |u|, at most the largest normal."""
    shift, sub_limit, sub_scale, quantum, max_bits = _grid(format)
    normal = umag & ~((1 << shift) - 1)
    grid = (torch.floor(_bits_to_float(umag) * sub_scale) * quantum).view(torch.int32)
    return torch.minimum(torch.where(umag < sub_limit, grid, normal), torch.full_like(umag, max_bits))


def _mx_up(lo: torch.Tensor, format: MXFormat) -> torch.Tensor:
    """``mx_up`` of mx_common.hpp: the pattern of the element magnitude above the element magnitude ``lo``; the largest normal stays.
    (A NaN pattern gives a pattern nobody may use.)"""
    shift, sub_limit, _, quantum, max_bits = _grid(format)
    above = (_bits_to_float(lo) + quantum).view(torch.int32)
    return torch.minimum(torch.where(lo < sub_limit, above, lo + (1 << shift)), torch.full_like(lo, max_bits))


def _to_blocks(t: torch.Tensor, axis: int):
    """``t`` as ``lead + [nb, 32]`` with the block axis last (a short last block padded with zeros), and ``lead``."""
    length = t.shape[axis]
    nb = (length + MX_BLOCK - 1) // MX_BLOCK
    x = t.movedim(axis, -1)
    lead = list(x.shape[:-1])
    x = x.contiguous()
    if nb * MX_BLOCK != length: x = torch.nn.functional.pad(x, (0, nb * MX_BLOCK - length))
    return x.reshape(lead + [nb, MX_BLOCK]), lead


def _from_blocks(y: torch.Tensor, lead, length: int, axis: int) -> torch.Tensor:
    return y.reshape(lead + [-1])[..., :length].movedim(-1, axis).contiguous()


def _split_torch(w: torch.Tensor, format: MXFormat, axis: int, rule: MXScaleRule):
    x, lead = _to_blocks(w, axis)
    code = _mx_scale_code(x, format, rule)
    ubits = (x * _pow2(254 - code)).view(torch.int32)
    umag, sign = ubits & 0x7fffffff, ubits & -0x80000000
    lo = _mx_floor(umag, format)
    hi = _mx_up(lo, format)
    nan = umag > 0x7f800000
    open_ = (hi > lo) & ~nan                                           # Inf has lo == hi
    flo = _bits_to_float(lo)
    step = torch.where(open_, _bits_to_float(hi) - flo, torch.ones_like(flo))                    # a power of two
    rounding = torch.where(open_, (_bits_to_float(umag) - flo) * (1.0 / step), torch.zeros_like(flo))      # both exact
    floored = torch.where(nan, x, _bits_to_float(lo | sign) * _pow2(code))
    length = w.shape[axis]
    codes = code.reshape(lead + [-1]).movedim(-1, axis).to(torch.uint8).contiguous()
    return _from_blocks(floored, lead, length, axis), _from_blocks(rounding, lead, length, axis), codes


def _forward_torch(floored: torch.Tensor, rounding: torch.Tensor, codes: torch.Tensor, format: MXFormat, axis: int) -> torch.Tensor:
    x, lead = _to_blocks(floored, axis)
    r, _ = _to_blocks(rounding, axis)
    code = codes.movedim(axis, -1).reshape(lead + [-1, 1]).to(torch.int32)
    c = code.clamp(max=254)
    X = _pow2(c)
    ubits = (x * _pow2(254 - c)).view(torch.int32)                     # exact: floored is on the grid
    umag, sign = ubits & 0x7fffffff, ubits & -0x80000000
    up = _bits_to_float(_mx_up(umag, format) | sign) * X
    take = (r > .5) & (umag <= 0x7f800000) & (code != 0xff)            # a NaN rounding compares false
    return _from_blocks(torch.where(take, up, x), lead, floored.shape[axis], axis)


# ---- the two functions --------------------------------------------------------------------------------------------------------------
def mx_round_split(w: torch.Tensor, format, axis: int = -1, scale_rule=MXScaleRule.FLOOR, use_kernels: bool = True):
    """``(floored, rounding, scale_codes)`` of ``w`` with blocks of 32 along ``axis``: the element value just below every element on
    its block's grid (towards zero; what ``mx_fake_quant`` would take or the one below it), the element's position between that value
    and the next one above in [0, 1) -- 0 where there is none above: a saturated element --, and the blocks' E8M0 codes (uint8, the
    axis replaced by ceil(len / 32)): those of ``mx_fake_quant`` under ``scale_rule``.  A NaN keeps its bits and gets rounding 0.
    ``where(rounding > .5, up, floored)`` is ``mx_fake_quant(w)`` but at exact ties, which go down here.
    ``use_kernels=True``: the HIP kernel (the tensor must be on the GPU); ``False``: torch ops on any device -- identical bits."""
    format, scale_rule = MXFormat.of(format), MXScaleRule.of(scale_rule)
    axis = _check_input(w, axis)
    w = w.detach()
    if use_kernels: return mx_round_split_multi([(w, format, axis, scale_rule)])[0]
    return _split_torch(w, format, axis, scale_rule)


def _check_forward(floored, rounding, scale_codes, axis) -> int:
    axis = _check_input(floored, axis)
    if not isinstance(rounding, torch.Tensor) or rounding.dtype != torch.float32 or rounding.shape != floored.shape:
        raise RuntimeError(f'rounding must be a float32 tensor of shape {list(floored.shape)}')
    if scale_codes is None: raise RuntimeError('scale_codes must be the uint8 codes of mx_round_split, got None')
    _check_codes(floored, axis, scale_codes)
    if rounding.device != floored.device or scale_codes.device != floored.device:
        raise RuntimeError(f'rounding and scale_codes must be on the device of floored ({floored.device})')
    return axis


class _MXRoundFunction(Function):
    """One weight: the forward of DESIGN.md section 9.18, backward = the reference's round-tuning rule (``dy`` for the tensor and
    ``dy`` for the rounding, ``roundtune._RoundTuneFunction``)."""
    @ staticmethod
    def forward(ctx, floored, rounding, scale_codes, format, axis, use_kernels):
        f, r = floored.detach(), rounding.detach()
        if not use_kernels: return _forward_torch(f, r, scale_codes, format, axis)
        return mx_round_forward_multi([(f.contiguous(), r.contiguous(), scale_codes.contiguous(), format, axis)])[0]

    @ staticmethod
    def backward(ctx, dy: torch.Tensor):
        return dy, dy, None, None, None, None


def mx_round_forward(floored: torch.Tensor, rounding: torch.Tensor, scale_codes: torch.Tensor, format, axis: int = -1,
                     use_kernels: bool = True) -> torch.Tensor:
    """The weight a rounding selects: ``rounding > .5`` takes the element value above ``floored`` on its block's grid, anything else
    (a NaN included) ``floored`` itself; a NaN element and a block whose code is 0xFF pass through.  ``floored`` and ``scale_codes`` are
    ``mx_round_split``'s.  Autograd's backward is ``dy`` for ``floored`` and ``dy`` for ``rounding``.  ``use_kernels`` as for
    ``mx_round_split``."""
    format = MXFormat.of(format)
    axis = _check_forward(floored, rounding, scale_codes, axis)
    return _MXRoundFunction.apply(floored, rounding, scale_codes, format, axis, use_kernels)


# ---- delegator and group ------------------------------------------------------------------------------------------------------------
class MXRoundTuningGroup(LaunchGroup):
    """The MX round-tuning delegators of one block as ONE ``ppqhip_mx_round_fwd_multi`` launch per step (:meth:`prepare`).  Outputs
    are allocated and the job table is built once: floored weight, rounding, codes and outputs stay where they are through a block's
    training (Adam updates the rounding in place), so a captured HIP graph of the step finds them.  dR = dy exactly, so there is no
    backward launch."""
    def __init__(self, members):
        super().__init__(members)
        self.outs = [torch.empty_like(v.value) for _, _, v in members]
        self._items = [(v.value.detach(), d.rounding.detach(), d.scale_codes, d.format, d.axis) for d, _, v in members]
        self._jobs = mx_round_forward_jobs(self._items, self.outs)

    @ staticmethod
    def eligible(delegator, config, var) -> bool:
        w = var.value
        return delegator.use_kernels and isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()

    def prepare(self) -> None:
        """Start of a step: the delegator's forward of every member (ONE launch)."""
        self.outputs = mx_round_forward_multi(self._items, outs=self.outs, jobs=self._jobs)
        self.launches += 1


class MXRoundTuningDelegator:
    """``delegator(tensor, config)`` for ``TorchExecutor.register_quantize_delegate``: the weight of ``var`` under a learned rounding.
    Construction REPLACES ``var.value`` by the floored weight and keeps the original tensor for :meth:`withdraw`; ``rounding`` is the
    trainable tensor, ``scale_codes`` the blocks' fixed E8M0 codes.  A config that is not activated passes the tensor through, as
    ``MXDelegator`` does."""
    def __init__(self, var, config, format, axis: int, scale_rule=MXScaleRule.FLOOR, use_kernels: bool = True) -> None:
        self.var, self.config = var, config
        self.format, self.scale_rule = MXFormat.of(format), MXScaleRule.of(scale_rule)
        self.use_kernels = use_kernels
        if not var.is_parameter: raise TypeError(f'Variable {var.name} is not a parameter!')
        if var.value is None or not isinstance(var.value, torch.Tensor): raise ValueError(f'Unexpected value type of {var.name}')
        if self.format is MXFormat.MXFP8_E4M3 and self.scale_rule is MXScaleRule.EVEN:
            raise ValueError(f'{var.name}: a weight tuned on the MXFP8_E4M3 grid is not a fixed point of mx_fake_quant under EVEN (DESIGN.md section 9.18)')
        self.axis = _check_input(var.value, axis)
        self._backup = var.value                            # the tensor itself: nothing here writes into it
        floored, rounding, self.scale_codes = mx_round_split(var.value, self.format, self.axis, self.scale_rule, use_kernels)
        var.value = floored
        self._initial_up = rounding > .5                    # for MXRoundTuningPass.stats['flipped']
        self._rounding = rounding.requires_grad_(True)
        self.group, self.slot = None, None                  # set by MXRoundTuningGroup: this weight rides the block's launch

    @ property
    def rounding(self) -> torch.Tensor:
        return self._rounding

    def trainable_tensors(self) -> List[torch.Tensor]:
        return [self._rounding]

    def _select(self, rounding: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            return mx_round_forward(self.var.value, rounding, self.scale_codes, self.format, self.axis, self.use_kernels)

    def flipped(self) -> torch.Tensor:
        """How many elements the trained rounding puts on another element value than the initial one (a device scalar); call it
        before :meth:`finalize`.  A rounding that crossed .5 on a saturated element changes nothing and is not counted."""
        a, b = self._select(self._initial_up.to(torch.float32)), self._select(self._rounding.detach())
        return (a.view(torch.int32) != b.view(torch.int32)).sum()

    def finalize(self) -> None:
        """``var.value`` becomes the weight the final rounding selects: a tensor on the MX grid."""
        self.var.value = self._select(self._rounding.detach())
        if self._backup.is_leaf: self._backup.requires_grad_(False)

    def withdraw(self) -> None:
        """``var.value`` is the original tensor again."""
        self.var.value = self._backup

    def __call__(self, tensor: torch.Tensor, config=None) -> torch.Tensor:
        if not _activated(config): return tensor
        if self.group is not None and self.group.outputs is not None and tensor is self.var.value:
            return _GroupedRound.apply(tensor, self._rounding, self.group, self.slot)
        return _MXRoundFunction.apply(tensor, self._rounding, self.scale_codes, self.format, self.axis, self.use_kernels)


# ---- the pass -----------------------------------------------------------------------------------------------------------------------
class MXRoundTuningPass(LearnedStepSizePass):
    """Block-wise round tuning of MX weights (``block_size`` = the depth limit, default 5) on ``LearnedStepSizePass.finetune``'s frame
    (DESIGN.md section 4.5), with ``RoundTuningPass``'s losses, launch group and keep / withdraw rule.  What is this pass's own:

    * the pre-loss runs with the graph's own delegators (``quantize_graph_mx``'s ``MXDelegator``);
    * an :class:`MXRoundTuningDelegator` on the weight of every Conv / Gemm / MatMul whose input 1 is a parameter with an ACTIVATED
      config that carries ``detail['MX_FORMAT']`` -- format and scale rule from the config, the axis from ``mx_block_axis``; the bias
      of a three-input op is trained as it is, but biases alone are not tuned.  The delegate the executor held for the config is
      saved and registered again at the end -- the very object;
    * the step is captured only when every delegate inside the block is known to launch without a synchronisation;
    * a kept block is finalised: every weight is the forward of its final rounding.

    Weights that take no part are left untouched and listed in ``skipped`` (name -> reason): no MX config, a config that is not
    activated, and MXFP8_E4M3 under EVEN, whose tuned weights ``mx_fake_quant`` would change.
    ``group_weights`` / ``use_hip_graph`` / ``fused_adam`` are ``RoundTuningPass``'s; ``use_kernels=False`` runs the delegators on the
    torch restatement (a measuring aid).  ``report`` = [(block, pre_loss, post_loss)]; ``stats['flipped']`` of
    ``stats['tuned_elements']`` weight elements of the kept blocks ended on another element value than round-to-nearest gives."""
    def __init__(self, interested_layers: List[str] = [], steps: int = 500, lr: float = 1e-4, block_size: int = 5,
                 expire_device: str = 'cpu', collecting_device: str = 'cuda', optimizer: Any = None, *,
                 group_weights: bool = True, use_hip_graph: bool = True, fused_adam: bool = True, use_kernels: bool = True):
        super().__init__(name='MX Rounding Tuning Pass', interested_layers=list(interested_layers or []), steps=steps, lr=lr,
                         block_size=block_size, expire_device=expire_device, collecting_device=collecting_device,
                         optimizer=optimizer, group_weights=group_weights, use_hip_graph=use_hip_graph, fused_adam=fused_adam)
        self.use_kernels = use_kernels
        self.loss_fn = torch.nn.MSELoss()
        self.stats.update(mx_weights=0, skipped_weights=0, flipped=0, tuned_elements=0)
        self.skipped: Dict[str, str] = {}
        self.keep_roundings = False                 # an inspection aid: True keeps every trained rounding (weight name -> tensor) in
        self.roundings = {}                         # `roundings`, taken before the block finalises or withdraws

    def optimize(self, graph, dataloader, executor, collate_fn=None, **kwargs):
        self.roundings, self.skipped = {}, {}
        return super().optimize(graph, dataloader, executor, collate_fn=collate_fn, **kwargs)

    @ staticmethod
    def refusal(config):
        """Why the weight of ``config`` takes no part, or None."""
        if 'MX_FORMAT' not in getattr(config, 'detail', {}): return 'its config is not an MX config'
        if state_value(config.state) != QuantizationStates.ACTIVATED.value: return 'its config is not activated'
        if MXFormat.of(config.detail['MX_FORMAT']) is MXFormat.MXFP8_E4M3 and _config_rule(config) is MXScaleRule.EVEN:
            return 'MXFP8_E4M3 under EVEN: a tuned weight is not a fixed point of mx_fake_quant'
        return None

    def _capturable(self, block, executor) -> bool:
        """The block's step is captured only when every delegate inside it is one whose forward is known to launch on the current
        stream without a synchronisation: this pass's own and the graph's ``MXDelegator`` (kernel or torch restatement alike)."""
        held = getattr(executor, '_delegates', {})
        for op in block.rps:
            if not hasattr(op, 'config'): continue
            for cfg, _ in op.config_with_variable:
                d = held.get(cfg)
                if d is not None and not isinstance(d, (MXDelegator, MXRoundTuningDelegator)): return False
        return True

    def _check_block(self, block) -> None:
        if self._world() != 1:
            raise ValueError('MXRoundTuningPass runs in one process: data-parallel round tuning is not supported')

    def _delegate(self, block, executor, job: BlockTraining) -> None:
        for op in block.rps:
            if not hasattr(op, 'config') or op.type not in MX_OPERATIONS: continue
            if len(op.inputs) > 1 and op.inputs[1].is_parameter:
                cfg, var = op.config.input_quantization_config[1], op.inputs[1]
                reason = self.refusal(cfg)
                if reason is not None:
                    if var.name not in self.skipped: self.stats['skipped_weights'] += 1
                    self.skipped[var.name] = reason
                elif cfg not in job.delegators:
                    if self.use_kernels and not (isinstance(var.value, torch.Tensor) and var.value.is_cuda):
                        raise TypeError(f'MXRoundTuningPass: {var.name} is not a CUDA tensor (the kernels have no CPU path)')
                    d = MXRoundTuningDelegator(var, cfg, cfg.detail['MX_FORMAT'], mx_block_axis(op.type, 1), _config_rule(cfg), self.use_kernels)
                    job.register(executor, cfg, d, keep_held=True)     # the graph's own delegate comes back at the end
            _train_bias(op, job)

    def _nothing_to_train(self, job: BlockTraining, uniq) -> bool:
        return not job.delegators                          # biases alone are not tuned

    # losses, the one launch group and the keep / withdraw rule are RoundTuningPass's
    _pre_loss, _post_loss, _step_loss = RoundTuningPass._pre_loss, RoundTuningPass._post_loss, RoundTuningPass._step_loss
    _build_groups, _settle = RoundTuningPass._build_groups, RoundTuningPass._settle
    _group_class, _weights_stat = MXRoundTuningGroup, 'mx_weights'

    @ staticmethod
    def _keep(delegator) -> torch.Tensor:
        """``flipped()`` reads the floored weight, so it comes before ``finalize()`` here."""
        flipped = delegator.flipped()
        delegator.finalize()
        return flipped

