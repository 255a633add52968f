"""GPU tests of round tuning (ppq_amd/roundtune.py, csrc/roundtune.hip).

Kernel level: the forward is compared BIT FOR BIT with the test-side torch restatement of
ppq/quantization/algorithm/training.py:490-527 (tests/golden/roundtune_cases.py) run by torch on the same GPU, and with the
reference's own CPU outputs (tests/golden/roundtune.npz): the expression is a division, three additions / subtractions, a
clamp and a multiplication, each a correctly rounded IEEE fp32 operation on the CPU and on the GPU alike, so there is no
library function whose last bits could differ and the comparison with the CPU goldens is exact too.  dR is the identity.

Pass level: RoundTuningPass against a test-side eager restatement of optim/training.py:910-999 on the same blocks, the grouped
against the single-job launches, graph replay against eager steps, the keep / withdraw contract, the launch count, the early
exit and the effect end to end.  The vendor convolutions are switched to PyTorch's deterministic native kernels where two
runs are compared bit for bit (tests/test_gpu_adaround.py explains why)."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import roundtune_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BLOCK_SIZE = 5


def _bits(t: torch.Tensor) -> np.ndarray:
    """Bit patterns, every NaN mapped to one canonical pattern (a NaN's payload carries no value)."""
    a = t.detach().float().contiguous().cpu().numpy()
    return np.where(np.isnan(a), np.float32('nan'), a).view(np.uint32)


# A job has at most 1024 workgroups of 256 lanes (csrc/channel_axis.hpp): a lane takes a second trip through the float4 loop from
# 262,145 float4, through the element-wise loop (the unaligned variants) from 262,145 elements.  The three forms of the float4
# loop: per tensor (four channel computations per float4 with one channel; n % 4 = 1), elem_per_channel = 209,924 (a multiple of
# 4: one channel per float4; 262,405 float4) and elem_per_channel = 349,867 (odd: four channels per float4; 262,400 float4,
# n % 4 = 1).
_TRIP2 = (('trip2_pt', (1025, 1025), None, -128, 127), ('trip2_plane', (5, 52481, 2, 2), 0, -8, 7), ('trip2_lanes', (3, 349867), 0, -8, 7))


def _cases(extra: bool = True):
    """(name, t, r, scale, offset, axis, qmin, qmax, dy) on the GPU: the golden cases (t = the floored weight, r = the
    perturbed R), larger / unaligned-plane ones with special values, and the smallest ones (_TRIP2) that send a lane through
    each loop of the kernel's walk a second time."""
    out = []
    for k, (name, shape, axis, qmin, qmax, _, _) in enumerate(RC.CASES):
        w, s, o, noise, dy = RC.case_tensors(k)
        r0, t = RC.initial_rounding(w, s, axis)
        out.append((name, t, r0 + noise, s, o, axis, qmin, qmax, dy))
    if extra:
        g = torch.Generator().manual_seed(78)
        for name, shape, axis, qmin, qmax in (('conv_big_i4', (64, 32, 3, 3), 0, -8, 7), ('gemm_big_pt', (257, 129), None, -128, 127),
                                              ('conv_plane7', (32, 16, 7, 7), 0, -128, 127), ('convT_big_axis1', (16, 24, 3, 3), 1, -8, 7)) + _TRIP2:
            w = torch.randn(shape, generator=g) * 0.3
            C = 1 if axis is None else shape[axis]
            s = (torch.rand(C, generator=g) * 0.02 + 0.01) if axis is not None else torch.tensor(0.013)
            o = torch.zeros_like(s)
            r0, t = RC.initial_rounding(w, s, axis)
            r = r0 + torch.randn(shape, generator=g) * 0.3
            # specials: NaN / inf weights and R, R exactly on and next to the threshold
            flat_t, flat_r = t.view(-1), r.view(-1)
            flat_t[:4] = torch.tensor([float('nan'), float('inf'), -float('inf'), -0.0])
            flat_r[4:12] = torch.tensor([float('nan'), float('inf'), -float('inf'), 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))),
                                         float(np.nextafter(np.float32(0.5), np.float32(0))), -0.0, 1.0])
            out.append((name, t, r, s, o, axis, qmin, qmax, torch.randn(shape, generator=g)))
    return [(name, t.to(DEV), r.to(DEV), s.to(DEV), o.to(DEV), axis, qmin, qmax, dy.to(DEV))
            for name, t, r, s, o, axis, qmin, qmax, dy in out]


def _unaligned(t: torch.Tensor) -> torch.Tensor:
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    u = buf[1:].view(t.shape)
    u.copy_(t)
    assert u.data_ptr() % 16 != 0
    return u


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
def test_forward_kernel_is_bit_exact_against_torch_on_the_device():
    from ppq_amd.ffi import roundtune_forward_multi
    cases = _cases()
    items = [(t, r, s, o, axis, qmin, qmax) for _, t, r, s, o, axis, qmin, qmax, _ in cases]
    single = [roundtune_forward_multi([it])[0] for it in items]
    for (name, t, r, s, o, axis, qmin, qmax, _), got in zip(cases, single):
        want = RC.forward(t, r, s, o, axis, qmin, qmax)
        assert np.array_equal(_bits(got), _bits(want)), (name, int((_bits(got) != _bits(want)).sum()))
        un = roundtune_forward_multi([(_unaligned(t), _unaligned(r), s, o, axis, qmin, qmax)])[0]
        assert np.array_equal(_bits(un), _bits(want)), name                     # the element-wise path
        out = _unaligned(torch.zeros_like(t))
        roundtune_forward_multi([(t, r, s, o, axis, qmin, qmax)], outs=[out])   # only the output is off by 4 bytes
        assert np.array_equal(_bits(out), _bits(want)), name
    grouped = roundtune_forward_multi(items * 2)                                # 24 jobs: two launches of <= 16
    assert len(grouped) > 16
    for k, got in enumerate(grouped):
        assert np.array_equal(_bits(got), _bits(single[k % len(items)])), k


def test_forward_kernel_against_the_reference_goldens():
    """The reference's CPU outputs, bit for bit (see the module docstring), single job and all cases in one launch; the inputs
    include floored weights whose t / s is not an integer in fp32 and elements the clamp changes at both ends
    (tests/test_host_roundtune.py asserts that they do)."""
    from ppq_amd.ffi import roundtune_forward_multi
    gold = dict(np.load(os.path.join(HERE, 'golden', 'roundtune.npz')))
    items = []
    for k, (name, shape, axis, qmin, qmax, _, _) in enumerate(RC.CASES):
        p = f'c{k}_'
        t, r, s, o = (torch.from_numpy(gold[p + x]).to(DEV) for x in ('wfloor', 'r', 'scale', 'offset'))
        items.append((t, r, s, o, axis, qmin, qmax))
        r0, floored = RC.initial_rounding(torch.from_numpy(gold[p + 'w']).to(DEV), s, axis)
        assert np.array_equal(_bits(r0), gold[p + 'r0'].view(np.uint32)), name
        assert np.array_equal(_bits(floored), gold[p + 'wfloor'].view(np.uint32)), name
        got = roundtune_forward_multi([items[-1]])[0]
        assert np.array_equal(_bits(got), gold[p + 'fwd'].view(np.uint32)), (name, int((_bits(got) != gold[p + 'fwd'].view(np.uint32)).sum()))
        assert np.array_equal(_bits(RC.finalize(t, r, s, axis)), gold[p + 'final'].view(np.uint32)), name
    for k, got in enumerate(roundtune_forward_multi(items)):
        assert np.array_equal(_bits(got), gold[f'c{k}_fwd'].view(np.uint32)), k


def test_ffi_argument_checks():
    from ppq_amd.ffi import roundtune_forward_multi
    name, t, r, s, o, axis, qmin, qmax, _ = _cases(extra=False)[0]
    with pytest.raises(RuntimeError, match='not shaped like the weight'):
        roundtune_forward_multi([(t, r.view(-1), s, o, axis, qmin, qmax)])
    with pytest.raises(RuntimeError, match='scale / offset need'):
        roundtune_forward_multi([(t, r, s[:-1], o[:-1], axis, qmin, qmax)])
    with pytest.raises(RuntimeError, match='not contiguous'):
        roundtune_forward_multi([(t, r.transpose(0, 1).contiguous().transpose(0, 1), s, o, axis, qmin, qmax)])
    with pytest.raises(RuntimeError, match='not on the GPU'):
        roundtune_forward_multi([(t, r.cpu(), s, o, axis, qmin, qmax)])
    with pytest.raises(RuntimeError, match='differ in length'):
        roundtune_forward_multi([(t, r, s, o, axis, qmin, qmax)], outs=[])


# ---- 2. dR = dy --------------------------------------------------------------------------------------------------------------
def _delegator(t_unused, w, s, o, axis, qmin, qmax, name='w'):
    from ppq_amd import LinearQuantizationConfig, QuantizationStates
    from ppq_amd.harness import Variable
    from ppq_amd.roundtune import RoundTuningDelegator
    cfg = LinearQuantizationConfig(channel_axis=axis, quant_min=qmin, quant_max=qmax)
    cfg.scale, cfg.offset, cfg.state = s.clone(), o.clone(), QuantizationStates.ACTIVATED
    var = Variable(name, value=w.clone(), is_parameter=True)
    return RoundTuningDelegator(var=var, config=cfg), cfg, var


def test_dr_equals_dy_through_the_function_and_the_group():
    from ppq_amd.roundtune import RoundTuningGroup
    members = []
    for k, (name, shape, axis, qmin, qmax, _, _) in enumerate(RC.CASES):
        w, s, o, noise, dy = (x.to(DEV) for x in RC.case_tensors(k))
        d, cfg, var = _delegator(None, w, s, o, axis, qmin, qmax, name)
        with torch.no_grad(): d.rounding.add_(noise)
        want = RC.forward(var.value, d.rounding.detach(), s, o, axis, qmin, qmax)
        # one job through the Function
        y = d(var.value, cfg)
        assert np.array_equal(_bits(y), _bits(want)), name
        (y * dy).sum().backward()
        assert np.array_equal(_bits(d.rounding.grad), _bits(dy)), name
        d.rounding.grad = None
        members.append((d, cfg, var, dy, want))
    group = RoundTuningGroup([(d, cfg, var) for d, cfg, var, _, _ in members])
    assert all(RoundTuningGroup.eligible(d, cfg, var) for d, cfg, var, _, _ in members)
    group.prepare()
    assert group.launches == 1
    loss = 0.0
    for k, (d, cfg, var, dy, want) in enumerate(members):
        y = d(var.value, cfg)
        assert y.data_ptr() == group.outs[k].data_ptr()                         # the group's output, no launch of its own
        assert np.array_equal(_bits(y), _bits(want)), k
        loss = loss + (y * dy).sum()
        if k % 2 == 0: loss = loss + (d(var.value, cfg) * (dy * 0.5)).sum()      # a weight read twice in one forward
    loss.backward()
    group.flush()
    assert group.launches == 1                                                   # no backward launch
    for k, (d, cfg, var, dy, _) in enumerate(members):
        want = dy + dy * 0.5 if k % 2 == 0 else dy
        assert np.array_equal(_bits(d.rounding.grad), _bits(want)), k
    group.outputs = None
    group.release()
    assert all(d.group is None for d, *_ in members)


# ---- the pass ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _deterministic():
    prev = (torch.backends.cudnn.enabled, torch.are_deterministic_algorithms_enabled(),
            torch.is_deterministic_algorithms_warn_only_enabled())
    torch.backends.cudnn.enabled = False
    torch.use_deterministic_algorithms(True, warn_only=True)
    try: yield
    finally:
        torch.backends.cudnn.enabled = prev[0]
        torch.use_deterministic_algorithms(prev[1], warn_only=prev[2])


def _int4_weights(graph):
    for op in graph.operations.values():
        for cfg, var in op.config_with_variable:
            if var.is_parameter and cfg.state.value == 1:
                cfg.num_of_bits, cfg.quant_min, cfg.quant_max = 4, -8, 7


def _setup(seed=5):
    """The small-CNN INT4 setup of tests/test_gpu_adaround.py::_setup."""
    from ppq_amd import harness
    from ppq_amd.calibration import RuntimeCalibrationPass
    torch.manual_seed(0)
    graph = harness.small_cnn_graph(seed=seed, width=16)
    harness.quantize_graph(graph, 'minmax')
    _int4_weights(graph)
    ex = harness.TorchExecutor(graph, DEV)
    harness.ParameterQuantizePass().optimize(graph)
    g = torch.Generator().manual_seed(7)
    batches = [torch.rand(8, 3, 24, 24, generator=g).to(DEV) for _ in range(4)]
    RuntimeCalibrationPass(check_steps=False).optimize(graph, dataloader=batches, executor=ex, calib_steps=4)
    return graph, ex, batches


def _snapshot(graph):
    return {v.name: v.value.detach().clone() for op in graph.operations.values() for v in op.inputs
            if v.is_parameter and isinstance(v.value, torch.Tensor)}


def _weights(graph):
    """{weight name: (op, config, bias name or None)} of the operations the pass tunes."""
    from ppq_amd.roundtune import ROUND_TUNING_OP
    out = {}
    for op in graph.operations.values():
        if hasattr(op, 'config') and op.type in ROUND_TUNING_OP and len(op.inputs) > 1 and op.inputs[1].is_parameter:
            out[op.inputs[1].name] = (op, op.config.input_quantization_config[1], op.inputs[2].name if len(op.inputs) == 3 else None)
    return out


def _initial(run_or_before, graph, name):
    """(R, floored weight) of weight `name` from the tensors the pass started with."""
    op, cfg, _ = _weights(graph)[name]
    return RC.initial_rounding(run_or_before[name], cfg.scale.detach(), cfg.channel_axis)


class _Run:
    """One pass on a fresh small CNN: the parameters before and after, the trained R of every weight (taken before its block
    finalised or withdrew), the pass."""
    def __init__(self, pass_cls=None, **kw):
        from ppq_amd.roundtune import RoundTuningPass
        self.graph, self.ex, self.batches = _setup()
        self.before = _snapshot(self.graph)
        self.p = (pass_cls or RoundTuningPass)(**kw)
        self.p.keep_roundings = True
        self.p.optimize(self.graph, self.batches, self.ex)
        self.after = _snapshot(self.graph)
        self.r = self.p.roundings


class _TorchRoundTune:
    """training.py:529-590 with the torch ops of roundtune_cases, for the restatement."""
    def __init__(self, var, config):
        from ppq_amd import QuantizationProperty
        self.var, self.config = var, config
        self.axis = config.channel_axis if config.policy.has_property(QuantizationProperty.PER_CHANNEL) else None
        self.backup = var.value.detach().clone()
        with torch.no_grad():
            r, floored = RC.initial_rounding(var.value, config.scale, self.axis)
        var.value = floored
        self.rounding = r.requires_grad_(True)

    def __call__(self, tensor, config):
        return RC.forward(tensor, self.rounding, config.scale, config.offset, self.axis, config.quant_min, config.quant_max)

    def finalize(self):
        with torch.no_grad(): self.var.value = RC.finalize(self.var.value, self.rounding, self.config.scale, self.axis)

    def withdraw(self):
        with torch.no_grad(): self.var.value.copy_(self.backup)


def _restatement_class():
    """A test-side eager restatement of optim/training.py:910-999 over the same blocks (the pass's block split and data
    plumbing): torch-op delegators, torch.optim.Adam, MSELoss steps and post-loss, torch_mean_square_error pre-loss.  It takes
    decisions (a) (a withdrawn block is not finalised) and (b) (the bias is restored on withdraw) of INTEGRATION.md section 6,
    nothing else."""
    from ppq_amd.blocks import block_forward, compute_block_loss, torch_mean_square_error
    from ppq_amd.roundtune import RoundTuningPass

    class Restated(RoundTuningPass):
        def finetune(self, block, executor, qt_inputs, fp_outputs):
            self.enable_block_gradient(block)
            pre = compute_block_loss(block, qt_inputs, fp_outputs, executor, torch_mean_square_error)
            params, delegators, biases = [], {}, []
            for op in block.rps:
                if not hasattr(op, 'config'): continue
                if op.type in {'Gemm', 'MatMul', 'ConvTranspose', 'PPQBiasFusedMatMul', 'Conv'}:
                    if op.inputs[1].is_parameter:
                        cfg, var = op.config.input_quantization_config[1], op.inputs[1]
                        d = _TorchRoundTune(var, cfg)
                        params.append(d.rounding); executor.register_quantize_delegate(cfg, d); delegators[cfg] = d
                    if len(op.inputs) == 3 and op.inputs[-1].is_parameter:
                        op.inputs[-1].value.requires_grad = True
                        params.append(op.inputs[-1].value)
                        biases.append((op.inputs[-1].value, op.inputs[-1].value.detach().clone()))
            opt = torch.optim.Adam(params, lr=self.lr)
            mse = torch.nn.MSELoss()
            names = [v.name for v in block.ep.outputs]
            for idx in range(self.steps):
                qt_input, fp_output = qt_inputs[idx % len(qt_inputs)], fp_outputs[idx % len(qt_inputs)]
                opt.zero_grad()
                outs = block_forward(executor, block.rps, qt_input, names, with_gradient=True)
                loss = 0.0
                for i, name in enumerate(names): loss += mse(outs[i], fp_output[name])
                loss.backward(); opt.step()
            post = compute_block_loss(block, qt_inputs, fp_outputs, executor, mse)
            self.roundings.update({d.var.name: d.rounding.detach().clone() for d in delegators.values()})
            for cfg, d in delegators.items():
                d.withdraw() if post > pre else d.finalize()
                executor.remove_quantize_delegate(cfg)
            if post > pre:
                with torch.no_grad():
                    for t, backup in biases: t.copy_(backup)
            self.disable_block_gradient(block)
            return pre, post
    return Restated


def _check_clean(graph, ex):
    for op in graph.operations.values():
        for v in op.inputs:
            if v.is_parameter and isinstance(v.value, torch.Tensor):
                assert not v.value.requires_grad and v.value.grad is None and v.value.is_leaf, v.name
        if hasattr(op, 'config'):
            for c, _ in op.config_with_variable:
                for t in (c.scale, c.offset):
                    if isinstance(t, torch.Tensor): assert not t.requires_grad and t.grad is None
    assert not ex._delegates


def _assert_identical(a: _Run, b: _Run):
    """Bit for bit: the reports (both losses of every block), every trained R, every weight and bias."""
    assert a.p.report == b.p.report, (a.p.report, b.p.report)
    assert set(a.r) == set(b.r) == set(_weights(a.graph)) and len(a.r) >= 3
    for name in a.r: assert np.array_equal(_bits(a.r[name]), _bits(b.r[name])), name
    assert set(a.after) == set(b.after)
    for key in a.after: assert np.array_equal(_bits(a.after[key]), _bits(b.after[key])), key


def _assert_trained(run: _Run, steps: int, lr: float):
    """Every R moved from its initial value, no element by more than Adam can move it in `steps` steps."""
    for name, r in run.r.items():
        d = (r - _initial(run.before, run.graph, name)[0]).abs()
        assert float((d > 0).float().mean()) >= 0.5, name
        assert float(d.max()) <= steps * 2.1 * lr, name


# ---- 3. the reference's finetune ---------------------------------------------------------------------------------------------
def test_pass_equals_an_eager_restatement_of_the_reference():
    from ppq_amd.blocks import split_graph_into_blocks
    with _deterministic():
        ref = _Run(_restatement_class(), steps=10, lr=1e-3, use_hip_graph=False, group_weights=False)
        ours = _Run(steps=10, lr=1e-3, use_hip_graph=False, group_weights=False)
    p = ours.p
    assert p.stats['roundtune_weights'] >= 3 and p.stats['graph_blocks'] == 0 and p.stats['grouped_weights'] == 0
    assert p.stats['skipped_weights'] == 0
    assert [str(b) for b in split_graph_into_blocks(ours.graph, ours.graph.topological_sort(), BLOCK_SIZE)] == [r[0] for r in p.report]
    print('report', p.report, 'stats', p.stats)
    _assert_identical(ref, ours)
    _assert_trained(ours, 10, 1e-3)
    _check_clean(ours.graph, ours.ex)


def test_grouped_equals_single_job():
    with _deterministic():
        single = _Run(steps=6, lr=1e-3, use_hip_graph=False, group_weights=False)
        grouped = _Run(steps=6, lr=1e-3, use_hip_graph=False, group_weights=True)
    assert single.p.stats['grouped_weights'] == 0 and grouped.p.stats['grouped_weights'] == grouped.p.stats['roundtune_weights'] >= 3
    _assert_identical(single, grouped)
    _assert_trained(grouped, 6, 1e-3)
    assert single.p.stats['flipped'] == grouped.p.stats['flipped']


# ---- 4. graph replay ---------------------------------------------------------------------------------------------------------
def test_graph_replay_against_eager_steps():
    """The capturable fused Adam differs from torch.optim.Adam in the last bits of the step size, so R
    is compared under the bound tests/test_gpu_adaround.py::_assert_replay_close states for V: `steps * 2.1 * lr` at most, 1e-6
    on the median element.  A final weight differs by a whole scale step where a rounding decision flips, which it may only
    where the eager R lies within that bound of .5; nowhere else may a weight differ at all, and biases stay within the bound."""
    steps, lr = 6, 1e-3
    bound = steps * 2.1 * lr
    with _deterministic():
        eager = _Run(steps=steps, lr=lr, use_hip_graph=False)
        graphed = _Run(steps=steps, lr=lr, use_hip_graph=True)
    p = graphed.p
    assert p.stats['graph_failures'] == 0 and p.graph_error is None, (p.stats, p.graph_error)
    assert p.stats['graph_blocks'] == len(p.report) and p.stats['graph_replays'] == (steps - 1) * len(p.report)
    assert eager.p.stats['graph_blocks'] == 0
    assert eager.p.report[0][1] == graphed.p.report[0][1]
    assert [b > a for _, a, b in eager.p.report] == [b > a for _, a, b in graphed.p.report], (eager.p.report, graphed.p.report)
    assert set(eager.r) == set(graphed.r)
    near_total, differ_total = 0, 0
    for name, (op, cfg, bias) in _weights(eager.graph).items():
        d = (eager.r[name] - graphed.r[name]).abs()
        assert float(d.max()) <= bound and float(d.median()) <= 1e-6, (name, float(d.max()), float(d.median()))
        near = (eager.r[name] - 0.5).abs() <= bound
        differ = eager.after[name] != graphed.after[name]
        near_total += int(near.sum()); differ_total += int(differ.sum())
        assert not bool((differ & ~near).any()), (name, int((differ & ~near).sum()))
        if bias is not None:
            assert float((eager.after[bias] - graphed.after[bias]).abs().max()) <= bound, bias
    print(f'{near_total} weight elements have an eager R within {bound} of .5; {differ_total} of them differ between eager and replay')
    _assert_trained(graphed, steps, lr)
    _check_clean(graphed.graph, graphed.ex)


# ---- 5. the contract ---------------------------------------------------------------------------------------------------------
def _prof_launches(fn):
    from ppq_amd import _lib
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    try: fn()
    finally:
        torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 32)()
    n = _lib.lib.ppqhip_prof_collect(arr, 32)
    return {arr[i].name.decode(): arr[i].launches for i in range(n)}


def test_kept_blocks_are_finalised_clean_exit_and_one_launch_per_step():
    from ppq_amd.blocks import split_graph_into_blocks
    from ppq_amd.roundtune import RoundTuningPass
    steps = 5
    graph, ex, batches = _setup()
    before = _snapshot(graph)
    p = RoundTuningPass(steps=steps, lr=1e-3, use_hip_graph=False)
    p.keep_roundings = True
    launches = _prof_launches(lambda: p.optimize(graph, batches, ex))
    after = _snapshot(graph)
    blocks = split_graph_into_blocks(graph, graph.topological_sort(), BLOCK_SIZE)
    assert [str(b) for b in blocks] == [r[0] for r in p.report]
    n_blocks, n_weights = p.stats['blocks'], p.stats['roundtune_weights']
    assert n_blocks >= 1 and n_weights >= 3 and p.stats['grouped_weights'] == n_weights
    # ONE grouped launch per step per block; the pre-loss runs before any delegator exists (none); the post-loss runs with
    # the group's outputs dropped: one single-job launch per weight per batch.  No backward launch of any kind.
    assert launches.get('roundtune_fwd', 0) == steps * n_blocks + len(batches) * n_weights, launches
    assert launches.get('adaround_fwd', 0) == 0 and launches.get('adaround_bwd', 0) == 0, launches
    weights = _weights(graph)
    flipped = tuned = kept = 0
    for block, (_, pre, post) in zip(blocks, p.report):
        assert np.isfinite(pre) and np.isfinite(post)
        for op in block.rps:
            if len(op.inputs) < 2 or op.inputs[1].name not in weights: continue
            name = op.inputs[1].name
            _, cfg, bias = weights[name]
            r0, floored = _initial(before, graph, name)
            if post > pre:
                assert np.array_equal(_bits(after[name]), _bits(before[name])), name
                assert np.array_equal(_bits(after[bias]), _bits(before[bias])), bias
            else:
                kept += 1
                want = RC.finalize(floored, p.roundings[name], cfg.scale.detach(), cfg.channel_axis)
                assert np.array_equal(_bits(after[name]), _bits(want)), name                 # floor(W/s)*s + (R > .5)*s
                flipped += int(((r0 > .5) != (p.roundings[name] > .5)).sum())
                tuned += r0.numel()
    assert kept >= 1, p.report
    assert (p.stats['flipped'], p.stats['tuned_elements']) == (flipped, tuned), (p.stats, flipped, tuned)
    print('report', p.report, 'flipped', flipped, 'of', tuned)
    _check_clean(graph, ex)


def test_a_block_that_ends_worse_is_restored_bit_for_bit():
    """Forced with a hostile learning rate: Adam moves every bias by about lr = 1 per step, far outside the activations'
    range, so every block ends worse.  Weight AND bias come back bit for bit ((a), (b)), nothing is finalised or counted."""
    from ppq_amd.roundtune import RoundTuningPass
    for graphed in (False, True):
        graph, ex, batches = _setup()
        before = _snapshot(graph)
        p = RoundTuningPass(steps=4, lr=1.0, use_hip_graph=graphed)
        p.keep_roundings = True
        p.optimize(graph, batches, ex)
        assert p.report and all(post > pre for _, pre, post in p.report), p.report
        after = _snapshot(graph)
        assert set(after) == set(before)
        for name in before: assert np.array_equal(_bits(after[name]), _bits(before[name])), name
        for name, r in p.roundings.items():                                    # it did train: R is not where it began
            assert float(((r - _initial(before, graph, name)[0]).abs() > 0).float().mean()) >= 0.5, name
        assert p.stats['flipped'] == 0 and p.stats['tuned_elements'] == 0
        _check_clean(graph, ex)


def test_a_training_step_that_raises_leaves_the_block_as_it_was_found():
    """The failure path of the block-training frame (tests/test_host_block_training.py runs it on the CPU
    through the MX pass): the third gradient forward of the first block raises -- a Python exception, before that step launches
    anything -- with the weights floored and two optimizer steps on R and the biases.  Everything is back bit for bit, no
    delegate of the pass is registered, nothing keeps ``requires_grad``."""
    from block_training_double import StepRefused, assert_same_bits, refuse_gradient_forward, snapshot
    from ppq_amd.roundtune import RoundTuningPass
    graph, ex, batches = _setup()
    before = snapshot(graph)
    with refuse_gradient_forward(ex, at=3) as seen, pytest.raises(StepRefused, match='gradient forward 3 refused'):
        RoundTuningPass(steps=4, lr=1e-2, use_hip_graph=False).optimize(graph, batches, ex)
    assert seen[0] == 3
    assert_same_bits(snapshot(graph), before)
    _check_clean(graph, ex)


def test_early_exit_leaves_nothing_trainable(monkeypatch):
    """(c): a block with nothing to train returns (0, 0) with nothing requires_grad (the reference leaves it set)."""
    from ppq_amd import roundtune
    graph, ex, batches = _setup()
    before = _snapshot(graph)
    monkeypatch.setattr(roundtune, 'ROUND_TUNING_OP', set())
    p = roundtune.RoundTuningPass(steps=2, use_hip_graph=False)
    p.optimize(graph, batches, ex)
    assert p.report and all(r[1:] == (0.0, 0.0) for r in p.report)
    assert p.stats['blocks'] == 0 and p.stats['roundtune_weights'] == 0
    after = _snapshot(graph)
    for name in before: assert np.array_equal(_bits(after[name]), _bits(before[name])), name
    _check_clean(graph, ex)


def test_weights_without_an_activated_config_are_skipped_untouched():
    """(d): the reference would floor such a weight in the delegator's constructor and never call the delegator for it."""
    from ppq_amd.core import QuantizationStates
    from ppq_amd.roundtune import RoundTuningPass
    graph, ex, batches = _setup()
    weights = _weights(graph)
    for _, cfg, _ in weights.values(): cfg.state = QuantizationStates.FP32
    before = _snapshot(graph)
    p = RoundTuningPass(steps=3, lr=1e-3, use_hip_graph=False)
    launches = _prof_launches(lambda: p.optimize(graph, batches, ex))
    assert p.stats['skipped_weights'] == len(weights) >= 3 and p.stats['roundtune_weights'] == 0
    assert launches.get('roundtune_fwd', 0) == 0
    after = _snapshot(graph)
    for name in weights: assert np.array_equal(_bits(after[name]), _bits(before[name])), name
    _check_clean(graph, ex)


# ---- 6. the effect, end to end -------------------------------------------------------------------------------------------------
def test_effect_end_to_end_with_a_learning_rate_that_flips_roundings():
    """lr = 1e-2 for 40 steps: Adam moves R by up to 0.4, enough to carry a large part of the elements across .5 (the default
    1e-4 x 500 steps moves it by 0.05 at most).  Asserted: the pass's own contract (no kept block ends with a larger loss
    than it began with -- exact), roundings did flip, the error analysis runs on the tuned graph.  The NOISE:SIGNAL figures are
    printed, not asserted: nobody has measured what they should be."""
    from ppq_amd.analyse import graphwise_error_analyse
    from ppq_amd.roundtune import RoundTuningPass
    graph, ex, batches = _setup()
    base = graphwise_error_analyse(graph, DEV, batches, method='snr', steps=3, verbose=False, executor=ex)
    before = _snapshot(graph)
    p = RoundTuningPass(steps=40, lr=1e-2)
    p.optimize(graph, batches, ex)
    assert p.stats['graph_failures'] == 0, p.graph_error
    after = _snapshot(graph)
    kept = [(name, pre, post) for name, pre, post in p.report if not post > pre]
    for name, pre, post in p.report:
        assert np.isfinite(pre) and np.isfinite(post) and pre > 0, (name, pre, post)
    assert all(post <= pre for _, pre, post in kept)
    assert len(kept) >= 1 and p.stats['flipped'] > 0 and p.stats['tuned_elements'] >= p.stats['flipped'], (p.report, p.stats)
    assert any(not torch.equal(after[n], before[n]) for n in _weights(graph))
    tuned = graphwise_error_analyse(graph, DEV, batches, method='snr', steps=3, verbose=False, executor=ex)
    assert set(tuned) == set(base) and all(np.isfinite(v) for v in tuned.values())
    _check_clean(graph, ex)
    print('report', p.report)
    print(f"flipped {p.stats['flipped']} of {p.stats['tuned_elements']}")
    for name in base: print(f'NOISE:SIGNAL {name}: {base[name]:.6f} -> {tuned[name]:.6f}')
