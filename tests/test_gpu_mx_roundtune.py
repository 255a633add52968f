"""GPU tests of MX round tuning (ppq_amd/mx_roundtune.py, csrc/mx_roundtune.hip).

Kernel level: split and forward against the table oracle (tests/mx_round_reference.py), bit for bit, for every format and scale rule
on the smallest shapes that reach every body of the split (rows4, rows1 with a short last block, an unaligned view, strided with
inner 9 and with a MatMul weight's inner 32) and both paths of the forward; chunked and grouped calls; dR = dy.

Pass level: MXRoundTuningPass on a tiny MXFP4 / MXFP8 graph against a test-side eager restatement made of the ``use_kernels=False``
functions, the grouped against the single-job launches, graph replay against eager steps, the keep / withdraw contract, the restored
delegates, the launch count, the refusals and the effect end to end.  The vendor convolutions are switched to PyTorch's
deterministic native kernels where two runs are compared bit for bit (tests/test_gpu_adaround.py explains why).  There is no
tolerance anywhere but in the extra replay test against the reference's optimizer (see there)."""
import contextlib

import numpy as np
import pytest
import torch

import mx_reference as R
import mx_round_reference as RR
import mx_scale_reference as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FORMATS, RULES = R.FORMATS, S.RULES
# (shape, axis, view offset by one float): rows4; rows1 with a short last block; the unaligned view; strided, inner 9, a short last
# block; a MatMul weight [in, out] (strided, inner 32)
SHAPES = [((5, 96), -1, False), ((3, 70), -1, False), ((5, 96), -1, True), ((40, 70, 3, 3), 1, False), ((64, 32), -2, False)]


def _gpu(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _offset(t: torch.Tensor) -> torch.Tensor:
    """A contiguous copy of ``t`` that starts one float behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    u = buf[1:].view(t.shape)
    u.copy_(t)
    assert u.data_ptr() % 16 == 4
    return u


def _same(got, want, what):
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = np.uint32 if got.dtype == np.float32 else got.dtype
    bad = np.flatnonzero(got.view(view).ravel() != want.view(view).ravel())
    assert bad.size == 0, f'{what}: {bad.size} elements differ, first at {bad[:4]}: {got.ravel()[bad[:4]]} != {want.ravel()[bad[:4]]}'


def _crafted(shape, axis: int, fmt: str, seed: int) -> np.ndarray:
    """Values over 16 octaves with, along the block axis, an all-zero block, a block of values ON the grid and of exact ties (X = 1),
    a block whose amax saturates, and at the front of the storage +-0, float32 subnormals, +-Inf and NaN."""
    x = R.layout_input(shape, seed=seed)
    xm = np.moveaxis(x, axis, -1)                                                    # a view: the rows are written through
    rows, n = list(np.ndindex(*xm.shape[:-1])), min(32, xm.shape[-1])
    t = R.table(fmt)
    mids = (t[:-1] + t[1:]) / 2
    grid = np.concatenate([[2.0 ** R.EMAX[fmt]], t[1:9], -mids[:8], t[-7:], mids[-7:]])[:n]
    xm[rows[-1]][:n] = 0
    xm[rows[-2]][:len(grid)] = grid
    xm[rows[-3]][n - 1] = 1.99 * 8
    return RR.plant_specials(x, fmt)


def _roundings(shape, seed: int) -> np.ndarray:
    r = np.random.default_rng(seed).random(shape, dtype=np.float32)
    r.reshape(-1)[:len(RR.ROUNDINGS)] = RR.ROUNDINGS
    return r


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', FORMATS)
def test_kernels_are_bit_exact_against_the_oracle(fmt):
    from ppq_amd import ffi, mx_round_forward, mx_round_split
    for k, (shape, axis, offset) in enumerate(SHAPES):
        x = _crafted(shape, axis, fmt, seed=k)
        r = _roundings(shape, 31 + k)
        for rule in RULES:
            what = (fmt, rule, shape, axis, offset)
            want = RR.split(x, fmt, axis, rule)
            w = _offset(_gpu(x)) if offset else _gpu(x)
            floored, rounding, codes = mx_round_split(w, fmt, axis, rule)
            for name, g, e in zip(('floored', 'rounding', 'codes'), (floored, rounding, codes), want): _same(g, e, (what, name))
            torch_arm = mx_round_split(w, fmt, axis, rule, use_kernels=False)       # the restatement on the device: the same bits
            for name, g, e in zip(('floored', 'rounding', 'codes'), torch_arm, want): _same(g, e, (what, 'torch', name))
            rr = np.array(r)
            rr.reshape(-1)[len(RR.ROUNDINGS):] = np.where(np.arange(rr.size - len(RR.ROUNDINGS)) % 3 == 0, want[1].reshape(-1)[len(RR.ROUNDINGS):],
                                                          rr.reshape(-1)[len(RR.ROUNDINGS):])      # every third: the split's own rounding
            c = np.array(want[2])
            c.reshape(-1)[-1] = 0xff                                                # a foreign block code: passes through
            expect = RR.forward(want[0], rr, c, fmt, axis)
            fl, rt, ct = (_offset(floored), _offset(_gpu(rr)), _gpu(c)) if offset else (floored, _gpu(rr), _gpu(c))
            _same(mx_round_forward(fl, rt, ct, fmt, axis), expect, (what, 'forward'))
            _same(mx_round_forward(fl, rt, ct, fmt, axis, use_kernels=False), expect, (what, 'torch forward'))
            out = _offset(torch.zeros_like(floored))                                # only the output is off by 4 bytes
            ffi.mx_round_forward_multi([(floored, _gpu(rr), ct, fmt, axis % len(shape))], outs=[out])
            _same(out, expect, (what, 'forward into an unaligned output'))


def test_property_a_and_b_on_the_device():
    """(a) the split's own rounding selects ``mx_fake_quant`` but at ties; (b) a random selection is a fixed point -- through the
    kernels, on MXFP4 under every rule."""
    from ppq_amd import mx_fake_quant, mx_round_forward, mx_round_split
    x = _gpu(RR.scaled_blocks(5, 128))
    for rule in RULES:
        floored, rounding, codes = mx_round_split(x, 'MXFP4_E2M1', -1, rule)
        sel = mx_round_forward(floored, rounding, codes, 'MXFP4_E2M1')
        fq = mx_fake_quant(x, 'MXFP4_E2M1', scale_rule=rule)
        assert int(((sel.view(torch.int32) != fq.view(torch.int32)) & (rounding != .5)).sum()) == 0, rule
        out = mx_round_forward(floored, _gpu(_roundings((128, 64), 9)), codes, 'MXFP4_E2M1')
        again_codes = torch.zeros_like(codes)
        again = mx_fake_quant(out, 'MXFP4_E2M1', scale_codes=again_codes, scale_rule=rule)
        assert torch.equal(again.view(torch.int32), out.view(torch.int32)), rule
        if rule == 'FLOOR': assert torch.equal(again_codes, codes)


def _mixed_jobs(count: int):
    """``count`` tiny tensors of mixed shapes, formats and rules."""
    shapes = [((2, 40), -1), ((3, 32), -1), ((2, 33, 3), 1), ((40, 2), 0), ((1, 7), -1), ((4, 8, 2, 2), 1)]
    jobs = []
    for k in range(count):
        shape, axis = shapes[k % len(shapes)]
        jobs.append((R.layout_input(shape, seed=100 + k), FORMATS[k % len(FORMATS)], axis, RULES[(k // 2) % len(RULES)]))
    return jobs


def test_chunked_and_grouped_calls_equal_single_jobs():
    """45 jobs: two launches of either kernel (32 jobs per launch); every job against the oracle and against its single-job call."""
    from ppq_amd import ffi
    jobs = _mixed_jobs(45)
    items = [(_gpu(x), fmt, axis, rule) for x, fmt, axis, rule in jobs]
    grouped = ffi.mx_round_split_multi(items)
    assert len(grouped) == 45
    fwd_items = []
    for k, ((x, fmt, axis, rule), item, got) in enumerate(zip(jobs, items, grouped)):
        want = RR.split(x, fmt, axis, rule)
        single = ffi.mx_round_split_multi([item])[0]
        for name, g, s, e in zip(('floored', 'rounding', 'codes'), got, single, want):
            _same(g, e, (k, fmt, rule, name)); _same(s, e, (k, fmt, rule, name, 'single'))
        fwd_items.append((got[0], _gpu(_roundings(x.shape, k)), got[2], fmt, axis))
    outs = ffi.mx_round_forward_multi(fwd_items)
    for k, ((x, fmt, axis, rule), item, out) in enumerate(zip(jobs, fwd_items, outs)):
        expect = RR.forward(item[0].cpu().numpy(), item[1].cpu().numpy(), item[2].cpu().numpy(), fmt, axis)
        _same(out, expect, (k, fmt, 'forward'))
        _same(ffi.mx_round_forward_multi([item])[0], expect, (k, fmt, 'forward', 'single'))


def test_ffi_argument_checks():
    from ppq_amd import ffi
    x = _gpu(R.layout_input((4, 64), seed=1))
    floored, rounding, codes = ffi.mx_round_split_multi([(x, 'MXFP4_E2M1', -1)])[0]
    item = (floored, rounding, codes, 'MXFP4_E2M1', -1)
    with pytest.raises(RuntimeError, match='not shaped like the weight'): ffi.mx_round_forward_multi([(floored, rounding.view(-1), codes, 'MXFP4_E2M1', -1)])
    with pytest.raises(RuntimeError, match='not contiguous'): ffi.mx_round_forward_multi([(floored, rounding.t().contiguous().t(), codes, 'MXFP4_E2M1', -1)])
    with pytest.raises(RuntimeError, match='not on the GPU'): ffi.mx_round_forward_multi([(floored, rounding.cpu(), codes, 'MXFP4_E2M1', -1)])
    with pytest.raises(RuntimeError, match='scale_codes must be'): ffi.mx_round_forward_multi([(floored, rounding, codes[:, :1], 'MXFP4_E2M1', -1)])
    with pytest.raises(RuntimeError, match='differ in length'): ffi.mx_round_forward_multi([item], outs=[])
    with pytest.raises(RuntimeError, match='overlaps an input'): ffi.mx_round_forward_multi([item], outs=[floored])
    with pytest.raises(ValueError, match='unknown MX format'): ffi.mx_round_split_multi([(x, 'MXFP5', -1)])
    with pytest.raises(RuntimeError, match='out of range'): ffi.mx_round_split_multi([(x, 'MXFP4_E2M1', 2)])
    assert ffi.mx_round_split_multi([]) == [] and ffi.mx_round_forward_multi([]) == []


# ---- 2. dR = dy -----------------------------------------------------------------------------------------------------------------------
def _delegator(x: np.ndarray, fmt: str, axis: int, rule: str, name: str):
    from ppq_amd import MXRoundTuningDelegator
    from ppq_amd.harness import Variable
    from ppq_amd.mx import MXFormat, MXScaleRule, _mx_config
    cfg = _mx_config(MXFormat[fmt], DEV, MXScaleRule[rule])
    var = Variable(name, value=_gpu(x), is_parameter=True)
    return MXRoundTuningDelegator(var, cfg, fmt, axis, rule), cfg, var


def test_dr_equals_dy_through_the_function_and_the_group():
    from ppq_amd import MXRoundTuningGroup
    g = torch.Generator().manual_seed(3)
    members = []
    for k, (x, fmt, axis, rule) in enumerate(_mixed_jobs(8)):
        d, cfg, var = _delegator(x, fmt, axis, rule, f'w{k}')
        with torch.no_grad(): d.rounding.copy_(_gpu(_roundings(x.shape, k)))
        want = RR.forward(var.value.cpu().numpy(), d.rounding.detach().cpu().numpy(), d.scale_codes.cpu().numpy(), fmt, axis)
        dy = torch.randn(x.shape, generator=g).to(DEV)
        y = d(var.value, cfg)                                                       # one job through the Function
        _same(y, want, (k, 'forward'))
        (y * dy).sum().backward()
        _same(d.rounding.grad, dy.cpu().numpy(), (k, 'dR'))
        d.rounding.grad = None
        members.append((d, cfg, var, dy, want))
    group = MXRoundTuningGroup([(d, cfg, var) for d, cfg, var, _, _ in members])
    assert all(MXRoundTuningGroup.eligible(d, cfg, var) for d, cfg, var, _, _ in members)
    group.prepare()
    assert group.launches == 1
    loss = 0.0
    for k, (d, cfg, var, dy, want) in enumerate(members):
        y = d(var.value, cfg)
        assert y.data_ptr() == group.outs[k].data_ptr()                             # the group's output, no launch of its own
        _same(y, want, (k, 'grouped'))
        loss = loss + (y * dy).sum()
        if k % 2 == 0: loss = loss + (d(var.value, cfg) * (dy * 0.5)).sum()          # a weight read twice in one forward
    loss.backward()
    group.flush()
    assert group.launches == 1                                                       # no backward launch
    for k, (d, cfg, var, dy, _) in enumerate(members):
        _same(d.rounding.grad, (dy + dy * 0.5 if k % 2 == 0 else dy).cpu().numpy(), (k, 'grouped dR'))
    group.outputs = None
    group.release()
    assert all(d.group is None for d, *_ in members)


# ---- the pass -------------------------------------------------------------------------------------------------------------------------
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


WEIGHTS = {'c1_w': ('Conv', 'c1_b'), 'c2_w': ('Conv', 'c2_b'), 'fc_w': ('Gemm', 'fc_b')}
FMT = 'MXFP4_E2M1'


def _axis(name: str) -> int:
    return 1 if WEIGHTS[name][0] == 'Conv' else -1


def _setup(weight_rule='FLOOR'):
    """The tiny graph with MXFP4 weights and MXFP8_E4M3 activations on the device, four batches of four 8 x 8 images."""
    from ppq_amd import harness, quantize_graph_mx
    graph = RR.tiny_graph()
    ex = harness.TorchExecutor(graph, DEV)
    delegators = quantize_graph_mx(graph, ex, FMT, 'MXFP8_E4M3', weight_scale_rule=weight_rule)
    g = torch.Generator().manual_seed(7)
    batches = [torch.rand(4, 8, 8, 8, generator=g).to(DEV) for _ in range(4)]
    return graph, ex, batches, delegators


def _snapshot(graph):
    return {v.name: v.value.detach().clone() for op in graph.operations.values() for v in op.inputs
            if v.is_parameter and isinstance(v.value, torch.Tensor)}


def _check_clean(graph, ex, delegators):
    for op in graph.operations.values():
        for v in op.inputs:
            if v.is_parameter and isinstance(v.value, torch.Tensor):
                assert not v.value.requires_grad and v.value.grad is None and v.value.is_leaf, v.name
    assert set(ex._delegates) == set(delegators) and all(ex._delegates[c] is d for c, d in delegators.items())     # the very objects


class _Run:
    """One pass on a fresh tiny graph: the parameters before and after, every trained rounding, the pass."""
    def __init__(self, pass_cls=None, **kw):
        from ppq_amd import MXRoundTuningPass
        self.graph, self.ex, self.batches, self.delegators = _setup()
        self.before = _snapshot(self.graph)
        self.p = (pass_cls or MXRoundTuningPass)(**kw)
        self.p.keep_roundings = True
        self.p.optimize(self.graph, self.batches, self.ex)
        self.after = _snapshot(self.graph)
        self.r = self.p.roundings


class _TorchMXRound:
    """The delegator restated with the ``use_kernels=False`` functions and plain autograd bookkeeping."""
    def __init__(self, var, fmt, axis, rule):
        from ppq_amd import mx_round_split
        self.var, self.fmt, self.axis = var, fmt, axis
        self.backup = var.value.detach().clone()
        floored, rounding, self.codes = mx_round_split(var.value, fmt, axis, rule, use_kernels=False)
        var.value = floored
        self.rounding = rounding.requires_grad_(True)

    def __call__(self, tensor, config):
        from ppq_amd import mx_round_forward
        return mx_round_forward(tensor, self.rounding, self.codes, self.fmt, self.axis, use_kernels=False)

    def finalize(self):
        with torch.no_grad(): self.var.value = self(self.var.value, None).detach()

    def withdraw(self):
        self.var.value = self.backup


def _restatement_class():
    """A test-side eager restatement of the pass over the same blocks: torch-op delegators, torch.optim.Adam, MSELoss steps and
    post-loss, torch_mean_square_error pre-loss, the graph's delegates put back."""
    from ppq_amd import MXRoundTuningPass
    from ppq_amd.blocks import block_forward, compute_block_loss, torch_mean_square_error

    class Restated(MXRoundTuningPass):
        def finetune(self, block, executor, qt_inputs, fp_outputs):
            self.enable_block_gradient(block)
            pre = compute_block_loss(block, qt_inputs, fp_outputs, executor, torch_mean_square_error)
            params, delegators, saved, biases = [], {}, {}, []
            for op in block.rps:
                if op.type not in ('Conv', 'Gemm', 'MatMul'): continue
                cfg, var = op.config.input_quantization_config[1], op.inputs[1]
                d = _TorchMXRound(var, cfg.detail['MX_FORMAT'], _axis(var.name), cfg.detail.get('MX_SCALE_RULE', 'FLOOR'))
                saved[cfg] = executor._delegates[cfg]
                params.append(d.rounding); executor.register_quantize_delegate(cfg, d); delegators[cfg] = d
                op.inputs[2].value.requires_grad = True
                params.append(op.inputs[2].value)
                biases.append((op.inputs[2].value, op.inputs[2].value.detach().clone()))
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
                executor.register_quantize_delegate(cfg, saved[cfg])
            if post > pre:
                with torch.no_grad():
                    for t, backup in biases: t.copy_(backup)
            self.disable_block_gradient(block)
            return pre, post
    return Restated


def _assert_identical(a: _Run, b: _Run):
    """Bit for bit: the reports (both losses of every block), every trained rounding, every weight and bias."""
    assert a.p.report == b.p.report, (a.p.report, b.p.report)
    assert set(a.r) == set(b.r) == set(WEIGHTS)
    for name in a.r: _same(a.r[name], b.r[name].cpu().numpy(), name)
    assert set(a.after) == set(b.after)
    for key in a.after: _same(a.after[key], b.after[key].cpu().numpy(), key)


def _assert_trained(run: _Run, steps: int, lr: float):
    """Every rounding moved from the split's, no element by more than Adam can move it in ``steps`` steps."""
    for name, r in run.r.items():
        r0 = torch.from_numpy(RR.split(run.before[name].cpu().numpy(), FMT, _axis(name))[1]).to(DEV)
        d = (r - r0).abs()
        assert float((d > 0).float().mean()) >= 0.5, name
        assert float(d.max()) <= steps * 2.1 * lr, name


def test_pass_equals_an_eager_restatement_of_the_torch_functions():
    with _deterministic():
        ref = _Run(_restatement_class(), steps=20, lr=1e-3, use_hip_graph=False, group_weights=False)
        ours = _Run(steps=20, lr=1e-3, use_hip_graph=False, group_weights=False)
    p = ours.p
    assert p.stats['mx_weights'] == 3 and p.stats['graph_blocks'] == 0 and p.stats['grouped_weights'] == 0 and p.skipped == {}
    print('report', p.report, 'stats', p.stats)
    _assert_identical(ref, ours)
    _assert_trained(ours, 20, 1e-3)
    _check_clean(ours.graph, ours.ex, ours.delegators)


def test_grouped_equals_single_job():
    with _deterministic():
        single = _Run(steps=20, lr=1e-3, use_hip_graph=False, group_weights=False)
        grouped = _Run(steps=20, lr=1e-3, use_hip_graph=False, group_weights=True)
    assert single.p.stats['grouped_weights'] == 0 and grouped.p.stats['grouped_weights'] == grouped.p.stats['mx_weights'] == 3
    _assert_identical(single, grouped)
    assert single.p.stats['flipped'] == grouped.p.stats['flipped']


def test_graph_replay_equals_eager_steps_bit_for_bit():
    """Replay against eager steps of the SAME optimizer: the replayed arm steps with the capturable Adam (fused where torch has it,
    ``_make_optimizer``), so the eager arm is handed that optimizer as its ``optimizer`` class -- a user's optimizer keeps
    ``_graphable`` off.  Report, roundings, weights and biases are equal bit for bit: a replay that dropped a step, staged a stale
    batch or missed the group's launch would show."""
    steps, lr = 20, 1e-3
    with _deterministic():
        graphed = _Run(steps=steps, lr=lr, use_hip_graph=True)
        fused = graphed.p.stats.get('fused_adam_blocks', 0) > 0

        def capturable_adam(params, lr):
            return torch.optim.Adam(params, lr=lr, capturable=True, fused=True) if fused else torch.optim.Adam(params, lr=lr, capturable=True)
        eager = _Run(steps=steps, lr=lr, use_hip_graph=True, optimizer=capturable_adam)
    p = graphed.p
    assert p.stats['graph_failures'] == 0 and p.graph_error is None, (p.stats, p.graph_error)
    assert p.stats['graph_blocks'] == len(p.report) >= 1 and p.stats['graph_replays'] == (steps - 1) * len(p.report)
    assert eager.p.stats['graph_blocks'] == 0 and eager.p.stats['graph_replays'] == 0 and eager.p.stats['eager_steps'] == steps * len(p.report)
    print('fused', fused, 'report', p.report)
    _assert_identical(eager, graphed)
    _assert_trained(graphed, steps, lr)
    _check_clean(graphed.graph, graphed.ex, graphed.delegators)


def test_graph_replay_against_eager_steps_of_the_reference_optimizer():
    """An extra: the replayed arm against eager steps of ``torch.optim.Adam``, the reference's optimizer.  The capturable fused Adam
    differs from it in the last bits of the step size, so the roundings are compared under the bound
    tests/test_gpu_roundtune.py states: ``steps * 2.1 * lr`` at most, 1e-6 on the median element.  A final weight may differ only
    where the eager rounding lies within that bound of .5; biases stay within the bound."""
    steps, lr = 20, 1e-3
    bound = steps * 2.1 * lr
    with _deterministic():
        eager = _Run(steps=steps, lr=lr, use_hip_graph=False)
        graphed = _Run(steps=steps, lr=lr, use_hip_graph=True)
    p = graphed.p
    assert p.stats['graph_failures'] == 0 and p.graph_error is None, (p.stats, p.graph_error)
    assert p.stats['graph_blocks'] == len(p.report) >= 1 and p.stats['graph_replays'] == (steps - 1) * len(p.report)
    assert eager.p.stats['graph_blocks'] == 0
    assert eager.p.report[0][1] == graphed.p.report[0][1]
    assert [b > a for _, a, b in eager.p.report] == [b > a for _, a, b in graphed.p.report], (eager.p.report, graphed.p.report)
    for name, (_, bias) in WEIGHTS.items():
        d = (eager.r[name] - graphed.r[name]).abs()
        assert float(d.max()) <= bound and float(d.median()) <= 1e-6, (name, float(d.max()), float(d.median()))
        near = (eager.r[name] - 0.5).abs() <= bound
        differ = eager.after[name] != graphed.after[name]
        assert not bool((differ & ~near).any()), (name, int((differ & ~near).sum()))
        assert float((eager.after[bias] - graphed.after[bias]).abs().max()) <= bound, bias
    _assert_trained(graphed, steps, lr)
    _check_clean(graphed.graph, graphed.ex, graphed.delegators)


def _prof_launches(fn):
    from ppq_amd import _lib
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    try: fn()
    finally:
        torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 64)()
    n = _lib.lib.ppqhip_prof_collect(arr, 64)
    return {arr[i].name.decode(): arr[i].launches for i in range(n)}


def test_kept_blocks_are_finalised_delegates_restored_and_one_launch_per_step():
    from ppq_amd import MXRoundTuningPass, mx_fake_quant, mx_round_forward
    steps = 20
    graph, ex, batches, delegators = _setup()
    before = _snapshot(graph)
    p = MXRoundTuningPass(steps=steps, lr=1e-3, use_hip_graph=False)
    p.keep_roundings = True
    launches = _prof_launches(lambda: p.optimize(graph, batches, ex))
    after = _snapshot(graph)
    n_blocks, n_weights = p.stats['blocks'], p.stats['mx_weights']
    assert n_blocks == len(p.report) >= 1 and n_weights == p.stats['grouped_weights'] == 3
    kept = [r for r in p.report if not r[2] > r[1]]
    assert len(kept) == n_blocks, p.report                                           # lr = 1e-3 improves this graph's one block
    # ONE grouped launch per step per block; the post-loss runs with the group's outputs dropped: one single-job launch per weight
    # per batch; a kept weight takes three more (the two selections `flipped` compares, and `finalize`).  One split per weight.
    assert launches.get('mx_round_fwd', 0) == steps * n_blocks + len(batches) * n_weights + 3 * n_weights, launches
    assert launches.get('mx_round_split', 0) == n_weights, launches
    flipped = 0
    for name in WEIGHTS:
        floored, rounding, codes = RR.split(before[name].cpu().numpy(), FMT, _axis(name))
        lo = floored
        hi = RR.forward(floored, np.ones_like(rounding), codes, FMT, _axis(name))
        w = after[name].cpu().numpy()
        assert np.all((w.view(np.uint32) == lo.view(np.uint32)) | (w.view(np.uint32) == hi.view(np.uint32))), name       # lo or hi of its original
        _same(after[name], RR.forward(floored, p.roundings[name].cpu().numpy(), codes, FMT, _axis(name)), name)           # the final rounding's
        again_codes = torch.zeros_like(_gpu(codes))
        assert torch.equal(mx_fake_quant(after[name], FMT, _axis(name), scale_codes=again_codes).view(torch.int32), after[name].view(torch.int32)), name
        _same(again_codes, codes, (name, 'codes'))                                   # the block scales did not move
        flipped += int((w.view(np.uint32) != RR.nearest(before[name].cpu().numpy(), FMT, _axis(name))[0].view(np.uint32)).sum())
    assert (p.stats['flipped'], p.stats['tuned_elements']) == (flipped, sum(before[n].numel() for n in WEIGHTS)), (p.stats, flipped)
    _check_clean(graph, ex, delegators)
    # a forward with the graph's own delegators has the bits of a forward with tuning delegators on the final roundings
    with _deterministic():
        plain = ex.forward(batches[0])[0].clone()
        tuned = {}
        for op in graph.operations.values():
            if op.type in ('Conv', 'Gemm'):
                name, cfg = op.inputs[1].name, op.config.input_quantization_config[1]
                f, _, c = (_gpu(a) for a in RR.split(before[name].cpu().numpy(), FMT, _axis(name)))
                tuned[cfg] = (lambda f, r, c, a: lambda tensor, config: mx_round_forward(f, r, c, FMT, a))(f, p.roundings[name], c, _axis(name))
        for cfg, fn in tuned.items(): ex.register_quantize_delegate(cfg, fn)
        try: with_tuning = ex.forward(batches[0])[0].clone()
        finally:
            for cfg in tuned: ex.register_quantize_delegate(cfg, delegators[cfg])
    _same(plain, with_tuning.cpu().numpy(), 'forward after the pass')
    print('report', p.report, 'flipped', flipped)


def test_a_block_that_ends_worse_is_restored_bit_for_bit():
    """Forced with a hostile learning rate: Adam moves every bias by about lr = 1 per step, far outside the activations' range, so the
    block ends worse.  Weight AND bias come back bit for bit -- the weight as the very tensor --, nothing is finalised or counted."""
    from ppq_amd import MXRoundTuningPass
    for graphed in (False, True):
        graph, ex, batches, delegators = _setup()
        before = _snapshot(graph)
        tensors = {v.name: v.value for op in graph.operations.values() for v in op.inputs if v.name in WEIGHTS}
        p = MXRoundTuningPass(steps=4, lr=1.0, use_hip_graph=graphed)
        p.optimize(graph, batches, ex)
        assert p.report and all(post > pre for _, pre, post in p.report), p.report
        after = _snapshot(graph)
        assert set(after) == set(before)
        for name in before: _same(after[name], before[name].cpu().numpy(), name)
        for op in graph.operations.values():
            for v in op.inputs:
                if v.name in WEIGHTS: assert v.value is tensors[v.name]
        assert p.stats['flipped'] == 0 and p.stats['tuned_elements'] == 0
        _check_clean(graph, ex, delegators)


def test_e4m3_even_and_linear_weights_are_skipped_untouched():
    from ppq_amd import LinearQuantizationConfig, MXRoundTuningPass, QuantizationStates, harness, quantize_graph_mx
    graph = RR.tiny_graph()
    ex = harness.TorchExecutor(graph, DEV)
    delegators = dict(quantize_graph_mx(graph, ex, 'MXFP8_E4M3', 'MXFP8_E4M3', operations=['c1'], weight_scale_rule='EVEN'))
    delegators.update(quantize_graph_mx(graph, ex, FMT, 'MXFP8_E4M3', operations=['c2', 'fc']))
    fc = graph.operations['fc']
    old = fc.config.input_quantization_config[1]
    linear = LinearQuantizationConfig(quant_min=-128, quant_max=127)
    linear.scale, linear.offset = torch.full((1,), 0.01, device=DEV), torch.zeros(1, device=DEV)
    linear.state = QuantizationStates.ACTIVATED
    fc.config.input_quantization_config[1] = linear
    ex.remove_quantize_delegate(old)
    del delegators[old]
    g = torch.Generator().manual_seed(7)
    batches = [torch.rand(4, 8, 8, 8, generator=g).to(DEV) for _ in range(4)]
    before = _snapshot(graph)
    p = MXRoundTuningPass(steps=20, lr=1e-3, use_hip_graph=False)
    p.optimize(graph, batches, ex)
    after = _snapshot(graph)
    assert set(p.skipped) == {'c1_w', 'fc_w'} and p.stats['skipped_weights'] == 2 and p.stats['mx_weights'] == 1, (p.skipped, p.stats)
    assert 'EVEN' in p.skipped['c1_w'] and 'not an MX config' in p.skipped['fc_w']
    for name in ('c1_w', 'fc_w'): _same(after[name], before[name].cpu().numpy(), name)
    assert not torch.equal(after['c2_w'], before['c2_w'])
    _check_clean(graph, ex, delegators)
    fc.config.input_quantization_config[1].state = QuantizationStates.FP32          # and a config that is not activated
    graph.operations['c2'].config.input_quantization_config[1].state = QuantizationStates.FP32
    p = MXRoundTuningPass(steps=3, lr=1e-3, use_hip_graph=False)
    p.optimize(graph, batches, ex)
    assert 'not activated' in p.skipped['c2_w'] and p.stats['mx_weights'] == 0 and all(r[1:] == (0.0, 0.0) for r in p.report)
    for name in WEIGHTS: _same(_snapshot(graph)[name], after[name].cpu().numpy(), name)


def test_effect_end_to_end_with_a_learning_rate_that_flips_roundings():
    """lr = 1e-2 for 20 steps: Adam moves a rounding by up to 0.2, enough to carry the elements that start within 0.2 of .5 across
    (the default 1e-4 x 500 steps moves it by 0.05 at most).  The value was chosen on the GPU so that roundings flip on this graph
    (77 of 3,680 elements there; 40 at lr = 1e-3).
    Asserted: no kept block ends with a larger loss than it began with -- exact --, and roundings did flip."""
    from ppq_amd import MXRoundTuningPass
    graph, ex, batches, delegators = _setup()
    before = _snapshot(graph)
    p = MXRoundTuningPass(steps=20, lr=1e-2)
    p.optimize(graph, batches, ex)
    assert p.stats['graph_failures'] == 0, p.graph_error
    after = _snapshot(graph)
    kept = [(name, pre, post) for name, pre, post in p.report if not post > pre]
    for name, pre, post in p.report: assert np.isfinite(pre) and np.isfinite(post) and pre > 0, (name, pre, post)
    assert all(post <= pre for _, pre, post in kept)
    assert len(kept) >= 1 and p.stats['flipped'] > 0 and p.stats['tuned_elements'] >= p.stats['flipped'], (p.report, p.stats)
    assert any(not torch.equal(after[n], before[n]) for n in WEIGHTS)
    _check_clean(graph, ex, delegators)
    print('report', p.report, f"flipped {p.stats['flipped']} of {p.stats['tuned_elements']}")
