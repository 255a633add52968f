"""GPU tests of AdaRound (ppq_amd/adaround.py, csrc/adaround.hip).

Kernel level: the forward and the main-path dV are compared BIT FOR BIT with the test-side torch restatement of legacy.py
(tests/golden/adaround_cases.py) run by torch on the same GPU -- same fp32 operations in the same order, torch.sigmoid's
`1 / (1 + exp(-v))` with the same device exp.  The regulariser's dV is compared with a float64 restatement within a bound
derived per element (see _reg_bound).  Against the reference's CPU outputs (tests/golden/adaround.npz) the only source of
difference is exp / log / pow of the CPU libraries: those comparisons use the same derived bounds.

Pass level: AdaroundPass against a test-side eager restatement of legacy.py:205-297 on the same blocks, the grouped against
the single-job launches, graph replay against eager, the regulariser modes, the keep / withdraw contract and the launch
count.  The vendor convolutions are switched to PyTorch's deterministic native kernels (cudnn off) where two runs are
compared bit for bit: MIOpen does not repeat every convolution bit for bit between calls (profiles/r07_epilogue_ab.txt)."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import adaround_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24


def _bits(t: torch.Tensor) -> np.ndarray:
    """Bit patterns, every NaN mapped to one canonical pattern (a NaN's payload carries no value)."""
    a = t.detach().float().contiguous().cpu().numpy()
    return np.where(np.isnan(a), np.float32('nan'), a).view(np.uint32)


def _item(w, v, s, o, axis, qmin, qmax):
    return (w, v, s, o, axis, qmin, qmax)


# A job has at most 1024 workgroups of 256 lanes (csrc/channel_axis.hpp): a lane takes a second trip through the float4 loop from
# 262,145 float4, through the element-wise loop (the unaligned variants) from 262,145 elements.  The three forms of the float4
# loop: per tensor (four channel computations per float4 with one channel; n % 4 = 1), elem_per_channel = 209,924 (a multiple of
# 4: one channel per float4; 262,405 float4) and elem_per_channel = 349,867 (odd: four channels per float4; 262,400 float4,
# n % 4 = 1).
_TRIP2 = (('trip2_pt', (1025, 1025), None, -128, 127), ('trip2_plane', (5, 52481, 2, 2), 0, -8, 7), ('trip2_lanes', (3, 349867), 0, -8, 7))


def _cases(extra: bool = True):
    """(name, w, v, scale, offset, axis, qmin, qmax, dy) on the GPU: the golden cases, larger / unaligned ones, and the
    smallest ones (_TRIP2) that send a lane through each loop of the kernels' walk a second time."""
    out = []
    for k, (name, shape, axis, qmin, qmax, _) in enumerate(AC.CASES):
        w, s, o, noise, dy = AC.case_tensors(k)
        v = AC.initiate_rounding(w, s, axis) + noise
        out.append((name, w, v, s, o, axis, qmin, qmax, dy))
    if extra:
        g = torch.Generator().manual_seed(77)
        for name, shape, axis, qmin, qmax in (('conv_big_i4', (64, 32, 3, 3), 0, -8, 7), ('gemm_big_pt', (257, 129), None, -128, 127),
                                              ('conv_plane7', (32, 16, 7, 7), 0, -128, 127)) + _TRIP2:
            w = torch.randn(shape, generator=g) * 0.3
            C = 1 if axis is None else shape[axis]
            s = (torch.rand(C, generator=g) * 0.02 + 0.01) if axis is not None else torch.tensor(0.013)
            o = torch.zeros_like(s)
            v = torch.randn(shape, generator=g) * 3
            # specials: NaN / inf weights, saturating V, exact-boundary values
            flat_w, flat_v = w.view(-1), v.view(-1)
            flat_w[:4] = torch.tensor([float('nan'), float('inf'), -float('inf'), -0.0])
            flat_v[4:8] = torch.tensor([100.0, -100.0, float('nan'), 0.0])
            flat_v[8:12] = 0.0                                   # inside both masks: the -0.0 of dy must come through
            dy = torch.randn(shape, generator=g)
            dy.view(-1)[8:12] = -0.0
            out.append((name, w, v, s, o, axis, qmin, qmax, dy))
    res = []
    for name, w, v, s, o, axis, qmin, qmax, dy in out:
        res.append((name, w.to(DEV), v.to(DEV), s.to(DEV), o.to(DEV), axis, qmin, qmax, dy.to(DEV)))
    return res


def _unaligned(t: torch.Tensor) -> torch.Tensor:
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    u = buf[1:].view(t.shape)
    u.copy_(t)
    assert u.data_ptr() % 16 != 0
    return u


def test_forward_kernel_is_bit_exact_against_torch_on_the_device():
    from ppq_amd.ffi import adaround_forward_multi
    cases = _cases()
    items = [_item(w, v, s, o, axis, qmin, qmax) for _, w, v, s, o, axis, qmin, qmax, _ in cases]
    single = [adaround_forward_multi([it])[0] for it in items]
    for (name, w, v, s, o, axis, qmin, qmax, _), got in zip(cases, single):
        want = AC.forward(w, v, s, o, axis, qmin, qmax)
        assert np.array_equal(_bits(got), _bits(want)), (name, int((_bits(got) != _bits(want)).sum()))
        un = adaround_forward_multi([_item(_unaligned(w), _unaligned(v), s, o, axis, qmin, qmax)])[0]
        assert np.array_equal(_bits(un), _bits(want)), name                     # the element-wise kernel
    grouped = adaround_forward_multi(items * 3)                                 # 27 jobs: two launches of <= 16
    for k, got in enumerate(grouped):
        assert np.array_equal(_bits(got), _bits(single[k % len(items)])), k


def test_main_path_dv_is_bit_exact_against_torch_autograd():
    from ppq_amd.ffi import adaround_backward_multi
    reg = torch.zeros(3, device=DEV)
    cases = _cases()
    items = [_item(w, v, s, o, axis, qmin, qmax) for _, w, v, s, o, axis, qmin, qmax, _ in cases]
    dys = [c[8] for c in cases]
    got_all = adaround_backward_multi(items, dys, reg)
    for (name, w, v, s, o, axis, qmin, qmax, dy), got in zip(cases, got_all):
        want = AC.grad_v(w, v, s, o, axis, qmin, qmax, dy)
        assert np.array_equal(_bits(got), _bits(want)), (name, int((_bits(got) != _bits(want)).sum()))
        one = adaround_backward_multi([_item(w, v, s, o, axis, qmin, qmax)], [dy], reg)[0]
        assert np.array_equal(_bits(one), _bits(got)), name
        un = adaround_backward_multi([_item(_unaligned(w), _unaligned(v), s, o, axis, qmin, qmax)], [_unaligned(dy)], reg)[0]
        assert np.array_equal(_bits(un), _bits(got)), name
    # -0.0 gradients keep their sign when the term is off (adding +0.0 would turn them into +0.0)
    k = [c[0] for c in cases].index('conv_plane7')
    got = got_all[k].view(-1)[8:12]
    assert all(np.signbit(got.cpu().numpy())) and torch.all(got == 0)


def _reg_bound(v64, s_sg_err=6.0):
    """float64 restatement of the regulariser's dV term r and a per-element bound for the float32 kernel.

    Forward error analysis, first order in u = 2^-24 (every fp32 operation correctly rounded, expf / powf within 2 ulp of
    the device libraries' documented 1 ulp): sg = 1 / (1 + exp(-v)) carries |d sg| <= sg * (2 + 1 + 1 + 2) u (exp, add, div,
    and the exp error propagated through the quotient); a = sg * 1.2f - 0.1f adds 1.2 |d sg| + u (1.2 sg + |a|); x = 2|h -
    0.5| adds 2 |d a| + u (1 + x); pow(x, beta - 1) turns an absolute error dx into (beta - 1) dx / x relative, plus 2 u;
    (1 - sg) carries (|d sg| + u) / (1 - sg) relative; the remaining 7 products (k beta p, *2, *sgn, *1.2, *(1 - sg), *sg,
    and the float32 constants 1.2f, beta, k themselves) at most 10 u.  The bound is |r| times the sum, doubled for the
    second-order terms.  Elements whose mask or sign can flip within that error (a within |d a| of 0 or 1, h within |d x|
    of 0.5) are returned in `unsure` and not compared."""
    sg = 1.0 / (1.0 + np.exp(-v64))
    dsg = sg * s_sg_err * U
    a = sg * 1.2 - 0.1
    da = 1.2 * dsg + U * (1.2 * sg + np.abs(a))
    h = np.clip(a, 0, 1)
    d = h - 0.5
    x = np.abs(d) * 2
    dx = 2 * da + U * (1 + x)
    unsure = (np.abs(a) <= da) | (np.abs(a - 1) <= da) | (np.abs(d) * 2 <= dx)
    return sg, a, h, d, x, dx, dsg, unsure


def _reg_term64(v64, k, beta, bm1):
    sg, a, h, d, x, dx, dsg, unsure = _reg_bound(v64)
    inside = (a >= 0) & (a <= 1)
    p = np.power(x, bm1)
    r = -float(k) * (float(beta) * p) * 2 * np.sign(d) * inside * 1.2 * (1 - sg) * sg
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = (float(bm1) * dx / x + 2 * U) + (dsg + U) / (1 - sg) + dsg / sg + 10 * U
    bound = np.where(r == 0, 0.0, 2 * np.abs(r) * np.nan_to_num(rel, nan=np.inf, posinf=np.inf))      # r == 0: exact in both
    return r, bound, unsure


def test_regulariser_dv_within_the_derived_bound_of_a_float64_restatement():
    from ppq_amd.adaround import AdaroundRegTerm
    from ppq_amd.ffi import adaround_backward_multi
    cases = [c for c in _cases() if not c[0].startswith('conv_big') and not c[0].startswith('gemm_big')] + \
        [c for c in _cases() if c[0] == 'conv_big_i4']
    checked = 0
    for it, max_iter in AC.REG_POINTS:
        host = AdaroundRegTerm(max_iter=max_iter).host_values(it, AC.GAMMA)
        reg = torch.from_numpy(host).to(DEV)
        zero = torch.zeros(3, device=DEV)
        for name, w, v, s, o, axis, qmin, qmax, dy in cases:
            w = torch.where(torch.isfinite(w), w, torch.zeros_like(w))
            v = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
            item = _item(w, v, s, o, axis, qmin, qmax)
            main = adaround_backward_multi([item], [dy], zero)[0]
            got = adaround_backward_multi([item], [dy], reg)[0]
            r, bound, unsure = _reg_term64(v.double().cpu().numpy(), host[0], host[1], host[2])
            err = np.abs(got.double().cpu().numpy() - (main.double().cpu().numpy() + r))
            # the final fp32 add, and float32's underflow of sg for v < -87 (r64 ~ 1e-40 where the kernel's r is 0)
            lim = bound + np.abs(main.double().cpu().numpy() + r) * U + 2.0 ** -120
            ok = (err <= lim) | unsure
            assert ok.all(), (name, it, float(err[~ok].max()), float(lim[~ok].min()))
            assert (~unsure).mean() > 0.95, name
            checked += int((~unsure).sum())
            # and the reference's own float32 autograd on this device agrees to the same bound
            want = AC.grad_v(w, v, s, o, axis, qmin, qmax, dy, it=it, max_iter=max_iter)
            err_t = np.abs(want.double().cpu().numpy() - got.double().cpu().numpy())
            assert ((err_t <= 2 * lim) | unsure).all(), name
    assert checked > 10000


def test_kernels_against_the_reference_goldens():
    """The reference's CPU outputs: forward within one quantisation step's rounding of the soft term (a CPU/GPU exp difference
    moves h by a few ulp), dV within the bounds above plus the same exp difference."""
    from ppq_amd.adaround import AdaroundRegTerm
    from ppq_amd.ffi import adaround_backward_multi, adaround_forward_multi
    gold = dict(np.load(os.path.join(HERE, 'golden', 'adaround.npz')))
    for k, (name, shape, axis, qmin, qmax, _) in enumerate(AC.CASES):
        p = f'c{k}_'
        w, s, o, v, dy = (torch.from_numpy(gold[p + x]).to(DEV) for x in ('w', 'scale', 'offset', 'v', 'dy'))
        item = _item(w, v, s, o, axis, qmin, qmax)
        init = AC.initiate_rounding(w, s, axis)                                  # torch log on the device vs the CPU's
        assert torch.allclose(init.cpu(), torch.from_numpy(gold[p + 'init']), rtol=16 * U, atol=16 * U * 4), name
        fwd = adaround_forward_multi([item])[0].cpu().numpy()
        s_el = np.broadcast_to(AC._view(s.cpu(), axis, w.dim()).numpy(), fwd.shape)
        t_mag = np.maximum(np.abs(gold[p + 'fwd'] / s_el), 1.0) + np.abs(qmax) + np.abs(qmin)
        assert (np.abs(fwd - gold[p + 'fwd']) <= s_el * 16 * U * t_mag).all(), name
        v64 = v.double().cpu().numpy()
        sg = 1 / (1 + np.exp(-v64))
        zero = torch.zeros(3, device=DEV)
        main = adaround_backward_multi([item], [dy], zero)[0].double().cpu().numpy()
        rel = 16 * U * (1 + sg / (1 - sg))
        assert (np.abs(main - gold[p + 'dv0']) <= np.abs(gold[p + 'dv0']) * rel + 1e-30).all(), name
        for j, (it, max_iter) in enumerate(AC.REG_POINTS):
            host = AdaroundRegTerm(max_iter=max_iter).host_values(it, AC.GAMMA)
            got = adaround_backward_multi([item], [dy], torch.from_numpy(host).to(DEV))[0].double().cpu().numpy()
            r, bound, unsure = _reg_term64(v64, host[0], host[1], host[2])
            lim = 2 * bound + np.abs(gold[p + f'dv{j + 1}']) * rel + 1e-30
            assert ((np.abs(got - gold[p + f'dv{j + 1}']) <= lim) | unsure).all(), (name, it)
        assert np.array_equal(AC.finalize(w, v, s, o, axis, qmin, qmax).cpu().numpy().view(np.uint32),
                              gold[p + 'final'].view(np.uint32)), name


# ---- the pass ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _deterministic():
    """Repeatable training runs, so that two of them can be compared bit for bit: PyTorch's native convolutions instead of MIOpen
    (which does not repeat every convolution bit for bit between calls, profiles/r07_epilogue_ab.txt) and PyTorch's
    deterministic algorithms (rocBLAS without atomics)."""
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
    snap = {}
    for op in graph.operations.values():
        for v in op.inputs:
            if v.is_parameter and isinstance(v.value, torch.Tensor): snap[('p', v.name)] = v.value.detach().clone()
        if hasattr(op, 'config'):
            for i, (c, v) in enumerate(op.config_with_variable):
                if isinstance(c.scale, torch.Tensor): snap[('s', op.name, i)] = c.scale.detach().clone()
    return snap


class _Run:
    """One pass on a fresh small CNN: the tensors before and after, the trained V of every AdaRound weight (taken before its
    block finalised or withdrew), the pass."""
    def __init__(self, pass_cls=None, **kw):
        from ppq_amd.adaround import AdaroundPass
        self.graph, self.ex, batches = _setup()
        self.before = _snapshot(self.graph)
        self.p = (pass_cls or AdaroundPass)(**kw)
        self.p.keep_roundings = True
        self.p.optimize(self.graph, batches, self.ex)
        self.after = _snapshot(self.graph)
        self.v = self.p.roundings

    def initial_v(self, name):
        """initiate_rounding of weight `name` from the tensors the pass started with (scale tuning off)."""
        for op in self.graph.operations.values():
            if hasattr(op, 'config') and len(op.inputs) > 1 and op.inputs[1].name == name:
                c = op.config.input_quantization_config[1]
                return AC.initiate_rounding(self.before[('p', name)], c.scale.detach(), c.channel_axis)
        raise KeyError(name)


class _TorchAdaRound:
    """legacy.py:67-136 with the torch ops (adaround_cases), for the restatement."""
    def __init__(self, var, config, steps):
        from ppq_amd.adaround import AdaroundRegTerm
        self.var, self.config, self.is_parameter = var, config, True
        self.axis = config.channel_axis if config.policy.has_property(__import__('ppq_amd').QuantizationProperty.PER_CHANNEL) else None
        self.reg = AdaroundRegTerm(max_iter=steps)
        self.rounding = AC.initiate_rounding(var.value.detach(), config.scale.detach(), self.axis).requires_grad_(True)
        self.param_backup = var.value.detach().clone()

    def trainable_tensors(self): return [self.rounding]

    def __call__(self, tensor, config):
        return AC.forward(tensor, self.rounding, config.scale, config.offset, self.axis, config.quant_min, config.quant_max)

    def regularization_loss(self, step): return self.reg.forward(r=self.rounding, iter=step)

    def finalize(self):
        with torch.no_grad():
            self.var.value = AC.finalize(self.var.value, self.rounding, self.config.scale, self.config.offset, self.axis,
                                         self.config.quant_min, self.config.quant_max)

    def withdraw(self):
        with torch.no_grad(): self.var.value.copy_(self.param_backup)


def _restatement_class():
    """A test-side eager restatement of legacy.py:205-297 over the same blocks (the pass's block split and data plumbing):
    per-weight CuLSQ scale tuning (Adam + MultiStepLR), torch-op AdaRound delegators, default torch.optim.Adam, the regulariser
    evaluated at the shadowed index.  Keeps every trained V in `roundings`, as the pass does with keep_roundings."""
    from ppq_amd.adaround import AdaroundPass
    from ppq_amd.blocks import COMPUTING_OP, block_forward, compute_block_loss, torch_mean_square_error
    from ppq_amd.core import QuantizationStates, state_value
    from ppq_amd.lsq import LSQDelegator

    class Restated(AdaroundPass):
        def finetune(self, block, executor, qt_inputs, fp_outputs):
            self.enable_block_gradient(block)
            pre = compute_block_loss(block, qt_inputs, fp_outputs, executor, torch_mean_square_error)
            steps = self.tune_steps
            for op in block.rps:
                if op.type in COMPUTING_OP and hasattr(op, 'config'):
                    c, v = op.config.input_quantization_config[1], op.inputs[1]
                    d = LSQDelegator(config=c, var=v, is_parameter_trainable=False)
                    params = d.trainable_tensors()
                    opt = torch.optim.Adam(params, lr=self.lr)
                    sch = torch.optim.lr_scheduler.MultiStepLR(opt, [int(steps / 2), int(steps * 2 / 3)])
                    initial = torch_mean_square_error(d(tensor=v.value, config=c), v.value)
                    for _ in range(steps):
                        opt.zero_grad()
                        loss = torch_mean_square_error(d(tensor=v.value, config=c), v.value)
                        loss.backward(); opt.step(); sch.step()
                    if torch_mean_square_error(d(tensor=v.value, config=c), v.value) > initial: d.withdraw()
            delegators, params = {}, []
            for op in block.rps:
                if not hasattr(op, 'config'): continue
                for cfg, var in op.config_with_variable:
                    if state_value(cfg.state) != QuantizationStates.ACTIVATED.value or not var.is_parameter: continue
                    d = _TorchAdaRound(var, cfg, self.steps)
                    params.extend(d.trainable_tensors()); executor.register_quantize_delegate(cfg, d); delegators[cfg] = d
            opt = torch.optim.Adam(params, lr=self.lr)
            names = [v.name for v in block.ep.outputs]
            for idx in range(self.steps):
                qt_input, fp_output = qt_inputs[idx % len(qt_inputs)], fp_outputs[idx % len(qt_inputs)]
                opt.zero_grad()
                outs = block_forward(executor, block.rps, qt_input, names, with_gradient=True)
                loss = 0.0
                for idx, name in enumerate(names): loss += torch_mean_square_error(outs[idx], fp_output[name])
                for d in delegators.values(): loss += d.regularization_loss(idx) * self.gamma
                loss.backward(); opt.step()
            post = compute_block_loss(block, qt_inputs, fp_outputs, executor, torch_mean_square_error)
            self.roundings.update({d.var.name: d.rounding.detach().clone() for d in delegators.values()})
            for cfg, d in delegators.items():
                d.withdraw() if post > pre else d.finalize()
                executor.remove_quantize_delegate(cfg)
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
    """Bit for bit: the reports, every trained V, every parameter and scale."""
    assert a.p.report == b.p.report, (a.p.report, b.p.report)
    assert set(a.v) == set(b.v) and len(a.v) >= 3
    for name in a.v: assert np.array_equal(_bits(a.v[name]), _bits(b.v[name])), name
    assert set(a.after) == set(b.after)
    for key in a.after: assert np.array_equal(_bits(a.after[key]), _bits(b.after[key])), key


def _assert_trained(r: _Run, steps: int, lr: float = 1e-3):
    """Every V moved from its initiate_rounding value, no element by more than Adam can move it in `steps` steps."""
    for name, v in r.v.items():
        d = (v - r.initial_v(name)).abs()
        assert float((d > 0).float().mean()) >= 0.5, name
        assert float(d.max()) <= steps * 2.1 * lr, name


def test_pass_equals_an_eager_restatement_of_the_reference():
    """AdaroundPass(use_hip_graph=False, group_weights=False) against the restatement of legacy.py:205-297 (torch-op delegators,
    default Adam) on the same blocks, with the scale tuning off: the reports, every trained V and every final tensor are
    identical bit for bit (the kernels are bit-exact against torch, tests above, and both runs are repeatable)."""
    from ppq_amd.blocks import split_graph_into_blocks
    with _deterministic():
        ref = _Run(_restatement_class(), steps=10, use_hip_graph=False, group_weights=False, tune_steps=0)
        ours = _Run(steps=10, use_hip_graph=False, group_weights=False, tune_steps=0)
    p = ours.p
    assert p.stats['adaround_weights'] >= 3 and p.stats['graph_blocks'] == 0 and p.stats['grouped_weights'] == 0
    assert [str(b) for b in split_graph_into_blocks(ours.graph, ours.graph.topological_sort(), 4)] == [r[0] for r in p.report]
    _assert_identical(ref, ours)
    _assert_trained(ours, 10)
    _check_clean(ours.graph, ours.ex)


def _assert_close_after_tuning(a: _Run, b: _Run, tune_steps: int, lr: float = 1e-3):
    """Two passes with the scale tuning on, whose per-channel LSQ scale gradients differ in summation order (the single-weight
    backward adds its partials with float atomics, ppq_amd/csrc/linear.hip): the LSQ tests' policy on EVERY tensor.  The
    first pre-loss is identical (nothing trained yet); a scale ends within `tune_steps` Adam steps; a final weight
    (q - o) * s on its grid differs by at most two grid steps of its channel (a floor or a rounding decision flipped) plus
    (qmax - qmin) times its scale's difference; at least half the tensors are identical."""
    assert a.p.report[0][1] == b.p.report[0][1]
    exact = 0
    for key in a.after:
        x, y = a.after[key], b.after[key]
        exact += bool(torch.equal(x, y))
        if key[0] == 's': assert float((x - y).abs().max()) <= tune_steps * 2.1 * lr, key
    for op in a.graph.operations.values():
        if not (hasattr(op, 'config') and op.type in ('Conv', 'Gemm')): continue
        i = 1
        c = op.config.input_quantization_config[i]
        sa, sb = a.after[('s', op.name, i)], b.after[('s', op.name, i)]
        shape = [-1] + [1] * (a.after[('p', op.inputs[1].name)].dim() - 1)
        lim = 2 * torch.maximum(sa, sb).view(shape) + (c.quant_max - c.quant_min) * (sa - sb).abs().view(shape) + 1e-7
        d = (a.after[('p', op.inputs[1].name)] - b.after[('p', op.inputs[1].name)]).abs()
        assert bool((d <= lim).all()), op.name
    assert exact >= (len(a.after) + 1) // 2, f'only {exact} of {len(a.after)} tensors identical'


def test_pass_with_scale_tuning_against_the_restatement():
    with _deterministic():
        ref = _Run(_restatement_class(), steps=4, use_hip_graph=False, group_weights=False, tune_steps=30)
        ours = _Run(steps=4, use_hip_graph=False, group_weights=False, tune_steps=30)
    assert ours.p.stats['tuned_weights'] >= 3
    _assert_close_after_tuning(ref, ours, 30)
    _check_clean(ours.graph, ours.ex)


def test_grouped_equals_single_job():
    """The grouped launches (one forward + one backward per step for all AdaRound weights of a block) against one job per
    weight, scale tuning off: bit for bit.  With the tuning on (LSQWeightGroup, whose scale gradient is summed in a fixed order,
    against the single-weight LSQ backward's atomics): the LSQ tests' policy."""
    with _deterministic():
        single = _Run(steps=6, use_hip_graph=False, group_weights=False, tune_steps=0)
        grouped = _Run(steps=6, use_hip_graph=False, group_weights=True, tune_steps=0)
        assert single.p.stats['grouped_weights'] == 0 and grouped.p.stats['grouped_weights'] >= 3
        _assert_identical(single, grouped)
        _assert_trained(grouped, 6)
        t_single = _Run(steps=2, use_hip_graph=False, group_weights=False, tune_steps=30)
        t_grouped = _Run(steps=2, use_hip_graph=False, group_weights=True, tune_steps=30)
    _assert_close_after_tuning(t_single, t_grouped, 30)


def _assert_replay_close(eager: _Run, graphed: _Run, steps: int, lr: float = 1e-3):
    """The LSQ tests' policy for the capturable Adam (same formula, device-side step counts: last-bit differences in the step
    size): every tensor and every V within `steps` lr-sized steps; and V agrees to 1e-6 on the median element -- a replay that
    did not train (or trained on a stale regulariser buffer) is off by lr-sized steps everywhere."""
    p = graphed.p
    assert p.stats['graph_failures'] == 0 and p.graph_error is None, (p.stats, p.graph_error)
    assert p.stats['graph_blocks'] == len(p.report) and p.stats['graph_replays'] == (steps - 1) * len(p.report)
    assert eager.p.stats['graph_blocks'] == 0
    assert eager.p.report[0][1] == graphed.p.report[0][1]
    for key in eager.after:
        assert float((eager.after[key] - graphed.after[key]).abs().max()) <= steps * 2.1 * lr, key
    assert set(eager.v) == set(graphed.v)
    for name in eager.v:
        d = (eager.v[name] - graphed.v[name]).abs()
        assert float(d.max()) <= steps * 2.1 * lr and float(d.median()) <= 1e-6, (name, float(d.max()), float(d.median()))


def test_graph_replay_equals_eager_steps():
    with _deterministic():
        eager = _Run(steps=6, use_hip_graph=False, tune_steps=0)
        graphed = _Run(steps=6, use_hip_graph=True, tune_steps=0)
    _assert_replay_close(eager, graphed, 6)
    _assert_trained(graphed, 6)
    _check_clean(graphed.graph, graphed.ex)


def test_regulariser_modes():
    """The default (the reference's shadowed index: never active on these 1-output blocks) trains exactly as gamma = 0 does,
    bit for bit; anneal_regularization=True (active from step 2 of 10) trains V differently, eagerly and replayed alike (the
    replays read the regulariser buffer before_step refreshes)."""
    from ppq_amd.adaround import AdaroundPass
    assert not AdaroundPass(steps=10)._reg_table(1, DEV).any() and not AdaroundPass(steps=10, gamma=0.0)._reg_table(1, DEV).any()
    with _deterministic():
        default = _Run(steps=10, use_hip_graph=False, tune_steps=0)
        no_reg = _Run(steps=10, use_hip_graph=False, tune_steps=0, gamma=0.0)
        anneal = _Run(steps=10, use_hip_graph=False, tune_steps=0, anneal_regularization=True, gamma=1000.0)
        anneal_g = _Run(steps=10, use_hip_graph=True, tune_steps=0, anneal_regularization=True, gamma=1000.0)
    _assert_identical(default, no_reg)
    for name in default.v:
        assert float((default.v[name] - anneal.v[name]).abs().median()) > 1e-4, name
    _assert_replay_close(anneal, anneal_g, 10)



def test_keep_withdraw_contract_clean_exit_and_one_launch_each_per_step():
    from ppq_amd import _lib
    from ppq_amd.blocks import split_graph_into_blocks
    graph, ex, batches = _setup()
    before = _snapshot(graph)
    from ppq_amd.adaround import AdaroundPass
    p = AdaroundPass(steps=5, use_hip_graph=False, tune_steps=0)
    torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(1)
    try:
        p.optimize(graph, batches, ex)
    finally:
        torch.cuda.synchronize(); _lib.lib.ppqhip_prof_enable(0)
    arr = (_lib.ProfEntry * 32)()
    n = _lib.lib.ppqhip_prof_collect(arr, 32)
    launches = {arr[i].name.decode(): arr[i].launches for i in range(n)}
    blocks = split_graph_into_blocks(graph, graph.topological_sort(), 4)
    assert [str(b) for b in blocks] == [r[0] for r in p.report]
    n_blocks = p.stats['blocks']
    assert launches.get('adaround_bwd', 0) == 5 * n_blocks, launches
    # forward: ONE grouped launch per step per block, and the post-loss forwards (one per weight per batch)
    assert launches.get('adaround_fwd', 0) == 5 * n_blocks + len(batches) * p.stats['adaround_weights'], launches
    after = _snapshot(graph)
    for block, (_, pre, post) in zip(blocks, p.report):
        assert np.isfinite(pre) and np.isfinite(post)
        for op in block.rps:
            if not hasattr(op, 'config') or op.type not in ('Conv', 'Gemm'): continue
            w, c = after[('p', op.inputs[1].name)], op.config.input_quantization_config[1]
            q = w / c.scale.view([-1] + [1] * (w.dim() - 1))
            on_grid = bool(((q - q.round()).abs() <= 1e-3).all())
            if post <= pre: assert on_grid, op.name                                   # finalize: the hard rounding
            else: assert torch.equal(w, before[('p', op.inputs[1].name)]), op.name    # withdraw (tune_steps=0: no W training)
    _check_clean(graph, ex)


def test_a_training_step_that_raises_leaves_the_block_as_it_was_found():
    """The failure path of the block-training frame (tests/test_host_block_training.py runs it on the CPU
    through the MX pass): the third gradient forward of the first block raises -- a Python exception, before that step launches
    anything -- after two optimizer steps on V and the activation scales.  ``tune_block_weight_scale`` runs before the first
    delegator exists and is not taken back, so "as found" is the first block after its scale tuning: a twin graph taken to that
    point.  Every tensor equals the twin's bit for bit, no delegate of the pass is registered, nothing keeps ``requires_grad``."""
    from block_training_double import StepRefused, assert_same_bits, refuse_gradient_forward, snapshot
    from ppq_amd.adaround import AdaroundPass
    from ppq_amd.blocks import split_graph_into_blocks
    kw = dict(steps=4, use_hip_graph=False, tune_steps=5, is_scale_trainable=True)
    with _deterministic():
        twin, _, _ = _setup()
        p = AdaroundPass(**kw)
        first = split_graph_into_blocks(twin, twin.topological_sort(), p.block_size)[0]
        p.enable_block_gradient(first); p.tune_block_weight_scale(first); p.disable_block_gradient(first)
        graph, ex, batches = _setup()
        untuned = snapshot(graph)
        with refuse_gradient_forward(ex, at=3) as seen, pytest.raises(StepRefused, match='gradient forward 3 refused'):
            AdaroundPass(**kw).optimize(graph, batches, ex)
    assert seen[0] == 3
    as_found = snapshot(twin)
    assert any(not torch.equal(as_found[k], untuned[k]) for k in as_found)           # the tuning did move the first block
    assert_same_bits(snapshot(graph), as_found)
    _check_clean(graph, ex)


def test_early_exit_leaves_nothing_trainable():
    """(d): a block with nothing to train returns (0, 0) with nothing requires_grad (the reference leaves it set)."""
    from ppq_amd.adaround import AdaroundPass
    from ppq_amd.core import QuantizationStates
    graph, ex, batches = _setup()
    for op in graph.operations.values():
        if hasattr(op, 'config'):
            for cfg, var in op.config_with_variable:
                if var.is_parameter and cfg.state == QuantizationStates.ACTIVATED: cfg.state = QuantizationStates.FP32
    p = AdaroundPass(steps=2, use_hip_graph=False, tune_steps=0)
    p.optimize(graph, batches, ex)
    assert all(r[1:] == (0.0, 0.0) for r in p.report) and p.report
    _check_clean(graph, ex)


def test_yolov6s_int4_adaround_few_steps():
    """The YOLOv6-s-like detector, INT4 per-channel weights, block_size 4, a few steps: box-independent assertions only
    (tests/test_gpu_finetune.py explains why)."""
    from ppq_amd import harness
    from ppq_amd.adaround import AdaroundPass
    from ppq_amd.blocks import split_graph_into_blocks
    from ppq_amd.calibration import RuntimeCalibrationPass
    graph = harness.yolov6s_graph(seed=3)
    harness.quantize_graph(graph, 'minmax')
    _int4_weights(graph)
    ex = harness.TorchExecutor(graph, DEV)
    harness.ParameterQuantizePass().optimize(graph)
    g = torch.Generator().manual_seed(9)
    batches = [torch.rand(2, 3, 160, 160, generator=g).to(DEV) for _ in range(4)]
    RuntimeCalibrationPass(check_steps=False).optimize(graph, dataloader=batches, executor=ex, calib_steps=4)
    p = AdaroundPass(steps=4, tune_steps=10)
    pre, post = p.optimize(graph, batches, ex)
    blocks = split_graph_into_blocks(graph, graph.topological_sort(), 4)
    assert len(blocks) == len(p.report) and p.stats['adaround_weights'] == 56
    assert p.stats['graph_failures'] == 0, p.graph_error
    assert np.isfinite([pre, post]).all() and 0 < post <= pre
    _check_clean(graph, ex)
    outs = ex.forward(batches[0], list(graph.outputs))
    assert all(torch.isfinite(o).all() for o in outs)
    print(f'AdaRound on {len(blocks)} blocks: block loss {pre:.4f} -> {post:.4f}; kept {sum(1 for _, a, b in p.report if b <= a)}')
