"""MX round tuning without a GPU: the ``use_kernels=False`` arm of ppq_amd.mx_roundtune against the table
oracle (tests/mx_round_reference.py) bit for bit, the two properties the pass relies on -- (a) the initial rounding selects what
``mx_fake_quant`` gives, (b) every selection is a fixed point of ``mx_fake_quant`` -- with the MXFP8_E4M3 / EVEN counter-example built
by hand, the packed export of a tuned weight, and the argument checks of the C entry points and of the Python functions (they run
before any launch, so they need no device).  Everything is compared with == on bits."""
import ctypes

import numpy as np
import pytest
import torch

import mx_reference as R
import mx_round_reference as RR
import mx_scale_reference as S
from ppq_amd import (MXFormat, MXRoundTuningDelegator, MXRoundTuningPass, MXScaleRule, _lib, export_graph_mx, ffi, mx_dequantize, mx_fake_quant,
                     mx_round_forward, mx_round_split, quantize_graph_mx)

FORMATS, RULES = R.FORMATS, S.RULES
COMBOS = [(f, r) for f in FORMATS for r in RULES]


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a))


def _same(got, want, what):
    got, want = got.numpy() if isinstance(got, torch.Tensor) else got, np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = np.uint32 if got.dtype == np.float32 else got.dtype
    bad = np.flatnonzero(got.view(view).ravel() != want.view(view).ravel())
    assert bad.size == 0, f'{what}: {bad.size} elements differ, first at {bad[:4]}: {got.ravel()[bad[:4]]} != {want.ravel()[bad[:4]]}'


def _roundings(shape, seed: int) -> np.ndarray:
    """Uniform roundings with the corner values of the contract planted at the front."""
    r = np.random.default_rng(seed).random(shape, dtype=np.float32)
    r.reshape(-1)[:len(RR.ROUNDINGS)] = RR.ROUNDINGS
    return r


def _check_both(x: np.ndarray, fmt: str, rule: str, axis: int, what):
    """Split and forward of the torch arm against the oracle; returns (floored, rounding, codes) as arrays."""
    floored, rounding, codes = mx_round_split(_t(x), fmt, axis, rule, use_kernels=False)
    want = RR.split(x, fmt, axis, rule)
    for name, g, w in zip(('floored', 'rounding', 'codes'), (floored, rounding, codes), want): _same(g, w, (what, name))
    for k, r in enumerate((want[1], _roundings(x.shape, 17))):                      # the split's own rounding and a wild one
        out = mx_round_forward(floored, _t(r), codes, fmt, axis, use_kernels=False)
        _same(out, RR.forward(want[0], r, want[2], fmt, axis), (what, 'forward', k))
    return want


# ---- the torch arm against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt, rule', COMBOS)
def test_torch_arm_equals_the_oracle_on_random_and_special_blocks(fmt, rule):
    for name, blocks in (('scaled', RR.scaled_blocks(1)), ('gaussian', S.gaussian_blocks()[:64]), ('special', RR.special_rows(fmt))):
        _check_both(blocks, fmt, rule, -1, (fmt, rule, name))


@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arm_layouts(fmt):
    for k, (shape, axis) in enumerate(R.LAYOUTS):
        x = RR.plant_specials(R.layout_input(shape, seed=k), fmt)
        for rule in ('FLOOR', 'MSE'): _check_both(x, fmt, rule, axis, (fmt, rule, shape, axis))


def test_known_answers_fp4():
    """MXFP4 under X = 1 (an element of 4.0 leads the block): the grid is 0, .5, 1, 1.5, 2, 3, 4, 6."""
    x = np.zeros(32, np.float32)
    x[:10] = [4.0, 0.3, -1.3, 2.6, 5.1, -7, 0.75, 6.0, -0.0, 3.0]
    floored, rounding, codes = mx_round_split(_t(x), 'MXFP4_E2M1', use_kernels=False)
    assert codes.tolist() == [127]
    assert floored[:10].tolist() == [4.0, 0.0, -1.0, 2.0, 4.0, -6.0, 0.5, 6.0, -0.0, 3.0]
    want = np.array([0, 0.3 / 0.5, (1.3 - 1) / 0.5, (2.6 - 2) / 1, (5.1 - 4) / 2, 0, 0.5, 0, 0, 0])
    got = rounding[:10].numpy().astype(np.float64)
    assert np.all(np.abs(got - want) < 1e-6) and got[6] == 0.5 and got[5] == 0.0
    assert torch.signbit(floored[8]) and not torch.signbit(floored[1])
    up = mx_round_forward(floored, torch.ones(32), codes, 'MXFP4_E2M1', use_kernels=False)
    assert up[:10].tolist() == [6.0, 0.5, -1.5, 3.0, 6.0, -6.0, 1.0, 6.0, -0.5, 4.0]


# ---- property (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt, rule', COMBOS)
def test_the_initial_rounding_selects_round_to_nearest_even_but_at_ties(fmt, rule):
    ties = mismatches = 0
    for blocks in (RR.scaled_blocks(2, 512), RR.special_rows(fmt)):
        x = _t(blocks)
        floored, rounding, codes = mx_round_split(x, fmt, -1, rule, use_kernels=False)
        selected = mx_round_forward(floored, rounding, codes, fmt, use_kernels=False)
        nearest = mx_fake_quant(x, fmt, use_kernels=False, scale_rule=rule)
        differ = selected.view(torch.int32) != nearest.view(torch.int32)
        tie = rounding == .5
        mismatches += int((differ & ~tie).sum())
        ties += int(tie.sum())
        assert torch.equal(selected[tie], floored[tie])                             # a tie goes down here
    assert mismatches == 0 and ties > 0, (mismatches, ties)


# ---- property (b) ---------------------------------------------------------------------------------------------------------------------
def _weight_like(rows: np.ndarray) -> np.ndarray:
    """The rows a weight can hold and DESIGN.md section 9.17 does not except from idempotence: no +-Inf (a saturated Inf is a new amax)
    and no amax in float32's last binade (a raised scale takes the product cast(v / X) * X to 2^128 = Inf there)."""
    amax = np.abs(np.where(np.isfinite(rows), rows, np.float32(0))).max(axis=1)
    return rows[~np.isinf(rows).any(axis=1) & (amax < 2.0 ** 127)]


def _changed_blocks(fmt: str, rule: str, x: np.ndarray, seed: int):
    """(blocks of 32 of ``x`` [n, 32 k] whose random selection ``mx_fake_quant`` changes, blocks whose codes it changes)."""
    x = _t(x)
    floored, _, codes = mx_round_split(x, fmt, -1, rule, use_kernels=False)
    out = mx_round_forward(floored, _t(_roundings(tuple(x.shape), seed + 100)), codes, fmt, use_kernels=False)
    again_codes = torch.zeros_like(codes)
    again = mx_fake_quant(out, fmt, scale_codes=again_codes, use_kernels=False, scale_rule=rule)
    changed = (again.view(torch.int32) != out.view(torch.int32)).reshape(x.shape[0], -1, 32).any(dim=-1)
    return int(changed.sum()), int((again_codes != codes).sum())


@pytest.mark.parametrize('fmt, rule', COMBOS)
def test_every_selection_is_a_fixed_point_of_the_fake_quant(fmt, rule):
    """On 1,024 random blocks over 2^+-100 and on the special blocks a weight can hold (zeros, subnormals, NaN, ties, values on the
    grid, a saturating amax)."""
    for x in (RR.scaled_blocks(3, 512), _weight_like(RR.special_rows(fmt))):
        changed, codes_changed = _changed_blocks(fmt, rule, x, seed=3)
        if (fmt, rule) == ('MXFP8_E4M3', 'EVEN'):
            assert changed > 0                                                       # the one combination the pass refuses
            continue
        assert changed == 0
        if rule == 'FLOOR': assert codes_changed == 0                                # the largest element keeps its binade


def test_e4m3_even_counter_example():
    """amax = 1.97 rounds up into the next binade under EVEN: code 120, X = 2^-7, u = 252.16 between 240 and 256.  Taking 240 makes
    the block's largest element 1.875, which EVEN does not bump: code 119, u = 480 -- above E4M3's largest normal 448 = 1.75 * 2^8."""
    x = np.zeros(32, np.float32)
    x[:2] = [1.97, 0.5]
    floored, rounding, codes = mx_round_split(_t(x), 'MXFP8_E4M3', -1, 'EVEN', use_kernels=False)
    assert codes.tolist() == [120] and floored[0].item() == 1.875 and 0.5 < rounding[0].item() < 1
    again_codes = torch.zeros_like(codes)
    again = mx_fake_quant(floored, 'MXFP8_E4M3', scale_codes=again_codes, use_kernels=False, scale_rule='EVEN')
    assert again_codes.tolist() == [119] and again[0].item() == 1.75 and again[1].item() == 0.5
    for rule in ('FLOOR', 'CEIL', 'MSE'):                                            # the same block under the other rules
        f, _, c = mx_round_split(_t(x), 'MXFP8_E4M3', -1, rule, use_kernels=False)
        assert torch.equal(mx_fake_quant(f, 'MXFP8_E4M3', use_kernels=False, scale_rule=rule), f), rule
    assert MXRoundTuningPass.refusal(_config('MXFP8_E4M3', 'EVEN')) is not None and MXRoundTuningPass.refusal(_config('MXFP8_E4M3', 'CEIL')) is None


def _config(fmt: str, rule: str = 'FLOOR'):
    from ppq_amd.mx import _mx_config
    return _mx_config(MXFormat[fmt], 'cpu', MXScaleRule[rule])


# ---- the tuned weight in the export -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', ['FLOOR', 'CEIL'])
def test_export_and_dequantize_give_the_tuned_weights_bits(rule):
    from ppq_amd import harness
    graph = RR.tiny_graph()
    ex = harness.TorchExecutor(graph, 'cpu')
    quantize_graph_mx(graph, ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=False, weight_scale_rule=rule)
    tuned = {}
    for k, op in enumerate(op for op in graph.operations.values() if op.type in ('Conv', 'Gemm')):
        cfg, var = op.config.input_quantization_config[1], op.inputs[1]
        d = MXRoundTuningDelegator(var, cfg, cfg.detail['MX_FORMAT'], 1 if op.type == 'Conv' else -1, rule, use_kernels=False)
        with torch.no_grad(): d.rounding.copy_(_t(_roundings(tuple(var.value.shape), k)))
        d.finalize()
        tuned[var.name] = var.value
    packed = export_graph_mx(graph, use_kernels=False)
    assert set(packed) == set(tuned) and len(tuned) == 3
    for name, w in tuned.items():
        assert not w.requires_grad
        _same(mx_dequantize(packed[name], use_kernels=False), w.numpy(), name)


def test_delegator_replaces_withdraws_and_passes_through():
    from ppq_amd.core import QuantizationStates
    from ppq_amd.harness import Variable
    w = _t(R.layout_input((6, 70), seed=4))
    var, cfg = Variable('w', value=w, is_parameter=True), _config('MXFP4_E2M1')
    d = MXRoundTuningDelegator(var, cfg, 'MXFP4_E2M1', -1, 'FLOOR', use_kernels=False)
    floored, rounding, codes = RR.split(w.numpy(), 'MXFP4_E2M1')
    _same(var.value, floored, 'floored'); _same(d.rounding.detach(), rounding, 'rounding'); _same(d.scale_codes, codes, 'codes')
    assert d.trainable_tensors() == [d.rounding] and d.rounding.requires_grad and int(d.flipped()) == 0
    y = d(var.value, cfg)
    _same(y.detach(), RR.forward(floored, rounding, codes, 'MXFP4_E2M1'), 'forward')
    dy = torch.randn(6, 70)
    (y * dy).sum().backward()
    _same(d.rounding.grad, dy.numpy(), 'dR == dy')
    with torch.no_grad(): d.rounding.copy_(1 - d.rounding)                            # every open element to the other side
    other = RR.forward(floored, 1 - rounding, codes, 'MXFP4_E2M1')                   # a saturated element and an exact tie stay
    assert int(d.flipped()) == int((other != RR.forward(floored, rounding, codes, 'MXFP4_E2M1')).sum()) > 300
    cfg.state = QuantizationStates.FP32
    assert d(var.value, cfg) is var.value                                            # not activated: passes through
    d.withdraw()
    assert var.value is w
    with pytest.raises(ValueError, match='not a fixed point'):
        MXRoundTuningDelegator(var, _config('MXFP8_E4M3', 'EVEN'), 'MXFP8_E4M3', -1, 'EVEN', use_kernels=False)
    assert var.value is w


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_python_argument_checks():
    x = torch.zeros(4, 64)
    floored, rounding, codes = mx_round_split(x, 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(TypeError): mx_round_split(np.zeros(4), 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='Invalid dtype'): mx_round_split(x.half(), 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='out of range'): mx_round_split(x, 'MXFP4_E2M1', axis=2, use_kernels=False)
    with pytest.raises(ValueError, match='unknown MX format'): mx_round_split(x, 'MXFP4_E3M0', use_kernels=False)
    with pytest.raises(ValueError, match='unknown MX scale rule'): mx_round_split(x, 'MXFP4_E2M1', scale_rule='ROUND', use_kernels=False)
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_round_split(x, 'MXFP4_E2M1')
    with pytest.raises(RuntimeError, match='not on the GPU'): mx_round_forward(floored, rounding, codes, 'MXFP4_E2M1')
    with pytest.raises(RuntimeError, match='rounding must be'): mx_round_forward(floored, rounding[:2], codes, 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='rounding must be'): mx_round_forward(floored, rounding.double(), codes, 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='scale_codes'): mx_round_forward(floored, rounding, None, 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='scale_codes'): mx_round_forward(floored, rounding, codes[:, :1], 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(RuntimeError, match='scale_codes'): mx_round_forward(floored, rounding, codes.int(), 'MXFP4_E2M1', use_kernels=False)
    with pytest.raises(ValueError, match='unknown MX format'): mx_round_forward(floored, rounding, codes, 7, use_kernels=False)


def test_c_entry_points_check_arguments_without_a_device():
    """Format, rule, sizes, null pointers, alignment, the job table and overlap are checked on the host before anything is launched."""
    lib = _lib.lib
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data
    w, fl, r, c, out = p, p + 1024, p + 2048, p + 3072, p + 3328

    def split(*job):
        jobs = np.zeros(1, dtype=ffi._MX_ROUND_SPLIT_JOB)
        jobs[0] = job
        return lib.ppqhip_mx_round_split_multi(jobs.ctypes.data, 1, None), _lib.last_error()

    def fwd(*job):
        jobs = np.zeros(1, dtype=ffi._MX_ROUND_FWD_JOB)
        jobs[0] = job
        return lib.ppqhip_mx_round_fwd_multi(jobs.ctypes.data, 1, None), _lib.last_error()

    what = 'mx_round_split_multi'
    assert split(w, fl, r, c, 1, 64, 1, 6, 0) == (-1, f'{what}: job 0: unknown MX format 6')
    assert split(w, fl, r, c, 1, 64, 1, 4 | 4 << 8, 0) == (-1, f'{what}: job 0: unknown MX scale rule in format {4 | 4 << 8}')
    assert split(w, fl, r, c, 1, 64, 1, -1, 0)[0] == -1
    assert split(w, fl, r, c, -1, 64, 1, 4, 0) == (-1, f'{what}: job 0: negative size')
    assert split(w, fl, r, c, 1 << 20, 1 << 20, 1, 4, 0) == (-1, f'{what}: job 0: more than 2^31 - 1 elements')
    for k in range(4):
        job = [w, fl, r, c, 1, 64, 1, 4 | 3 << 8, 0]
        job[k] = 0
        assert split(*job) == (-1, f'{what}: job 0 has a null pointer')
    assert split(w + 2, fl, r, c, 1, 64, 1, 4, 0) == (-1, f'{what}: job 0: a float pointer is not 4-byte aligned')
    assert split(w, fl, r + 1, c, 1, 64, 1, 4, 0) == (-1, f'{what}: job 0: a float pointer is not 4-byte aligned')
    assert split(w, w, r, c, 1, 64, 1, 4, 0) == (-1, f'{what}: an output overlaps an input')              # no in-place split
    assert split(w, fl, fl + 4, c, 1, 64, 1, 4, 0) == (-1, f'{what}: two outputs overlap in memory')
    assert split(w, fl, r, fl + 255, 1, 64, 1, 4, 0) == (-1, f'{what}: two outputs overlap in memory')    # the codes' first byte in floored
    assert split(w, fl, r, w + 128, 1, 64, 1, 4, 0) == (-1, f'{what}: an output overlaps an input')
    assert split(w, fl, r, c, 0, 64, 1, 4, 0)[0] == 0                                                    # empty: nothing to launch
    assert split(0, 0, 0, 0, 1, 0, 1, 4 | 2 << 8, 0)[0] == 0
    assert lib.ppqhip_mx_round_split_multi(None, 0, None) == 0
    assert lib.ppqhip_mx_round_split_multi(None, 2, None) == -1 and _lib.last_error() == f'{what}: bad job table'
    assert lib.ppqhip_mx_round_split_multi(buf.ctypes.data, -1, None) == -1 and _lib.last_error() == f'{what}: bad job table'
    jobs = np.zeros(2, dtype=ffi._MX_ROUND_SPLIT_JOB)
    jobs[0] = (w, fl, r, c, 1, 64, 1, 4, 0)
    jobs[1] = (w, fl + 128, r + 512, c + 8, 1, 64, 1, 9, 0)
    assert lib.ppqhip_mx_round_split_multi(jobs.ctypes.data, 2, None) == -1 and _lib.last_error() == f'{what}: job 1: unknown MX format 9'
    jobs[1]['format'] = 0
    assert lib.ppqhip_mx_round_split_multi(jobs.ctypes.data, 2, None) == -1 and _lib.last_error() == f'{what}: two outputs overlap in memory'

    what = 'mx_round_fwd_multi'
    assert fwd(fl, r, c, out, 1, 64, 1, 6, 0) == (-1, f'{what}: job 0: unknown MX format 6')
    assert fwd(fl, r, c, out, 1, 64, 1, 4 | 1 << 8, 0) == (-1, f'{what}: job 0: format {4 | 1 << 8} carries a scale rule, but the codes are given')
    assert fwd(fl, r, c, out, 1, 64, 1, -1, 0)[0] == -1
    assert fwd(fl, r, c, out, 1, -64, 1, 4, 0) == (-1, f'{what}: job 0: negative size')
    assert fwd(fl, r, c, out, 1 << 20, 1 << 20, 1, 4, 0) == (-1, f'{what}: job 0: more than 2^31 - 1 elements')
    for k in range(4):
        job = [fl, r, c, out, 1, 64, 1, 4, 0]
        job[k] = 0
        assert fwd(*job) == (-1, f'{what}: job 0 has a null pointer')
    assert fwd(fl, r, c, out + 3, 1, 64, 1, 4, 0) == (-1, f'{what}: job 0: a float pointer is not 4-byte aligned')
    assert fwd(fl, r, c, fl, 1, 64, 1, 4, 0) == (-1, f'{what}: an output overlaps an input')              # no in-place forward
    assert fwd(fl, r, c, r + 252, 1, 64, 1, 4, 0) == (-1, f'{what}: an output overlaps an input')
    assert fwd(fl, r, out + 8, out, 1, 64, 1, 4, 0) == (-1, f'{what}: an output overlaps an input')       # the codes inside the output
    assert fwd(fl, r, c, out, 1, 64, 0, 4, 0)[0] == 0
    assert lib.ppqhip_mx_round_fwd_multi(None, 0, None) == 0
    assert lib.ppqhip_mx_round_fwd_multi(None, 1, None) == -1 and _lib.last_error() == f'{what}: bad job table'
    jobs = np.zeros(2, dtype=ffi._MX_ROUND_FWD_JOB)
    jobs[0] = (fl, r, c, out, 1, 64, 1, 4, 0)
    jobs[1] = (fl, r, c, out + 128, 1, 64, 1, 0, 0)                                                      # shared inputs are fine ...
    assert lib.ppqhip_mx_round_fwd_multi(jobs.ctypes.data, 2, None) == -1 and _lib.last_error() == f'{what}: two outputs overlap in memory'
    # the layouts of ppqhip_mx_round_split_job / ppqhip_mx_round_fwd_job
    assert ctypes.sizeof(ctypes.c_void_p) * 4 + 8 * 3 + 8 == ffi._MX_ROUND_SPLIT_JOB.itemsize == ffi._MX_ROUND_FWD_JOB.itemsize


def test_an_executor_that_refuses_the_delegator_finds_its_weights_as_they_were():
    """The reference's executor admits a delegate by isinstance: a refusal half-way through a block withdraws every weight that was
    floored so far -- the refused one included -- and leaves the graph's own delegates registered."""
    from ppq_amd import harness

    class Picky(harness.TorchExecutor):
        def register_quantize_delegate(self, config, delegator):
            if isinstance(delegator, MXRoundTuningDelegator) and delegator.var.name == 'c2_w': raise TypeError('not a delegator of mine')
            super().register_quantize_delegate(config, delegator)

    graph = RR.tiny_graph()
    ex = Picky(graph, 'cpu')
    held = dict(quantize_graph_mx(graph, ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=False))
    tensors = {v.name: v.value for op in graph.operations.values() for v in op.inputs if v.is_parameter}
    batches = [torch.rand(2, 8, 8, 8, generator=torch.Generator().manual_seed(k)) for k in range(2)]
    p = MXRoundTuningPass(steps=2, use_hip_graph=False, use_kernels=False)
    with pytest.raises(TypeError, match='not a delegator of mine'): p.optimize(graph, batches, ex)
    for op in graph.operations.values():
        for v in op.inputs:
            if v.is_parameter: assert v.value is tensors[v.name] and not v.value.requires_grad, v.name
    assert set(ex._delegates) == set(held) and all(ex._delegates[c] is d for c, d in held.items())
