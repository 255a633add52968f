"""The MX scale rules without a GPU: the oracle (tests/mx_scale_reference.py) against the floor oracle and
its own properties, the ``use_kernels=False`` arms of ppq_amd.mx against the oracle bit for bit for every format and rule, the
plumbing through graph, export and delegator, and the argument encoding of the C entry points (checked before any launch)."""
import numpy as np
import pytest
import torch

import mx_pack_reference as P
import mx_reference as R
import mx_scale_reference as S
from ppq_amd import MXDelegator, MXFormat, MXScaleRule, _lib, ffi, harness, mx_dequantize, mx_fake_quant, mx_quantize
from ppq_amd.mx import _config_rule, export_graph_mx, quantize_graph_mx

FORMATS = R.FORMATS
RULES = S.RULES
NEW_RULES = S.NEW_RULES


def torch_arm(x: np.ndarray, fmt: str, axis: int, rule: str):
    t = torch.from_numpy(np.ascontiguousarray(x))
    shape = list(t.shape)
    shape[axis % t.dim()] = (shape[axis % t.dim()] + 31) // 32
    codes = torch.zeros(shape, dtype=torch.uint8)
    y = mx_fake_quant(t, fmt, axis, scale_codes=codes, use_kernels=False, scale_rule=rule)
    return y.numpy(), codes.numpy()


def check_both_arms(x: np.ndarray, fmt: str, axis: int, rule: str, what):
    """The fake quant and the packed export of the torch arm against the oracle: values, codes, scales and the round trip."""
    want, want_codes, _ = S.quantize(x, fmt, axis, rule)
    got, got_codes = torch_arm(x, fmt, axis, rule)
    assert np.array_equal(got_codes, want_codes), f'{what}: scale codes differ'
    bad = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
    assert bad.size == 0, f'{what}: {bad.size} elements differ, first at {bad[:4]}'
    t = torch.from_numpy(np.ascontiguousarray(x))
    packed = mx_quantize(t, fmt, axis, use_kernels=False, scale_rule=rule)
    mask = P.nan_mask(x, fmt, axis)
    dead = np.moveaxis(mask, axis % x.ndim, -1)                                            # a block that is NaN as a whole: scale 0xFF
    dead = np.stack([dead[..., b * 32:(b + 1) * 32].all(axis=-1) for b in range(want_codes.shape[axis % x.ndim])], axis=-1)
    if fmt in P.HAS_NAN: dead = np.zeros_like(dead)
    want_scales = np.where(dead, 0xff, np.moveaxis(want_codes, axis % x.ndim, -1))
    assert np.array_equal(packed.scales.numpy(), want_scales), f'{what}: packed scales differ'
    back = mx_dequantize(packed, use_kernels=False).numpy()
    assert P.same_but_nan(back, got, mask, fmt), f'{what}: the round trip is not the fake quant'


# ------------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('fmt', FORMATS)
def test_floor_is_the_floor_oracle(fmt):
    for x, axis in S.layout_cases() + [(b, -1) for _, b in S.block_cases(fmt)]:
        y, c, e = S.quantize(x, fmt, axis, 'FLOOR')
        ry, rc = R.quantize(x, fmt, axis)
        assert e is None and np.array_equal(R.bits(y), R.bits(ry)) and np.array_equal(c, rc)


def random_blocks(seed: int, n: int = 4000) -> np.ndarray:
    """Gaussian times a log-normal block scale."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 32)) * np.exp(rng.standard_normal((n, 1)) * 3.0)).astype(np.float32)


@pytest.mark.parametrize('fmt', FORMATS)
def test_oracle_properties(fmt):
    blocks = np.concatenate([random_blocks(21), S.gaussian_blocks().reshape(-1, 32), S.crafted(fmt)])
    code = {rule: S.scale_codes(blocks, fmt, rule)[0] for rule in RULES}
    err = {rule: S.squared_error(blocks, code[rule], fmt) for rule in RULES}
    assert np.all(err['MSE'] <= np.minimum(err['FLOOR'], err['CEIL']))                    # per block
    for rule in NEW_RULES: assert np.all((code[rule] == code['FLOOR']) | (code[rule] == np.minimum(code['FLOOR'] + 1, 254))), rule
    assert np.all(code['EVEN'] <= code['CEIL'])                                           # EVEN's bumps are a subset of CEIL's
    assert (code['CEIL'] > code['FLOOR']).any() and (code['EVEN'] > code['FLOOR']).any() and (code['MSE'] > code['FLOOR']).any()
    assert (code['EVEN'] < code['CEIL']).any()
    # under CEIL no finite element saturates (a code clamped at 254 excepted: there is no larger scale)
    top = R._table(fmt)[-1]
    finite = np.where(np.isfinite(blocks), blocks, 0).astype(np.float64)
    free = code['CEIL'] < 254
    assert np.all(np.abs(np.ldexp(finite, (127 - code['CEIL'])[:, None]))[free] <= top)
    for rule in RULES:                                                                    # value idempotence
        y = S.values_under(blocks, code[rule], fmt)
        over = np.isinf(y).any(axis=1)                                                    # 2^128: only from float32's last binade
        assert np.all(np.abs(finite[over]).max(axis=1) >= 2.0 ** 127) and not (over.any() and rule == 'FLOOR')
        again, again_code, _ = S.quantize_blocks(y, fmt, rule)
        rows = ~over & ~np.isinf(blocks).any(axis=1)                                      # an Inf that saturated is a new amax
        assert np.array_equal(R.bits(again)[rows], R.bits(y)[rows]), rule
        if rule in ('FLOOR', 'EVEN', 'MSE'):                                              # ... and these three keep their codes too
            keep = np.isfinite(blocks).all(axis=1) & (np.abs(y).max(axis=1) > 0)
            if rule == 'FLOOR': assert np.array_equal(again_code[keep], code[rule][keep]), rule
            else: assert np.all(again_code[keep] <= code[rule][keep]), rule
    # under CEIL the second application may choose a smaller scale: the first one's amax may have rounded down a binade
    assert np.all(S.scale_codes(S.values_under(blocks, code['CEIL'], fmt), fmt, 'CEIL')[0] <= code['CEIL'])


@pytest.mark.parametrize('fmt', FORMATS)
def test_float32_difference_is_exact(fmt):
    """d = cast(v / X) * X - v in float32 equals the float64 difference under both candidates -- also for blocks scaled down
    into float32's subnormals and up to its largest values."""
    base = random_blocks(5, 1500)
    for scale in (1.0, 2.0 ** -120, 2.0 ** -140, 2.0 ** 100):
        blocks = (base.astype(np.float64) * scale).astype(np.float32)
        c0 = S.scale_codes(blocks, fmt, 'FLOOR')[0]
        for code in (c0, np.minimum(c0 + 1, 254)):
            y = S.values_under(blocks, code, fmt)
            d32 = (y - blocks).astype(np.float32)
            d64 = y.astype(np.float64) - blocks.astype(np.float64)
            assert np.array_equal(d32.astype(np.float64), d64)
            assert np.array_equal((d32.astype(np.float64) * d32.astype(np.float64)), d64 * d64)


@pytest.mark.parametrize('fmt', FORMATS)
def test_crafted_blocks(fmt):
    names = [n for n, _ in S.crafted_blocks(fmt)]
    blocks = S.crafted(fmt)
    code = {rule: S.scale_codes(blocks, fmt, rule)[0] for rule in RULES}
    at = names.index
    for k in (-20, 0, 9):
        assert code['CEIL'][at(f'top*2^{k}')] == code['FLOOR'][at(f'top*2^{k}')]
        assert code['CEIL'][at(f'top*2^{k}+ulp')] == code['FLOOR'][at(f'top*2^{k}+ulp')] + 1
    assert code['EVEN'][at('even threshold')] == code['FLOOR'][at('even threshold')] + 1
    assert code['EVEN'][at('even threshold-ulp')] == code['FLOOR'][at('even threshold-ulp')]
    for rule in RULES:
        assert code[rule].max() <= 254
        for name in ('all zero', 'all NaN', 'all Inf'): assert code[rule][at(name)] == 0, (rule, name)
        assert code[rule][at('subnormal amax')] <= (1 if fmt == 'MXINT8' else 0)
    if fmt == 'MXINT8':
        for rule in RULES: assert code[rule][at('exponent 254')] == 254 and code[rule][at('exponent 254 low')] == 254
    else:
        assert code['CEIL'][at('exponent 254')] == code['FLOOR'][at('exponent 254')] + 1 <= 254
    assert code['FLOOR'][at('e == emax')] == 0 and code['CEIL'][at('e == emax')] == 1
    # Inf and NaN take no part in amax or in the error
    for name, strip in (('NaN with finite', [7]), ('Inf with finite', [3, 11])):
        whole = blocks[at(name)]
        cut = whole.copy(); cut[strip] = 0
        for rule in RULES:
            c, e = S.scale_codes(whole[None], fmt, rule)
            c2, e2 = S.scale_codes(cut[None], fmt, rule)
            assert c[0] == c2[0], (rule, name)
            if e is not None: assert e[0][0] == e2[0][0] and e[1][0] == e2[1][0]
    c, e = S.scale_codes(blocks[at('candidates alike')][None], fmt, 'MSE')
    assert e[0][0] == e[1][0] == 0.0 and c[0] == code['FLOOR'][at('candidates alike')]     # a tie keeps c0
    if fmt == 'MXFP4_E2M1':
        c, e = S.scale_codes(blocks[at('fp4 7.5')][None], fmt, 'MSE')
        assert (e[0][0], e[1][0]) == (2.25, 0.25) and c[0] == code['FLOOR'][at('fp4 7.5')] + 1
    found = S.ceil_bumps_mse_does_not(fmt, random_blocks(21))
    assert found.size > 0, 'no block where CEIL bumps and MSE does not'


@pytest.mark.parametrize('fmt', FORMATS)
def test_no_near_ties_in_the_gpu_inputs(fmt):
    """The GPU test compares MSE codes with ==: its inputs hold no block whose two errors differ by a rounding of the sums."""
    for x, axis in S.layout_cases() + [(b, -1) for _, b in S.block_cases(fmt)]:
        _, _, errors = S.quantize(x, fmt, axis, 'MSE')
        assert S.near_ties(errors) == 0, (fmt, x.shape)


# ------------------------------------------------------------------------------------------------------- the torch arm on the CPU
@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('fmt', FORMATS)
def test_torch_arms_equal_the_oracle(fmt, rule):
    for k, (x, axis) in enumerate(S.layout_cases()): check_both_arms(x, fmt, axis, rule, f'{fmt} {rule} layout {k}')
    for name, blocks in S.block_cases(fmt): check_both_arms(blocks, fmt, -1, rule, f'{fmt} {rule} {name}')
    crafted = S.crafted(fmt)
    check_both_arms(np.ascontiguousarray(crafted.T), fmt, 0, rule, f'{fmt} {rule} crafted, strided')


def test_keyword_default_is_floor():
    x = torch.from_numpy(R.layout_input((3, 40), seed=2))
    for fmt in FORMATS:
        plain = mx_fake_quant(x, fmt, use_kernels=False)
        for rule in (MXScaleRule.FLOOR, 'FLOOR', 0, None):
            assert torch.equal(mx_fake_quant(x, fmt, use_kernels=False, scale_rule=rule).view(torch.int32), plain.view(torch.int32))
        a, b = mx_quantize(x, fmt, use_kernels=False), mx_quantize(x, fmt, use_kernels=False, scale_rule='FLOOR')
        assert torch.equal(a.elements, b.elements) and torch.equal(a.scales, b.scales)


# ------------------------------------------------------------------------------------------------------------------------ plumbing
def test_rule_enum_and_encoding():
    assert [r.value for r in MXScaleRule] == [0, 1, 2, 3] and [r.name for r in MXScaleRule] == list(RULES)
    for r in MXScaleRule: assert MXScaleRule.of(r) is r and MXScaleRule.of(r.name) is r and MXScaleRule.of(r.value) is r
    assert MXScaleRule.of(None) is MXScaleRule.FLOOR
    for bad in ('ROUND', 4, -1, True, 1.0):
        with pytest.raises(ValueError, match='unknown MX scale rule'): MXScaleRule.of(bad)
    assert ffi.MX_RULE_SHIFT == 8
    assert ffi.mx_format_arg('MXFP4_E2M1') == 4 and ffi.mx_format_arg(MXFormat.MXFP4_E2M1, MXScaleRule.MSE) == 4 | 3 << 8
    assert ffi.mx_format_arg('MXINT8', 'CEIL') == 5 | 1 << 8
    with pytest.raises(ValueError, match='unknown MX scale rule'): ffi.mx_format_arg('MXINT8', 7)
    x = torch.zeros(2, 32)
    with pytest.raises(ValueError, match='unknown MX scale rule'): mx_fake_quant(x, 'MXINT8', use_kernels=False, scale_rule='NEAREST')
    with pytest.raises(ValueError, match='unknown MX scale rule'): mx_quantize(x, 'MXINT8', use_kernels=False, scale_rule=9)


def test_c_entry_points_check_the_rule_without_a_device():
    """An unknown rule is refused by the entry points that make scales; a rule byte by those that do not -- before any launch."""
    lib = _lib.lib
    buf = np.zeros(512, np.float32)
    p = buf.ctypes.data
    mse = 3 << 8
    assert lib.ppqhip_mx_fq(p, p + 1024, None, 1, 64, 1, 4 | 4 << 8, None) == -1
    assert _lib.last_error() == f'mx_fq: job 0: unknown MX scale rule in format {4 | 4 << 8}'
    assert lib.ppqhip_mx_fq(p, p + 1024, None, 1, 64, 1, 6 | mse, None) == -1 and _lib.last_error() == 'mx_fq: job 0: unknown MX format 6'
    assert lib.ppqhip_mx_pack(p, p + 1024, p + 1536, 1, 64, 1, 1 << 16, None) == -1
    assert _lib.last_error() == f'mx_pack: job 0: unknown MX scale rule in format {1 << 16}'
    assert lib.ppqhip_mx_fq(p, p, None, 0, 64, 1, 4 | mse, None) == 0                       # a known rule, nothing to launch
    assert lib.ppqhip_mx_pack(p, p, p, 0, 64, 1, 4 | mse, None) == 0
    jobs = np.zeros(2, dtype=ffi._MX_JOB)
    jobs[0] = (p, p + 512, 0, 1, 64, 1, 4 | mse, 0)
    jobs[1] = (p + 256, p + 1024, 0, 1, 64, 1, 0 | 5 << 8, 0)
    assert lib.ppqhip_mx_fq_multi(jobs.ctypes.data, 2, None) == -1
    assert _lib.last_error() == f'mx_fq_multi: job 1: unknown MX scale rule in format {5 << 8}'
    pjobs = np.zeros(1, dtype=ffi._MX_PACK_JOB)
    pjobs[0] = (p, p + 1024, p + 1536, 1, 64, 1, 2 | 4 << 8, 0)
    assert lib.ppqhip_mx_pack_multi(pjobs.ctypes.data, 1, None) == -1
    assert _lib.last_error() == f'mx_pack_multi: job 0: unknown MX scale rule in format {2 | 4 << 8}'
    # no scales are made here: the rule byte is not a format
    assert lib.ppqhip_mx_unpack(p + 1024, p + 1536, p, 1, 64, 1, 4 | mse, None) == -1
    assert _lib.last_error() == f'mx_unpack: job 0: unknown MX format {4 | mse}'
    e, s = p + 1024, p + 1536
    for fa, fb in ((4 | mse, 4), (4, 4 | 1 << 8)):
        assert lib.ppqhip_mx_gemm(e, s, fa, e, s, fb, None, p, 1, 1, 32, None) == -1 and 'unknown MX format' in _lib.last_error()
        assert lib.ppqhip_mx_conv2d(e, s, fa, e, s, fb, None, p, 1, 32, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, None) == -1
        assert 'unknown MX format' in _lib.last_error()
    assert lib.ppqhip_mx_gemm_fused(e, s, 4, e, s, 4, None, None, 0, p, None, None, 4 | 2 << 8, 1, 1, 32, None) == -1
    assert 'out_format: unknown MX format' in _lib.last_error()
    assert lib.ppqhip_mx_conv2d_fused(e, s, 4, e, s, 4, None, None, 0, p, None, None, 4 | 2 << 8, 1, 32, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, None) == -1
    assert 'out_format: unknown MX format' in _lib.last_error()


def test_graph_stores_the_rules_and_export_honours_them():
    g = harness.small_cnn_graph(seed=3)
    ex = harness.TorchExecutor(g, 'cpu')
    d = quantize_graph_mx(g, ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=False, weight_scale_rule='MSE', activation_scale_rule=MXScaleRule.EVEN)
    seen = set()
    for op in g.operations.values():
        if not isinstance(op, harness.QuantableOperation): continue
        for v, c in zip(op.inputs, op.config.input_quantization_config):
            if c not in d: continue
            want = MXScaleRule.MSE if v.is_parameter else MXScaleRule.EVEN
            assert d[c].scale_rule is want and c.detail['MX_SCALE_RULE'] == want.name and _config_rule(c) is want
            seen.add(want)
    assert seen == {MXScaleRule.MSE, MXScaleRule.EVEN}
    for delegators in (d, None):                                                          # read off the delegator, and off the config
        packed = export_graph_mx(g, delegators, use_kernels=False)
        assert packed
        moved = 0
        for name, t in packed.items():
            w = g.variables[name].value
            want = mx_quantize(w, 'MXFP4_E2M1', t.axis, use_kernels=False, scale_rule='MSE')
            floor = mx_quantize(w, 'MXFP4_E2M1', t.axis, use_kernels=False)
            assert torch.equal(t.elements, want.elements) and torch.equal(t.scales, want.scales), name
            moved += int((t.scales != floor.scales).sum())
        assert moved > 0                                                                  # the rule was not FLOOR under another name
    # an absent entry is FLOOR
    g2 = harness.small_cnn_graph(seed=3)
    d2 = quantize_graph_mx(g2, harness.TorchExecutor(g2, 'cpu'), 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=False)
    for c, dl in d2.items(): assert 'MX_SCALE_RULE' not in c.detail and dl.scale_rule is MXScaleRule.FLOOR and _config_rule(c) is MXScaleRule.FLOOR


def test_cpu_executor_runs_a_forward_under_a_rule():
    x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    outs = {}
    for rule in RULES:
        g = harness.small_cnn_graph(seed=3)
        ex = harness.TorchExecutor(g, 'cpu')
        quantize_graph_mx(g, ex, 'MXFP4_E2M1', 'MXFP4_E2M1', use_kernels=False, weight_scale_rule=rule, activation_scale_rule=rule)
        outs[rule] = ex.forward(x)[0]
        assert torch.isfinite(outs[rule]).all()
    assert not torch.equal(outs['FLOOR'], outs['CEIL']) and not torch.equal(outs['FLOOR'], outs['MSE'])
    # a delegator of one's own, on the executor's seam
    d = MXDelegator('MXFP6_E2M3', -1, use_kernels=False, scale_rule='CEIL')
    t = torch.from_numpy(R.layout_input((3, 40), seed=2))
    assert torch.equal(d(t).view(torch.int32), mx_fake_quant(t, 'MXFP6_E2M3', -1, use_kernels=False, scale_rule='CEIL').view(torch.int32))
    g = harness.small_cnn_graph(seed=3)
    ex = harness.TorchExecutor(g, 'cpu')
    base = ex.forward(x)[0]
    configs = quantize_graph_mx(g, ex, 'MXFP4_E2M1', 'MXFP4_E2M1', use_kernels=False)
    for c, dl in configs.items(): ex.register_quantize_delegate(c, MXDelegator(dl.format, dl.axis, use_kernels=False, scale_rule='CEIL'))
    assert torch.equal(ex.forward(x)[0], outs['CEIL']) and not torch.equal(base, outs['CEIL'])
