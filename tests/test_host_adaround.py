"""Host-side tests of AdaRound (ppq_amd/adaround.py): the test-side torch restatement of legacy.py against the reference's own
outputs (tests/golden/adaround.npz, written by tests/golden/make_adaround.py), the regulariser's host values, the reference's
shadowed regulariser index, the refusals and the plugin registration.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import adaround_cases as AC  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'adaround.npz')))


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def test_restatement_equals_the_reference_goldens_bit_for_bit(golden):
    for k, (name, shape, axis, qmin, qmax, asym) in enumerate(AC.CASES):
        p = f'c{k}_'
        w, s, o, v, dy = (torch.from_numpy(golden[p + x]) for x in ('w', 'scale', 'offset', 'v', 'dy'))
        assert tuple(w.shape) == shape, name
        assert np.array_equal(_bits(AC.initiate_rounding(w, s, axis)), _bits(golden[p + 'init'])), name
        assert np.array_equal(_bits(AC.forward(w, v, s, o, axis, qmin, qmax)), _bits(golden[p + 'fwd'])), name
        assert np.array_equal(_bits(AC.grad_v(w, v, s, o, axis, qmin, qmax, dy)), _bits(golden[p + 'dv0'])), name
        for j, (it, max_iter) in enumerate(AC.REG_POINTS):
            got = AC.grad_v(w, v, s, o, axis, qmin, qmax, dy, it=it, max_iter=max_iter)
            assert np.array_equal(_bits(got), _bits(golden[p + f'dv{j + 1}'])), (name, it)
            assert not np.array_equal(_bits(got), _bits(golden[p + 'dv0'])), (name, it)      # the term is active there
        assert np.array_equal(_bits(AC.finalize(w, v, s, o, axis, qmin, qmax)), _bits(golden[p + 'final'])), name
        # the soft forward is NOT the hard finalize: the goldens exercise both roundings
        assert not np.array_equal(_bits(golden[p + 'fwd']), _bits(golden[p + 'final'])), name


def test_case_inputs_are_the_recorded_ones(golden):
    """adaround_cases.case_tensors is deterministic: the GPU tests rebuild the same inputs without the golden file."""
    for k, (_, _, axis, *_rest) in enumerate(AC.CASES):
        w, s, o, noise, dy = AC.case_tensors(k)
        p = f'c{k}_'
        for name, t in (('w', w), ('scale', s), ('offset', o), ('dy', dy)):
            assert np.array_equal(_bits(t), _bits(golden[p + name])), (k, name)
        assert np.array_equal(_bits(AC.initiate_rounding(w, s, axis) + noise), _bits(golden[p + 'v'])), k


def test_time_decay_and_regulariser_host_values_are_exact(golden):
    from ppq_amd.adaround import AdaroundRegTerm, TimeDecay
    td = TimeDecay(100)
    got = np.array([td(t) for t in golden['timedecay_t']], np.float64)
    assert np.array_equal(got.view(np.uint64), golden['timedecay_beta'].view(np.uint64))
    reg = AdaroundRegTerm(max_iter=100)
    assert np.array_equal(reg.host_values(19, 1.0), np.zeros(3, np.float32))             # warm-up: the term is the integer 0
    for it in (20, 50, 99):
        beta = td(it)
        want = np.array([np.float32(np.float32(1.0) * np.float32(0.01)), np.float32(beta), np.float32(beta - 1.0)], np.float32)
        assert np.array_equal(reg.host_values(it, 1.0).view(np.uint32), want.view(np.uint32)), it
    # k is gamma * alpha rounded twice in float32 (the two scalar multiplications autograd performs), not in double
    k = reg.host_values(50, 0.3)[0]
    assert k == np.float32(np.float32(0.3) * np.float32(0.01))
    assert reg.host_values(20, 1.0)[1] == np.float32(20.0)
    # beta - 1 is formed in double, then cast: it may differ from float32(beta) - 1
    bm1 = [reg.host_values(t, 1.0) for t in range(20, 100)]
    assert all(r[2] == np.float32(float(td(t)) - 1.0) for t, r in zip(range(20, 100), bm1))


def test_regulariser_index_is_the_shadowed_output_index():
    """legacy.py:254-274: `idx` of the step loop is shadowed by `for idx, name in enumerate(output_names)`, so the regulariser
    is evaluated at len(outputs) - 1 on every step: with 10 steps (warm-up until 2.0) a 1-output block never activates it, a
    3-output block has it active with beta = TimeDecay(2) = 20 on every step; anneal_regularization uses the true step."""
    from ppq_amd.adaround import AdaroundPass, TimeDecay
    p = AdaroundPass(steps=10)
    one = p._reg_table(1, 'cpu').numpy()
    assert one.shape == (10, 3) and not one.any()
    three = p._reg_table(3, 'cpu').numpy()
    assert np.all(three == np.array([np.float32(0.01), np.float32(20.0), np.float32(19.0)], np.float32))
    p = AdaroundPass(steps=10, anneal_regularization=True)
    tab = p._reg_table(1, 'cpu').numpy()
    assert not tab[:2].any() and tab[2:, 0].min() > 0
    assert np.array_equal(tab[:, 1], np.array([0, 0] + [np.float32(TimeDecay(10)(t)) for t in range(2, 10)], np.float32))
    assert AdaroundPass(steps=8000)._reg_table(6, 'cpu')[:, 0].abs().max() == 0          # the reference's default: never active


def test_reference_defaults_and_protocol():
    import inspect

    from ppq_amd.adaround import AdaroundPass, AdaRoundDelegator
    sig = inspect.signature(AdaroundPass.__init__)
    names = [n for n, prm in sig.parameters.items() if prm.kind is prm.POSITIONAL_OR_KEYWORD][1:]
    assert names == ['name', 'interested_layers', 'is_scale_trainable', 'steps', 'lr', 'gamma', 'collecting_device', 'block_size']
    p = AdaroundPass()
    assert (p.steps, p.lr, p.gamma, p.block_size, p.is_scale_trainable, p.interested_layers) == (8000, 1e-3, 1.0, 4, False, [])
    assert not p.anneal_regularization and p.tune_steps == 900
    assert list(inspect.signature(AdaRoundDelegator.__init__).parameters)[1:] == ['var', 'config', 'steps']


def _param(value, is_parameter=True):
    from ppq_amd.harness import Variable
    return Variable('w', value=value, is_parameter=is_parameter)


def _cfg(**kw):
    from ppq_amd import LinearQuantizationConfig, QuantizationStates
    cfg = LinearQuantizationConfig(**kw)
    C = 4 if kw.get('channel_axis') is not None else 1
    cfg.scale = torch.full([C], 0.05) if C > 1 else torch.tensor(0.05)
    cfg.offset = torch.zeros_like(cfg.scale)
    cfg.state = QuantizationStates.ACTIVATED
    return cfg


def test_refusals_raise_type_and_value_errors(monkeypatch):
    from ppq_amd import FloatingQuantizationConfig, QuantizationStates
    from ppq_amd.adaround import AdaroundPass, AdaRoundDelegator
    from ppq_amd.blocks import TrainableBlock
    w = torch.randn(4, 3, 3, 3)
    with pytest.raises(TypeError, match='works only with parameter'):                     # legacy.py:79-81
        AdaRoundDelegator(var=_param(w, is_parameter=False), config=_cfg(channel_axis=0), steps=10)
    cfg = _cfg(channel_axis=0); cfg.state = QuantizationStates.PASSIVE
    with pytest.raises(TypeError, match='passive'):                                       # legacy.py:82-84
        AdaRoundDelegator(var=_param(w), config=cfg, steps=10)
    with pytest.raises(TypeError, match='LINEAR'):                                        # (d): dynamic grids are refused
        AdaRoundDelegator(var=_param(w), config=_cfg(channel_axis=0, dynamic=True), steps=10)
    fcfg = FloatingQuantizationConfig(channel_axis=0)
    fcfg.scale, fcfg.offset, fcfg.state = torch.ones(4), torch.zeros(4), QuantizationStates.ACTIVATED
    with pytest.raises(TypeError):
        AdaRoundDelegator(var=_param(w), config=fcfg, steps=10)

    class _Op:
        name, type = 'conv', 'Conv'

        def __init__(self, c): self.config, self.inputs, self.outputs, self._c = object(), [], [], c

        @ property
        def config_with_variable(self): return [(self._c, _param(w))]
    block = TrainableBlock(sp=None, ep=None, rps=[_Op(fcfg)])
    with pytest.raises(TypeError, match='FLOATING / DYNAMIC'):
        AdaroundPass(steps=1)._check_block(block)
    p = AdaroundPass(steps=1)
    monkeypatch.setattr(p, '_world', lambda: 2)
    with pytest.raises(ValueError, match='one process'):
        p._check_block(TrainableBlock(sp=None, ep=None, rps=[]))


def test_delegator_one_time_expressions_on_the_host():
    """initiate_rounding / finalize / withdraw are the reference's torch expressions (legacy.py:90-120); a CPU tensor cannot
    take the kernel path (no CPU fallback)."""
    from ppq_amd.adaround import AdaRoundDelegator
    w, s, o, noise, _ = AC.case_tensors(0)
    cfg = _cfg(channel_axis=0, quant_min=-128, quant_max=127)
    cfg.scale, cfg.offset = s.clone(), o.clone()
    var = _param(w.clone())
    d = AdaRoundDelegator(var=var, config=cfg, steps=10)
    assert d.rounding.requires_grad and d.trainable_tensors() == [d.rounding]
    assert torch.equal(d.rounding.detach(), AC.initiate_rounding(w, s, 0))
    with torch.no_grad(): d.rounding.add_(noise)
    with pytest.raises(RuntimeError, match='not on the GPU'):
        d(var.value, cfg)
    d.finalize()
    assert torch.equal(var.value, AC.finalize(w, AC.initiate_rounding(w, s, 0) + noise, s, o, 0, -128, 127))
    assert not var.value.requires_grad
    d.withdraw()
    assert torch.equal(var.value, w)


def test_plugin_registration_admits_the_adaround_delegator():
    from oracle import reference_import as RI
    if RI.find_reference() is None: pytest.skip('reference not present on this machine')
    RI.load()
    from ppq.executor.torch import TorchQuantizeDelegator

    import ppq_amd
    from ppq_amd.adaround import AdaRoundDelegator
    try:
        ppq_amd.install_plugins_into_ppq(observers=False)
        assert issubclass(AdaRoundDelegator, TorchQuantizeDelegator)
    finally:
        ppq_amd.uninstall_from_ppq()
