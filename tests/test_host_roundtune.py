"""Host-side tests of round tuning (ppq_amd/roundtune.py): the test-side torch restatement of
ppq/quantization/algorithm/training.py:490-590 against the reference's own outputs (tests/golden/roundtune.npz, written by
tests/golden/make_roundtune.py), the conditions on the recorded inputs without which those comparisons would be vacuous, the
constructor's refusals, the one-time expressions and the plugin registration.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import roundtune_cases as RC  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'roundtune.npz')))


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _case(golden, k):
    p = f'c{k}_'
    return {x: torch.from_numpy(golden[p + x]) for x in ('w', 'scale', 'offset', 'dy', 'r0', 'wfloor', 'r', 'fwd', 'dr', 'final')}


def test_restatement_equals_the_reference_goldens_bit_for_bit(golden):
    assert len(RC.CASES) >= 6
    for k, (name, shape, axis, qmin, qmax, asym, _) in enumerate(RC.CASES):
        c = _case(golden, k)
        assert tuple(c['w'].shape) == shape, name
        r0, wfloor = RC.initial_rounding(c['w'], c['scale'], axis)
        assert np.array_equal(_bits(r0), _bits(c['r0'])), name
        assert np.array_equal(_bits(wfloor), _bits(c['wfloor'])), name
        assert np.array_equal(_bits(RC.forward(c['wfloor'], c['r'], c['scale'], c['offset'], axis, qmin, qmax)), _bits(c['fwd'])), name
        dr = RC.grad_r(c['wfloor'], c['r'], c['scale'], c['offset'], axis, qmin, qmax, c['dy'])
        assert np.array_equal(_bits(dr), _bits(c['dr'])), name
        assert np.array_equal(_bits(c['dr']), _bits(c['dy'])), name                        # the identity: dR = dy
        assert np.array_equal(_bits(RC.finalize(c['wfloor'], c['r'], c['scale'], axis)), _bits(c['final'])), name
        assert all(v.dtype == np.float32 for key, v in golden.items() if key.startswith(f'c{k}_')), name


def test_recorded_inputs_meet_the_conditions_the_comparisons_rely_on(golden):
    """Every case: R on both sides of .5, and the perturbation moves elements across .5.  At least one case: the clamp
    changes elements at each end.  At least one case: floored-weight elements whose t / s is not an integer in fp32 -- the
    input on which a reciprocal shortcut or a stray rint in the kernel would show."""
    both_ends, non_integer = 0, 0
    for k, (name, shape, axis, qmin, qmax, asym, _) in enumerate(RC.CASES):
        c = _case(golden, k)
        assert int((c['r0'] > .5).sum()) > 0 and int((c['r0'] <= .5).sum()) > 0, name
        assert int(((c['r0'] > .5) != (c['r'] > .5)).sum()) > 0, name
        s, o = RC._view(c['scale'], axis, c['w'].ndim), RC._view(c['offset'], axis, c['w'].ndim)
        q = (c['wfloor'] / s) + (c['r'] > .5) + o
        both_ends += bool((q < qmin).any() and (q > qmax).any())
        non_integer += int(((c['wfloor'] / s) != (c['wfloor'] / s).round()).sum())
    assert both_ends >= 1 and non_integer >= 1, (both_ends, non_integer)


def test_case_inputs_are_the_recorded_ones(golden):
    """roundtune_cases.case_tensors is deterministic: the GPU tests rebuild the same inputs without the golden file."""
    for k, (_, _, axis, *_rest) in enumerate(RC.CASES):
        w, s, o, noise, dy = RC.case_tensors(k)
        c = _case(golden, k)
        for name, t in (('w', w), ('scale', s), ('offset', o), ('dy', dy)):
            assert np.array_equal(_bits(t), _bits(c[name])), (k, name)
        assert np.array_equal(_bits(RC.initial_rounding(w, s, axis)[0] + noise), _bits(c['r'])), k


def test_reference_defaults_and_protocol():
    import inspect

    from ppq_amd import roundtune
    from ppq_amd.roundtune import RoundTuningDelegator, RoundTuningPass
    sig = inspect.signature(RoundTuningPass.__init__)
    names = [n for n, prm in sig.parameters.items() if prm.kind is prm.POSITIONAL_OR_KEYWORD][1:]
    assert names == ['interested_layers', 'steps', 'lr', 'block_size', 'expire_device', 'collecting_device', 'optimizer']
    assert [n for n, prm in sig.parameters.items() if prm.kind is prm.KEYWORD_ONLY] == ['group_weights', 'use_hip_graph', 'fused_adam']
    p = RoundTuningPass()
    assert (p.steps, p.lr, p.block_size, p.interested_layers, p.optimizer) == (500, 1e-4, 5, [], None)
    assert isinstance(p.loss_fn, torch.nn.MSELoss) and p.name == 'PPQ Rounding Tuning Pass'
    assert {'roundtune_weights', 'skipped_weights', 'flipped', 'tuned_elements'} <= set(p.stats)
    assert list(inspect.signature(RoundTuningDelegator.__init__).parameters)[1:] == ['var', 'config']
    assert roundtune.RoundTruningDelegator is RoundTuningDelegator                          # the reference's spelling


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


def test_constructor_refusals_and_their_messages(monkeypatch):
    """training.py:538-548, in the reference's order and words; a refused construction leaves the weight untouched."""
    from ppq_amd import FloatingQuantizationConfig, QuantizationStates
    from ppq_amd.blocks import TrainableBlock
    from ppq_amd.roundtune import RoundTuningDelegator, RoundTuningPass
    w = torch.randn(4, 3, 3, 3)
    fcfg = FloatingQuantizationConfig(channel_axis=0)
    fcfg.scale, fcfg.offset, fcfg.state = torch.ones(4), torch.zeros(4), QuantizationStates.ACTIVATED
    var = _param(w.clone())
    with pytest.raises(TypeError, match='Except Linear Quantization Policy'):
        RoundTuningDelegator(var=var, config=fcfg)
    with pytest.raises(TypeError, match='Except Static Quantization Policy'):
        RoundTuningDelegator(var=var, config=_cfg(channel_axis=0, dynamic=True))
    with pytest.raises(TypeError, match='Variable w is not a parameter!'):
        RoundTuningDelegator(var=_param(w, is_parameter=False), config=_cfg(channel_axis=0))
    with pytest.raises(ValueError, match='Unexpected value type of w'):
        RoundTuningDelegator(var=_param(None), config=_cfg(channel_axis=0))
    cfg = _cfg(channel_axis=0); cfg.scale = None
    with pytest.raises(ValueError, match='Quantization Scale has not been correctly set'):
        RoundTuningDelegator(var=var, config=cfg)
    assert torch.equal(var.value, w)
    p = RoundTuningPass(steps=1)
    monkeypatch.setattr(p, '_world', lambda: 2)
    with pytest.raises(ValueError, match='one process'):
        p.finetune(TrainableBlock(sp=None, ep=None, rps=[]), None, [{}], [{}])


def test_delegator_one_time_expressions_on_the_host(golden):
    """R, the floored weight, finalize and withdraw are the reference's torch expressions (training.py:555-578); a CPU tensor
    cannot take the kernel path (no CPU fallback)."""
    from ppq_amd.roundtune import RoundTuningDelegator
    for k in (0, 3):                                       # per channel and per tensor
        name, shape, axis, qmin, qmax, asym, _ = RC.CASES[k]
        c = _case(golden, k)
        cfg = _cfg(channel_axis=axis, quant_min=qmin, quant_max=qmax)
        cfg.scale, cfg.offset = c['scale'].clone(), c['offset'].clone()
        var = _param(c['w'].clone())
        original = var.value
        d = RoundTuningDelegator(var=var, config=cfg)
        assert d.rounding.requires_grad and d.trainable_tensors() == [d.rounding]
        assert np.array_equal(_bits(d.rounding.detach()), _bits(c['r0']))
        assert var.value is not original and not var.value.requires_grad                   # REPLACED by the floored weight
        assert np.array_equal(_bits(var.value), _bits(c['wfloor']))
        with torch.no_grad(): d.rounding.copy_(c['r'])
        assert int(d.flipped()) == int(((c['r0'] > .5) != (c['r'] > .5)).sum()) > 0
        with pytest.raises(RuntimeError, match='not on the GPU'):
            d(var.value, cfg)
        d.finalize()
        assert np.array_equal(_bits(var.value), _bits(c['final']))
        d.withdraw()
        assert np.array_equal(_bits(var.value), _bits(c['w']))


def test_plugin_registration_admits_the_round_tuning_delegator():
    from oracle import reference_import as RI
    if RI.find_reference() is None: pytest.skip('reference not present on this machine')
    RI.load()
    from ppq.executor.torch import TorchQuantizeDelegator

    import ppq_amd
    from ppq_amd.roundtune import RoundTuningDelegator
    try:
        ppq_amd.install_plugins_into_ppq(observers=False)
        assert issubclass(RoundTuningDelegator, TorchQuantizeDelegator)
    finally:
        ppq_amd.uninstall_from_ppq()
