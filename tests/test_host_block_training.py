"""The block-training frame of the four block-wise passes (``LearnedStepSizePass.finetune``) where it needs
no GPU: what a block looks like after a training step raised, and the empty dataset, which is refused before the block is touched.
The failure path runs through ``MXRoundTuningPass(use_kernels=False)`` -- the pass whose delegators REPLACE the weights and whose
graph holds delegates of its own, so everything the rollback has to put back is there."""
import pytest
import torch

import mx_round_reference as RR
from block_training_double import StepRefused, assert_nothing_trainable, refuse_gradient_forward, snapshot, assert_same_bits
from ppq_amd import MXRoundTuningPass, harness, quantize_graph_mx


def _setup():
    graph = RR.tiny_graph()
    ex = harness.TorchExecutor(graph, 'cpu')
    held = dict(quantize_graph_mx(graph, ex, 'MXFP4_E2M1', 'MXFP8_E4M3', use_kernels=False))
    batches = [torch.rand(2, 8, 8, 8, generator=torch.Generator().manual_seed(k)) for k in range(2)]
    return graph, ex, held, batches


def _parameters(graph) -> dict:
    return {v.name: v.value for op in graph.operations.values() for v in op.inputs if v.is_parameter}


def _pass():
    return MXRoundTuningPass(steps=4, lr=1e-2, use_hip_graph=False, use_kernels=False)


def _whole_graph_block(graph):
    from ppq_amd.blocks import TrainableBlock
    ops = graph.topological_sort()
    return TrainableBlock(sp=ops[0], ep=ops[-1], rps=ops)


def test_a_training_step_that_raises_leaves_the_block_as_it_was_found():
    graph, ex, held, batches = _setup()
    tensors, values = _parameters(graph), snapshot(graph)
    assert len(tensors) == 6                                                         # three weights, three biases
    with refuse_gradient_forward(ex, at=3) as seen, pytest.raises(StepRefused, match='gradient forward 3 refused'):
        _pass().optimize(graph, batches, ex)
    assert seen[0] == 3                                                              # two steps trained, the third raised
    for name, v in _parameters(graph).items(): assert v is tensors[name], name       # the original tensor objects
    assert_nothing_trainable(graph)
    assert_same_bits(snapshot(graph), values)                                        # the biases had two Adam steps: copied back
    assert set(ex._delegates) == set(held) and all(ex._delegates[c] is d for c, d in held.items())

    # the block trains as if nothing had happened
    again = _pass()
    again.optimize(graph, batches, ex)
    fresh_graph, fresh_ex, _, _ = _setup()
    fresh = _pass()
    fresh.optimize(fresh_graph, batches, fresh_ex)
    assert again.report == fresh.report and again.stats == fresh.stats and fresh.stats['flipped'] > 0
    assert_same_bits(snapshot(graph), snapshot(fresh_graph))
    assert_nothing_trainable(graph)
    assert set(ex._delegates) == set(held) and all(ex._delegates[c] is d for c, d in held.items())


def test_a_post_loss_that_raises_is_rolled_back_too(monkeypatch):
    graph, ex, held, batches = _setup()
    tensors, values = _parameters(graph), snapshot(graph)
    p = _pass()

    def refuse(*a, **kw): raise StepRefused('post-loss refused')
    monkeypatch.setattr(p, '_post_loss', refuse)
    with pytest.raises(StepRefused, match='post-loss refused'): p.optimize(graph, batches, ex)
    for name, v in _parameters(graph).items(): assert v is tensors[name], name
    assert_nothing_trainable(graph)
    assert_same_bits(snapshot(graph), values)
    assert set(ex._delegates) == set(held) and all(ex._delegates[c] is d for c, d in held.items())


def _passes():
    from ppq_amd.adaround import AdaroundPass
    from ppq_amd.lsq import LearnedStepSizePass
    from ppq_amd.roundtune import RoundTuningPass
    return [LearnedStepSizePass, AdaroundPass, RoundTuningPass, MXRoundTuningPass]


@pytest.mark.parametrize('pass_cls', _passes(), ids=lambda c: c.__name__)
def test_an_empty_dataset_is_refused_before_the_block_is_touched(pass_cls):
    from ppq_amd.adaround import AdaroundPass
    from ppq_amd.core import QuantizationStates
    graph, ex, held, _ = _setup()
    block = _whole_graph_block(graph)
    if pass_cls is AdaroundPass:             # its block check comes first and refuses the MX weights of this graph: take them out of it
        for op in block.rps:
            for cfg, var in (op.config_with_variable if hasattr(op, 'config') else []):
                if var.is_parameter: cfg.state = QuantizationStates.FP32
    tensors = _parameters(graph)
    with pytest.raises(ValueError, match='Dataset is empty.'):
        pass_cls(steps=2, use_hip_graph=False).finetune(block, ex, [], [])
    for name, v in _parameters(graph).items(): assert v is tensors[name], name
    assert_nothing_trainable(graph)
    assert set(ex._delegates) == set(held) and all(ex._delegates[c] is d for c, d in held.items())
