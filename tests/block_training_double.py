"""A test double for the failure path of the block-training frame, and the before / after comparison its
tests share.  Not a test module."""
import contextlib

import torch


class StepRefused(RuntimeError):
    pass


@contextlib.contextmanager
def refuse_gradient_forward(executor, at: int):
    """While active, the ``at``-th ``partial_graph_forward(..., with_gradient=True)`` of ``executor`` -- the forward of the
    ``at``-th training step, the first block's while ``at`` <= its steps -- raises :class:`StepRefused` before it runs anything.
    The forwards without gradient (pre-loss, post-loss, collection) pass through and are not counted."""
    real, seen = executor.partial_graph_forward, [0]

    def forward(operations, feed_dict, output_names, with_gradient: bool = False):
        if with_gradient:
            seen[0] += 1
            if seen[0] == at: raise StepRefused(f'gradient forward {at} refused')
        return real(operations, feed_dict, output_names, with_gradient=with_gradient)
    executor.partial_graph_forward = forward
    try: yield seen
    finally: del executor.partial_graph_forward


def snapshot(graph) -> dict:
    """A copy of every tensor a block-wise pass may touch: parameters, scales, offsets."""
    snap = {}
    for op in graph.operations.values():
        for v in op.inputs:
            if v.is_parameter and isinstance(v.value, torch.Tensor): snap[('p', v.name)] = v.value.detach().clone()
        if hasattr(op, 'config'):
            for i, (c, _) in enumerate(op.config_with_variable):
                if isinstance(c.scale, torch.Tensor): snap[('s', op.name, i)] = c.scale.detach().clone()
                if isinstance(c.offset, torch.Tensor): snap[('o', op.name, i)] = c.offset.detach().clone()
    return snap


def assert_same_bits(got: dict, want: dict) -> None:
    assert set(got) == set(want)
    for key, t in want.items():
        g = got[key]
        assert g.dtype == t.dtype and g.shape == t.shape, key
        assert torch.equal(g.reshape(-1).contiguous().view(torch.uint8), t.reshape(-1).contiguous().view(torch.uint8)), key


def assert_nothing_trainable(graph) -> None:
    for op in graph.operations.values():
        for v in op.inputs:
            if v.is_parameter and isinstance(v.value, torch.Tensor):
                assert not v.value.requires_grad and v.value.grad is None and v.value.is_leaf, v.name
        if hasattr(op, 'config'):
            for c, v in op.config_with_variable:
                for t in (c.scale, c.offset):
                    if isinstance(t, torch.Tensor): assert not t.requires_grad and t.grad is None, (op.name, v.name)
