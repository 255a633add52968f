"""The convolution-epilogue planner (harness.plan_epilogues) on graphs, configs and hooks alone: no device.

Each condition that must keep a group unfused is checked to do so for ITS group only."""
import torch

from ppq_amd import harness
from ppq_amd.core import QuantizationStates
from ppq_amd.observer import CalibrationHook, OperationObserver


def _resnet(method='kl', **kw):
    g = harness.resnet50_graph(seed=0)
    harness.quantize_graph(g, method, hist_bins=2048, **kw)
    hooks = {n: OperationObserver(op, monitor_parameter=False).hook for n, op in g.operations.items()}
    return g, hooks


def _plan(g, hooks, **kw):
    kw.setdefault('keep', set(g.outputs))
    return harness.plan_epilogues(g.topological_sort(), hooks, **kw)


def _names(groups):
    return {tuple(op.name for op in grp.ops) for grp in groups}


def _split(groups):
    return (sum(grp.kind == 'P1' for grp in groups), sum(grp.kind == 'P2' for grp in groups),
            sum(grp.kind == 'P2' and len(grp.convs) == 2 for grp in groups))


def test_resnet50_split_kl_and_cfg3():
    for method, kw in (('kl', {}), ('mse', dict(symmetrical=False, weight_symmetrical=False)), ('percentile', {})):
        g, hooks = _resnet(method, **kw)
        groups = _plan(g, hooks)
        assert _split(groups) == (33, 16, 4), method
        assert _split(_plan(g, None)) == (33, 16, 4)
        for grp in groups:
            if grp.kind == 'P2':      # operand order of the Add: convs[0] produces its input 0
                assert grp.add.inputs[0] is grp.convs[0].outputs[0]
                if len(grp.convs) == 2: assert grp.add.inputs[1] is grp.convs[1].outputs[0]


def test_groups_are_consecutive_and_disjoint():
    g, hooks = _resnet()
    order = [op.name for op in g.topological_sort()]
    seen = set()
    for grp in _plan(g, hooks):
        names = [op.name for op in grp.ops]
        i = order.index(names[0])
        assert order[i:i + len(names)] == names
        assert not seen & set(names)
        seen |= set(names)


def _group_of(groups, op_name):
    return [grp for grp in groups if any(op.name == op_name for op in grp.ops)]


def _only_one_lost(g, hooks, before, op_name, **kw):
    after = _plan(g, hooks, **kw)
    lost = _names(before) - _names(after)
    assert lost == _names(_group_of(before, op_name)) and len(lost) == 1, (op_name, lost)
    assert _names(after) <= _names(before)


def test_observed_intermediate_disables_its_group():
    g, hooks = _resnet()
    before = _plan(g, hooks)
    # P1: the conv output (not written by the kernel) observed by the conv's own hook
    conv = g.operations['conv2']
    hooks['conv2']._observer_table[conv.config.output_quantization_config[0]] = object()
    _only_one_lost(g, hooks, before, 'conv2')
    g, hooks = _resnet()
    before = _plan(g, hooks)
    # P2: the Add output observed as the Relu's input
    grp = [x for x in before if x.kind == 'P2'][5]
    hooks[grp.relu.name]._observer_table[grp.relu.config.input_quantization_config[0]] = object()
    _only_one_lost(g, hooks, before, grp.relu.name)


def test_observed_written_tensor_keeps_its_group():
    g, hooks = _resnet()
    before = _plan(g, hooks)
    for grp in before:
        if grp.kind == 'P2':          # conv3's INITIAL output config is observed: the kernel writes that tensor
            assert grp.convs[0].config.output_quantization_config[0] in hooks[grp.convs[0].name]._observer_table


def test_activated_or_delegated_intermediate_disables_its_group():
    g, hooks = _resnet()
    before = _plan(g, hooks)
    cfg = g.operations['conv7'].config.output_quantization_config[0]
    saved = cfg.state
    cfg.state = QuantizationStates.ACTIVATED
    _only_one_lost(g, hooks, before, 'conv7')
    cfg.state = saved
    # a delegated config: the executor's passes_through says no
    add = [x for x in before if x.kind == 'P2'][2].add
    target = add.config.output_quantization_config[0]
    _only_one_lost(g, hooks, before, add.name, passes_through=lambda c: c is not target and not QuantizationStates.is_activated(c.state))
    # a config between conv3 and the Add (the Add would read a quantised tensor)
    target = add.config.input_quantization_config[1]
    target_state = target.state
    target.state = QuantizationStates.ACTIVATED
    _only_one_lost(g, hooks, before, add.name)
    target.state = target_state


def test_unknown_hook_type_disables_its_group():
    g, hooks = _resnet()
    before = _plan(g, hooks)

    class OtherHook(CalibrationHook):
        pass
    h = hooks['relu2']
    hooks['relu2'] = OtherHook(h._operation, h._observer_table)
    _only_one_lost(g, hooks, before, 'relu2')
    hooks['relu2'] = object()
    _only_one_lost(g, hooks, before, 'relu2')


def test_autograd_disables_everything():
    g, hooks = _resnet()
    assert _plan(g, hooks, grad_enabled=True) == []


def test_second_consumer_or_requested_output_disables_its_group():
    g, hooks = _resnet()
    before = _plan(g, hooks)
    conv = g.operations['conv2']
    extra = harness.Operation('spy', 'Identity', {}, [conv.outputs[0]], [])
    conv.outputs[0].dest_ops.append(extra)
    _only_one_lost(g, hooks, before, 'conv2')
    conv.outputs[0].dest_ops.remove(extra)
    _only_one_lost(g, hooks, before, 'conv2', keep=set(g.outputs) | {conv.outputs[0].name})
    grp = [x for x in before if x.kind == 'P2'][7]
    _only_one_lost(g, hooks, before, grp.add.name, keep=set(g.outputs) | {grp.add.outputs[0].name})


def test_non_consecutive_members_disable_their_group():
    g, hooks = _resnet()
    before = _plan(g, hooks)
    ops = g.topological_sort()
    i = [op.name for op in ops].index('relu2')
    ops.insert(i, ops.pop(i + 1))                 # conv3 now sits between conv2 and relu2 (still a valid order)
    after = harness.plan_epilogues(ops, hooks, set(g.outputs))
    assert ('conv2', 'relu2') not in _names(after)
    assert _names(after) - _names(before) == set()
    assert len(_names(before) - _names(after)) <= 2    # conv2's group, and the group conv3 started


def test_other_graphs_vit_and_small_cnn():
    g = harness.vit_graph(seed=0, depth=2, dim=64, heads=4, mlp_dim=128, image=32)
    harness.quantize_graph_fp8(g)
    assert _plan(g, None) == []                   # no Conv -> Relu / Add -> Relu chains in a ViT
    g = harness.small_cnn_graph(seed=0)
    harness.quantize_graph(g, 'kl')
    assert _split(_plan(g, None)) == (1, 1, 0)
    # the residual operand of small_cnn's Add is c1's relu output, which also feeds c2: read as is
    grp = [x for x in _plan(g, None) if x.kind == 'P2'][0]
    assert [op.name for op in grp.ops] == ['c2', 'add', 'add_relu']


def test_executor_off_switch_and_grad_mode():
    g, hooks = _resnet()
    ex = harness.TorchExecutor(g, device='cpu')
    with torch.no_grad():
        assert len(ex._epilogue_plan(g.topological_sort(), hooks, list(g.outputs))) == 49
        ex.fuse_epilogues = False
        assert ex._epilogue_plan(g.topological_sort(), hooks, list(g.outputs)) == {}
        ex.fuse_epilogues = True
    with torch.enable_grad():
        assert ex._epilogue_plan(g.topological_sort(), hooks, list(g.outputs)) == {}
