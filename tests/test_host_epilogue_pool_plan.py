"""The pooled P1 group of harness.plan_epilogues -- Conv(bias) -> Relu -> MaxPool in one launch -- and the elision of the Relu
store (harness.elidable_stores), on graphs, configs and hooks alone: no device.

The stem of ResNet-50 forms the group; each condition that must keep the pool out does so, and the stem then stays the plain
Conv -> Relu group it was, with every other group untouched."""
import pytest

from ppq_amd import harness
from ppq_amd.core import QuantizationStates
from ppq_amd.observer import CalibrationHook, OperationObserver

STEM, PLAIN = ('conv1', 'relu1', 'maxpool'), ('conv1', 'relu1')


def _resnet(method='kl'):
    g = harness.resnet50_graph(seed=0)
    harness.quantize_graph(g, method, hist_bins=2048)
    hooks = {n: OperationObserver(op, monitor_parameter=False).hook for n, op in g.operations.items()}
    return g, hooks


def _plan(g, hooks, **kw):
    kw.setdefault('keep', set(g.outputs))
    return harness.plan_epilogues(g.topological_sort(), hooks, **kw)


def _names(groups):
    return {tuple(op.name for op in grp.ops) for grp in groups}


def _refused(g, hooks, before, **kw):
    """The stem lost its pool and nothing else changed."""
    after = _names(_plan(g, hooks, **kw))
    assert STEM not in after and PLAIN in after
    assert after - {PLAIN} == _names(before) - {STEM}


def test_the_stem_of_resnet50_forms_the_pooled_group():
    for hooks_on in (True, False):
        g, hooks = _resnet()
        groups = _plan(g, hooks if hooks_on else None)
        stem = [grp for grp in groups if grp.ops[0].name == 'conv1']
        assert len(stem) == 1 and tuple(op.name for op in stem[0].ops) == STEM
        grp = stem[0]
        assert grp.kind == 'P1' and grp.pool is g.operations['maxpool'] and grp.relu is g.operations['relu1'] and grp.add is None
        assert harness.pool_window(grp.pool) == (3, 2, 1)
        pooled = [x for x in groups if x.pool is not None]
        assert pooled == [grp] and len(groups) == 49            # the only MaxPool of the network; no group was lost for it


def test_a_second_consumer_or_a_requested_relu_output_refuses_the_pool():
    g, hooks = _resnet()
    before = _plan(g, hooks)
    v = g.operations['relu1'].outputs[0]
    spy = harness.Operation('spy', 'Identity', {}, [v], [])
    v.dest_ops.append(spy)
    _refused(g, hooks, before)
    v.dest_ops.remove(spy)
    assert STEM in _names(_plan(g, hooks))
    _refused(g, hooks, before, keep=set(g.outputs) | {v.name})
    # the pooled tensor itself may be asked for: the launch writes it
    assert STEM in _names(_plan(g, hooks, keep=set(g.outputs) | {g.operations['maxpool'].outputs[0].name}))


def test_an_activated_relu_output_config_refuses_the_pool():
    g, hooks = _resnet()
    before = _plan(g, hooks)
    relu, pool = g.operations['relu1'], g.operations['maxpool']
    for cfg in (relu.config.output_quantization_config[0], pool.config.input_quantization_config[0]):
        saved = cfg.state
        cfg.state = QuantizationStates.ACTIVATED
        _refused(g, hooks, before)
        cfg.state = saved
    assert STEM in _names(_plan(g, hooks))
    target = pool.config.input_quantization_config[0]                            # a delegated config: the executor's rule
    _refused(g, hooks, before, passes_through=lambda c: c is not target and not QuantizationStates.is_activated(c.state))


def test_a_pool_hook_that_observes_its_input_refuses_the_pool():
    g, hooks = _resnet()
    before = _plan(g, hooks)
    pool = g.operations['maxpool']
    table = hooks['maxpool']._observer_table
    assert pool.config.input_quantization_config[0] not in table
    table[pool.config.input_quantization_config[0]] = object()
    _refused(g, hooks, before)
    del table[pool.config.input_quantization_config[0]]
    table[pool.config.output_quantization_config[0]] = object()                  # the pooled tensor is written: it may be observed
    assert STEM in _names(_plan(g, hooks))
    del table[pool.config.output_quantization_config[0]]

    class OtherHook(CalibrationHook):
        pass
    hooks['maxpool'] = OtherHook(pool, table)
    _refused(g, hooks, before)


@pytest.mark.parametrize('attributes', [dict(ceil_mode=1), dict(dilations=2), dict(dilations=[1, 2]), dict(kernel_shape=[3, 2]),
                                        dict(strides=[2, 1]), dict(pads=[1, 0]), dict(pads=[1, 1, 1, 1])])
def test_pool_attributes_the_launch_has_no_form_for_refuse_the_pool(attributes):
    g, hooks = _resnet()
    before = _plan(g, hooks)
    g.operations['maxpool'].attributes.update(attributes)
    _refused(g, hooks, before)


def test_default_and_paired_pool_attributes_are_taken():
    g, hooks = _resnet()
    pool = g.operations['maxpool']
    pool.attributes.update(kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1], dilations=[1, 1], ceil_mode=0)
    assert STEM in _names(_plan(g, hooks)) and harness.pool_window(pool) == (3, 2, 1)
    pool.attributes.clear()
    pool.attributes.update(kernel_shape=2)
    assert harness.pool_window(pool) == (2, 1, 0)


def test_non_consecutive_members_refuse_the_pool():
    g, hooks = _resnet()
    ops = g.topological_sort()
    i = [op.name for op in ops].index('maxpool')
    ops.insert(i, ops.pop(i + 1))                  # conv2 now sits between relu1 and maxpool... which it reads: not a valid
    after = _names(harness.plan_epilogues(ops, hooks, set(g.outputs)))      # order to run, but the planner only looks at positions
    assert STEM not in after and PLAIN in after


def _jobs(grp): return {grp.relu.name: ('minmax', None)}


def test_the_relu_store_is_elided_only_when_nothing_else_reads_it():
    g, hooks = _resnet('minmax')
    grp = [x for x in _plan(g, hooks) if x.pool is not None][0]
    relu, pool = grp.relu, grp.pool
    assert harness.elidable_stores(grp, hooks, _jobs(grp)) == {'relu1'}
    assert harness.elidable_stores(grp, None, _jobs(grp)) == set()               # hook-less forwards store both tensors
    assert harness.elidable_stores(grp, hooks, {}) == set()                      # the observer got no sink
    assert harness.elidable_stores(grp, hooks, _jobs(grp), recorder=[]) == set() # reuse_activations records this forward
    plain = [x for x in _plan(g, hooks) if x.ops[0].name == 'conv2'][0]          # a P1 group without a pool has nothing to elide
    assert plain.pool is None and harness.elidable_stores(plain, hooks, {plain.relu.name: ('minmax', None)}) == set()
    # an observer whose observe() was replaced may read the values
    ob = hooks['relu1']._observer_table[relu.config.output_quantization_config[0]]

    class Spy(type(ob)):
        def observe(self, value): return super().observe(value)
    hooks['relu1']._observer_table[relu.config.output_quantization_config[0]] = Spy.__new__(Spy)
    assert harness.elidable_stores(grp, hooks, _jobs(grp)) == set()
    hooks['relu1']._observer_table[relu.config.output_quantization_config[0]] = ob
    # the pool's hook observes the tensor on its input side
    hooks['maxpool']._observer_table[pool.config.input_quantization_config[0]] = object()
    assert harness.elidable_stores(grp, hooks, _jobs(grp)) == set()
    del hooks['maxpool']._observer_table[pool.config.input_quantization_config[0]]
    # kept, or read by somebody else
    v = relu.outputs[0]
    kept = harness.EpilogueGroup('P1', grp.ops, grp.convs, None, relu, {v.name}, pool)
    assert harness.elidable_stores(kept, hooks, _jobs(grp)) == set()
    spy = harness.Operation('spy', 'Identity', {}, [v], [])
    v.dest_ops.append(spy)
    assert harness.elidable_stores(grp, hooks, _jobs(grp)) == set()
    v.dest_ops.remove(spy)
    assert harness.elidable_stores(grp, hooks, _jobs(grp)) == {'relu1'}
