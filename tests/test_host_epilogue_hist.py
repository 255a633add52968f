"""Host side of the histogram sinks and the store elision of the convolution epilogues: which stores the executor may leave
out (harness.elidable_stores, on hand-built groups), the queue's bookkeeping for prepaid histogram rows, and the declaration
of the new entry points on both sides of the C ABI.  No device."""
import os
import re

import torch

from ppq_amd import _lib, harness
from ppq_amd.observer import ObservationQueue, OperationObserver, TorchHistObserver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('ppqhip_bias_act_hist', 'ppqhip_bias_add_act_hist', 'ppqhip_bias_add_act_stats2')


def _graph():
    """Conv-Relu, Conv + Conv-Add-Relu, Conv + identity-Add-Relu, GAP-Flatten-Gemm (the graph of the GPU pass tests)."""
    gen = torch.Generator().manual_seed(0)
    g = harness.BaseGraph('epilogue_hist_host')
    x = g.create_variable('input'); g.inputs['input'] = x

    def conv(inp, cin, cout, name, k=3):
        w = g.create_variable(name + '_w', harness._he([cout, cin, k, k], gen), True)
        b = g.create_variable(name + '_b', torch.randn(cout, generator=gen) * 0.1, True)
        return g.create_operation('Conv', name, [inp, w, b], {'strides': 1, 'pads': k // 2})

    y = g.create_operation('Relu', 'relu1', [conv(x, 3, 8, 'c1')])
    z, d = conv(y, 8, 8, 'c2'), conv(y, 8, 8, 'down', 1)
    y = g.create_operation('Relu', 'relu2', [g.create_operation('Add', 'add2', [z, d])])
    z = conv(y, 8, 8, 'c3')
    y = g.create_operation('Relu', 'relu3', [g.create_operation('Add', 'add3', [z, y])])
    y = g.create_operation('Flatten', 'flatten', [g.create_operation('GlobalAveragePool', 'gap', [y])])
    w = g.create_variable('fc_w', torch.randn([10, 8], generator=gen) * 0.3, True)
    y = g.create_operation('Gemm', 'fc', [y, w, g.create_variable('fc_b', torch.zeros(10), True)])
    g.outputs[y.name] = y
    return g


def _planned():
    """(graph, hooks, {Add name: its P2 group}) for a KL calibration of _graph()."""
    g = _graph()
    harness.quantize_graph(g, 'kl', hist_bins=2048)
    hooks = {}
    for name, op in g.operations.items():
        if not hasattr(op, 'config'): continue
        for cfg, var in op.config_with_variable:
            if not var.is_parameter: cfg.observer_algorithm = 'kl'
        hooks[name] = OperationObserver(operation=op, monitor_parameter=False).hook
    groups = harness.plan_epilogues(g.topological_sort(), hooks, set(g.outputs))
    p2 = {grp.add.name: grp for grp in groups if grp.kind == 'P2'}
    assert set(p2) == {'add2', 'add3'} and sum(grp.kind == 'P1' for grp in groups) == 1
    return g, hooks, p2


def _jobs(grp): return {op.name: ('minmax', None) for op in grp.ops if op.type in ('Conv', 'Relu')}


def test_elidable_stores_of_planned_groups():
    g, hooks, p2 = _planned()
    assert harness.elidable_stores(p2['add2'], hooks, _jobs(p2['add2'])) == {'c2', 'down'}
    assert harness.elidable_stores(p2['add3'], hooks, _jobs(p2['add3'])) == {'c3'}
    p1 = next(grp for grp in harness.plan_epilogues(g.topological_sort(), hooks, set(g.outputs)) if grp.kind == 'P1')
    assert harness.elidable_stores(p1, hooks, _jobs(p1)) == set()                 # bias_act has nothing to elide


def test_a_store_with_a_reader_stays():
    g, hooks, p2 = _planned()
    grp = p2['add2']
    jobs = _jobs(grp)
    c2, down = g.operations['c2'], g.operations['down']
    v = c2.outputs[0]
    # a second consumer
    v.dest_ops.append(g.operations['gap'])
    try: assert harness.elidable_stores(grp, hooks, jobs) == {'down'}
    finally: v.dest_ops.pop()
    # a graph output / a requested output: the planner's keep set (such a group is not even planned; hand-built here)
    kept = harness.EpilogueGroup('P2', grp.ops, grp.convs, grp.add, grp.relu, {v.name})
    assert harness.elidable_stores(kept, hooks, jobs) == {'down'}
    replanned = harness.plan_epilogues(g.topological_sort(), hooks, set(g.outputs) | {v.name})
    assert [grp.add.name for grp in replanned if grp.kind == 'P2'] == ['add3']
    # reuse_activations is recording the tensors of this forward
    assert harness.elidable_stores(grp, hooks, jobs, recorder=[]) == set()
    # a missing sink
    assert harness.elidable_stores(grp, hooks, {k: j for k, j in jobs.items() if k != 'c2'}) == {'down'}
    assert harness.elidable_stores(grp, hooks, {}) == set()
    # no hooks at all (an inference forward)
    assert harness.elidable_stores(grp, None, jobs) == set()
    # an observe that is not the library's own may read the tensor: a spy on the class, a subclass
    orig = TorchHistObserver.observe
    TorchHistObserver.observe = lambda self, value: orig(self, value)
    try: assert harness.elidable_stores(grp, hooks, jobs) == set()
    finally: TorchHistObserver.observe = orig
    assert harness.elidable_stores(grp, hooks, jobs) == {'c2', 'down'}
    ob = hooks['down']._observer_table[down.config.output_quantization_config[0]]

    class Reader(TorchHistObserver): pass
    ob.__class__ = Reader
    assert harness.elidable_stores(grp, hooks, jobs) == {'c2'}
    ob.__class__ = TorchHistObserver
    # another hook of the group observes the variable: the Add's input side
    add = grp.add
    cfg = add.config.input_quantization_config[0]
    hooks['add2']._observer_table[cfg] = ob
    try: assert harness.elidable_stores(grp, hooks, jobs) == {'down'}
    finally: del hooks['add2']._observer_table[cfg]
    assert harness.elidable_stores(grp, hooks, jobs) == {'c2', 'down'}


def test_hist_observer_jobs_follow_the_phase():
    """stat_job: the running range in phase 1; in phase 2 the rows job only with a queue (else observe launches at once)."""
    g, hooks, p2 = _planned()
    ob = hooks['c3']._observer_table[g.operations['c3'].config.output_quantization_config[0]]
    assert type(ob) is TorchHistObserver and ob.reads_only_its_job()
    assert ob.stat_job(torch.zeros(4))[0] == 'minmax'
    ob._phase, ob._hist_scale = 'Collating Hist', 0.01
    assert ob.stat_job(torch.zeros(4)) is None                    # no queue
    assert ob._hist is None and ob._rows is None                  # ... and nothing was allocated for it


def test_hist_observer_rows_job(monkeypatch):
    """With a queue, phase 2 hands out what observe() would give ObservationQueue.add_hist: the observer's own rows
    [hist_rows, bins], the rule of its policy with its parameters, clip_outliers on -- and observe() then queues exactly
    that pair.  Per-channel observers, and one whose rows were folded away, have no rows job."""
    from ppq_amd import observer as obs
    from ppq_amd.core import QuantizationProperty as P

    class FakeCUDA:
        @staticmethod
        def hist_rows(): return 6
    monkeypatch.setattr(obs, 'CUDA', FakeCUDA)
    g, hooks, p2 = _planned()
    x = torch.zeros(4)
    for asym in (False, True):
        ob = TorchHistObserver('x', g.operations['c3'].config.output_quantization_config[0], hist_bins=128)
        ob.queue = q = ObservationQueue()
        ob._hist_bins = 128                                       # (the config's own bin count would win in __init__)
        ob._phase, ob._hist_scale, ob._min, ob._max = 'Collating Hist', 0.25, -1.5, 2.0
        if asym:
            pol = ob._quant_cfg.policy
            monkeypatch.setattr(type(pol), 'has_property', lambda self, p, real=type(pol).has_property:
                                (p == P.ASYMMETRICAL) if p in (P.ASYMMETRICAL, P.SYMMETRICAL) else real(self, p))
        job = ob.stat_job(x)
        rows = job[1]
        assert rows is ob._rows and rows.shape == (6, 128) and rows.dtype == torch.int32 and int(rows.sum()) == 0
        assert job == (('hist_rows', rows, True, -1.5, 2.0, True) if asym else ('hist_rows', rows, False, 0.25, 0.0, True))
        assert ob.stat_job(x)[1] is rows                          # the same buffers every time
        ob.observe(x)
        (key, items), = q._hist.items()
        assert key[0] == asym and key[1] == 128 and items[0][0] is x and items[0][1] is rows
        assert items[0][2:] == ((-1.5, 2.0) if asym else (0.25, 0.0)) and ob._rows_dirty
        q.prepay(x, rows)
        ob.observe(x)                                             # prepaid: claimed, not queued again
        assert len(q) == 1 and not q._prepaid
        ob._rows = None                                           # folded at a render: observe would take the _hist path
        assert ob.stat_job(x) is None
        monkeypatch.undo(); monkeypatch.setattr(obs, 'CUDA', FakeCUDA)
    # per channel: no per-tensor job in either phase
    ob = TorchHistObserver('x', g.operations['c3'].config.output_quantization_config[0], hist_bins=128)
    ob.queue = ObservationQueue()
    pol = ob._quant_cfg.policy
    monkeypatch.setattr(type(pol), 'has_property', lambda self, p, real=type(pol).has_property:
                        (p == P.PER_CHANNEL) if p in (P.PER_CHANNEL, P.PER_TENSOR) else real(self, p))
    assert ob.stat_job(x) is None
    ob._phase = 'Collating Hist'
    assert ob.stat_job(x) is None and ob._rows is None


def test_queue_claims_prepaid_histogram_rows_once():
    q = ObservationQueue()
    v, w = torch.zeros(8), torch.zeros(8)
    rows, other = torch.zeros(4, 16, dtype=torch.int32), torch.zeros(4, 16, dtype=torch.int32)
    q.prepay(v, rows)
    q.add_hist(v, other, False, 0.1)          # same tensor, other rows: queued
    q.add_hist(w, rows, False, 0.1)           # same rows, another tensor: queued
    assert len(q) == 2
    q.add_hist(v, rows, False, 0.1)           # the prepaid pair: dropped ...
    assert len(q) == 2
    q.add_hist(v, rows, False, 0.1)           # ... once
    assert len(q) == 3


def test_new_entry_points_are_declared_on_both_sides():
    header = open(os.path.join(ROOT, 'include', 'ppq_hip.h')).read()
    declared = set(re.findall(r'\b(ppqhip_[a-z0-9_]+)\s*\(', header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(_lib.lib, name), name
    assert _lib.lib.ppqhip_version() == _lib.ABI_VERSION == 4          # added under the same ABI version
    # the elide argument sits in front of the stream on both sides
    for name in ('ppqhip_bias_add_act_hist', 'ppqhip_bias_add_act_stats2'):
        proto = re.search(name + r'\s*\(([^;]*)\)\s*;', header).group(1)
        params = [p.strip() for p in proto.split(',')]
        assert params[-2] == 'int elide' and params[-1] == 'void* stream' and len(params) == len(_lib.PROTOTYPES[name][1])
