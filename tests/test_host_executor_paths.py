"""The three entry points of harness.TorchExecutor -- ``forward``, ``partial_graph_forward``, ``forward_cached`` -- walk the same
operations the same way: the same quantise / hook / forward calls in the same order, the same values, and each keeps its own store
(``Variable.value`` or the caller's cache), early stop and clearing.  No device: every run leaves a trace of
``(event, operation, identities)``, and the quantise wrapper rounds to a grid of its config's own, so that a call that moved shows
in the values too.

Without a device ``_run_epilogue`` declines every group before it runs anything (the operands are not on the GPU).  ``cpu_epilogue``
stands in for it where a test is about what the walk does with a group that DID run: the members one by one, in the unfused order."""
import pytest
import torch

from ppq_amd import harness
from ppq_amd.observer import CalibrationHook

N_INPUTS = {'c1': 3, 'c1_relu': 1, 'c2': 3, 'add': 2, 'add_relu': 1, 'gap': 1, 'flatten': 1, 'fc': 3}     # in execution order
HIDDEN = ('c1_out', 'add_out')                 # what a P1 / P2 epilogue launch never writes on its own


def expected(hooked, ops=N_INPUTS):
    """Per operation: quantise inputs, pre-hook, forward, quantise outputs, post-hook."""
    trace = []
    for op in ops:
        ins = tuple((op, 'in', i) for i in range(N_INPUTS[op]))
        trace += [('quantize', op, c) for c in ins]
        if hooked: trace.append(('pre_hook', op, ins))
        trace.append(('forward', op, N_INPUTS[op]))
        trace.append(('quantize', op, (op, 'out', 0)))
        if hooked: trace.append(('post_hook', op, ((op, 'out', 0),)))
    return trace


class RecordingHook(CalibrationHook):
    """Observes nothing, records its calls.  ``plain(...)`` is the same on an instance whose type is CalibrationHook itself: the
    only hook type whose operations the epilogue planner groups."""
    def __init__(self, rig, op):
        super().__init__(op, {})
        self.pre_forward_hook = lambda inputs, quant_inputs, quant_configs: rig.hooked('pre_hook', op, inputs, quant_inputs, quant_configs)
        self.post_forward_hook = lambda outputs, quant_outputs, quant_configs: rig.hooked('post_hook', op, outputs, quant_outputs, quant_configs)

    @ classmethod
    def plain(cls, rig, op):
        hook = CalibrationHook(op, {})
        hook.pre_forward_hook, hook.post_forward_hook = (getattr(cls(rig, op), n) for n in ('pre_forward_hook', 'post_forward_hook'))
        return hook


class Rig:
    def __init__(self, monkeypatch, quantized=True, fuse_epilogues=True, epilogue_runs=False):
        self.graph = g = harness.small_cnn_graph(seed=0)
        if quantized: harness.quantize_graph(g, 'minmax')
        self.ex = ex = harness.TorchExecutor(g, 'cpu')
        ex.fuse_epilogues = fuse_epilogues
        self.trace, self.epilogues, self.written = [], [], []
        self.x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
        self.names = [v.name for op in g.topological_sort() for v in op.outputs]
        self.label = {}
        if quantized:
            for op in g.operations.values():
                for side, cfgs in (('in', op.config.input_quantization_config), ('out', op.config.output_quantization_config)):
                    for i, c in enumerate(cfgs): self.label[id(c)] = (op.name, side, i)
        steps = {key: 2.0 ** -(4 + k % 3) for k, key in enumerate(self.label)}
        quantize, forward, run_epilogue = ex.quantize_function, harness._forward, ex._run_epilogue

        def quantize_function(tensor, config=None):
            self.trace.append(('quantize', self.label[id(config)][0], self.label[id(config)]))
            return torch.round(quantize(tensor, config) / steps[id(config)]) * steps[id(config)]

        def _forward(op, inputs):
            self.trace.append(('forward', op.name, len(inputs)))
            return forward(op, inputs)

        def _run_epilogue(grp, raw_of, hooks):
            self.epilogues.append([m.name for m in grp.ops])
            return self.cpu_epilogue(grp, raw_of, hooks) if epilogue_runs else run_epilogue(grp, raw_of, hooks)

        ex.quantize_function, ex._run_epilogue = quantize_function, _run_epilogue
        monkeypatch.setattr(harness, '_forward', _forward)
        rig = self

        def set_value(var, value):               # every write of an activation's Variable.value
            if not var.is_parameter and value is not None: rig.written.append(var.name)
            var.__dict__['value'] = value
        monkeypatch.setattr(harness.Variable, 'value', property(lambda var: var.__dict__['value'], set_value), raising=False)

    def cpu_epilogue(self, grp, raw_of, hooks):
        hooks, values = hooks or {}, {}
        if any(raw_of(conv.inputs[0]) is None for conv in grp.convs): return None        # declines before anything ran, like the real one
        for op in grp.ops:
            hook, cfg = hooks.get(op.name), op.config
            raw = [values[v.name] if v.name in values else raw_of(v) for v in op.inputs]
            qin = [self.ex.quantize_function(x, c) for x, c in zip(raw, cfg.input_quantization_config)]
            if hook is not None: qin = hook.pre_forward_hook(inputs=raw, quant_inputs=qin, quant_configs=list(cfg.input_quantization_config))
            y = harness._forward(op, qin)
            outs = [self.ex.quantize_function(y, cfg.output_quantization_config[0])]
            if hook is not None: outs = hook.post_forward_hook(outputs=[y], quant_outputs=outs, quant_configs=list(cfg.output_quantization_config))
            values[op.outputs[0].name] = outs[0]
        return values

    def hooked(self, event, op, raw, quant, configs):
        assert len(raw) == len(quant) and (configs is None or len(configs) == len(raw))
        self.trace.append((event, op.name, None if configs is None else tuple(self.label[id(c)] for c in configs)))
        return quant

    def hooks(self, make=RecordingHook):
        return {name: make(self, op) for name, op in self.graph.operations.items()}

    def run(self, fn, *args, **kw):
        """(outputs, trace, variables written) of one call."""
        del self.trace[:], self.written[:], self.epilogues[:]
        out = fn(*args, **kw)
        return out, list(self.trace), list(self.written)

    def activations(self):
        return [v for v in self.graph.variables.values() if not v.is_parameter]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('epilogue_runs', [False, True], ids=['epilogue_declines', 'epilogue_runs'])
def test_the_three_entry_points_make_the_same_calls_and_values(monkeypatch, epilogue_runs):
    rig = Rig(monkeypatch, epilogue_runs=epilogue_runs)
    ex, ops = rig.ex, rig.graph.topological_sort()
    outs = list(rig.graph.outputs)
    want, trace, written = rig.run(ex.forward, rig.x)
    assert trace == expected(hooked=False) and rig.epilogues == [['c1', 'c1_relu'], ['c2', 'add', 'add_relu']]
    assert sorted(written) == sorted(rig.names + ['input']) and all(v.value is None for v in rig.activations())
    got, trace, written = rig.run(ex.partial_graph_forward, ops, {'input': rig.x}, outs)
    assert same(got, want) and trace == expected(hooked=False)
    assert sorted(written) == sorted(rig.names + ['input']) and all(v.value is None for v in rig.activations())
    cache = {}
    got, trace, written = rig.run(ex.forward_cached, rig.x, outs, cache)
    assert same(got, want) and trace == expected(hooked=False)
    assert written == [] and all(v.value is None for v in rig.activations())              # the cache is its only store
    assert set(cache) == {'input', *rig.names} - set(HIDDEN if epilogue_runs else ())
    every = ex.forward(rig.x, rig.names)                                                  # and every intermediate tensor
    assert same(ex.partial_graph_forward(ops, {'input': rig.x}, rig.names), every)
    assert same(ex.forward_cached(rig.x, rig.names, {}), every)
    assert not torch.equal(every[0], every[1]) and not same(every, harness.TorchExecutor(rig.graph, 'cpu').forward(rig.x, rig.names))


@pytest.mark.parametrize('fuse_epilogues', [True, False])
@pytest.mark.parametrize('make', [RecordingHook, RecordingHook.plain], ids=['subclass', 'plain'])
def test_hooked_forward_runs_every_operation_in_the_unfused_order(monkeypatch, fuse_epilogues, make):
    """A grouped forward (plain CalibrationHooks, epilogues on) quantises and hooks member by member like the ungrouped one."""
    rig = Rig(monkeypatch, fuse_epilogues=fuse_epilogues, epilogue_runs=True)
    want = rig.ex.forward(rig.x, rig.names)
    got, trace, _ = rig.run(rig.ex.forward, rig.x, rig.names, rig.hooks(make))
    assert trace == expected(hooked=True) and same(got, want)
    # requested intermediates keep their groups apart; with the graph's own outputs the groups form, for plain hooks only
    _, trace, _ = rig.run(rig.ex.forward, rig.x, None, rig.hooks(make))
    assert trace == expected(hooked=True)
    assert rig.epilogues == ([['c1', 'c1_relu'], ['c2', 'add', 'add_relu']] if fuse_epilogues and make == RecordingHook.plain else [])


@pytest.mark.parametrize('epilogue_runs', [False, True], ids=['epilogue_declines', 'epilogue_runs'])
def test_stop_early_only_with_requested_outputs_and_no_hooks(monkeypatch, epilogue_runs):
    rig = Rig(monkeypatch, epilogue_runs=epilogue_runs)
    want = rig.ex.forward(rig.x, rig.names)
    got, trace, _ = rig.run(rig.ex.forward, rig.x, ['c1_relu_out'])
    assert trace == expected(False, ['c1', 'c1_relu']) and torch.equal(got[0], want[1])
    assert all(v.value is None for v in rig.activations())
    got, trace, _ = rig.run(rig.ex.forward, rig.x, ['c1_relu_out'], rig.hooks())
    assert trace == expected(True) and torch.equal(got[0], want[1])
    _, trace, _ = rig.run(rig.ex.forward, rig.x)                                          # no names: the graph's outputs, the whole walk
    assert trace == expected(False)


@pytest.mark.parametrize('epilogue_runs', [False, True], ids=['epilogue_declines', 'epilogue_runs'])
def test_forward_cached_runs_only_what_its_cache_lacks(monkeypatch, epilogue_runs):
    rig = Rig(monkeypatch, epilogue_runs=epilogue_runs)
    ex = rig.ex
    want = ex.forward(rig.x, rig.names)
    cache = {}
    got, trace, _ = rig.run(ex.forward_cached, rig.x, ['c1_relu_out'], cache)
    assert trace == expected(False, ['c1', 'c1_relu']) and torch.equal(got[0], want[1])
    assert set(cache) == {'input', 'c1_relu_out'} | ({'c1_out'} - set(HIDDEN if epilogue_runs else ()))
    held = dict(cache)
    got, trace, written = rig.run(ex.forward_cached, rig.x, list(rig.graph.outputs), cache)
    assert trace == expected(False, ['c2', 'add', 'add_relu', 'gap', 'flatten', 'fc']) and torch.equal(got[0], want[-1]) and written == []
    assert all(cache[k] is v for k, v in held.items())                                    # what was there is reused, not replaced
    assert set(cache) == {'input', *rig.names} - set(HIDDEN if epilogue_runs else ())
    got, trace, _ = rig.run(ex.forward_cached, rig.x, list(rig.graph.outputs), cache)
    assert trace == [] and torch.equal(got[0], want[-1])
    if epilogue_runs:                                # a hidden tensor asked for later is recomputed, on its own
        got, trace, _ = rig.run(ex.forward_cached, rig.x, ['add_out'], cache)
        assert trace == expected(False, ['add']) and torch.equal(got[0], want[rig.names.index('add_out')])
    with pytest.raises(ValueError, match='forward_cached: graph input input was not fed'): ex.forward_cached({}, ['fc_out'], {})
    with pytest.raises(ValueError, match='partial_graph_forward: input of c2 was not fed'):
        ex.partial_graph_forward(rig.graph.topological_sort()[2:], {}, ['fc_out'])


def test_only_forward_with_gradient_and_with_gradient_record_autograd(monkeypatch):
    rig = Rig(monkeypatch)
    ex, ops = rig.ex, rig.graph.topological_sort()
    rig.graph.variables['fc_w'].value.requires_grad_(True)
    want = ex.forward(rig.x)
    assert not want[0].requires_grad
    got, trace, _ = rig.run(ex.forward_with_gradient, rig.x)
    assert got[0].requires_grad and torch.equal(got[0], want[0]) and trace == expected(False) and rig.epilogues == []
    got, trace, _ = rig.run(ex.forward_with_gradient, rig.x, ['c1_relu_out'], rig.hooks())
    assert trace == expected(True) and not got[0].requires_grad                           # nothing upstream of it requires grad
    assert not ex.partial_graph_forward(ops, {'input': rig.x}, ['fc_out'])[0].requires_grad
    assert ex.partial_graph_forward(ops, {'input': rig.x}, ['fc_out'], with_gradient=True)[0].requires_grad
    assert not ex.forward_cached(rig.x, ['fc_out'], {})[0].requires_grad
    assert all(v.value is None for v in rig.activations())


PACKED = object()                                    # what a group override hands to an override that takes_packed


def test_overrides_replace_the_input_side_and_see_the_packed_form_in_forward_only(monkeypatch):
    rig = Rig(monkeypatch)
    ex, ops = rig.ex, rig.graph.topological_sort()
    want = ex.forward(rig.x, rig.names)
    seen = []

    def c2(op, raw):
        seen.append(raw[0])
        rig.trace.append(('override', op.name, len(raw)))
        return want[2] + 1.0

    def head(members, inputs, need_float):           # c1 + c1_relu as one call: float for the Add, packed for c2
        rig.trace.append(('group', members[0].name, tuple(sorted(need_float))))
        assert [len(i) for i in inputs] == [3, 1] and inputs[1] == [None]
        return {'c1_relu_out': want[1]}, {'c1_out': PACKED, 'c1_relu_out': PACKED}

    def tail(override=True, hooked=False):
        rest = expected(hooked, ['c2', 'add', 'add_relu', 'gap', 'flatten', 'fc'])
        return [('override', 'c2', 3)] + rest[rest.index(('forward', 'c2', 3)) + 1:] if override else rest
    ex.register_operation_override('c2', c2, takes_packed=True)
    changed, trace, _ = rig.run(ex.forward, rig.x)
    assert trace == expected(False, ['c1', 'c1_relu']) + tail() and not torch.equal(changed[0], want[-1])
    _, trace, _ = rig.run(ex.forward, rig.x, None, {'c2': RecordingHook(rig, rig.graph.operations['c2'])})
    hooked_c2 = expected(True, ['c2'])
    assert trace == expected(False, ['c1', 'c1_relu']) + hooked_c2 + tail(False)[len(hooked_c2) - 2:]      # a hooked operation ignores it
    ex.register_group_override(['c1', 'c1_relu'], head)
    for call, packed in ((lambda: ex.forward(rig.x), True), (lambda: ex.partial_graph_forward(ops, {'input': rig.x}, ['fc_out']), False),
                         (lambda: ex.forward_cached(rig.x, ['fc_out'], cache), False)):
        cache = {}
        del seen[:]
        got, trace, _ = rig.run(call)
        assert trace == [('group', 'c1', ('c1_relu_out',))] + tail() and same(got, changed)
        assert len(seen) == 1 and (seen[0] is PACKED if packed else seen[0] is want[1])
        assert set(cache) <= {'input', *rig.names} - {'c1_out'}                           # of a group override, only the last output
    assert all(v.value is None for v in rig.activations())


def test_a_hooked_operation_that_is_not_quantable_gets_no_configs(monkeypatch):
    """The one behaviour the shared step changed: before it, ``forward`` read the config lists of the previous quantable operation
    here, or failed with UnboundLocalError where there was none -- as in this graph, so this test cannot pass on the loops it
    replaced."""
    rig = Rig(monkeypatch, quantized=False)
    want = rig.ex.forward(rig.x)
    got, trace, _ = rig.run(rig.ex.forward, rig.x, None, rig.hooks())
    assert same(got, want)
    assert trace == [e for op, n in N_INPUTS.items() for e in (('pre_hook', op, None), ('forward', op, n), ('post_hook', op, None))]
