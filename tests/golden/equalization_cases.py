"""Layerwise-equalization case graphs shared by tests/golden/make_equalization.py (which records what the reference's
LayerwiseEqualizationPass does to them on the CPU) and the equalization tests.

A case is a small topology given as data -- (type, name, inputs, attributes) per operation -- plus the pass settings.  The
maker builds it with the reference's graph API, the tests with ``harness_graph``.  Parameter names are ``<op>_w`` / ``<op>_b``,
the output of an operation is ``<op>_out`` (the harness's convention).  Conv attributes: cin, cout, k, group, bias; Gemm
attributes: cin, cout, transB, bias (``transB = 1`` stores [cout, cin], ``transB = 0`` [cin, cout]).

The weights are seeded normal values times a per-output-channel and a per-input-channel factor (ROWMUL / COLMUL), so that one
case holds channels under the value threshold (s == 1), channels clipped at 0.1 and at 10, and unclipped ones.

``seed`` (default 3000 + k) seeds the parameters: make_equalization.py refuses a case whose recording contains a scale on which
the CPU's square root is not the correctly rounded one, and such a case gets another seed.

``executable``: the harness can run the graph (its Gemm is ``F.linear``, so a ``transB = 0`` Gemm is weights only)."""
import torch

ROWMUL = [1.0, 0.02, 12.0, 0.01, 2.0, 0.3]
COLMUL = [1.0, 0.02, 0.01, 8.0, 0.5]


def _conv(name, src, cin, cout, k, group=1, bias=True):
    return ('Conv', name, [src], dict(cin=cin, cout=cout, k=k, group=group, bias=bias))


def _gemm(name, src, cin, cout, transB, bias=True):
    return ('Gemm', name, [src], dict(cin=cin, cout=cout, transB=transB, bias=bias))


def _relu(name, src): return ('Relu', name, [src], {})


CASES = [
    dict(name='chain', iterations=2, including_bias=False, including_act=False, executable=True, input=(2, 3, 8, 8),
         ops=[_conv('c1', 'input', 3, 8, 3), _relu('r1', 'c1_out'),                # 27 elements per channel: % 4 != 0
              _conv('c2', 'r1_out', 8, 6, 1, bias=False), _relu('r2', 'c2_out'),   # 1x1, no bias
              _conv('c3', 'r2_out', 6, 4, 3)], outputs=['c3_out']),
    dict(name='add_pair', iterations=10, including_bias=True, including_act=False, executable=True, input=(2, 3, 8, 8),
         ops=[_conv('c1', 'input', 3, 8, 3), _relu('r1', 'c1_out'),
              _conv('c2', 'r1_out', 8, 8, 3), _conv('c3', 'r1_out', 8, 8, 1),
              ('Add', 'add', ['c2_out', 'c3_out'], {}), _relu('r2', 'add_out'),
              _conv('c4', 'r2_out', 8, 5, 3), _conv('c5', 'r2_out', 8, 7, 1)], outputs=['c4_out', 'c5_out']),
    dict(name='grouped', iterations=2, including_bias=False, including_act=False, executable=True, input=(2, 3, 8, 8),
         ops=[_conv('c1', 'input', 3, 8, 3), _relu('r1', 'c1_out'),
              _conv('dw', 'r1_out', 8, 8, 3, group=8), _relu('r2', 'dw_out'),      # depthwise: in / G == 1
              _conv('g2', 'r2_out', 8, 12, 3, group=2), _relu('r3', 'g2_out'),     # in / G == 4: key order != natural order
              _conv('c4', 'r3_out', 12, 4, 1)], outputs=['c4_out']),
    dict(name='gemm', iterations=2, seed=3103, including_bias=True, including_act=False, executable=False, input=(4, 10),
         ops=[_gemm('fc1', 'input', 10, 16, 1), _relu('r1', 'fc1_out'),
              _gemm('fc2', 'r1_out', 16, 12, 0), _relu('r2', 'fc2_out'),
              _gemm('fc3', 'r2_out', 12, 5, 1), _relu('r3', 'fc3_out'),
              _gemm('fc4', 'r3_out', 5, 7, 0, bias=False)], outputs=['fc4_out']),
    dict(name='zero_act', iterations=1, including_bias=True, including_act=True, executable=True, input=(2, 3, 8, 8), batches=3,
         ops=[_conv('c1', 'input', 3, 8, 3), _relu('r1', 'c1_out'),                # output channel 3 of c1 is all zero
              _conv('c2', 'r1_out', 8, 6, 3), _relu('r2', 'c2_out'),
              _conv('c3', 'r2_out', 6, 4, 1)], outputs=['c3_out'], zero=('c1', 3)),
    dict(name='nan_key', iterations=1, including_bias=False, including_act=False, executable=False, input=(2, 3, 8, 8),
         ops=[_conv('c1', 'input', 3, 6, 3), _relu('r1', 'c1_out'),                # one NaN in output channel 2 of c1
              _conv('c2', 'r1_out', 6, 4, 3)], outputs=['c2_out'], nan=('c1', 2)),
]
VALUE_THRESHOLD = 0.5


def case_parameters(k: int) -> dict:
    """{variable name: float32 CPU tensor} of case k: deterministic."""
    case = CASES[k]
    g = torch.Generator().manual_seed(case.get('seed', 3000 + k))
    out = {}
    for kind, name, _, a in case['ops']:
        if kind not in ('Conv', 'Gemm'): continue
        cout, cin = a['cout'], a['cin']
        row = torch.tensor([ROWMUL[o % len(ROWMUL)] for o in range(cout)])
        if kind == 'Conv':
            ipg = cin // a['group']
            w = torch.randn(cout, ipg, a['k'], a['k'], generator=g) * 0.3
            og = cout // a['group']
            col = torch.tensor([[COLMUL[((o // og) * ipg + i) % len(COLMUL)] for i in range(ipg)] for o in range(cout)])
            w = w * row.view(-1, 1, 1, 1) * col.view(cout, ipg, 1, 1)
        else:
            col = torch.tensor([COLMUL[i % len(COLMUL)] for i in range(cin)])
            w = torch.randn(cout, cin, generator=g) * 0.3 * row.view(-1, 1) * col.view(1, -1)
            if a['transB'] == 0: w = w.t().contiguous()
        out[name + '_w'] = w.float().contiguous()
        if a['bias']: out[name + '_b'] = (torch.randn(cout, generator=g) * 0.2 * row).float()
    if 'zero' in case:
        op, c = case['zero']
        out[op + '_w'][c] = 0.0
        out[op + '_b'][c] = 0.0
    if 'nan' in case:
        op, c = case['nan']
        out[op + '_w'][c, 0, 0, 0] = float('nan')
    return out


def case_batches(k: int) -> list:
    """The calibration batches of case k (float32 CPU tensors): deterministic."""
    case = CASES[k]
    g = torch.Generator().manual_seed(4000 + k)
    return [torch.rand(case['input'], generator=g) for _ in range(case.get('batches', 2))]


def harness_graph(k: int, parameters: dict = None):
    """Case k as a ``ppq_amd.harness`` graph (CPU parameters; ``parameters`` default: ``case_parameters(k)``)."""
    from ppq_amd import harness
    case = CASES[k]
    parameters = case_parameters(k) if parameters is None else parameters
    g = harness.BaseGraph(case['name'])
    made = {'input': g.create_variable('input')}
    g.inputs['input'] = made['input']
    for kind, name, inputs, a in case['ops']:
        ins = [made[n] for n in inputs]
        attrs = {}
        if kind in ('Conv', 'Gemm'):
            ins.append(g.create_variable(name + '_w', parameters[name + '_w'].clone(), True))
            if a['bias']: ins.append(g.create_variable(name + '_b', parameters[name + '_b'].clone(), True))
            attrs = {'strides': 1, 'pads': a['k'] // 2, 'group': a['group']} if kind == 'Conv' else {'transB': a['transB']}
        made[name + '_out'] = g.create_operation(kind, name, ins, attrs)
    for n in case['outputs']: g.outputs[n] = made[n]
    return g


def natural_order_keys(w: torch.Tensor, groups: int) -> torch.Tensor:
    """max |.| per INPUT channel of a Conv weight [O, I / G, k...] in the natural (group, cin_local) order -- what the
    reference's downstream key order is NOT for groups > 1 and I / G > 1."""
    og = w.shape[0] // groups
    v = w.reshape(groups, og, w.shape[1], -1).permute(0, 2, 1, 3).reshape(groups * w.shape[1], -1)
    return v.abs().amax(dim=1)
