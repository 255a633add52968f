"""SSD-equalization case graphs shared by tests/golden/make_ssd.py (which records what the reference's SSDEqualizationPass
does to them on the CPU) and the SSD tests.

A case is a small topology given as data -- (type, name, inputs, attributes) per operation -- in the style of
equalization_cases.py: parameter names are ``<op>_w`` / ``<op>_b``, the output of an operation is ``<op>_out``.  Conv attributes:
cin, cout, k, group, bias; Gemm attributes: cin, cout, transB, bias; MaxPool: k (kernel and stride).

The weights are seeded normal values times a per-output-channel and a per-input-channel factor (ROWMUL / COLMUL) -- the
per-channel imbalance equalization is for, wide enough for the DFQ scale to meet both of its clips -- and ``gain`` scales the
whole first weight of a case (a small one gives activations under the 0.01 floor).

Quantisation (TensorRT-style INT8, 'kl' activations with 2048 bins): ``per_channel`` -- per-channel or per-tensor weights;
``passive_bias`` -- the integer platforms' 32-bit bias whose scale is derived (PASSIVE_INIT), else FP32 bias.

``seed`` seeds the parameters: make_ssd.py refuses a case whose recording carries a mis-rounded CPU square root or quotient or
a decision closer than 5 %, and such a case gets another seed.  ``executable``: the harness can run the graph (its Gemm is
``F.linear``, so a ``transB = 0`` Gemm is weights only)."""
import torch

ROWMUL = [1.0, 0.02, 12.0, 0.01, 2.0, 0.3]
COLMUL = [1.0, 0.02, 0.01, 8.0, 0.5]
HIST_BINS = 2048
LOSS_THRESHOLD = 0.8
CHANNEL_RATIO = 0.5


def _conv(name, src, cin, cout, k, group=1, bias=True):
    return ('Conv', name, [src], dict(cin=cin, cout=cout, k=k, group=group, bias=bias))


def _gemm(name, src, cin, cout, transB, bias=True):
    return ('Gemm', name, [src], dict(cin=cin, cout=cout, transB=transB, bias=bias))


def _relu(name, src): return ('Relu', name, [src], {})
def _pool(name, src, k=2): return ('MaxPool', name, [src], dict(k=k))


CASES = [
    dict(name='chain', iterations=3, per_channel=False, passive_bias=False, executable=True, input=(4, 3, 16, 16), seed=5113,
         ops=[_conv('c1', 'input', 3, 12, 3), _relu('r1', 'c1_out'),               # two pairs that share c2
              _conv('c2', 'r1_out', 12, 8, 3), _relu('r2', 'c2_out'),
              _conv('c3', 'r2_out', 8, 4, 1)], outputs=['c3_out']),
    dict(name='pool', iterations=2, per_channel=True, passive_bias=False, executable=True, input=(4, 3, 16, 16), seed=5101,
         ops=[_conv('c1', 'input', 3, 8, 3), _relu('r1', 'c1_out'), _pool('p1', 'r1_out'),   # a MaxPool relay
              _conv('c2', 'p1_out', 8, 6, 3, bias=False)], outputs=['c2_out']),
    dict(name='depthwise', iterations=2, per_channel=False, passive_bias=False, executable=True, input=(4, 3, 16, 16), seed=5111,
         ops=[_conv('c1', 'input', 3, 8, 3), _relu('r1', 'c1_out'),
              _conv('dw', 'r1_out', 8, 8, 3, group=8), _relu('r2', 'dw_out'),      # depthwise: in / G == 1
              _conv('g2', 'r2_out', 8, 12, 3, group=2), _relu('r3', 'g2_out'),     # in / G == 4
              _conv('c4', 'r3_out', 12, 4, 1)], outputs=['c4_out']),
    dict(name='gemm', iterations=2, per_channel=False, passive_bias=False, executable=False, input=(4, 10), seed=5104,
         ops=[_gemm('fc1', 'input', 10, 16, 1), _relu('r1', 'fc1_out'),
              _gemm('fc2', 'r1_out', 16, 12, 0), _relu('r2', 'fc2_out'),
              _gemm('fc3', 'r2_out', 12, 6, 1), _relu('r3', 'fc3_out'),
              _gemm('fc4', 'r3_out', 6, 7, 0, bias=False)], outputs=['fc4_out']),
    dict(name='branch', iterations=2, per_channel=False, passive_bias=False, executable=True, input=(4, 3, 16, 16), seed=5106,
         ops=[_conv('c1', 'input', 3, 8, 3), _relu('r1', 'c1_out'),                # r1 feeds two operations: no pair starts at c1
              _conv('c2', 'r1_out', 8, 6, 3), _conv('c3', 'r1_out', 8, 5, 1),
              _relu('r2', 'c2_out'), _conv('c4', 'r2_out', 6, 4, 1)], outputs=['c4_out', 'c3_out']),
    dict(name='passive_bias', iterations=2, per_channel=False, passive_bias=True, executable=True, input=(4, 3, 16, 16), seed=5111,
         gain=0.0005,
         ops=[_conv('c1', 'input', 3, 8, 3), _relu('r1', 'c1_out'),
              _conv('c2', 'r1_out', 8, 6, 3), _relu('r2', 'c2_out'),
              _conv('c3', 'r2_out', 6, 4, 1)], outputs=['c3_out']),
]
# A pair wider than one workgroup of the SSD kernels (256 lanes): NOT among the recorded cases (CASES is what the golden-driven
# tests iterate over), for tests that compare the two arms of the pass on the device.  `batch_seed` stands in for the case index.
WIDE = dict(name='wide', iterations=2, per_channel=False, passive_bias=False, executable=True, input=(4, 3, 16, 16), seed=5120,
            batch_seed=6100,
            ops=[_conv('c1', 'input', 3, 264, 3), _relu('r1', 'c1_out'), _conv('c2', 'r1_out', 264, 40, 3)], outputs=['c2_out'])
BATCHES = 3
CALIB_STEPS = 8                      # more steps than batches: the calibration loops of the pass go round the loader


def case_index(name: str) -> int:
    return [c['name'] for c in CASES].index(name)


def _case(k) -> dict:
    """A case given as its index in CASES, or as the case dict itself (a case that is not recorded)."""
    return k if isinstance(k, dict) else CASES[k]


def case_parameters(k) -> dict:
    """{variable name: float32 CPU tensor} of case k: deterministic."""
    case = _case(k)
    g = torch.Generator().manual_seed(case['seed'])
    out, first = {}, True
    for kind, name, _, a in case['ops']:
        if kind not in ('Conv', 'Gemm'): continue
        cout, cin = a['cout'], a['cin']
        row = torch.tensor([ROWMUL[o % len(ROWMUL)] for o in range(cout)])
        gain = case.get('gain', 1.0) if first else 1.0
        first = False
        if kind == 'Conv':
            ipg, og = cin // a['group'], cout // a['group']
            col = torch.tensor([[COLMUL[((o // og) * ipg + i) % len(COLMUL)] for i in range(ipg)] for o in range(cout)])
            w = torch.randn(cout, ipg, a['k'], a['k'], generator=g) * 0.3 * row.view(-1, 1, 1, 1) * col.view(cout, ipg, 1, 1) * gain
        else:
            col = torch.tensor([COLMUL[i % len(COLMUL)] for i in range(cin)])
            w = torch.randn(cout, cin, generator=g) * 0.3 * row.view(-1, 1) * col.view(1, -1) * gain
            if a['transB'] == 0: w = w.t().contiguous()
        out[name + '_w'] = w.float().contiguous()
        if a['bias']: out[name + '_b'] = (torch.randn(cout, generator=g) * 0.2 * row * gain).float()
    return out


def case_batches(k) -> list:
    """The calibration batches of case k (float32 CPU tensors): deterministic."""
    case = _case(k)
    g = torch.Generator().manual_seed(case['batch_seed'] if isinstance(k, dict) else 6000 + k)
    return [torch.rand(case['input'], generator=g) for _ in range(BATCHES)]


def harness_graph(k, parameters: dict = None, quantize: bool = True):
    """Case k (an index in CASES or a case dict) as a ``ppq_amd.harness`` graph with CPU parameters (default:
    ``case_parameters(k)``), quantised as the module docstring says."""
    from ppq_amd import harness
    case = _case(k)
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
        elif kind == 'MaxPool': attrs = {'kernel_shape': a['k'], 'strides': a['k'], 'pads': 0}
        made[name + '_out'] = g.create_operation(kind, name, ins, attrs)
    for n in case['outputs']: g.outputs[n] = made[n]
    if quantize:
        harness.quantize_graph(g, 'kl', per_channel_weight=case['per_channel'], hist_bins=HIST_BINS, passive_bias=case['passive_bias'])
    return g
