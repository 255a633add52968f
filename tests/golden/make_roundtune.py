"""Record the REFERENCE's round-tuning outputs (ppq/quantization/algorithm/training.py:490-590) on CPU for the cases of
roundtune_cases.py.

Run where the reference is importable (oracle/reference_import.find_reference); no GPU test imports it:

    python tests/golden/make_roundtune.py

Writes tests/golden/roundtune.npz: per case the inputs (w, scale, offset, dy), the reference's RoundTruningDelegator state
after construction (the initial R, the floored weight), R after the perturbation of roundtune_cases, the delegator's
__call__ at that R, dR by autograd for sum(out * dy), and the finalised weight.  The conditions the tests rely on (see
check_conditions) are asserted before anything is written.  Import shims as in make_golden.py."""
import importlib.machinery
import os
import sys
from unittest.mock import MagicMock

os.environ['PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION'] = 'python'
sys.dont_write_bytecode = True
for _name in ['onnx', 'onnx.helper', 'onnx.numpy_helper', 'onnx.mapping', 'onnx.onnx_pb', 'onnx.checker',
              'onnx.external_data_helper', 'onnx.shape_inference', 'onnx.version_converter']:
    _m = MagicMock(); _m.__spec__ = importlib.machinery.ModuleSpec(_name, None); _m.__path__ = []
    sys.modules[_name] = _m
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle.reference_import import find_reference  # noqa: E402

assert find_reference() is not None, 'the reference is not importable here'
sys.path.insert(0, find_reference())

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ppq.core import (PPQ_CONFIG, QuantizationPolicy, QuantizationProperty, QuantizationStates,  # noqa: E402
                      RoundingPolicy, TensorQuantizationConfig)
from ppq.IR import Variable  # noqa: E402
from ppq.quantization.algorithm.training import RoundTruningDelegator  # noqa: E402

assert PPQ_CONFIG.USING_CUDA_KERNEL is False
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from roundtune_cases import CASES, _view, case_tensors  # noqa: E402

P = QuantizationProperty


def config(axis, qmin, qmax, asym, bits):
    pol = P.LINEAR + (P.PER_CHANNEL.value if axis is not None else P.PER_TENSOR.value) \
        + (P.ASYMMETRICAL.value if asym else P.SYMMETRICAL.value)
    cfg = TensorQuantizationConfig(policy=QuantizationPolicy(pol), rounding=RoundingPolicy.ROUND_HALF_EVEN, num_of_bits=bits,
                                   quant_min=qmin, quant_max=qmax, observer_algorithm='minmax', channel_axis=axis)
    cfg.state = QuantizationStates.ACTIVATED
    return cfg


def check_conditions(arrays: dict) -> dict:
    """The conditions on the inputs without which the tests would pass vacuously; returns the counts per case.  Every case:
    both R > .5 and R <= .5 occur, and the perturbation moves at least one element across .5.  At least one case: the clamp
    changes elements at each end; at least one case: floored-weight elements whose t / s is not an integer in fp32."""
    counts = {}
    for k, (name, shape, axis, qmin, qmax, asym, _) in enumerate(CASES):
        p = f'c{k}_'
        r0, r, t = (torch.from_numpy(arrays[p + x]) for x in ('r0', 'r', 'wfloor'))
        s = _view(torch.from_numpy(arrays[p + 'scale']), axis, t.ndim)
        o = _view(torch.from_numpy(arrays[p + 'offset']), axis, t.ndim)
        q = (t / s) + (r > .5) + o
        c = dict(up=int((r0 > .5).sum()), down=int((r0 <= .5).sum()), crossed=int(((r0 > .5) != (r > .5)).sum()),
                 clamp_low=int((q < qmin).sum()), clamp_high=int((q > qmax).sum()),
                 non_integer=int(((t / s) != (t / s).round()).sum()))
        assert c['up'] > 0 and c['down'] > 0 and c['crossed'] > 0, (name, c)
        counts[name] = c
    assert any(c['clamp_low'] > 0 and c['clamp_high'] > 0 for c in counts.values()), counts
    assert any(c['non_integer'] > 0 for c in counts.values()), counts
    return counts


def main():
    out = {}
    for k, (name, shape, axis, qmin, qmax, asym, _) in enumerate(CASES):
        w, scale, offset, noise, dy = case_tensors(k)
        cfg = config(axis, qmin, qmax, asym, 4 if qmax - qmin < 16 else 8)
        cfg.scale, cfg.offset = scale.clone(), offset.clone()
        var = Variable(name=name, value=w.clone(), is_parameter=True)
        d = RoundTruningDelegator(var=var, config=cfg)
        r0 = d._rounding.detach().clone()
        wfloor = var.value.detach().clone()
        with torch.no_grad(): d._rounding.add_(noise)
        r = d._rounding.detach().clone()
        fwd = d(var.value, cfg).detach().clone()
        d._rounding.grad = None
        (d(var.value, cfg) * dy).sum().backward()
        dr = d._rounding.grad.detach().clone()
        d.finalize()
        p = f'c{k}_'
        out.update({p + 'w': w.numpy(), p + 'scale': scale.numpy(), p + 'offset': offset.numpy(), p + 'dy': dy.numpy(),
                    p + 'r0': r0.numpy(), p + 'wfloor': wfloor.numpy(), p + 'r': r.numpy(), p + 'fwd': fwd.numpy(),
                    p + 'dr': dr.numpy(), p + 'final': var.value.detach().numpy()})
    for name, c in check_conditions(out).items(): print(name, c)
    np.savez_compressed(os.path.join(HERE, 'roundtune.npz'), **out)
    print('roundtune.npz', len(CASES), 'cases', os.path.getsize(os.path.join(HERE, 'roundtune.npz')), 'bytes')


if __name__ == '__main__':
    main()
