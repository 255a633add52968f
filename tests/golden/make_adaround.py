"""Record the REFERENCE's AdaRound outputs (ppq/quantization/optim/legacy.py) on CPU for the cases of adaround_cases.py.

Run where the reference is importable (oracle/reference_import.find_reference); no GPU test imports it:

    python tests/golden/make_adaround.py

Writes tests/golden/adaround.npz: per case the inputs (w, scale, offset, V = initiate_rounding + noise, dy) and the
reference's own AdaRoundDelegator outputs -- initiate_rounding, __call__ on V, dV by autograd for sum(out * dy) with the
regulariser off and at the (iteration, max_iter) points of REG_POINTS (gamma = 1), finalize -- and TimeDecay values.
Import shims as in make_golden.py."""
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
from ppq.quantization.optim.legacy import AdaRoundDelegator, TimeDecay  # noqa: E402

assert PPQ_CONFIG.USING_CUDA_KERNEL is False
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from adaround_cases import CASES, GAMMA, REG_POINTS, case_tensors, initiate_rounding  # noqa: E402

P = QuantizationProperty


def config(axis, qmin, qmax, asym, bits):
    pol = P.LINEAR + (P.PER_CHANNEL.value if axis is not None else P.PER_TENSOR.value) \
        + (P.ASYMMETRICAL.value if asym else P.SYMMETRICAL.value)
    cfg = TensorQuantizationConfig(policy=QuantizationPolicy(pol), rounding=RoundingPolicy.ROUND_HALF_EVEN, num_of_bits=bits,
                                   quant_min=qmin, quant_max=qmax, observer_algorithm='minmax', channel_axis=axis)
    cfg.state = QuantizationStates.ACTIVATED
    return cfg


def main():
    out = {}
    for k, (name, shape, axis, qmin, qmax, asym) in enumerate(CASES):
        w, scale, offset, noise, dy = case_tensors(k)
        cfg = config(axis, qmin, qmax, asym, 4 if qmax - qmin < 16 else 8)
        cfg.scale, cfg.offset = scale.clone(), offset.clone()
        var = Variable(name=name, value=w.clone(), is_parameter=True)
        d = AdaRoundDelegator(var=var, config=cfg, steps=REG_POINTS[0][1])
        init = d.rounding.detach().clone()
        assert torch.equal(init, initiate_rounding(w, scale, axis))
        v = (init + noise).detach()
        with torch.no_grad(): d.rounding.copy_(v)
        fwd = d(var.value, cfg).detach().clone()
        grads = []
        for it in [None] + [p[0] for p in REG_POINTS]:
            d.rounding.grad = None
            loss = (d(var.value, cfg) * dy).sum()
            if it is not None: loss = loss + d.regularization_loss(it) * GAMMA
            loss.backward()
            grads.append(d.rounding.grad.detach().clone())
        d.finalize()
        p = f'c{k}_'
        out.update({p + 'w': w.numpy(), p + 'scale': scale.numpy(), p + 'offset': offset.numpy(), p + 'v': v.numpy(),
                    p + 'dy': dy.numpy(), p + 'init': init.numpy(), p + 'fwd': fwd.numpy(), p + 'final': var.value.detach().numpy()})
        for j, g in enumerate(grads): out[p + f'dv{j}'] = g.numpy()
    td = TimeDecay(100)
    ts = np.array([0, 10, 20, 21, 33.5, 50, 77, 99, 100], np.float64)
    out['timedecay_t'] = ts
    out['timedecay_beta'] = np.array([td(t) for t in ts], np.float64)
    np.savez_compressed(os.path.join(HERE, 'adaround.npz'), **out)
    print('adaround.npz', len(CASES), 'cases', os.path.getsize(os.path.join(HERE, 'adaround.npz')), 'bytes')


if __name__ == '__main__':
    main()
