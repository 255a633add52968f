"""AdaRound weight cases shared by tests/golden/make_adaround.py (which records the reference's outputs for them) and the
AdaRound tests, plus the test-side torch restatement of legacy.py:55-64 / :90-132 that the tests compare against.

Each case: name, weight shape, channel axis (None: per tensor), quant_min, quant_max, asymmetric offsets."""
import numpy as np
import torch

CASES = [
    ('conv_i8_sym_axis0', (8, 3, 3, 3), 0, -128, 127, False),
    ('conv_i4_axis0_odd', (6, 5, 3, 3), 0, -8, 7, False),            # 270 elements: n % 4 == 2
    ('conv_u8_asym_axis0', (5, 4, 3, 3), 0, 0, 255, True),
    ('conv_i8_per_tensor', (7, 3, 5, 5), None, -128, 127, False),     # 525: n % 4 == 1
    ('gemm_i8_2d', (10, 13), 0, -128, 127, False),
    ('convtranspose_i4_axis1', (4, 6, 3, 3), 1, -8, 7, False),
]
REG_POINTS = [(20, 100), (50, 100), (99, 100)]       # (iteration, max_iter): beta = 20 at the end of warm-up, mid, near the end
GAMMA = 1.0


def case_tensors(k: int):
    """w, scale, offset, V perturbation, dy of case k (float32, CPU): deterministic."""
    name, shape, axis, qmin, qmax, asym = CASES[k]
    g = torch.Generator().manual_seed(1000 + k)
    w = torch.randn(shape, generator=g) * 0.2
    C = 1 if axis is None else shape[axis]
    absmax = w.abs().amax(dim=tuple(i for i in range(len(shape)) if i != axis)) if axis is not None else w.abs().max().reshape(1)
    scale = (absmax / (qmax - qmin) * 2.0).float().reshape(C)
    if asym: offset = torch.randint(100, 140, (C,), generator=g).float()
    else: offset = torch.zeros(C)
    noise = torch.randn(shape, generator=g) * 1.5
    dy = torch.randn(shape, generator=g)
    if axis is None: scale, offset = scale.reshape(()), offset.reshape(())
    return w, scale, offset, noise, dy


def _view(t, axis, ndim):
    if axis is None: return t
    return t.view([1 if a != axis else -1 for a in range(ndim)])


def initiate_rounding(w, scale, axis, zeta=1.1, gamma=-0.1):
    """legacy.py:90-105."""
    s = _view(scale, axis, w.ndim)
    r = (w / s) - (w / s).floor()
    r = - torch.log((zeta - gamma) / (r - gamma) - 1)
    return torch.zeros_like(r).copy_(r)


def rectified_sigmoid(v, zeta=1.1, gamma=-0.1):
    """legacy.py:55-56."""
    return ((zeta - gamma) * torch.sigmoid(v) + gamma).clamp(0, 1)


def forward(w, v, scale, offset, axis, qmin, qmax):
    """legacy.py:122-132."""
    s, o = _view(scale, axis, w.ndim), _view(offset, axis, w.ndim)
    t = (w / s).floor() + rectified_sigmoid(v)
    t = torch.clamp(t + o, qmin, qmax)
    return (t - o) * s


def reg_loss(v, it, max_iter, alpha=0.01, warm_ratio=0.2, beta_start=20, beta_end=2):
    """legacy.py:58-64 with TimeDecay (:22-33)."""
    if it < max_iter * warm_ratio: return 0
    start = warm_ratio * max_iter
    rel_t = (it - start) / (max_iter - start)
    beta = beta_end + 0.5 * (beta_start - beta_end) * (1 + np.cos(rel_t * np.pi))
    return alpha * (1 - torch.pow((rectified_sigmoid(v) - 0.5).abs() * 2, beta)).sum()


def grad_v(w, v, scale, offset, axis, qmin, qmax, dy, it=None, max_iter=None, gamma=GAMMA):
    """dV of sum(forward * dy) [+ reg_loss * gamma] by torch autograd."""
    v = v.detach().clone().requires_grad_(True)
    loss = (forward(w, v, scale, offset, axis, qmin, qmax) * dy).sum()
    if it is not None: loss = loss + reg_loss(v, it, max_iter) * gamma
    loss.backward()
    return v.grad


def finalize(w, v, scale, offset, axis, qmin, qmax):
    """legacy.py:107-116."""
    s, o = _view(scale, axis, w.ndim), _view(offset, axis, w.ndim)
    weight = (w / s).floor() + (v >= 0).float()
    weight = torch.clamp(weight + o, qmin, qmax)
    return (weight - o) * s
