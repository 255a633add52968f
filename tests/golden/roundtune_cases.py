"""Round-tuning weight cases shared by tests/golden/make_roundtune.py (which records the reference's outputs for them) and the
round-tuning tests, plus the test-side torch restatement of ppq/quantization/algorithm/training.py:490-590 that the tests
compare against.

Each case: name, weight shape, channel axis (None: per tensor), quant_min, quant_max, asymmetric offsets, scale factor.  The
scale is absmax / (qmax - qmin) * 2 times the factor: a factor below 1 pushes the ends of the weight distribution outside
[qmin, qmax], so that the reference's own clamp changes elements at both ends."""
import torch

CASES = [
    ('conv_i8_sym_axis0', (8, 3, 3, 3), 0, -128, 127, False, 1.0),
    ('conv_i4_axis0_odd', (6, 5, 3, 3), 0, -8, 7, False, 1.0),           # 270 elements: n % 4 == 2
    ('conv_u8_asym_axis0', (5, 4, 3, 3), 0, 0, 255, True, 1.0),
    ('conv_i8_per_tensor', (7, 3, 5, 5), None, -128, 127, False, 1.0),    # 525: n % 4 == 1
    ('gemm_i8_2d', (10, 13), 0, -128, 127, False, 1.0),
    ('convtranspose_i4_axis1', (4, 6, 3, 3), 1, -8, 7, False, 1.0),
    ('conv_i4_axis0_clamped', (6, 4, 3, 3), 0, -8, 7, False, 0.45),       # the clamp is active at both ends
    ('gemm_i8_per_tensor_clamped', (9, 11), None, -128, 127, False, 0.6),  # 99: n % 4 == 3
]
NOISE = 0.25                                                              # std of the perturbation of R: crosses .5 for ~1 in 6


def case_tensors(k: int):
    """w, scale, offset, R perturbation, dy of case k (float32, CPU): deterministic."""
    name, shape, axis, qmin, qmax, asym, factor = CASES[k]
    g = torch.Generator().manual_seed(2000 + k)
    w = torch.randn(shape, generator=g) * 0.2
    C = 1 if axis is None else shape[axis]
    absmax = w.abs().amax(dim=tuple(i for i in range(len(shape)) if i != axis)) if axis is not None else w.abs().max().reshape(1)
    scale = (absmax / (qmax - qmin) * 2.0 * factor).float().reshape(C)
    if asym: offset = torch.randint(100, 140, (C,), generator=g).float()
    else: offset = torch.zeros(C)
    noise = torch.randn(shape, generator=g) * NOISE
    dy = torch.randn(shape, generator=g)
    if axis is None: scale, offset = scale.reshape(()), offset.reshape(())
    return w, scale, offset, noise, dy


def _view(t, axis, ndim):
    if axis is None: return t
    return t.view([1 if a != axis else -1 for a in range(ndim)])


def initial_rounding(w, scale, axis):
    """training.py:555-563: (R, the floored weight)."""
    s = _view(scale, axis, w.ndim)
    return (w / s) - (w / s).floor(), (w / s).floor() * s


class _Impl(torch.autograd.Function):
    """training.py:490-527: no rounding of t / s, a hard R > .5, the identity as backward for the weight and for R."""
    @ staticmethod
    def forward(ctx, t, s, o, qmin, qmax, r):
        q = (t / s) + (r > .5) + o
        q = torch.clamp(q, qmin, qmax)
        return (q - o) * s

    @ staticmethod
    def backward(ctx, dy):
        return dy, None, None, None, None, dy


def forward(t, r, scale, offset, axis, qmin, qmax):
    """training.py:580-590 on the floored weight t."""
    return _Impl.apply(t, _view(scale, axis, t.ndim), _view(offset, axis, t.ndim), qmin, qmax, r)


def grad_r(t, r, scale, offset, axis, qmin, qmax, dy):
    """dR of sum(forward * dy) by torch autograd."""
    r = r.detach().clone().requires_grad_(True)
    (forward(t, r, scale, offset, axis, qmin, qmax) * dy).sum().backward()
    return r.grad


def finalize(t, r, scale, axis):
    """training.py:572-574."""
    return t + (r > .5) * _view(scale, axis, t.ndim)
