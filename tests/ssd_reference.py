"""NumPy oracle for the three operations of SSD equalization that csrc/ssd.hip computes (ppq_amd/ssd.py; the reference's
ppq/quantization/optim/ssd.py): the two weight ranges of a pair, its four candidate scales and the four candidate parameter
sets.  Float32 throughout, every step one NumPy operation: NumPy's float32 product, quotient and square root are correctly
rounded, which is the contract of the kernels (see ``scales`` on why torch's CPU square root is not the yardstick).  Imports
nothing but NumPy; tests/test_host_ssd.py pins it to every recording of tests/golden/ssd.npz and to ``ppq_amd.ssd.calculate_scale``.

NaN, as the kernels document it (torch's ``max`` / ``min`` / ``clamp`` / ``where`` semantics; NumPy's ``max``, ``min``,
``minimum``, ``clip`` propagate a NaN the same way and ``x < NaN`` is False in both):

* a NaN element makes the range of its channel NaN (``ranges``);
* a NaN range of channel c makes the algorithm-0 scale of channel c NaN, and of no other channel;
* through the cross-channel max, a NaN in the FIRST range or in the ACTIVATION range makes every channel's scale NaN for
  algorithms 1, 2 and 3; a NaN in the LAST range does so for algorithms 2 and 3 (algorithm 1 does not read the last range)."""
import numpy as np

F = np.float32


def channel_max(weight: np.ndarray, axis: int, group: int = 1) -> np.ndarray:
    """max |w| per channel of one endpoint's weight, in the three forms ``equalization.endpoint_layout`` addresses:

    * ``axis == 0``: channel c is row c of ``[C, ...]`` (an upstream Conv, a Gemm stored [out, in] upstream, [in, out] downstream);
    * ``axis == 1`` of a 2-D weight: channel c is column c of ``[rows, C]``;
    * ``axis == 1`` of a Conv weight ``[G * og, ipg, k...]`` (downstream): channel ``g * ipg + i`` -- SSD's natural
      (group, cin_local) order -- is the ``og`` slices ``w[g * og : (g + 1) * og, i]``."""
    a = np.abs(np.asarray(weight, dtype=F))
    if axis == 0: return a.reshape(a.shape[0], -1).max(axis=1)
    assert axis == 1
    if a.ndim == 2:
        assert group == 1
        return a.max(axis=0)
    G, og, ipg = group, a.shape[0] // group, a.shape[1]
    return a.reshape(G, og, ipg, -1).transpose(0, 2, 1, 3).reshape(G * ipg, -1).max(axis=1)


def ranges(first_weight: np.ndarray, last_weight: np.ndarray, group: int = 1, first_axis: int = 0, last_axis: int = 1) -> np.ndarray:
    """prepare_weight_for_equalization (optim/ssd.py:152-210): ``[2, C]`` -- max |w| per output channel of the pair's first
    weight and per input channel of its last one (``group``: the groups of a last Conv).  ``first_axis`` / ``last_axis``: which
    axis of each weight is the pair's channel (``channel_max``)."""
    first = channel_max(first_weight, first_axis)
    last = channel_max(last_weight, last_axis, group)
    assert first.shape == last.shape, (first.shape, last.shape)
    return np.stack([first, last]).astype(F)


def scales(first: np.ndarray, last: np.ndarray, act: np.ndarray, ratio: float) -> np.ndarray:
    """one_step_equalization (optim/ssd.py:288-320), ``[4, C]``, with every step the correctly rounded fp32 operation (numpy's
    division and square root are; torch's CPU square root is not always, see make_equalization.ieee_scale).  A HIP kernel cannot
    (and should not) reproduce a mis-rounded step, so a recorded case that differs from this is refused and re-seeded
    (tests/golden/make_ssd.py)."""
    first, last, act = (np.asarray(v, dtype=F) for v in (first, last, act))
    eps, ratio = F(1e-8), F(ratio)
    with np.errstate(all='ignore'):
        s0 = np.clip(np.sqrt((last / (first + eps)).astype(F)), F(0.1), F(10))
        t1, t2 = F(first.max() * ratio), F(last.max() * ratio)
        f = np.where(first < t1, t1, first).astype(F); l = np.where(last < t2, t2, last).astype(F)
        ks = (f.max() / (f + eps)).astype(F); nks = (l.max() / (l + eps)).astype(F)
        a = np.where(act < F(0.01), F(0.01), act).astype(F)
        as_ = (a.max() / (a + eps)).astype(F)
        s1 = np.minimum(ks, as_)
        t = np.minimum(np.minimum((ks / nks).astype(F), (as_ / nks).astype(F)), F(8))
        s2 = np.clip((t / t.min()).astype(F), F(1), F(2))
        s3 = np.clip(np.sqrt((as_ * np.sqrt((ks / nks).astype(F))).astype(F)), F(1), F(2))
    return np.stack([s0, s1, s2, s3]).astype(F)


def algo2_before_normalisation(first: np.ndarray, last: np.ndarray, act: np.ndarray, ratio: float) -> np.ndarray:
    """min(ks / nks, as / nks, 8) of ``scales``: the vector whose cross-channel MINIMUM normalises algorithm 2 (for tests that
    have to know which channel holds it)."""
    first, last, act = (np.asarray(v, dtype=F) for v in (first, last, act))
    eps, ratio = F(1e-8), F(ratio)
    with np.errstate(all='ignore'):
        t1, t2 = F(first.max() * ratio), F(last.max() * ratio)
        f = np.where(first < t1, t1, first).astype(F); l = np.where(last < t2, t2, last).astype(F)
        ks = (f.max() / (f + eps)).astype(F); nks = (l.max() / (l + eps)).astype(F)
        a = np.where(act < F(0.01), F(0.01), act).astype(F)
        as_ = (a.max() / (a + eps)).astype(F)
        return np.minimum(np.minimum((ks / nks).astype(F), (as_ / nks).astype(F)), F(8))


def scale_tensor(x: np.ndarray, scale: np.ndarray, axis: int, divide: bool = False, group: int = 1) -> np.ndarray:
    """One tensor of write_back (optim/ssd.py:212-262) under one scale ``[C]``: ``x * s`` (upstream: the first weight along its
    channel ``axis``, its bias) or the IEEE quotient ``x / s`` (downstream: the last weight), the channel forms of ``channel_max``."""
    x, scale = np.asarray(x, dtype=F), np.asarray(scale, dtype=F)
    if axis == 1 and x.ndim > 2:
        G, og, ipg = group, x.shape[0] // group, x.shape[1]
        v, s = x.reshape((G, og, ipg) + x.shape[2:]), scale.reshape((G, 1, ipg) + (1,) * (x.ndim - 2))
    else:
        assert group == 1
        v, s = x, scale.reshape([-1 if d == axis else 1 for d in range(x.ndim)])
    with np.errstate(all='ignore'):
        return ((v / s) if divide else (v * s)).astype(F).reshape(x.shape)


def apply(x: np.ndarray, scales: np.ndarray, axis: int, divide: bool = False, group: int = 1) -> np.ndarray:
    """The four candidates ``[4, *x.shape]`` of one tensor under the four rows of ``scales`` ``[4, C]``."""
    return np.stack([scale_tensor(x, s, axis, divide, group) for s in np.asarray(scales, dtype=F)])


def apply_pair(first: dict, last: dict, first_name: str, last_name: str, params: dict, scale: np.ndarray) -> dict:
    """write_back for a pair of the case graphs (tests/golden/ssd_cases.py: ``first`` / ``last`` are the attribute dicts of the
    two operations, parameters are ``<op>_w`` / ``<op>_b``) under ONE scale: {parameter name: candidate}.  The last bias is
    part of a candidate and never changes."""
    got = {first_name + '_w': scale_tensor(params[first_name + '_w'], scale, 0 if 'k' in first or first['transB'] else 1)}
    if first['bias']: got[first_name + '_b'] = scale_tensor(params[first_name + '_b'], scale, 0)
    if 'k' in last: got[last_name + '_w'] = scale_tensor(params[last_name + '_w'], scale, 1, True, last['group'])
    else: got[last_name + '_w'] = scale_tensor(params[last_name + '_w'], scale, 1 if last['transB'] else 0, True)
    if last['bias']: got[last_name + '_b'] = np.asarray(params[last_name + '_b'], dtype=F)
    return got
