"""The case graph of the statistical reports, shared by tests/golden/make_statistics.py (which records what the reference's
``statistical_analyse`` and ``parameter_analyse`` say about it on the CPU) and the statistics tests, and the float64 side of
every check: the same formulas evaluated in double on the same float32 series, and the bounds that follow from the arithmetic
of ppq_amd/csrc/stats.hip.

The graph: three Conv + Relu with biases and a MaxPool (passive: not analysed) on 3 batches of [4, 3, 16, 16]; TensorRT-style
INT8 ('kl' activations, per-channel weights, FP32 bias -- so a bias carries no quantisation noise at all: its noise series is
constant, its skewness and kurtosis NaN).  Operations as data in the style of ssd_cases.py: parameters ``<op>_w`` / ``<op>_b``,
outputs ``<op>_out``."""
import numpy as np
import torch

SEED = 7301                            # make_statistics.py refuses a seed that misses one of its conditions
HIST_BINS = 2048                       # of the calibration (the report's own histogram has BINS)
BATCHES = 3
STEPS = 8                              # more steps than batches: every batch is used, n = BATCHES * FETCHS
FETCHS = 1024
BINS = 32
INPUT = (4, 3, 16, 16)
OPS = [('Conv', 'c1', ['input'], dict(cin=3, cout=8, k=3)), ('Relu', 'r1', ['c1_out'], {}),
       ('MaxPool', 'p1', ['r1_out'], dict(k=2)),
       ('Conv', 'c2', ['p1_out'], dict(cin=8, cout=12, k=3)), ('Relu', 'r2', ['c2_out'], {}),
       ('Conv', 'c3', ['r2_out'], dict(cin=12, cout=6, k=1)), ('Relu', 'r3', ['c3_out'], {})]
OUTPUTS = ['r3_out']
KINDS = ('Noise', 'Quantized', 'Float')
SCALARS = ('Mean', 'Std', 'Skewness', 'Kurtosis', 'Max', 'Min')
KEYS = ['Op name', 'Op type', 'Is parameter', 'Is input', 'Is output', 'Variable name', 'Noise:Signal Power Ratio'] + \
       [f'{kind} {field}' for kind in KINDS for field in ('Mean', 'Std', 'Skewness', 'Kurtosis', 'Hist', 'Max', 'Min')]
EDGE_WINDOW = 2.0 ** -16               # three fp32 roundings at positions below 32 stay under 32 * 3 * 2^-24 < 2^-17
EDGE_CAP = 0.02


def case_parameters(seed: int = SEED) -> dict:
    g = torch.Generator().manual_seed(seed)
    out = {}
    for kind, name, _, a in OPS:
        if kind != 'Conv': continue
        fan_in = a['cin'] * a['k'] * a['k']
        out[name + '_w'] = (torch.randn(a['cout'], a['cin'], a['k'], a['k'], generator=g) * (2.0 / fan_in) ** 0.5).float()
        out[name + '_b'] = (torch.randn(a['cout'], generator=g) * 0.1).float()
    return out


def case_batches(seed: int = SEED) -> list:
    g = torch.Generator().manual_seed(seed + 1)
    return [torch.randn(INPUT, generator=g) for _ in range(BATCHES)]


def harness_graph(parameters: dict = None, quantize: bool = True):
    """The case as a ``ppq_amd.harness`` graph with CPU parameters."""
    from ppq_amd import harness
    parameters = case_parameters() if parameters is None else parameters
    g = harness.BaseGraph('statistics_case')
    made = {'input': g.create_variable('input')}
    g.inputs['input'] = made['input']
    for kind, name, inputs, a in OPS:
        ins, attrs = [made[n] for n in inputs], {}
        if kind == 'Conv':
            ins += [g.create_variable(name + '_w', parameters[name + '_w'].clone(), True),
                    g.create_variable(name + '_b', parameters[name + '_b'].clone(), True)]
            attrs = {'strides': 1, 'pads': a['k'] // 2, 'group': 1}
        elif kind == 'MaxPool': attrs = {'kernel_shape': a['k'], 'strides': a['k'], 'pads': 0}
        made[name + '_out'] = g.create_operation(kind, name, ins, attrs)
    for n in OUTPUTS: g.outputs[n] = made[n]
    if quantize: harness.quantize_graph(g, 'kl', hist_bins=HIST_BINS)
    return g


# ---- the float64 side ------------------------------------------------------------------------------------------------
def float64_series(x: np.ndarray) -> dict:
    """Mean, Std (n - 1), Skewness, Kurtosis, Max, Min of one float32 series, every step in float64 (the formulas of
    analyse/graphwise.py:227-293).  A constant series has std 0: skewness and kurtosis are NaN, as 0 / 0 is."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    mean = x.sum() / n
    with np.errstate(all='ignore'):
        std = np.sqrt(((x - mean) ** 2).sum() / (n - 1)) if n > 1 else np.nan
        t = (x - mean) / std
        return {'Mean': mean, 'Std': std, 'Skewness': (t ** 3).sum() / n, 'Kurtosis': (t ** 4).sum() / n - 3.0, 'Max': x.max(), 'Min': x.min()}


def float64_snr(qt: np.ndarray, fp: np.ndarray) -> float:
    """torch_snr_error(qt, fp) in float64 on the float32 noise series fl32(qt - fp)."""
    er = (np.asarray(qt, np.float32) - np.asarray(fp, np.float32)).astype(np.float64)
    return float((er ** 2).sum() / ((np.asarray(fp, np.float64) ** 2).sum() + 1e-7))


def noise_of(qt: np.ndarray, fp: np.ndarray) -> np.ndarray:
    return np.asarray(qt, np.float32) - np.asarray(fp, np.float32)


def ulp32(v) -> float:
    """The spacing of float32 at |v| (of the smallest normal number below it)."""
    v = abs(float(v))
    return float(np.spacing(np.float32(max(v, 2.0 ** -126))))


def moment_bound(value64: float, n: int, scale: float = None) -> float:
    """mean_f / std_f against the float64 value: one float32 ulp of the rounded value, on top of the double accumulation
    error n * 2^-52 relative to the sum of the terms' magnitudes -- for the std (terms >= 0) the value itself, for the mean
    ``scale`` = mean |x|."""
    return ulp32(np.float32(value64)) + n * 2.0 ** -52 * (abs(value64) if scale is None else scale)


def shape_bounds(x: np.ndarray) -> tuple:
    """(skewness bound, kurtosis bound) of the kernel's values against float64_series for a series with std > 0.

    t = fl32(fl32(x - mean_f) / std_f), t2 = fl32(t t), t3 = fl32(t2 t), t4 = fl32(t2 t2) carry u = 2^-24 per rounding, and
    std_f two more (its own rounding and the ulp moment_bound allows): t is off by <= 4u relative, t3 by <= (3 * 4 + 2) u,
    t4 by <= (4 * 4 + 3) u -- plus the shift of mean_f, |dm| <= 1.5 ulp32(mean) (rounding and the allowed ulp), which moves t
    by dm / std: t^3 by 3 t^2 dm / std, t^4 by 4 |t|^3 dm / std.  The double sums add n * 2^-52 relative, the results one
    float32 rounding each and the kurtosis another for its `- 3`.  First order, so everything is doubled."""
    x = np.asarray(x, dtype=np.float64)
    n, u = x.size, 2.0 ** -24
    s = float64_series(x)
    t = np.abs((x - s['Mean']) / s['Std'])
    m2, m3, m4 = (t ** 2).sum() / n, (t ** 3).sum() / n, (t ** 4).sum() / n
    dm = 1.5 * ulp32(np.float32(s['Mean'])) / s['Std']
    skew = 2 * (14 * u * m3 + 3 * m2 * dm + n * 2.0 ** -52 * m3 + u * abs(s['Skewness']))
    kurt = 2 * (19 * u * m4 + 4 * m3 * dm + n * 2.0 ** -52 * m4 + u * (m4 + abs(s['Kurtosis'])))
    return skew, kurt


def snr_bound(value64: float, n: int) -> float:
    """(float)noise / ((float)signal + 1e-7f): the fp32 squares (u each), the two roundings to float, the sum and the quotient."""
    return (6 * 2.0 ** -24 + n * 2.0 ** -51) * abs(value64) + 1e-45


def histogram_range(x: np.ndarray) -> tuple:
    """(lo, hi) of torch.histc(x, min=x.min(), max=x.max()): equal ends are moved one apart to each side."""
    lo, hi = np.float32(np.min(x)), np.float32(np.max(x))
    if lo == hi: lo, hi = np.float32(lo - np.float32(1)), np.float32(hi + np.float32(1))
    return lo, hi


def edge_samples(x: np.ndarray, bins: int = BINS) -> int:
    """How many samples sit within EDGE_WINDOW of an interior bin edge, by their float64 position (x - lo) * bins / (hi - lo):
    only those can land in another bin under another evaluation order of the same position rule."""
    lo, hi = histogram_range(x)
    pos = (np.asarray(x, np.float64) - float(lo)) * bins / (float(hi) - float(lo))
    near = np.abs(pos - np.rint(pos)) <= EDGE_WINDOW
    return int((near & (np.rint(pos) >= 1) & (np.rint(pos) <= bins - 1)).sum())


def position_bins(x: torch.Tensor, bins: int) -> torch.Tensor:
    """The position rule of csrc/stats.hip with elementwise torch operations (each one fp32 operation), on x's device:
    pos = ((x - lo) * bins) / (hi - lo), bin = min((int)pos, bins - 1).  Returns the int64 counts [bins]."""
    lo, hi = x.min(), x.max()
    if bool(lo == hi): lo, hi = lo - 1.0, hi + 1.0
    pos = quotient32((x - lo) * float(bins), hi - lo)
    return torch.bincount(pos.to(torch.int64).clamp_(0, bins - 1), minlength=bins)


def quotient32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The correctly rounded float32 quotient a / b (53 >= 2 * 24 + 2: the double quotient of two floats rounds to it),
    whatever division the device's elementwise kernel uses."""
    return (a.double() / b.double()).float()
