"""Seeded inputs of the analysis tests (tests/test_host_analyse.py, tests/test_gpu_analyse.py) and of make_analyse.py, which
records what the REFERENCE computes for them into analyse.npz.  Inputs are regenerated from here, never stored."""
import torch

# (num_of_fetches, num_of_elements, seed): fewer elements than fetches, the ResNet-50 activation sizes, the int32 limit
INDEXER_CASES = [(4096, 7, 10086), (4096, 4096, 10086), (4096, 150528, 10086), (4096, 802816, 10086),
                 (512, 2 ** 31 - 1, 10086), (64, 5, 0x20211230), (100, 1000, 0x20211230)]

# name -> shape; rows of <= 1024 elements, of one workgroup, split rows, a row length that is no multiple of 4, 1-D, 4-D
MEASURE_CASES = [('tiny', (4, 37)), ('wave', (5, 1000)), ('block', (3, 4096)), ('split', (2, 100352)), ('odd', (3, 8195)),
                 ('one_dim', (257,)), ('four_dim', (2, 3, 8, 8))]
METHODS = ('snr', 'mse', 'cosine')
REDUCTIONS = ('mean', 'sum', 'none')


def measure_tensors(k: int):
    """(y_pred, y_real) of MEASURE_CASES[k]: per-row signal power far above 1, noise of a twentieth of the signal."""
    gen = torch.Generator().manual_seed(1000 + k)
    shape = MEASURE_CASES[k][1]
    real = torch.randn(shape, generator=gen) * 1.5 + 0.25
    pred = real + torch.randn(shape, generator=gen) * 0.05
    return pred, real


RECORDER_BATCHES = (4, 1, 7, 3)                   # uneven batch sizes of one recorded sequence
RECORDER_ROW = 4096


def recorder_tensors(i: int):
    gen = torch.Generator().manual_seed(2000 + i)
    shape = (RECORDER_BATCHES[i], RECORDER_ROW)
    real = torch.randn(shape, generator=gen) + 0.5
    pred = real + torch.randn(shape, generator=gen) * (0.02 * (i + 1))
    return pred, real


# MeasurePrinter: (name, data, constructor arguments)
PRINTER_CASES = [
    ('percent_large_first', {'conv_1': 0.0123, 'conv_22': 0.5, 'fc': 0.0004, 'a_rather_long_layer_name': 0.25},
     dict(measure='NOISE:SIGNAL POWER RATIO', order='large_to_small', percentage=True)),
    ('plain_small_first', {'conv_1': 1.5, 'conv_22': 0.031, 'fc': 12.25},
     dict(measure='MSE LOSS(UNSCALED)', order='small_to_large', percentage=False)),
    ('top_two', {'x': 0.3, 'y': 0.1, 'z': 0.2}, dict(measure='COSINE SIMILARITY', order='large_to_small', percentage=True, k=2)),
    ('nan_row', {'good': 0.25, 'bad': float('nan'), 'other': 0.5}, dict(measure='MEASUREMENT', order=None, percentage=False)),
]


# ---- the tolerance of every comparison against the reference's recorded fp32 results ----------------------------------------
# The reference sums `count` fp32 terms in fp32, in an order torch does not specify: its own noise, signal and pp are known to
# gamma = (count - 1) * 2^-24 relative, its pr to gamma * sqrt(pp * signal) absolute.  Through the three formulas (first order
# in the numerator, 1 / (1 - gamma) for the denominator):
#   snr = noise / (signal + 1e-7):             |snr| * 2 gamma / (1 - gamma)
#   mse = noise / count:                       |mse| * gamma / (1 - gamma)
#   cosine = pr / (sqrt(pp) * sqrt(signal)):   gamma + |cos| * gamma / (1 - gamma)
# plus 2 fp32 ulps of the value (of 1.0 for the cosine) for the last operations.  A reduction over `rows` per-row values is one
# more fp32 sum of the reference: (rows - 1) * 2^-24 of the sum of their magnitudes ('sum'), divided by rows ('mean').
import numpy as np  # noqa: E402


def measure_bound(method: str, count: int, value) -> np.ndarray:
    """Absolute tolerance for the per-row measure(s) `value` (the reference's) of rows of `count` elements."""
    value = np.abs(np.asarray(value, dtype=np.float64))
    gamma = (count - 1) * 2.0 ** -24
    assert gamma < 0.5
    if method == 'cosine': return gamma + value * gamma / (1 - gamma) + 2 * 2.0 ** -23
    ulp = np.spacing(value.astype(np.float32)).astype(np.float64)
    return value * (2 if method == 'snr' else 1) * gamma / (1 - gamma) + 2 * ulp


def reduced_bound(method: str, count: int, rows, reduction: str) -> float:
    """Absolute tolerance for torch.mean / torch.sum of the reference's per-row values `rows`."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1)
    total = measure_bound(method, count, rows).sum() + (len(rows) - 1) * 2.0 ** -24 * np.abs(rows).sum()
    total += 2 * float(np.spacing(np.float32(np.abs(rows).sum())))
    return float(total / len(rows) if reduction == 'mean' else total)


def analysis_bound(method: str, count: int, rows: int, value: float) -> float:
    """Absolute tolerance for one result of an analysis: a batch-size weighted mean (in double) of per-batch fp32 means over
    `rows` per-row measures of `count` elements each.  The per-row bound above is affine in the row's magnitude, whose mean is
    |value| for the non-negative snr and mse and at most 1 for the cosine; ulp(v) <= 2^-23 |v| replaces the per-row ulps; the
    fp32 mean over the rows adds (rows - 1) * 2^-24 for its sum and one rounding for its division."""
    gamma = (count - 1) * 2.0 ** -24
    assert gamma < 0.5
    mag = 1.0 if method == 'cosine' else abs(float(value))
    part = {'snr': mag * 2 * gamma / (1 - gamma), 'mse': mag * gamma / (1 - gamma), 'cosine': gamma + mag * gamma / (1 - gamma)}[method]
    return part + 2 * 2.0 ** -23 * mag + ((rows - 1) * 2.0 ** -24 + 2.0 ** -23) * mag + 1e-12 * mag
