"""The oracle of the clipping-search tests: the contract that ppq_amd/csrc/search.hip states for itself, in NumPy, together with the
histograms and the cases the search tests run.  No torch, no GPU, nothing shared with the kernels.

KL (``kl_contract``) restates TorchHistObserver.hist_to_scale_offset (observer/range.py:241-269) with torch_KL_divergence
(measure/statistic.py:12) under the arithmetic the kernel documents: every sum of histogram counts (hist_sum, the tail, each group)
and q_sum are computed exactly and rounded to float32 ONCE; every division and the ``p[r-1] + tail`` add are float32; the divergence
is a float64 dot product with eps = 1e-30.  The reference itself sums float32 tensors in an unspecified order, oracle.kl_search in
NumPy's pairwise order: both are float32 orders of the same sums, and tests/test_host_search.py measures how far they are from this
one.  ``kl_contract_scalar`` is the same contract written bin by bin with Python integers; the host test holds the two bit-equal.

MSE needs no restatement: oracle.mse_candidates + oracle.mse_loss are already the reference's enumeration and float32 loss; this
module adds the reference's selection (``mse_first_minimum``: ``sorted(...)[0]``) and the kernel's cell numbering.

Not a test module."""
import math

import numpy as np

EPS = 1e-30
MSE_INTERVAL = 8                   # OBSERVER_MSE_COMPUTE_INTERVAL
HIST_SCALE = 0.01

# |oracle.kl_search - kl_contract| over every KL case below, measured on the CPU by tests/test_host_search.py (two float32 summation
# orders of the same histograms; no kernel took part).  The bound that tests may use against the oracle's order is FACTOR times the
# measurement: torch's reduction order in the reference is a third float32 order, and orders differ from each other by this much.
ORACLE_ABS_MEASURED = 4.18e-7      # 4.174e-7, at huge-2048-b2
ORACLE_ABS_FACTOR = 4
ORACLE_ABS_BOUND = ORACLE_ABS_FACTOR * ORACLE_ABS_MEASURED

# tol_j = KL_TOL * A_j: unit round-off 2^-53, at most 2^14 terms in any summation order, a few ulp of each log10.  Derived, not measured.
KL_TOL = 2.0 ** -38


# ------------------------------------------------------------------------------------------------------------------------------ KL
def _edited(hist: np.ndarray) -> np.ndarray:
    """range.py:244-245: float32 histogram, first int(bins * .002) bins zeroed, the next one set to 1."""
    assert hist.dtype == np.int32 and hist.ndim == 1
    z = int(hist.size * .002)
    hf = hist.astype(np.float32)
    hf[:z] = 0
    hf[z] = 1
    return hf


def _dot_terms(p: np.ndarray, q: np.ndarray):
    """(divergence, A, every term vanishes identically)."""
    pd, qd = p.astype(np.float64), q.astype(np.float64)
    with np.errstate(all='ignore'):
        lp, lq = np.log10(pd + EPS), np.log10(qd + EPS)
        vanishes = bool(np.all(np.isfinite(qd)) and np.all((pd == 0) | (pd == qd)))
        return float(np.sum(pd * (lp - lq))), float(np.sum(np.abs(pd) * (np.abs(lp) + np.abs(lq)))), vanishes


def kl_contract(hist: np.ndarray, bits: int):
    """(losses float64[ncand], A float64[ncand]); candidate j has bin_range (j + 1) * 2^(bits-1).
    A_j = sum_i |p_i| * (|log10(p_i + eps)| + |log10(q_i + eps)|) scales the admissible float64 error of loss j."""
    return kl_contract_detail(hist, bits)[:2]


def kl_contract_detail(hist: np.ndarray, bits: int):
    """kl_contract plus Z bool[ncand]: every term of candidate j vanishes identically (p_i == 0, or p_i and q_i are the same float32,
    so that log10(p_i + eps) - log10(q_i + eps) is x - x).  Such a loss is 0.0 in every summation order and with every log10; A_j == 0
    (p in {0, 1}, q == p) is the special case where the logarithms vanish as well."""
    bins, Q = hist.size, 1 << (bits - 1)
    assert 2 <= bits and bins >= Q and bins % Q == 0
    hf = _edited(hist)
    h64 = hf.astype(np.float64)                       # integer-valued, every partial sum below 2^53: float64 sums are exact
    hist_sum = np.float32(h64.sum())
    losses, A, Z = [], [], []
    for j in range(bins // Q):
        r, e = (j + 1) * Q, j + 1
        tail = np.float32(h64[r:].sum())
        g = hf[:r].reshape(Q, e)
        positive = g > 0
        cnt = positive.sum(axis=1)
        with np.errstate(all='ignore'):
            qg = g.astype(np.float64).sum(axis=1).astype(np.float32) / np.where(cnt == 0, 1, cnt).astype(np.float32)
            # q_sum = sum over the positive bins of their group's value: cnt copies of qg, a float32 times a small integer is exact in
            # float64, and fsum adds those exactly
            q_sum = np.float32(math.fsum((qg.astype(np.float64) * cnt).tolist()))
            p = hf[:r].copy()
            p[r - 1] = p[r - 1] + tail
            p = p / hist_sum
            q = np.where(positive, qg[:, None], np.float32(0)).reshape(-1) / q_sum
        assert p.dtype == np.float32 and q.dtype == np.float32
        loss, a, vanishes = _dot_terms(p, q)
        losses.append(loss); A.append(a); Z.append(vanishes)
    return np.array(losses, np.float64), np.array(A, np.float64), np.array(Z, bool)


def kl_contract_scalar(hist: np.ndarray, bits: int) -> np.ndarray:
    """The same contract bin by bin: Python integers for the counts, one np.float32() per documented rounding.  Slow; small bins only."""
    bins, Q = hist.size, 1 << (bits - 1)
    z = int(bins * .002)
    h = [0 if i < z else (1 if i == z else int(np.float32(int(v)))) for i, v in enumerate(hist)]      # float32(count), as an integer
    f32 = np.float32
    hist_sum = f32(sum(h))
    out = []
    with np.errstate(all='ignore'):
        for j in range(bins // Q):
            r, e = (j + 1) * Q, j + 1
            tail = f32(sum(h[r:]))
            qg, cnts = [], []
            for g in range(Q):
                grp = h[g * e:(g + 1) * e]
                cnt = sum(1 for v in grp if v > 0)
                qg.append(f32(sum(grp)) / f32(cnt if cnt else 1)); cnts.append(cnt)
            q_sum = f32(math.fsum(float(v) for g in range(Q) for v in [qg[g]] * cnts[g]))
            ps, qs = [], []
            for i in range(r):
                p = f32(h[i])
                if i == r - 1: p = p + tail
                ps.append(p / hist_sum)
                qs.append((qg[i // e] if h[i] > 0 else f32(0)) / q_sum)
            out.append(_dot_terms(np.array(ps, np.float32), np.array(qs, np.float32))[0])
    return np.array(out, np.float64)


def pick(losses, Q: int) -> int:
    """The host rule (range.py:271; ppq_amd/observer.py): a stable sort of the candidate records, first one wins -- with whatever
    Python's sort makes of NaN keys."""
    records = [{'kl': float(l), 'bin_range': (j + 1) * Q} for j, l in enumerate(losses)]
    return sorted(records, key=lambda x: x['kl'])[0]['bin_range']


def kl_near_minimum(losses: np.ndarray, A: np.ndarray) -> np.ndarray:
    """Indices of the finite candidates that a float64 evaluation in another order could rank first: those within 2 * tol of the
    smallest finite loss (tol = KL_TOL * A, the larger of the two candidates')."""
    finite = np.flatnonzero(np.isfinite(losses))
    if finite.size == 0: return finite
    m = finite[np.argmin(losses[finite])]
    tol = KL_TOL * np.maximum(A[finite], A[m])
    return finite[losses[finite] - losses[m] <= 2 * tol]


def kl_ambiguous(losses: np.ndarray, A: np.ndarray, Z: np.ndarray) -> bool:
    """More than one candidate near the minimum -- unless they are all exact zeros whose terms vanish identically (Z), which every
    order evaluates to the same 0.0: there the first one must win."""
    near = kl_near_minimum(losses, A)
    if near.size <= 1: return False
    return not bool(np.all(losses[near] == 0.0) and np.all(Z[near]))


# kl_case_id()s whose arg-min another summation order may move (kl_ambiguous); tests/test_host_search.py holds this list to what the
# references say.  With the seeds below there is none.
KL_AMBIGUOUS = ()

KL_FAMILIES = ('halfnormal', 'relu_hot', 'sparse', 'spike', 'ends', 'zero', 'flat', 'huge', 'longtail')
MSE_FAMILIES = ('normal', 'relu_hot', 'sparse', 'spike', 'ends', 'zero', 'flat', 'huge')
INT32_MAX = 2 ** 31 - 1
SEED = 2026


def histogram(family: str, bins: int, mse: bool = False) -> np.ndarray:
    """One int32 histogram; the random families are seeded by (SEED, family, bins)."""
    names = KL_FAMILIES + MSE_FAMILIES
    rng = np.random.default_rng([SEED, names.index(family), bins])
    i = np.arange(bins)
    h = np.zeros(bins, np.int64)
    if family == 'halfnormal':
        h = np.histogram(np.abs(rng.standard_normal(200000)), bins=bins, range=(0, 5))[0]
    elif family == 'normal':
        h = np.histogram(rng.standard_normal(200000), bins=bins, range=(-5, 5))[0]
    elif family == 'relu_hot':
        h = np.histogram(np.abs(rng.standard_normal(100000)), bins=bins, range=(0, 6))[0].astype(np.int64)
        h[0] += 100000
    elif family == 'sparse':
        k = rng.choice(bins, max(2, bins // 18), replace=False)
        h[k] = rng.integers(1, 1000, k.size)
    elif family == 'spike':
        h[bins // 3] = 12345
    elif family == 'ends':
        h[0], h[-1] = 777, 333
    elif family == 'zero':
        pass
    elif family == 'flat':
        h[:] = 7
    elif family == 'huge':
        h = np.full(bins, INT32_MAX, np.int64) if mse else (np.exp(-i / (bins / 6.0)) * INT32_MAX).astype(np.int64)
    elif family == 'longtail':                        # tests/golden/make_golden.py:228, scaled to `bins`
        h = (np.exp(-i / (bins * 90.0 / 2048.0)) * 50000).astype(np.int64)
        h[int(bins * 1500 / 2048):] = 0
        h[-1] = 3
    else:
        raise KeyError(family)
    assert h.min() >= 0 and h.max() <= INT32_MAX
    return h.astype(np.int32)


KL_CASES = [(128, b) for b in range(2, 9)] + [(192, 4), (192, 7), (1000, 4), (1024, 11), (2048, 2), (2048, 8), (2048, 11), (4096, 8),
                                              (16384, 8), (16384, 11)]


def kl_case_id(bins: int, bits: int, family: str) -> str:
    return f'{family}-{bins}-b{bits}'


# ----------------------------------------------------------------------------------------------------------------------------- MSE
# (bins, quant_min, quant_max, families, modes): modes 's' symmetric, 'a' asymmetric
MSE_CASES = [
    (64, 0, 15, MSE_FAMILIES, 'sa'),                  # bins < 256: the strided loads run less than once per thread
    (96, -8, 7, MSE_FAMILIES, 'sa'),
    (256, 0, 255, MSE_FAMILIES, 'sa'),                # S == 1
    (300, -127, 127, MSE_FAMILIES, 'sa'),             # 255 levels, bins no multiple of 256, S == 1
    (512, 0, 15, MSE_FAMILIES, 'sa'),
    (520, 0, 3, MSE_FAMILIES, 'sa'),                  # S == 130
    (64, -128, 127, MSE_FAMILIES, 'sa'),              # fewer bins than levels: the min-max candidate alone
    (2048, 0, 15, ('normal', 'spike'), 'a'),          # 32769 cells: more than 64 workgroups x 256 lanes, the grid-stride path
    (16384, 0, 255, ('normal',), 's'),                # the largest accepted histogram
]


def mse_min_values(bins: int):
    """Asymmetric min_value settings: -0.37 k (several starts valid; for k = 8, start 296 sits on the `> 0` boundary of range.py:477),
    0.0 (start 0 alone) and +0.01 (no start: the min-max candidate alone)."""
    k = 8 if bins >= 300 else 1
    return (-0.37 * k, 0.0, 0.01)


def mse_rows(bins: int, families, symmetric: bool):
    """The rows of one batched launch: (name, hist int32[bins], hist_scale, min_value)."""
    mins = (0.0,) if symmetric else mse_min_values(bins)
    return [(f'{fam}@{mn:+.2f}', histogram(fam, bins, mse=True), HIST_SCALE, mn) for fam in families for mn in mins]


def mse_cell(start: int, step: int, index: int, bins: int, levels: int) -> int:
    """The kernel's cell number of a candidate: 0 for the min-max candidate (enumeration index 0), else 1 + (start // 8) * S + step - 1."""
    if index == 0: return 0
    return 1 + (start // MSE_INTERVAL) * (bins // levels) + (step - 1)


def mse_first_minimum(O, hist: np.ndarray, hist_scale: float, min_value: float, quant_min: int, quant_max: int, symmetric: bool):
    """range.py:487 / :512 on the oracle's candidates and float32 loss: ``sorted(losses, key=mse)[0]``.
    Returns (start, end, step, cell, losses float64[n], cells int[n]) with the losses in enumeration order."""
    bins, levels = hist.size, quant_max - quant_min + 1
    cands = O.mse_candidates(bins, hist_scale, min_value, quant_min, quant_max, symmetric)
    h64 = np.ascontiguousarray(hist, dtype=np.int64)
    records = [{'mse': O.mse_loss(h64, s, st, e), 'start': s, 'end': e, 'step': st, 'index': i} for i, (s, st, e) in enumerate(cands)]
    best = sorted(records, key=lambda x: x['mse'])[0]
    cells = np.array([mse_cell(r['start'], r['step'], r['index'], bins, levels) for r in records])
    return (best['start'], best['end'], best['step'], mse_cell(best['start'], best['step'], best['index'], bins, levels),
            np.array([r['mse'] for r in records], np.float64), cells)
