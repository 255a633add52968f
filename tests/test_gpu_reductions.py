"""The float reductions of the hot path -- the LSQ scale gradients (LinearQuantize_T_B / _C_B / _C_B_Multi, the split
_T_B_Main + LSQ_Finish_Multi), the FP8 scale gradient (FloatingQuantize_T_B / _C_B), the rounding loss and the FP8
scale-search errors -- against a float64 restatement, on every size-dependent launch branch.

Two kinds of check:

1. **float64 reference with a derived bound.**  Each helper below forms the reference's per-element terms exactly as far
   as the clipping decision goes (mask from the correctly rounded float32 quotient, the rounding policy, the offset
   rounded as the kernel rounds it) and sums them in float64.  The kernel result must lie within

       |got - ref| <= gamma(m + d + e) * sum |term_i| * factor,      gamma(k) = k u / (1 - k u),  u = 2^-24

   Derivation (standard forward error analysis of a summation tree, Higham, *Accuracy and Stability of Numerical
   Algorithms*, 2nd ed., sec. 4.2): every float32 addition, product or quotient is correctly rounded, so it contributes
   a relative error of at most u to the value it produces.  A term t_i computed with e roundings carries
   (1 + d_i), |d_i| <= gamma(e); it then passes through at most m - 1 float32 additions inside one lane (the lane's
   running sum: m terms, the first added to an exact 0), then through the d levels of everything after the lane: the
   wave butterfly (6), the cross-wave step, the per-partial product with the factor, the float atomics that add the
   partials of one output in unspecified order (one level per partial that can reach the same address), and the final
   roundings.  A term that passes through k rounded operations ends as t_i * prod(1 + delta), |prod - 1| <= gamma(k),
   so the total error is at most gamma(m + d + e) * sum |t_i| * factor.  m and d are read off the launch geometry of
   the launcher (written out at each helper that computes them).  A double accumulation (lsq_finish*,
   fq_float_bwd_finish_kernel) adds at most count * 2^-53 relative, which is below one u for every count here: it is
   counted as one level.  Where the whole sum is double (float_scale_search_kernel) the same argument holds with
   u = 2^-53 and exact terms.

   e (per-term roundings): LSQ inside term (q - v) * dy * RN(1/s): 3 roundings + the reciprocal = 4; the clipped term
   (qmax - o) * dy: 1.  FP8 inside term (q - v) * inv_s * dy: 4; clipped cmax * dy * inv_s: 3.  Rounding loss
   |dq - v|: 1.  e = 4 is used throughout the gradient checks.

   grad_x is compared bit for bit with where(mask, dy, 0), at every size.

2. **Boundary sentinels.**  dy = 0 everywhere except at K <= 8 chosen positions, where x lies far outside the clip range
   and dy is a distinct power of 4.  Every term is then 0 or (qmax - o) * 4^k (resp. (qmin - o) * 4^k), the sum is an
   integer of fewer than 24 significant bits -- exact in float32 in any order -- and the only rounding is the one the
   kernel applies to each partial that holds a sentinel (the product with the factor, the float atomic that adds it).
   So the result is within 2 ulp per such partial of float32(sum * factor), while a dropped, doubled or misrouted
   sentinel moves it by at least the smallest weight, >= 124 * factor, i.e. many thousand ulp.  The positions are the
   ones that go wrong: first / last element, the 1-3 element scalar tail, tile / chunk / workgroup edges +-1, the
   second tile of a workgroup that walks several, partials past index 8192, channel edges, the last of > 8192
   channels, unaligned views.

The helpers restate the reference (ppq/csrc/cuda/*.cu; line numbers cited at each) and are checked on the CPU against
oracle/ppq_oracle.c by an unmarked test, so the CPU suite runs them too.
"""
import math
import sys

import numpy as np
import pytest
import torch

from oracle import fp8_integer as F

DEV = 'cuda'
U32 = 2.0 ** -24
U64 = 2.0 ** -53
KBLOCK = 256
I32_MIN, I32_MAX = -2147483648.0, 2147483647.0


def gamma(k: int, u: float = U32) -> float:
    return k * u / (1.0 - k * u)


# --------------------------------------------------------------------------------------------- float64 helpers
def _f32(v, like: torch.Tensor) -> torch.Tensor:
    return torch.as_tensor(v, dtype=torch.float32, device=like.device)


def quotient32(x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The correctly rounded float32 quotient x / s (53 >= 2 * 24 + 2: the double quotient rounds to it)."""
    return (x.double() / s.double()).float()


def round_policy(q32: torch.Tensor, rounding: int) -> torch.Tensor:
    """_round2int (common.cuh:88-114) of float32 values, saturated to int32, as float64 integers."""
    q = q32.double()
    up, down = torch.floor(q + 0.5), torch.ceil(q - 0.5)
    if rounding == 0: r = torch.round(q)                               # nearbyintf: half to even
    elif rounding == 1: r = up
    elif rounding == 2: r = down
    elif rounding == 3: r = torch.where(q > 0, down, up)
    elif rounding == 4: r = torch.where(q > 0, up, down)
    elif rounding == 6: r = torch.ceil(q)
    elif rounding == 7: r = torch.floor(q)
    else: r = torch.sign(q) * torch.floor(q.abs() + 0.5)               # roundf: half away from zero
    return r.clamp(I32_MIN, I32_MAX)


def _round_offset(o: torch.Tensor) -> torch.Tensor:
    """std::round(offset) (linear.cu:253), kept as float32."""
    o = o.double()
    return (torch.sign(o) * torch.floor(o.abs() + 0.5)).float()


def lsq_terms(x, dy, s, o_raw, qmin: int, qmax: int, rounding: int):
    """Per-element terms of QuantizeTensor_LT_B / _LC_B in float64 and the pass-through mask.
    linear.cu:255-274 (per tensor; term (q - v) * dy / s) and linear.cu:352-372 (per channel; term (q - v) / s * dy).
    s and o_raw are float32 and broadcast against x."""
    o = _round_offset(o_raw)
    r = round_policy(quotient32(x, s), rounding)
    t = r.float() + o                                                   # int + float -> float (linear.cu:259)
    qt = t.double().clamp(I32_MIN, I32_MAX).trunc()                    # -> int
    hi, lo = qt > qmax, qt < qmin
    oi = o.double().clamp(I32_MIN, I32_MAX).trunc()
    q = (qt - oi).float() * s                                           # DequantizeScalar<int, float, int>: float32
    xd, dyd, od = x.double(), dy.double(), o.double()
    inside = (q.double() - xd) * dyd / s.double()
    terms = torch.where(hi, (qmax - od) * dyd, torch.where(lo, (qmin - od) * dyd, inside))
    return terms, ~(hi | lo)


def lsq_t_factor(n: int, qmin: int, qmax: int) -> float:
    """rsqrtf(n * (qmax - qmin)) (linear.cu:306), the float32 the launcher computes."""
    return float(np.float32(1.0 / math.sqrt(float(n) * float(qmax - qmin))))


def lsq_c_factor(n: int, qmax: int) -> float:
    """rsqrtf(n * qmax) (linear.cu:402) -- NOT the (qmax - qmin) of the per-tensor factor."""
    return float(np.float32(1.0 / math.sqrt(float(n) * float(qmax))))


def fp8_terms(x, dy, s, o, exponent: int, mantissa: int, clip_min: float, clip_max: float):
    """Per-element terms of QuantizeTensor_FT_B / _FC_B (floating.cu:133-331), ROUND_HALF_EVEN: the value is quantised
    against [clip_min - 1, clip_max + 1]; a result on either sentinel is clipped, term s * (clip - o) * dy / s."""
    cmin_s, cmax_s = np.float32(clip_min) - np.float32(1), np.float32(clip_max) + np.float32(1)
    qt = F.quantize_unscaled(quotient32(x, s), exponent, mantissa, float(cmin_s), float(cmax_s))
    q = (qt - o) * s                                                    # float32, as the reference
    cmin = s * (_f32(clip_min, x) - o)
    cmax = s * (_f32(clip_max, x) - o)
    xd, dyd, sd = x.double(), dy.double(), s.double()
    hi, lo = qt == float(cmax_s), qt == float(cmin_s)
    inside = (q.double() - xd) / sd * dyd
    terms = torch.where(hi, cmax.double() * dyd / sd, torch.where(lo, cmin.double() * dyd / sd, inside))
    return terms, ~(hi | lo)


def fp8_denom(n: int, clip_max: float) -> float:
    """sqrtf((float)n * clip_max) (floating.cu:181), float32 as the launcher computes it."""
    return float(np.sqrt(np.float32(np.float32(n) * np.float32(clip_max))))


def rounding_loss_terms(x, s, o_raw, qmin: int, qmax: int, rounding: int, per_channel: bool):
    """_RoundingLoss_LT / _LC (train.cu:115-141 / :220-247): |fq(v) - v| where v is not clipped; the offset is rounded
    with nearbyint, the clip test uses s * (clip - o) with the int offset (LT) or the raw float offset (LC)."""
    oi = torch.round(o_raw.double()).clamp(I32_MIN, I32_MAX)
    r = round_policy(quotient32(x, s), rounding)
    qc = (r + oi).clamp(qmin, qmax)
    dq = (qc - oi).float() * s
    ofs = o_raw if per_channel else oi.float()
    clipped = (x > s * (_f32(qmax, x) - ofs)) | (x < s * (_f32(qmin, x) - ofs))
    return torch.where(clipped, torch.zeros_like(x, dtype=torch.float64), (dq.double() - x.double()).abs())


def fp8_search_err(x2d, exponent: int, mantissa: int, clip_min: float, clip_max: float, cand: float):
    """floating.py:112-118 / :129-...: one candidate scale, offset 0: the error fq(x) - x formed in float32 like the
    fake-quant output (q * s - x), per element."""
    s = _f32(cand, x2d)
    q = F.quantize_unscaled(quotient32(x2d, s), exponent, mantissa, clip_min, clip_max)
    return (q - 0.0) * s - x2d


def fp8_search_sse(x2d, exponent: int, mantissa: int, clip_min: float, clip_max: float, cand: float):
    """The row sums of the squared errors, in float64 (each square is exact in float64)."""
    e = fp8_search_err(x2d, exponent, mantissa, clip_min, clip_max, cand).double()
    return (e * e).sum(dim=-1)


# ------------------------------------------------------------------------------------------------- utilities
def ulp32(v: float) -> float:
    return float(np.spacing(np.float32(abs(v))))


def assert_bits(got: torch.Tensor, want: torch.Tensor, what: str):
    g, w = got.reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32)
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w).reshape(-1)
        i = int(bad[0])
        raise AssertionError(f'{what}: {bad.numel()} elements differ, first at {i}: '
                             f'{float(got.reshape(-1)[i])!r} vs {float(want.reshape(-1)[i])!r}')


def check_within(got: float, ref: float, bound: float, what: str):
    err = abs(got - ref)
    assert err <= bound, f'{what}: |{got!r} - {ref!r}| = {err:.3e} > derived bound {bound:.3e}'


def lsq_t_reference(x, dy, s, o, qmin, qmax, rounding, gx=None, chunk=1 << 22):
    """(sum, sum |.|) of the LT terms in float64, chunk by chunk; grad_x checked bit for bit on the way."""
    n = x.numel()
    xf, df = x.reshape(-1), dy.reshape(-1)
    gf = None if gx is None else gx.reshape(-1)
    tot, tab = 0.0, 0.0
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        t, mask = lsq_terms(xf[a:b], df[a:b], s, o, qmin, qmax, rounding)
        tot += float(t.sum()); tab += float(t.abs().sum())
        if gf is not None:
            assert_bits(gf[a:b], torch.where(mask, df[a:b], torch.zeros_like(df[a:b])), f'grad_x [{a}, {b})')
        del t, mask
    return tot, tab


def channel_view(x: torch.Tensor, axis):
    if axis is None: return x.reshape(1, 1, -1)
    C = x.shape[axis]
    outer = int(np.prod(x.shape[:axis])) if axis > 0 else 1
    return x.reshape(outer, C, -1)


def per_channel_reference(term_fn, x, dy, s, o, axis, gx=None, lim=1 << 22):
    """Per-channel (sum, sum |.|) of term_fn's terms, in slices of <= lim elements; grad_x bit for bit on the way."""
    x3, d3 = channel_view(x, axis), channel_view(dy, axis)
    g3 = None if gx is None else channel_view(gx, axis)
    outer, C, epc = x3.shape
    sv, ov = s.reshape(1, C, 1), o.reshape(1, C, 1)
    tot = torch.zeros(C, dtype=torch.float64, device=x.device); tab = torch.zeros_like(tot)
    step_o = max(1, lim // (C * epc))
    step_e = epc if C * epc <= lim else max(1, lim // C)
    for a in range(0, outer, step_o):
        for e in range(0, epc, step_e):
            sl = (slice(a, min(outer, a + step_o)), slice(None), slice(e, min(epc, e + step_e)))
            t, mask = term_fn(x3[sl], d3[sl], sv, ov)
            tot += t.sum(dim=(0, 2)); tab += t.abs().sum(dim=(0, 2))
            if g3 is not None:
                assert_bits(g3[sl], torch.where(mask, d3[sl], torch.zeros_like(d3[sl])), f'grad_x slice {a}, {e}')
            del t, mask
    return tot.cpu().numpy(), tab.cpu().numpy()


def num_cu() -> int:
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def stream_grid(work: int, per_block: int, max_blocks: int) -> int:
    """common.hpp: stream_grid."""
    return max(1, min(max_blocks, -(-work // per_block)))


def free_cuda():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------- launch geometry (read off the launchers)
def lt_geometry(CUDA, n: int, aligned: bool):
    """ppqhip_fq_linear_t_bwd / _main (linear.hip: lsq_t_u, lsq_t_grid, fq_linear_t_bwd_kernel): U = 1 float4 pair per lane
    up to 4 Mi elements, else 4; grid G = min(ceil(n / (4 * 256 * U)), 65536); each workgroup walks `per` tiles of
    256 * U float4.  m (terms per lane): 4 * U * per from the tiles + 1 from the scalar tail (vectorised); the whole tensor
    through the grid-stride scalar loop otherwise.  d: wave butterfly 6 + wave-0 butterfly over the 4 wave sums 6 +
    double finish 1 + (float) 1 + * grad_factor 1 = 15."""
    G = CUDA.lsq_t_partials(n)
    u = 1 if n <= (4 << 20) else 4
    tile = KBLOCK * u
    nvec = n >> 2
    tiles = -(-nvec // tile)
    per = max(1, -(-tiles // G))
    m = 4 * u * per + 1 if aligned else -(-n // (G * KBLOCK))
    return dict(G=G, U=u, tile_elems=4 * tile, per=per, nvec=nvec, m=m, d=15)


def lc_row_bound_levels(outer: int, epc: int):
    """fq_linear_c_bwd_row_kernel (elem_per_channel >= 256): one workgroup per (row, 4096-element chunk), <= 16 terms per
    lane (4 float4 or 16 scalar trips); d = block_sum 12 + tot * grad_factor 1 + one float atomic level per partial of the
    channel (outer * chunks of them)."""
    chunks = -(-epc // 4096)
    return 16, 12 + 1 + outer * chunks


def generic_grid(n: int) -> int:
    """fq_linear_c_bwd_generic_kernel / fq_float_bwd_generic_kernel: stream_grid(n, 256 * 8, num_cu * 2)."""
    return stream_grid(n, KBLOCK * 8, num_cu() * 2)


def generic_bound_levels(n: int, C: int, per_channel_elems: int):
    """Generic kernels (short rows): C <= 8192 -> LDS float atomics of the terms (<= min(count of the channel, trips * 256)
    per workgroup), one rounded partial * factor per workgroup, one global float atomic level per workgroup; C > 8192 ->
    every term * factor straight to a global float atomic (one level per element of the channel)."""
    G = generic_grid(n)
    if C <= 8192:
        trips = -(-n // (G * KBLOCK))
        return min(per_channel_elems, trips * KBLOCK), 1 + G
    return 1, 1 + per_channel_elems


# -------------------------------------------------------------------------------------------- CPU self-test
def test_float64_helpers_match_the_c_oracle_on_the_cpu():
    """The helpers above against oracle/ppq_oracle.c at small shapes: grad_x / masks bit for bit, every sum within the
    term-rounding part of the bound (the oracle forms each term in float32 -- e roundings -- and sums in double)."""
    from oracle import ppq_oracle as O
    rng = np.random.default_rng(2024)
    for rounding in range(8):
        for (qmin, qmax), oraw in (((0, 255), 3.4), ((-128, 127), -0.5), ((-8, 7), 2.5)):
            x = (rng.standard_normal(3001) * 3).astype(np.float32)
            dy = rng.standard_normal(3001).astype(np.float32)
            s = np.array([0.037], np.float32); o = np.array([oraw], np.float32)
            wx, ws = O.fq_linear_t_bwd(x, s, o, dy, qmin, qmax, rounding)
            t, mask = lsq_terms(torch.from_numpy(x), torch.from_numpy(dy), torch.from_numpy(s), torch.from_numpy(o),
                                qmin, qmax, rounding)
            assert_bits(torch.from_numpy(wx), torch.where(mask, torch.from_numpy(dy), torch.zeros(3001)), 'LT grad_x')
            gf = lsq_t_factor(x.size, qmin, qmax)
            ref = float(t.sum()) * gf
            check_within(float(ws[0]), ref, gamma(4 + 2) * float(t.abs().sum()) * gf + ulp32(ref), f'LT r={rounding}')
    for shape, axis in (([3, 5, 40], 1), ([6, 300], 0), ([4, 6, 7], 2)):
        x = (rng.standard_normal(shape) * 2).astype(np.float32); dy = rng.standard_normal(shape).astype(np.float32)
        C = shape[axis]
        s = (np.abs(rng.standard_normal(C)) * 0.05 + 0.01).astype(np.float32)
        o = rng.integers(-3, 4, C).astype(np.float32) + 0.5
        for rounding in (0, 1, 6):
            wx, ws = O.fq_linear_c_bwd(x, s, o, dy, axis, -128, 127, rounding)
            xt, dt = torch.from_numpy(x), torch.from_numpy(dy)
            ref, ab = per_channel_reference(lambda a, b, sv, ov: lsq_terms(a, b, sv, ov, -128, 127, rounding), xt, dt,
                                            torch.from_numpy(s), torch.from_numpy(o), axis, gx=torch.from_numpy(wx))
            gf = lsq_c_factor(x.size, 127)
            for c in range(C):
                check_within(float(ws[c]), ref[c] * gf, gamma(4 + 2) * ab[c] * gf + ulp32(ref[c] * gf), f'LC {shape} c{c}')
    for fmt in ((4, 3, -448.0, 448.0), (5, 2, -57344.0, 57344.0)):
        for shape, axis in (([4, 3, 70], 1), ([2000], None)):
            x = (rng.standard_normal(shape) * 150).astype(np.float32); dy = rng.standard_normal(shape).astype(np.float32)
            C = 1 if axis is None else shape[axis]
            s = np.array([0.5, 1.0, 0.3][:C], np.float32); o = np.zeros(C, np.float32)
            wx, ws = O.fq_float_c_bwd(x, s, o, dy, axis, *fmt, 0)
            ref, ab = per_channel_reference(lambda a, b, sv, ov: fp8_terms(a, b, sv, ov, *fmt), torch.from_numpy(x),
                                            torch.from_numpy(dy), torch.from_numpy(s), torch.from_numpy(o), axis,
                                            gx=torch.from_numpy(wx))
            den = fp8_denom(x.size, fmt[3])
            for c in range(C):
                check_within(float(ws[c]), ref[c] / den, gamma(4 + 2) * ab[c] / den + ulp32(ref[c] / den), f'FP8 {fmt} c{c}')
    for per_channel in (False, True):
        x = (rng.standard_normal([3, 6, 50]) * 0.5).astype(np.float32)
        s = (rng.random(6) * 0.05 + 0.01).astype(np.float32) if per_channel else np.array([0.02], np.float32)
        o = (rng.integers(-3, 3, s.size) + rng.random(s.size)).astype(np.float32)
        for rounding in (0, 2, 7):
            want = O.rounding_loss(x, s, o, -128, 127, rounding, channel_axis=1 if per_channel else None)
            xt = torch.from_numpy(x)
            sv = torch.from_numpy(s).reshape(1, -1, 1) if per_channel else torch.from_numpy(s)
            ov = torch.from_numpy(o).reshape(1, -1, 1) if per_channel else torch.from_numpy(o)
            t = rounding_loss_terms(xt, sv, ov, -128, 127, rounding, per_channel)
            ir = float(np.float32(1.0) / np.sqrt(np.float32(x.size)))
            check_within(float(want[0]), float(t.sum()) * ir, gamma(1 + 2) * float(t.sum()) * ir + ulp32(float(want[0])),
                         f'rounding loss pc={per_channel} r={rounding}')
    # FP8 search SSE: float32 error terms, as the fake-quant forward forms them
    x = (rng.standard_normal([3, 500]) * 40).astype(np.float32)
    for cand in (0.25, 1.0, 0.3):
        want = np.stack([O.fq_float_c(x, np.full(3, cand, np.float32), np.zeros(3, np.float32), 0, 4, 3, -448.0, 448.0, 0)])
        assert_bits(fp8_search_err(torch.from_numpy(x), 4, 3, -448.0, 448.0, cand), torch.from_numpy(want[0] - x),
                    f'search error, scale {cand}')


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope='module')
def CUDA():
    from ppq_amd import CUDA as C
    return C


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    if torch.cuda.is_available(): free_cuda()


@pytest.fixture(scope='module', autouse=True)
def _report_peak_memory():
    """Peak device memory of this file (run with -s to see it): the largest case must stay well under 8 GB."""
    if torch.cuda.is_available(): torch.cuda.reset_peak_memory_stats()
    yield
    if torch.cuda.is_available():
        print(f'\n[test_gpu_reductions] peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB', file=sys.stderr)


def _sentinel_dy(dy: torch.Tensor, x: torch.Tensor, pos, s: float, hi_first=True):
    """dy = 0 except at pos (distinct powers of 4); x at pos far outside the clip range, alternately above and below.
    Returns the list of (position, sign, weight)."""
    dy.zero_()
    out = []
    flat_x, flat_d = x.reshape(-1), dy.reshape(-1)
    for k, p in enumerate(pos):
        sign = 1.0 if (k % 2 == 0) == hi_first else -1.0
        flat_x[p] = sign * 1.0e6 * s
        flat_d[p] = float(4 ** k)
        out.append((p, sign, float(4 ** k)))
    return out


def _rounds(positions, k=8):
    p = sorted(set(positions))
    return [p[i:i + k] for i in range(0, len(p), k)]


def lt_sentinel_positions(n: int, g: dict, aligned: bool):
    pos = [0, n - 1]
    if aligned:
        vec_end = 4 * g['nvec']
        pos += list(range(vec_end, n))                                  # scalar tail after nvec << 2
        te, per, G = g['tile_elems'], g['per'], g['G']
        we = te * per
        tiles = -(-g['nvec'] // (te // 4))
        for k in (1, 2, tiles - 1):
            pos += [k * te - 1, k * te]
        for b in (1, G - 1, 8191, 8192, 8193):
            pos += [b * we - 1, b * we, b * we + te - 1, b * we + te]
        last = -(-g['nvec'] // (per * te // 4)) - 1                     # last workgroup with vector work
        pos += [last * we, last * we + te, vec_end - 1]
    else:
        st = g['G'] * KBLOCK
        pos += [st - 1, st, 2 * st - 1, n // 2]
    return [p for p in pos if 0 <= p < n]


LT_SIZES = [1, 4 << 20, (4 << 20) + 4, (24 << 20) + 3, 51380224, (1 << 28) + 4099]


@pytest.mark.gpu
@pytest.mark.parametrize('n', LT_SIZES)
def test_lsq_t_backward_against_float64_and_sentinels(CUDA, n):
    """LinearQuantize_T_B at every size-dependent branch: U = 1 (<= 4 Mi), U = 4, streaming loads (>= 24 Mi), more than
    8192 partials (the finish loop's second trip: 51,380,224 = the bench's B x 32 tensor, 12544 partials), per > 1 (> 2^28
    elements: 65536 workgroups walking two tiles each); the same through _T_B_Main + LSQ_Finish_Multi."""
    g = torch.Generator(device=DEV).manual_seed(n % 100003)
    qmin, qmax = -128, 127
    x = torch.randn(n, generator=g, device=DEV) * 3
    dy = torch.randn(n, generator=g, device=DEV)
    s = torch.tensor([0.031], device=DEV); o = torch.tensor([3.4], device=DEV)
    geo = lt_geometry(CUDA, n, aligned=True)
    gf = lsq_t_factor(n, qmin, qmax)
    gx, gs = CUDA.LinearQuantize_T_B(x, s, o, dy, qmin, qmax, 0)
    ref, ab = lsq_t_reference(x, dy, s, o, qmin, qmax, 0, gx=gx)
    del gx
    bound = gamma(geo['m'] + geo['d'] + 4) * ab * gf
    check_within(float(gs), ref * gf, bound, f'LT_B n={n} {geo}')
    partial = torch.full([CUDA.lsq_t_partials(n)], float('nan'), device=DEV)
    gs2 = torch.full([1], float('nan'), device=DEV)
    gx2 = CUDA.LinearQuantize_T_B_Main(x, s, o, dy, qmin, qmax, 0, partial)
    CUDA.LSQ_Finish_Multi([partial], [n], [qmin], [qmax], [gs2])
    check_within(float(gs2), ref * gf, bound, f'LT_B_Main + finish n={n}')
    del gx2
    # sentinels: exact sums, 2 ulp for the one rounding (the product with grad_factor)
    o_r = 3.0
    for rnd in _rounds(lt_sentinel_positions(n, geo, True)):
        marks = _sentinel_dy(dy, x, rnd, 0.031)
        S = sum((qmax - o_r if sg > 0 else qmin - o_r) * w for _, sg, w in marks)
        A = sum(abs((qmax - o_r if sg > 0 else qmin - o_r) * w) for _, sg, w in marks)
        want = float(np.float32(S * gf))
        gx, gs = CUDA.LinearQuantize_T_B(x, s, o, dy, qmin, qmax, 0)
        assert abs(float(gs) - want) <= 2 * ulp32(A * gf), (n, rnd, float(gs), want)
        gxm = CUDA.LinearQuantize_T_B_Main(x, s, o, dy, qmin, qmax, 0, partial)
        CUDA.LSQ_Finish_Multi([partial], [n], [qmin], [qmax], [gs2])
        assert abs(float(gs2) - want) <= 2 * ulp32(A * gf), ('main+finish', n, rnd, float(gs2), want)
        idx = torch.tensor(rnd, device=DEV)
        assert torch.all(gx[idx] == 0) and torch.all(gxm[idx] == 0), 'clipped sentinels pass no gradient'
        del gx, gxm
    del x, dy, partial


@pytest.mark.gpu
@pytest.mark.parametrize('n', [5, 4099, (4 << 20) + 7, (24 << 20) + 1])
def test_lsq_t_backward_unaligned_view(CUDA, n):
    """A view at storage offset 1 (4-B aligned only: vec_ok = 0, the whole tensor through the grid-stride scalar loop)."""
    g = torch.Generator(device=DEV).manual_seed(n)
    qmin, qmax = 0, 255
    xb = torch.randn(n + 1, generator=g, device=DEV) * 4 + 3
    db = torch.randn(n + 1, generator=g, device=DEV)
    x, dy = xb[1:], db[1:]
    assert x.data_ptr() % 16 != 0
    s = torch.tensor([0.043], device=DEV); o = torch.tensor([100.5], device=DEV)
    geo = lt_geometry(CUDA, n, aligned=False)
    gf = lsq_t_factor(n, qmin, qmax)
    gx, gs = CUDA.LinearQuantize_T_B(x, s, o, dy, qmin, qmax, 0)
    ref, ab = lsq_t_reference(x, dy, s, o, qmin, qmax, 0, gx=gx)
    check_within(float(gs), ref * gf, gamma(geo['m'] + geo['d'] + 4) * ab * gf, f'LT_B unaligned n={n}')
    o_r = 101.0
    for rnd in _rounds(lt_sentinel_positions(n, geo, False)):
        marks = _sentinel_dy(dy, x, rnd, 0.043)
        S = sum((qmax - o_r if sg > 0 else qmin - o_r) * w for _, sg, w in marks)
        A = sum(abs((qmax - o_r if sg > 0 else qmin - o_r) * w) for _, sg, w in marks)
        _, gs = CUDA.LinearQuantize_T_B(x, s, o, dy, qmin, qmax, 0)
        want = float(np.float32(S * gf))
        assert abs(float(gs) - want) <= 2 * ulp32(A * gf), (n, rnd, float(gs), want)


@pytest.mark.gpu
@pytest.mark.parametrize('rounding', range(8))
def test_lsq_t_backward_every_rounding_mode(CUDA, rounding):
    """Every rounding policy at one mid size (U = 4, the runtime-policy kernel for all but HALF_EVEN), with values on
    rounding ties (multiples of s / 2) mixed in."""
    n = (6 << 20) + 3
    g = torch.Generator(device=DEV).manual_seed(77 + rounding)
    s = torch.tensor([0.0625], device=DEV); o = torch.tensor([-2.5], device=DEV)
    x = torch.randn(n, generator=g, device=DEV) * 5
    x[::3] = torch.round(x[::3] / 0.03125) * 0.03125                 # exact half-steps of s: every policy decides
    dy = torch.randn(n, generator=g, device=DEV)
    qmin, qmax = -8, 7
    geo = lt_geometry(CUDA, n, aligned=True)
    gf = lsq_t_factor(n, qmin, qmax)
    gx, gs = CUDA.LinearQuantize_T_B(x, s, o, dy, qmin, qmax, rounding)
    ref, ab = lsq_t_reference(x, dy, s, o, qmin, qmax, rounding, gx=gx)
    check_within(float(gs), ref * gf, gamma(geo['m'] + geo['d'] + 4) * ab * gf, f'LT_B rounding={rounding}')


@pytest.mark.gpu
def test_lsq_finish_multi_over_96_jobs(CUDA):
    """LSQ_Finish_Multi with 100 jobs of mixed sizes: two launches (96 + 4).  Every grad_s starts as NaN, is compared with
    its float64 reference, and carries a sentinel-only twin, so a job the second launch drops or misroutes is caught."""
    rng = np.random.default_rng(5)
    sizes = [int(v) for v in rng.integers(1, 300000, 100)]
    sizes[97] = 70001; sizes[99] = 3
    items, refs = [], []
    for k, n in enumerate(sizes):
        x = torch.from_numpy((rng.standard_normal(n) * 2).astype(np.float32)).to(DEV)
        dy = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
        s = torch.tensor([0.02 + 0.001 * k], device=DEV); o = torch.tensor([float(k % 5)], device=DEV)
        items.append((x, dy, s, o))
    qmin, qmax = -128, 127
    partials = [torch.full([CUDA.lsq_t_partials(x.numel())], float('nan'), device=DEV) for x, *_ in items]
    gss = [torch.full([1], float('nan'), device=DEV) for _ in items]
    for (x, dy, s, o), p in zip(items, partials):
        gx = CUDA.LinearQuantize_T_B_Main(x, s, o, dy, qmin, qmax, 0, p)
        ref, ab = lsq_t_reference(x, dy, s, o, qmin, qmax, 0, gx=gx)
        refs.append((ref, ab))
    CUDA.LSQ_Finish_Multi(partials, sizes, [qmin] * 100, [qmax] * 100, gss)
    for k, ((x, *_), gs, (ref, ab)) in enumerate(zip(items, gss, refs)):
        n = x.numel(); geo = lt_geometry(CUDA, n, aligned=True)
        gf = lsq_t_factor(n, qmin, qmax)
        check_within(float(gs), ref * gf, gamma(geo['m'] + geo['d'] + 4) * ab * gf, f'finish job {k} n={n}')
    # sentinel twin: one marked element per job (its last), weight 4^(k % 8)
    wants = []
    for k, ((x, dy, s, o), p) in enumerate(zip(items, partials)):
        n = x.numel()
        dy.zero_(); x[n - 1] = 1.0e6; dy[n - 1] = float(4 ** (k % 8))
        CUDA.LinearQuantize_T_B_Main(x, s, o, dy, qmin, qmax, 0, p)
        wants.append(float(np.float32((qmax - float(k % 5)) * 4 ** (k % 8) * lsq_t_factor(n, qmin, qmax))))
        gss[k].fill_(float('nan'))
    CUDA.LSQ_Finish_Multi(partials, sizes, [qmin] * 100, [qmax] * 100, gss)
    got = [float(v) for v in gss]
    for k in range(100):
        assert abs(got[k] - wants[k]) <= 2 * ulp32(wants[k]), (k, got[k], wants[k])


# (shape, axis, aligned): row kernel epc 256 / 4096 / 4097 (ragged chunk, scalar path) / 4100 / 70000 (many chunks),
# streaming loads (n >= 24 Mi: [2, 512, 160, 160] = 26.2 M), generic with C <= 8192 (LDS) and C = 9000 / 20000 (global
# atomics), axis 0, 1 and last, an unaligned view
LC_CASES = [([3, 7, 256], 1, True), ([5, 4096], 0, True), ([2, 3, 4097], 1, True), ([3, 2, 4100], 1, True),
            ([4, 70000], 0, True), ([2, 512, 160, 160], 1, True), ([64, 37], 1, True), ([16, 3, 3, 3], 0, True),
            ([40, 9000], 1, True), ([13, 20000], 1, True), ([6, 20, 31], 2, True), ([4, 8, 1024], 1, False),
            ([3, 20, 20], 1, False)]


def _lc_geometry(shape, axis):
    C = shape[axis]
    outer = int(np.prod(shape[:axis])) if axis > 0 else 1
    epc = int(np.prod(shape[axis + 1:])) if axis + 1 < len(shape) else 1
    return C, outer, epc


def _lc_levels(n, C, outer, epc):
    if epc >= 256: return lc_row_bound_levels(outer, epc)
    return generic_bound_levels(n, C, outer * epc)


def _lc_sentinel_positions(C, outer, epc):
    """channel first / last element, 4096-chunk edges +-1, the last channel (C > 8192), the last element."""
    n = C * outer * epc
    pos = []
    for c in sorted({0, 1, C // 2, C - 1}):
        for r in sorted({0, outer - 1}):
            base = (r * C + c) * epc
            pos += [base, base + epc - 1]
            for k in range(1, min(3, -(-epc // 4096))):
                pos += [base + k * 4096 - 1, base + k * 4096]
    pos.append(n - 1)
    return [p for p in pos if 0 <= p < n]


def _make_view(shape, aligned, gen):
    n = int(np.prod(shape))
    b = torch.randn(n + (0 if aligned else 1), generator=gen, device=DEV)
    v = b if aligned else b[1:]
    return v.reshape(shape)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,axis,aligned', LC_CASES)
def test_lsq_c_backward_against_float64_and_sentinels(CUDA, shape, axis, aligned):
    g = torch.Generator(device=DEV).manual_seed(int(np.prod(shape)) + axis)
    C, outer, epc = _lc_geometry(shape, axis)
    n = C * outer * epc
    qmin, qmax = -128, 127
    x = _make_view(shape, aligned, g).mul_(3)
    dy = _make_view(shape, aligned, g)
    s = torch.rand(C, generator=g, device=DEV) * 0.05 + 0.01
    o = torch.randint(-4, 5, (C,), generator=g, device=DEV).float() + 0.5
    gf = lsq_c_factor(n, qmax)
    gx, gs = CUDA.LinearQuantize_C_B(x, s, o, dy, qmin, qmax, axis, 0)
    ref, ab = per_channel_reference(lambda a, b, sv, ov: lsq_terms(a, b, sv, ov, qmin, qmax, 0), x, dy, s, o, axis, gx=gx)
    m, d = _lc_levels(n, C, outer, epc)
    got = gs.cpu().numpy().astype(np.float64)
    bound = gamma(m + d + 4) * ab * gf
    bad = np.nonzero(np.abs(got - ref * gf) > bound)[0]
    assert bad.size == 0, (shape, axis, int(bad[0]), got[bad[0]], ref[bad[0]] * gf, bound[bad[0]])
    del gx
    # sentinels, per channel: within 2 ulp per rounded partial (every partial holding a sentinel is rounded once, its
    # atomic add once more)
    o_r = _round_offset(o).cpu().numpy().astype(np.float64)
    sv = s.cpu().numpy()
    for rnd in _rounds(_lc_sentinel_positions(C, outer, epc)):
        dy.zero_()
        S = np.zeros(C); A = np.zeros(C); K = np.zeros(C)
        xf, df = x.reshape(-1), dy.reshape(-1)
        for k, p in enumerate(rnd):
            c = (p // epc) % C
            sg = 1.0 if k % 2 == 0 else -1.0
            xf[p] = sg * 1.0e6 * float(sv[c]); df[p] = float(4 ** k)
            w = (qmax - o_r[c] if sg > 0 else qmin - o_r[c]) * 4 ** k
            S[c] += w; A[c] += abs(w); K[c] += 1
        gx, gs = CUDA.LinearQuantize_C_B(x, s, o, dy, qmin, qmax, axis, 0)
        got = gs.cpu().numpy().astype(np.float64)
        for c in np.nonzero(K)[0]:
            want = float(np.float32(S[c] * gf))
            assert abs(got[c] - want) <= 2 * K[c] * ulp32(A[c] * gf), (shape, axis, rnd, c, got[c], want)
        others = np.ones(C, bool); others[np.nonzero(K)[0]] = False
        assert np.all(got[others] == 0), (shape, axis, 'a channel without sentinels got a gradient')
        idx = torch.tensor(rnd, device=DEV)
        assert torch.all(gx.reshape(-1)[idx] == 0)
        del gx
    del x, dy


@pytest.mark.gpu
def test_lsq_c_backward_multi_against_float64(CUDA):
    """LinearQuantize_C_B_Multi (one workgroup per channel, fixed order): float64 bound per channel (m = the channel's terms
    per lane over its outer rows, d = block_sum 12 + grad_factor 1), grad_x bit for bit, plus a sentinel per job on its
    last channel's last element."""
    rng = np.random.default_rng(11)
    shapes = [((64, 32, 3, 3), 0), ((16, 4100), 0), ((3, 40, 70), 1), ((2, 24, 20, 20), 1), ((6, 5, 7, 3), 1),
              ((512, 1024), 0), ((8, 97), 1)]
    items = []
    for shape, axis in shapes:
        C = shape[axis]
        x = torch.from_numpy((rng.standard_normal(shape) * 0.5).astype(np.float32)).to(DEV)
        dy = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV)
        s = torch.from_numpy((np.abs(rng.standard_normal(C)) * 0.05 + 0.01).astype(np.float32)).to(DEV)
        o = torch.from_numpy(rng.integers(-2, 3, C).astype(np.float32)).to(DEV)
        items.append((x, s, o, dy, axis))
    qmin, qmax = -8, 7
    for phase in ('random', 'sentinel'):
        if phase == 'sentinel':
            for x, s, o, dy, axis in items:
                dy.zero_(); x.reshape(-1)[-1] = 1.0e6; dy.reshape(-1)[-1] = 16.0
        gxs, gss = CUDA.LinearQuantize_C_B_Multi([i[0] for i in items], [i[1] for i in items], [i[2] for i in items],
                                                 [i[3] for i in items], [qmin] * len(items), [qmax] * len(items),
                                                 [i[4] for i in items], 0)
        for (x, s, o, dy, axis), gx, gs in zip(items, gxs, gss):
            C, outer, epc = _lc_geometry(list(x.shape), axis)
            n = x.numel(); gf = lsq_c_factor(n, qmax)
            got = gs.cpu().numpy().astype(np.float64)
            if phase == 'random':
                ref, ab = per_channel_reference(lambda a, b, sv, ov: lsq_terms(a, b, sv, ov, qmin, qmax, 0), x, dy, s, o,
                                                axis, gx=gx)
                vec = epc % 4 == 0
                m = outer * (16 * -(-epc // 4096) if vec else -(-epc // KBLOCK))
                bound = gamma(m + 13 + 4) * ab * gf
                assert np.all(np.abs(got - ref * gf) <= bound), (tuple(x.shape), axis)
            else:
                want = float(np.float32((qmax - float(o[-1])) * 16.0 * gf))
                assert got[-1] == want and np.all(got[:-1] == 0), (tuple(x.shape), axis, got[-1], want)


FP8_CASES = [(None, [1], True), (None, [70001], True), (None, [(24 << 20) + 4], True), (None, [51380224], True),
             (1, [2, 5, 9001], True), (1, [3, 4, 4096 + 8], True), (1, [4, 3, 4096 * 3], False), (1, [64, 37], True),
             (1, [40, 9000], True), (3, [6, 3, 50, 20], True), (0, [3, 2, 300], True)]


E4M3, E5M2 = (4, 3, -448.0, 448.0), (5, 2, -57344.0, 57344.0)
FP8_PARAMS = [(E4M3,) + c for c in FP8_CASES] + [(E5M2,) + c for c in FP8_CASES if int(np.prod(c[1])) <= (1 << 22)]


@pytest.mark.gpu
@pytest.mark.parametrize('fmt,axis,shape,aligned', FP8_PARAMS)
def test_fp8_backward_against_float64_and_sentinels(CUDA, fmt, axis, shape, aligned):
    """FloatingQuantize_T_B / _C_B: row kernel (elem_per_channel >= 64, 4096-element chunks, one float partial each) +
    the double finish kernel (more than 8192 partials per channel at 51 M), streaming loads (>= 24 Mi), the generic
    kernel with LDS (C <= 8192) and global (C = 9000) atomics, unaligned rows.
    Bound levels: row path m = 16 (one chunk per workgroup, <= 16 terms per lane), d = wave 6 + LDS sequential 4 + double
    finish 1 + (float) 1 + / denom 1 = 13; generic path as the LSQ generic kernel with / denom for * grad_factor."""
    E, M, cmin, cmax = fmt
    g = torch.Generator(device=DEV).manual_seed(int(np.prod(shape)) + E)
    n = int(np.prod(shape))
    C = 1 if axis is None else shape[axis]
    x = _make_view(shape, aligned, g).mul_(cmax / 3)
    dy = _make_view(shape, aligned, g)
    s = torch.tensor([0.5, 2.0, 0.75, 1.0], device=DEV).repeat(-(-C // 4))[:C].contiguous()
    o = torch.zeros(C, device=DEV)
    den = fp8_denom(n, cmax)
    if axis is None: gx, gs = CUDA.FloatingQuantize_T_B(x, s, o, dy, E, M, cmin, cmax, 0)
    else: gx, gs = CUDA.FloatingQuantize_C_B(x, s, o, dy, E, M, cmin, cmax, axis, 0)
    ref, ab = per_channel_reference(lambda a, b, sv, ov: fp8_terms(a, b, sv, ov, E, M, cmin, cmax), x, dy, s, o, axis, gx=gx)
    del gx
    _, outer, epc = _lc_geometry(shape, axis) if axis is not None else (1, 1, n)
    if epc >= 64: m, d = 16, 13
    else:
        m, d = generic_bound_levels(n, C, outer * epc)
    got = gs.cpu().numpy().astype(np.float64)
    bound = gamma(m + d + 4) * ab / den
    assert np.all(np.abs(got - ref / den) <= bound), (shape, axis, np.max(np.abs(got - ref / den) - bound))
    # sentinels: s is a power of two or 0.75 -> cmax * 4^k * (1/s) exact for the powers; 0.75 channels skipped
    sv = s.cpu().numpy()
    if axis is None:
        pos = [0, n - 1, 4095, 4096, 8191 * 4096, 8192 * 4096 + 1, 12543 * 4096, (n // 4) * 4]
        rows_pos = [p for p in pos if p < n]
    else:
        rows_pos = [p for p in _lc_sentinel_positions(C, outer, epc) if sv[(p // epc) % C] != 0.75]
    for rnd in _rounds(rows_pos):
        dy.zero_()
        S = np.zeros(C); A = np.zeros(C); K = np.zeros(C)
        xf, df = x.reshape(-1), dy.reshape(-1)
        for k, p in enumerate(rnd):
            c = 0 if axis is None else (p // epc) % C
            sg = 1.0 if k % 2 == 0 else -1.0
            xf[p] = sg * 1.0e9; df[p] = float(4 ** k)
            w = (cmax if sg > 0 else cmin) * 4 ** k
            S[c] += w; A[c] += abs(w); K[c] += 1
        if axis is None: _, gs = CUDA.FloatingQuantize_T_B(x, s, o, dy, E, M, cmin, cmax, 0)
        else: _, gs = CUDA.FloatingQuantize_C_B(x, s, o, dy, E, M, cmin, cmax, axis, 0)
        got = gs.cpu().numpy().astype(np.float64)
        for c in np.nonzero(K)[0]:
            want = float(np.float32(S[c] / den))
            assert abs(got[c] - want) <= 2 * K[c] * ulp32(A[c] / den), (shape, axis, rnd, c, got[c], want)
        others = np.ones(C, bool); others[np.nonzero(K)[0]] = False
        assert np.all(got[others] == 0), (shape, axis, 'a channel without sentinels got a gradient')
    del x, dy


RL_CASES = [([1], None), ([2049], None), ([3 << 20], None), ([8, 300, 57, 57], 1), ([5, 7, 3], 2), ([2049], 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,axis', RL_CASES)
def test_rounding_loss_against_float64(CUDA, shape, axis):
    """RoundingLoss_LT / _LC: grid-stride kernel (stream_grid(n, 2048, num_cu * 4) workgroups), m = the grid-stride
    trips, d = wave 6 + LDS sequential 4 + * inv_root 1 + one float atomic level per workgroup (all add to one address),
    e = 1 (|dq - v|).  Several trips at 3 M and [8, 300, 57, 57]; channels crossing workgroup edges there.  The _B
    kernels bit for bit against sign(v - dq) * g / sqrtf(n) on the unclipped elements."""
    g = torch.Generator(device=DEV).manual_seed(int(np.prod(shape)) + 3)
    n = int(np.prod(shape))
    x = torch.randn(shape, generator=g, device=DEV) * 0.6
    pc = axis is not None
    C = shape[axis] if pc else 1
    s = (torch.rand(C, generator=g, device=DEV) * 0.02 + 0.005) if pc else torch.tensor([0.011], device=DEV)
    o = (torch.randint(-3, 3, (C,), generator=g, device=DEV).float() + 0.3) if pc else torch.tensor([1.6], device=DEV)
    qmin, qmax = -128, 127
    if pc:
        loss = CUDA.RoundingLoss_LC(x, s, o, axis, qmin, qmax, 0)
        x3 = channel_view(x, axis)
        t = rounding_loss_terms(x3, s.reshape(1, C, 1), o.reshape(1, C, 1), qmin, qmax, 0, True)
    else:
        loss = CUDA.RoundingLoss_LT(x, s, o, qmin, qmax, 0)
        t = rounding_loss_terms(x.reshape(-1), s, o, qmin, qmax, 0, False)
    ir = float(np.float32(1.0) / np.sqrt(np.float32(n)))
    G = stream_grid(n, KBLOCK * 8, num_cu() * 4)
    m = -(-n // (G * KBLOCK))
    ref = float(t.sum()) * ir
    check_within(float(loss), ref, gamma(m + 6 + 4 + 1 + G + 1) * float(t.sum()) * ir, f'rounding loss {shape} axis={axis}')
    # backward: exact
    dyv = torch.tensor([0.7], device=DEV)
    if pc:
        gx = CUDA.RoundingLoss_LC_B(x, dyv, s, o, axis, qmin, qmax, 0)
        sv, ov = s.reshape(1, C, 1), o.reshape(1, C, 1); xv = channel_view(x, axis)
    else:
        gx = CUDA.RoundingLoss_LT_B(x, dyv, s, o, qmin, qmax, 0)
        sv, ov, xv = s, o, x.reshape(-1)
    oi = torch.round(ov.double()).clamp(I32_MIN, I32_MAX)
    r = round_policy(quotient32(xv, sv), 0)
    dq = ((r + oi).clamp(qmin, qmax) - oi).float() * sv
    ofs = ov if pc else oi.float()
    clipped = (xv > sv * (_f32(qmax, xv) - ofs)) | (xv < sv * (_f32(qmin, xv) - ofs))
    root = np.float32(np.sqrt(np.float32(n)))
    want = torch.where(xv > dq, _f32(0.7, xv), _f32(-0.7, xv))
    want = (torch.where(clipped, torch.zeros_like(want), want).double() / float(root)).float()
    assert_bits(gx.reshape(-1), want.reshape(-1), f'rounding loss grad {shape}')


@pytest.mark.gpu
def test_float_scale_search_against_float64(CUDA):
    """FloatScaleSearch: per row, per candidate, the double sum of squared float32 errors; rows shorter and longer than 256
    lanes, several jobs, power-of-two candidates (the reciprocal fast path) and a non-power-of-two one (the division path).
    The sum is double with exact terms: bound (ceil(row_len / 256) + 6 + 4) * 2^-53 * sum."""
    g = torch.Generator(device=DEV).manual_seed(99)
    cands = [0.0078125, 0.125, 0.5, 1.0, 2.0, 0.3, 64.0]
    fmts = [(4, 3, -448.0, 448.0), (5, 2, -57344.0, 57344.0)]
    items = []
    for k, (rows, L) in enumerate(((3, 100), (5, 256), (2, 257), (4, 3000), (1, 70001), (7, 1))):
        E, M, lo, hi = fmts[k % 2]
        items.append((torch.randn(rows, L, generator=g, device=DEV) * (20 + 40 * k), E, M, lo, hi))
    out = CUDA.FloatScaleSearch(items, cands, 0).cpu().numpy()
    row = 0
    for v, E, M, lo, hi in items:
        L = v.shape[1]
        for j, c in enumerate(cands):
            ref = fp8_search_sse(v, E, M, lo, hi, c).cpu().numpy()
            bound = gamma(-(-L // KBLOCK) + 10, U64) * ref
            got = out[row:row + v.shape[0], j]
            assert np.all(np.abs(got - ref) <= bound), (tuple(v.shape), c, got, ref)
        row += v.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,axis,aligned', [([2, 600, 64], 1, True), ([40, 3, 1000], 1, True), ([40, 3, 1000], 1, False),
                                                ([50, 9, 7], 1, True), ([9000, 5], 1, True)])
def test_channel_sum_sentinels(CUDA, shape, axis, aligned):
    """ChannelSum's three launch forms (one workgroup per channel for C >= 2 per CU; row kernel + finish; generic for short
    rows): zeros except distinct powers of 4 at channel edges -> every channel sum is exact in any order, bit for bit,
    added onto the seed already in `sums`."""
    C, outer, epc = _lc_geometry(shape, axis)
    n = C * outer * epc
    x = _make_view(shape, aligned, torch.Generator(device=DEV).manual_seed(1)).zero_()
    for rnd in _rounds(_lc_sentinel_positions(C, outer, epc) + [n // 2]):
        x.zero_()
        want = np.full(C, 0.25)
        xf = x.reshape(-1)
        for k, p in enumerate(rnd):
            sg = 1.0 if k % 2 == 0 else -1.0
            xf[p] = sg * 4.0 ** k
            want[(p // epc) % C] += sg * 4.0 ** k
        sums = torch.full([C], 0.25, dtype=torch.float64, device=DEV)
        CUDA.ChannelSum(x, axis, sums)
        assert np.array_equal(sums.cpu().numpy(), want), (shape, rnd)
