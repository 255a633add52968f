"""GPU tests of the job-table boundary (csrc/job_table.hpp) for the entry points no other test takes past one launch:
``ppqhip_equalize_apply_multi`` (32 jobs per launch), ``ppqhip_ssd_scales_multi`` (24) and ``ppqhip_ssd_apply_multi`` (32).
One job more than a launch holds, on independent tensors of 4 to 8 channels with ``run`` 1 (4-byte accesses) and 4 (16-byte
accesses) and one job on a pointer one float off 16 bytes: every job of the chunked call equals its single-job call bit for
bit, and that equals the torch arm on the device (one IEEE operation per element; for the scales ``ssd.calculate_scale``)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _off_by_one(t: torch.Tensor) -> torch.Tensor:
    """A copy of ``t`` whose base pointer is one float behind a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 4, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _apply_cases(count: int, gen: torch.Generator) -> list:
    """(x, scale shape helper, run, inner, divide, torch arm) for ``count`` independent weights: C = 4 .. 8, an upstream Gemm
    stored [in, out] and a bias (run 1), an upstream Conv of 4 elements per channel and a downstream Conv of 2 x 2 (run 4)."""
    kinds = [
        (lambda C: (5, C), 1, False, lambda x, s: x * s.view(1, -1)),
        (lambda C: (C, 1, 2, 2), 4, False, lambda x, s: x * s.view(-1, 1, 1, 1)),
        (lambda C: (3, C, 2, 2), 4, True, lambda x, s: x / s.view(1, -1, 1, 1)),
        (lambda C: (C,), 1, False, lambda x, s: x * s),
    ]
    cases = []
    for k in range(count):
        C = 4 + k % 5
        shape, run, divide, arm = kinds[k % len(kinds)]
        x = torch.randn(shape(C), generator=gen).to(DEV)
        if k == 6: x = _off_by_one(x)                                      # a run-4 job that must take the 4-byte path
        cases.append((x, C, run, divide, arm))
    assert {c[2] for c in cases} == {1, 4} and cases[6][2] == 4 and {c[1] for c in cases} == {4, 5, 6, 7, 8}
    return cases


def test_equalize_apply_takes_one_job_more_than_a_launch_holds():
    from ppq_amd import ffi
    gen = torch.Generator().manual_seed(901)
    cases = _apply_cases(32 + 1, gen)
    scales = [(torch.rand(C, generator=gen) * 3 + 0.2).to(DEV) for _, C, *_ in cases]
    wants = [arm(x, s) for (x, _, _, _, arm), s in zip(cases, scales)]
    single = [x.clone() if x.data_ptr() % 16 == 0 else _off_by_one(x) for x, *_ in cases]
    for x, s, (_, C, run, divide, _) in zip(single, scales, cases): ffi.equalize_apply_multi([(x, s, run, C, 0, divide)])
    ffi.equalize_apply_multi([(x, s, run, C, 0, divide) for (x, C, run, divide, _), s in zip(cases, scales)])
    for k, ((x, *_), one, want) in enumerate(zip(cases, single, wants)):
        assert _same(x, one) and _same(one, want), k


def test_ssd_apply_takes_one_job_more_than_a_launch_holds():
    from ppq_amd import ffi
    gen = torch.Generator().manual_seed(902)
    cases = _apply_cases(32 + 1, gen)
    scales = [(torch.rand(4, C, generator=gen) * 3 + 0.2).to(DEV) for _, C, *_ in cases]
    wants = [torch.stack([arm(x, s[a]) for a in range(4)]) for (x, _, _, _, arm), s in zip(cases, scales)]
    kept = [x.clone() for x, *_ in cases]

    def outs(): return [torch.full((4,) + tuple(x.shape), float('nan'), device=DEV) for x, *_ in cases]
    single, multi = outs(), outs()
    for (x, C, run, divide, _), s, out in zip(cases, scales, single): ffi.ssd_apply_multi([(x, out, s, run, C, 0, divide)])
    ffi.ssd_apply_multi([(x, out, s, run, C, 0, divide) for (x, C, run, divide, _), s, out in zip(cases, scales, multi)])
    for k, ((x, *_), keep, out, one, want) in enumerate(zip(cases, kept, multi, single, wants)):
        assert _same(out, one) and _same(one, want) and _same(x, keep), k


def test_ssd_scales_takes_one_job_more_than_a_launch_holds():
    """25 pairs: a Conv (4 or 9 elements per channel) or a ``transB = 0`` Gemm in front of a Conv, a depthwise Conv or a
    ``transB = 1`` Gemm; the ranges are exact maxima, the four scales ``ssd.calculate_scale`` on the device."""
    from ppq_amd import ffi
    from ppq_amd import ssd as SSD
    gen = torch.Generator().manual_seed(903)
    ratio = 0.5
    items, wants = [], []
    for k in range(24 + 1):
        C = 4 + k % 5
        if k % 3 == 2:                                                     # [in, out]: channel c is column c (run 1)
            w1 = torch.randn(5, C, generator=gen).to(DEV)
            first, seg1 = w1.abs().amax(dim=0), (w1, 1, 1, 0, 5, C, 1)
        else:                                                              # [out, ...]: channel c is row c (run 4 or 9)
            w1 = torch.randn(C, 1, 2 + k % 3, 2 + k % 3, generator=gen).to(DEV)
            if k == 6: w1 = _off_by_one(w1)
            epc = w1.numel() // C
            first, seg1 = w1.reshape(C, -1).abs().amax(dim=1), (w1, 1, epc, 0, 1, 0, epc)
        if k % 4 == 1:                                                     # [out, in]: channel c is column c
            w2 = torch.randn(6, C, generator=gen).to(DEV)
            last, seg2 = w2.abs().amax(dim=0), (w2, 1, 1, 0, 6, C, 1)
        elif k % 4 == 3:                                                   # depthwise: group = C, one input channel per group
            w2 = torch.randn(C, 1, 2, 2, generator=gen).to(DEV)
            last, seg2 = w2.reshape(C, -1).abs().amax(dim=1), (w2, 1, 4, 4, 1, 4, 4)
        else:                                                              # Conv [3, C, 2, 2]
            w2 = torch.randn(3, C, 2, 2, generator=gen).to(DEV)
            last, seg2 = w2.abs().amax(dim=(0, 2, 3)), (w2, C, 3 * C * 4, 4, 3, C * 4, 4)
        act = (torch.rand(C, generator=gen) * 2).to(DEV)
        act[k % C] = 0.001                                                 # under the 0.01 floor
        items.append((seg1, seg2, act, ratio))
        wants.append((torch.stack([first, last]), torch.stack([SSD.calculate_scale(first, last, act, algo, ratio) for algo in range(4)])))

    def outs(): return [(torch.full((4, it[2].numel()), float('nan'), device=DEV), torch.full((2, it[2].numel()), float('nan'), device=DEV)) for it in items]
    single, multi = outs(), outs()
    for it, out in zip(items, single): ffi.ssd_scales_multi([it + out])
    ffi.ssd_scales_multi([it + out for it, out in zip(items, multi)])
    for k, ((scales, ranges), (one_scales, one_ranges), (want_ranges, want_scales)) in enumerate(zip(multi, single, wants)):
        assert _same(ranges, one_ranges) and _same(one_ranges, want_ranges), k
        assert _same(scales, one_scales) and _same(one_scales, want_scales), k
