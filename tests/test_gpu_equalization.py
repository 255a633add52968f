"""GPU tests of layerwise equalization: the two HIP kernels (csrc/equalize.hip) and the pass that drives them
(ppq_amd/equalization.py) against the reference's recorded scales and parameters (tests/golden/equalization.npz, written on the
CPU by tests/golden/make_equalization.py), against the torch arm on the device, and the activation maxima against
``max(abs())`` of the very tensors the launch read."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import equalization_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SNR_BOUND = 1e-7                     # the bound of the reference's own tests/test_layerwise_equalization.py


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'equalization.npz')))


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same(a, b) -> bool:
    """Bit equality; NaN equals NaN whatever its payload (the nan_key case)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)): return False
    keep = ~np.isnan(a)
    return np.array_equal(_bits(a[keep]), _bits(b[keep]))


def _to_device(g):
    for v in g.variables.values():
        if v.is_parameter: v.value = v.value.to(DEV)
    return g


def _case_graph(golden, k, at: str = 'init'):
    """Case k on the device with the recorded parameters of `at` ('init' or 'it<n>')."""
    params = {n[len(f'c{k}_{at}_'):]: torch.from_numpy(v.copy()) for n, v in golden.items() if n.startswith(f'c{k}_{at}_')}
    return _to_device(EC.harness_graph(k, params))


def _activations(golden, k):
    pre = f'c{k}_act_'
    return {n[len(pre):]: torch.from_numpy(v).to(DEV) for n, v in golden.items() if n.startswith(pre)} or None


def _pass(k, **kw):
    from ppq_amd.equalization import LayerwiseEqualizationPass
    case = EC.CASES[k]
    return LayerwiseEqualizationPass(iterations=case['iterations'], value_threshold=EC.VALUE_THRESHOLD,
                                     including_bias=case['including_bias'], including_act=case['including_act'], **kw)


def _pair_items(golden, k, g, q, scale):
    from ppq_amd import equalization as EQ
    case = EC.CASES[k]
    p = EQ.LayerwiseEqualizationPass(iterations=1)
    pair = p.find_equalization_pair(g, p.interested_operations(g))[q]
    acts = _activations(golden, k) or {}
    return EQ.pair_jobs(pair, scale, EC.VALUE_THRESHOLD, case['including_bias'], case['including_act'], 0.5, 0.5, acts)


@pytest.mark.parametrize('k', range(len(EC.CASES)))
def test_scale_kernel_equals_the_goldens_bit_for_bit(golden, k):
    """Every pair of every case in every iteration: the parameters the reference had BEFORE the iteration's pair go in, its
    scale must come out.  (Within an iteration pair q sees what pairs < q did: the recorded state is per iteration, so the
    kernel walks the pairs of the iteration in order and applies each scale with the apply kernel.)"""
    from ppq_amd import ffi
    case = EC.CASES[k]
    pairs = len([n for n in golden if n.startswith(f'c{k}_scale_it1_')])
    for it in range(1, case['iterations'] + 1):
        g = _case_graph(golden, k, 'init' if it == 1 else f'it{it - 1}')
        for q in range(pairs):
            want = golden[f'c{k}_scale_it{it}_p{q}']
            scale = torch.full((want.size,), -7.0, device=DEV)
            item, applies = _pair_items(golden, k, g, q, scale)
            ffi.equalize_scale_multi([item])
            assert _same(scale, want), (case['name'], it, q)
            ffi.equalize_apply_multi(applies)
        for v in g.variables.values():
            if v.is_parameter: assert _same(v.value, golden[f'c{k}_it{it}_{v.name}']), (case['name'], it, v.name)


def test_scale_kernel_all_pairs_in_one_launch_and_chunked(golden):
    """Independent pairs of several cases in ONE table (more jobs than one launch holds: the library chunks) equal the
    single-pair launches."""
    from ppq_amd import ffi
    items, wants = [], []
    for rep in range(20):                                                  # 20 x 3 first pairs > 32 jobs per launch
        for k in (0, 2, 3):
            g = _case_graph(golden, k)
            want = golden[f'c{k}_scale_it1_p0']
            scale = torch.zeros(want.size, device=DEV)
            items.append(_pair_items(golden, k, g, 0, scale)[0]); wants.append(want)
    ffi.equalize_scale_multi(items)
    for (scale, _, _), want in zip(items, wants): assert _same(scale, want)


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_apply_kernel_equals_torch_for_aligned_and_misaligned_pointers(golden, offset):
    """x * s and x / s are single IEEE operations: torch on the CPU is the reference.  Every job kind (row scale, column
    scale, bias, grouped downstream, both Gemm layouts), run % 4 == 0 and != 0, on pointers `offset` floats off 16 B."""
    from ppq_amd import ffi
    gen = torch.Generator().manual_seed(77 + offset)
    C = 8
    s = torch.rand(C, generator=gen) * 3 + 0.2
    s[1], s[2] = 0.1, 10.0

    def place(t):
        buf = torch.zeros(t.numel() + 8, device=DEV)
        v = buf[offset:offset + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == (4 * offset) % 16
        return v
    jobs, wants = [], []
    for shape, run, inner, og, divide, expect in [
            ((C, 3, 3, 3), 27, C, 0, False, lambda w: w * s.view(-1, 1, 1, 1)),                          # upstream Conv, run % 4 != 0
            ((C, 4, 2, 2), 16, C, 0, False, lambda w: w * s.view(-1, 1, 1, 1)),                          # upstream, one channel per float4
            ((5, C), 1, C, 0, False, lambda w: w * s.view(1, -1)),                                       # upstream Gemm [in, out]
            ((C,), 1, C, 0, False, lambda w: w * s),                                                     # bias
            ((6, C, 3, 3), 9, C, 0, True, lambda w: w / s.view(1, -1, 1, 1)),                            # downstream Conv, G = 1
            ((12, 4, 2, 2), 4, 4, 6, True, lambda w: (w.view(2, 6, 4, 2, 2) / s.view(2, 1, 4, 1, 1)).view(12, 4, 2, 2)),   # G = 2
            ((C, 1, 3, 3), 9, 1, 1, True, lambda w: w / s.view(-1, 1, 1, 1)),                            # depthwise
            ((7, C), 1, C, 0, True, lambda w: w / s.view(1, -1)),                                        # downstream Gemm [out, in]
            ((C, 12), 12, C, 0, True, lambda w: w / s.view(-1, 1))]:                                     # downstream Gemm [in, out]
        w = torch.randn(shape, generator=gen)
        wants.append(expect(w))
        jobs.append((place(w), place(s), run, inner, og, divide))
    ffi.equalize_apply_multi(jobs)
    for (x, *_), want in zip(jobs, wants): assert _same(x, want), tuple(want.shape)


def test_library_refuses_out_of_range_and_overlapping_jobs():
    from ppq_amd import ffi
    w, s = torch.zeros(8, 9, device=DEV), torch.ones(8, device=DEV)
    with pytest.raises(RuntimeError, match='reads element'):
        ffi.equalize_scale_multi([(s, 0.5, [(w, 1, 10, 0, 1, 0, 9, 1.0, False), (w, 1, 9, 0, 1, 0, 9, 1.0, True)])])
    with pytest.raises(RuntimeError, match='upstream and a downstream'):
        ffi.equalize_scale_multi([(s, 0.5, [(w, 1, 9, 0, 1, 0, 9, 1.0, False)])])
    with pytest.raises(RuntimeError, match='reads scale'):
        ffi.equalize_apply_multi([(w, s[:4], 9, 8, 0, False)])
    with pytest.raises(RuntimeError, match='overlap'):
        ffi.equalize_apply_multi([(w, s, 9, 8, 0, False), (w[2:], s, 9, 6, 0, True)])
    with pytest.raises(RuntimeError, match='not on the GPU'):
        ffi.equalize_apply_multi([(w.cpu(), s, 9, 8, 0, False)])
    assert not w.any()


@pytest.mark.parametrize('schedule', ['levelled', 'sequential'])
@pytest.mark.parametrize('k', range(len(EC.CASES)))
def test_pass_with_kernels_equals_the_goldens_bit_for_bit(golden, k, schedule):
    case = EC.CASES[k]
    g = _case_graph(golden, k)
    p = _pass(k, schedule=schedule)
    p.keep_scales = True
    p.optimize(g, dataloader=[], executor=None, activations=_activations(golden, k))
    pairs = len(p.pairs)
    assert len(p.scales) == pairs * case['iterations'] and p.stats['launches'] == 2 * p.stats['levels'] > 0
    for (it, q), s in p.scales.items(): assert _same(s, golden[f'c{k}_scale_it{it + 1}_p{q}']), (case['name'], it, q)
    for v in g.variables.values():
        if v.is_parameter: assert _same(v.value, golden[f'c{k}_it{case["iterations"]}_{v.name}']), (case['name'], v.name)
    last = np.concatenate([golden[f'c{k}_scale_it{case["iterations"]}_p{q}'] for q in range(pairs)])
    clipped = ((last == np.float32(0.1)) | (last == 10)) & (last != 1)
    assert p.stats == dict(pairs=pairs, levels=p.stats['levels'], launches=2 * p.stats['levels'], channels=int(last.size),
                           scaled_channels=int((last != 1).sum()), clipped_channels=int(clipped.sum()))


@pytest.mark.parametrize('k', range(len(EC.CASES)))
def test_device_torch_arm_against_the_goldens(golden, k):
    """The comparison arm on the device: expected bit-equal to the CPU goldens too.  Where it is not (the device's own sqrt /
    division), the kernels still follow the goldens (the test above); the difference is recorded, not asserted."""
    case = EC.CASES[k]
    g = _case_graph(golden, k)
    p = _pass(k, use_kernels=False)
    p.optimize(g, dataloader=[], executor=None, activations=_activations(golden, k))
    differ = [v.name for v in g.variables.values() if v.is_parameter and not _same(v.value, golden[f'c{k}_it{case["iterations"]}_{v.name}'])]
    print(case['name'], 'device torch arm differs from the CPU goldens in', differ or 'nothing')
    if differ:
        from conftest import record_parity_residue
        record_parity_residue('device_torch_arm_differs_from_cpu', 'test_device_torch_arm_against_the_goldens', case=case['name'], tensors=differ)


# yolov6s_graph is normalised to unit-variance activations: every up + down of its pairs is under the default threshold 0.5 and
# the pass would be the identity (measured: 0 scaled channels of 7968).  Threshold 0 makes it scale every channel.
GRAPHS = [('resnet50_graph', 0.5), ('yolov6s_graph', 0.0)]


@pytest.mark.parametrize('build,threshold', GRAPHS)
def test_kernel_arm_equals_torch_arm_and_levelled_equals_sequential(build, threshold):
    from ppq_amd import harness
    from ppq_amd.equalization import LayerwiseEqualizationPass
    graphs, stats = {}, {}
    for arm, kw in (('torch', dict(use_kernels=False)), ('levelled', dict(schedule='levelled')), ('sequential', dict(schedule='sequential'))):
        g = _to_device(getattr(harness, build)())
        p = LayerwiseEqualizationPass(iterations=3, value_threshold=threshold, including_bias=True, **kw)
        p.optimize(g, dataloader=[], executor=None)
        graphs[arm], stats[arm] = g, p.stats
    assert stats['levelled']['levels'] < stats['sequential']['levels'] / 2
    assert stats['levelled']['scaled_channels'] > 0 and stats['levelled']['clipped_channels'] >= 0
    for name, v in graphs['levelled'].variables.items():
        if not v.is_parameter: continue
        assert _same(v.value, graphs['sequential'].variables[name].value), name
        assert torch.isfinite(v.value).all(), name
    differ = [n for n, v in graphs['levelled'].variables.items() if v.is_parameter and not _same(v.value, graphs['torch'].variables[n].value)]
    print(build, 'kernel arm differs from the device torch arm in', len(differ), 'tensors', differ[:4])
    if differ:
        from conftest import record_parity_residue
        record_parity_residue('device_torch_arm_differs_from_kernels', 'test_kernel_arm_equals_torch_arm_and_levelled_equals_sequential',
                              graph=build, tensors=len(differ))
    assert not differ
    for key in ('pairs', 'channels', 'scaled_channels', 'clipped_channels'): assert stats['levelled'][key] == stats['torch'][key], key


def test_activation_maxima_equal_max_abs_of_the_same_tensors():
    """One forward, its outputs captured by a hook: the launch's maxima against max(abs()) of those very tensors (two
    forwards would compare two runs of the vendor convolutions, which are not bit-repeatable)."""
    from ppq_amd import harness
    from ppq_amd.equalization import LayerwiseEqualizationPass
    g = _to_device(harness.resnet50_graph(num_classes=10))
    seen = {}

    class Keeping(harness.TorchExecutor):
        def forward(self, inputs, output_names=None, hooks=None):
            outs = super().forward(inputs, output_names, hooks)
            for n, y in zip(output_names, outs):
                a = y.transpose(0, 1).reshape(y.shape[1], -1).abs().amax(dim=1)
                seen[n] = a if n not in seen else torch.maximum(seen[n], a)
            return outs
    gen = torch.Generator().manual_seed(5)
    batches = [torch.randn(2, 3, 64, 64, generator=gen).to(DEV) for _ in range(3)]
    p = LayerwiseEqualizationPass(iterations=1, including_act=True, including_bias=True)
    p.optimize(g, dataloader=batches, executor=Keeping(g, DEV))
    assert len(seen) == 54 and set(p.activations) == set(seen) and p.stats['collect_launches'] == 3
    for n, a in seen.items(): assert _same(p.activations[n], a), n
    assert all(v.value is None for v in g.variables.values() if not v.is_parameter)

    # identical maxima fed to both arms: the passes agree bit for bit
    a, b = (_to_device(harness.resnet50_graph(num_classes=10)) for _ in range(2))
    kw = dict(iterations=2, including_act=True, including_bias=True)
    LayerwiseEqualizationPass(**kw).optimize(a, activations=p.activations)
    LayerwiseEqualizationPass(use_kernels=False, **kw).optimize(b, activations=p.activations)
    for name, v in a.variables.items():
        if v.is_parameter: assert _same(v.value, b.variables[name].value), name


@pytest.mark.parametrize('build,threshold', GRAPHS)
def test_graph_outputs_are_preserved_on_the_device(build, threshold):
    from ppq_amd import harness
    from ppq_amd.equalization import LayerwiseEqualizationPass
    from ppq_amd.measure import torch_snr_error
    g = getattr(harness, build)()
    ex = harness.TorchExecutor(g, DEV)
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(3)).to(DEV)
    before = [y.clone() for y in ex.forward(x)]
    p = LayerwiseEqualizationPass(iterations=10, value_threshold=threshold)
    p.optimize(g, dataloader=[x], executor=ex)
    assert p.stats['scaled_channels'] > 0
    for y0, y1 in zip(before, ex.forward(x)):
        err = float(torch_snr_error(y1, y0))
        print(build, 'snr error', err)
        assert err < SNR_BOUND, (build, err)


def test_pass_then_calibration_runs_end_to_end():
    from ppq_amd import harness
    from ppq_amd import lib as PFL
    from ppq_amd.calibration import RuntimeCalibrationPass
    from ppq_amd.equalization import LayerwiseEqualizationPass
    gen = torch.Generator().manual_seed(0)
    batches = [torch.rand(4, 3, 32, 32, generator=gen).to(DEV) for _ in range(8)]
    for g, expect_pairs in ((harness.small_cnn_graph(), 0), (EC.harness_graph(1), 2)):
        if g.name == 'add_pair': batches = [torch.rand(4, 3, 8, 8, generator=gen).to(DEV) for _ in range(8)]
        harness.quantize_graph(g, 'minmax', per_channel_weight=False)
        ex = harness.TorchExecutor(g, DEV)
        eq = LayerwiseEqualizationPass(iterations=4, including_bias=True, including_act=True)
        PFL.Pipeline([eq, harness.ParameterQuantizePass(), RuntimeCalibrationPass(method='minmax')]).optimize(
            graph=g, dataloader=batches, executor=ex, calib_steps=8, collate_fn=None, verbose=False)
        assert eq.stats['pairs'] == expect_pairs
        for op in g.operations.values():
            for v in op.inputs:
                if v.is_parameter: assert torch.equal(v.stored_value, v.value) or op.type not in ('Conv', 'Gemm')
        assert all(torch.isfinite(y).all() for y in ex.forward(batches[0]))
