"""ppqhip_conv1x1 on MI355X against its contract (tests/pointwise_conv_reference.py: the ascending-k float32 fmaf chain from +0,
then `+ bias`), bit for bit: partial tiles in every direction, the K tail, the stride-2 gather, odd planes, both load widths,
special values, position / batch independence, memory left alone around y, HIP-graph replay and the refusals."""
import numpy as np
import pytest
import torch

from ppq_amd import _lib, ffi
from pointwise_conv_reference import conv1x1_float64, conv1x1_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# x, w, stride: what it covers
CASES = [
    ((3, 40, 7, 7), (70, 40), 1),        # P = 49 odd, unaligned rows, partial tiles in Co and P, K tail (40 = 32 + 8)
    ((2, 64, 14, 14), (256, 64), 1),     # several tiles in both directions, 16-byte loads
    ((2, 72, 14, 14), (96, 72), 2),      # stride-2 gather, K tail
    ((2, 64, 9, 5), (33, 64), 2),        # odd H and W, 5 x 3 out
    ((1, 2048, 7, 7), (8, 2048), 1),     # the longest chain of the network
    ((2, 64, 56, 56), (64, 64), 1),      # many tiles along P: the tile a pixel lands in must not matter
    ((2, 37, 5, 5), (130, 37), 1),       # c the K step (32) does not divide and no multiple of 4: dword loads with a K tail
    ((1, 36, 4, 4), (5, 36), 1),         # 16-byte loads WITH a K tail (c % 4 == 0, c % 32 != 0), a single partial tile
    ((2, 31, 8, 8), (64, 31), 1),        # c below one K step
]


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)).view(np.int32)


def _operands(case, seed):
    xs, ws, stride = case
    g = torch.Generator().manual_seed(seed)
    return torch.randn(xs, generator=g), torch.randn(ws, generator=g), torch.randn(ws[0], generator=g), stride


@pytest.fixture(scope='module')
def references():
    """case index -> (x, w, bias, stride, reference without bias, reference with bias); computed once, never written to."""
    out = {}
    for k, case in enumerate(CASES):
        x, w, b, stride = _operands(case, k)
        out[k] = (x, w, b, stride, conv1x1_reference(x.numpy(), w.numpy(), None, stride), conv1x1_reference(x.numpy(), w.numpy(), b.numpy(), stride))
    return out


@pytest.mark.parametrize('k', range(len(CASES)))
@pytest.mark.parametrize('with_bias', [False, True])
def test_bits_equal_the_contract(references, k, with_bias):
    x, w, b, stride, want0, want1 = references[k]
    want = want1 if with_bias else want0
    wd = w.to(DEV).view(*w.shape, 1, 1) if k % 2 else w.to(DEV)                       # [O, C, 1, 1] and [O, C]
    y = ffi.conv1x1(x.to(DEV), wd, b.to(DEV) if with_bias else None, stride)
    assert tuple(y.shape) == want.shape and y.is_contiguous()
    assert np.array_equal(_bits(y), want.view(np.int32)), int((_bits(y) != want.view(np.int32)).sum())
    again = ffi.conv1x1(x.to(DEV), wd, b.to(DEV) if with_bias else None, stride)      # a second launch repeats the bits
    assert np.array_equal(_bits(again), _bits(y))


def test_small_integers_are_exact_in_any_order():
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-8, 9, (2, 100, 6, 10), generator=g).float()
    w = torch.randint(-8, 9, (40, 100), generator=g).float()
    for stride in (1, 2):
        want, _ = conv1x1_float64(x.numpy(), w.numpy(), stride)
        y = ffi.conv1x1(x.to(DEV), w.to(DEV), None, stride)
        assert torch.equal(y.cpu().double(), torch.from_numpy(want))


def test_position_and_batch_independence(references):
    for k in (0, 2, 5):
        x, w, b, stride, _, want = references[k]
        xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
        whole = ffi.conv1x1(xd, wd, bd, stride)
        for n in range(x.shape[0]):
            one = ffi.conv1x1(xd[n:n + 1].contiguous(), wd, bd, stride)
            assert np.array_equal(_bits(one), _bits(whole[n:n + 1])), (k, n)
    # the same column of x everywhere: every pixel of a plane, in whatever tile it lands, carries the same bits
    g = torch.Generator().manual_seed(5)
    col, w = torch.randn(1, 64, 1, 1, generator=g), torch.randn(96, 64, generator=g)
    y = ffi.conv1x1(col.expand(3, 64, 20, 20).contiguous().to(DEV), w.to(DEV), None, 1)
    assert (_bits(y) == _bits(y)[0:1, :, 0:1, 0:1]).all()


def test_memory_around_y_is_left_alone(monkeypatch):
    x, w, b, stride = _operands(CASES[0], 3)
    n_out = 3 * 70 * 49
    buf = torch.full((n_out + 512,), 1234.5, device=DEV)
    y = buf[256:256 + n_out].view(3, 70, 7, 7)
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: y)                            # ffi.conv1x1 writes where we can see the borders
    out = ffi.conv1x1(x.to(DEV), w.to(DEV), b.to(DEV), stride)
    monkeypatch.undo()
    assert out.data_ptr() == y.data_ptr()
    assert (buf[:256] == 1234.5).all() and (buf[256 + n_out:] == 1234.5).all()
    assert np.array_equal(_bits(y), conv1x1_reference(x.numpy(), w.numpy(), b.numpy(), stride).view(np.int32))


def test_one_nan_poisons_exactly_its_column():
    x, w, _, _ = _operands(CASES[1], 4)
    x[1, 17, 3, 5] = float('nan')
    y = ffi.conv1x1(x.to(DEV), w.to(DEV), None, 1).cpu()
    bad = torch.isnan(y)
    want = torch.zeros_like(bad)
    want[1, :, 3, 5] = True
    assert torch.equal(bad, want)


def test_infinities_subnormals_and_signed_zeros_follow_the_chain():
    g = torch.Generator().manual_seed(6)
    x, w = torch.randn(2, 44, 6, 6, generator=g), torch.randn(50, 44, generator=g)
    x[0, 3, 1, 1], x[0, 9, 2, 2], x[1, 5, 0, 0] = float('inf'), float('-inf'), float('inf')
    w[7, 5] = 0.0                                                                     # 0 * inf: NaN in exactly y[1, 7, 0, 0]
    x[1, :, 4, 4] = torch.randn(44, generator=g) * 1e-30                              # products far below the subnormal range ...
    w[20:30] *= 1e-12                                                                 # ... and sums inside it
    x[1, :, 5, 5] = 1e-30; w[40] = -1e-30                                             # every product underflows to -0: the K tail must keep -0
    b = torch.randn(50, generator=g) * 1e-38
    for bias in (None, b):
        want = conv1x1_reference(x.numpy(), w.numpy(), None if bias is None else bias.numpy(), 1)
        got = ffi.conv1x1(x.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV), 1).cpu().numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and nan[1, 7, 0, 0]
        assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])
    assert want.shape == (2, 50, 6, 6) and conv1x1_reference(x.numpy(), w.numpy())[1, 40, 5, 5].view(np.int32) == np.int32(-2 ** 31)


def test_graph_replay_repeats_the_eager_bits(references):
    x, w, b, stride, _, want = references[2]
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    eager = ffi.conv1x1(xd, wd, bd, stride)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side): ffi.conv1x1(xd, wd, bd, stride)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side): y = ffi.conv1x1(xd, wd, bd, stride)
    for _ in range(2):
        y.fill_(-7.0)
        graph.replay(); torch.cuda.synchronize()
        assert np.array_equal(_bits(y), _bits(eager)) and np.array_equal(_bits(y), want.view(np.int32))


def test_refusals_launch_nothing():
    x, w = torch.randn(2, 8, 4, 4, device=DEV), torch.randn(6, 8, device=DEV)
    y = torch.full((2, 6, 4, 4), -3.0, device=DEV)
    lib, s = _lib.lib, torch.cuda.current_stream().cuda_stream
    assert lib.ppqhip_conv1x1(x.data_ptr(), w.data_ptr(), 0, y.data_ptr(), 2, 8, 4, 4, 6, 3, s) == -2
    assert lib.ppqhip_conv1x1(x.data_ptr(), w.data_ptr(), 0, x.data_ptr() + 64, 2, 8, 4, 4, 6, 1, s) == -1
    assert _lib.last_error() == 'conv1x1: an output overlaps an input'
    assert lib.ppqhip_conv1x1(x.data_ptr(), w.data_ptr(), 0, y.data_ptr(), 0, 8, 4, 4, 6, 1, s) == 0
    assert lib.ppqhip_conv1x1(x.data_ptr() + 2, w.data_ptr(), 0, y.data_ptr(), 1, 8, 4, 4, 6, 1, s) == _lib.NOT_FUSED
    assert lib.ppqhip_conv1x1(x.data_ptr(), w.data_ptr(), 0, 0, 2, 8, 4, 4, 6, 1, s) == -1
    torch.cuda.synchronize()
    assert (y == -3.0).all()
    with pytest.raises(RuntimeError, match='stride must be 1 or 2'): ffi.conv1x1(x, w, None, 3)
    with pytest.raises(RuntimeError, match='contiguous NCHW'): ffi.conv1x1(x.contiguous(memory_format=torch.channels_last), w, None, 1)
