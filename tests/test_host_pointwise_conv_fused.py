"""Host test of what ppqhip_conv1x1_epilogue (csrc/pointwise_conv.hip) turns away: every case below ends on the host, before
anything touches the device, so the operands are small host buffers that are never dereferenced.  The table pins the status, the
text of ``ppqhip_last_error()`` and, where two refusals apply, which one wins: the order of the checks in the entry point.  ``None``
for the text: PPQHIP_NOT_FUSED and PPQHIP_OK set none.  `out` is filled with a sentinel before every call and must still hold it."""
import numpy as np
import pytest

from ppq_amd import _lib

OK, INVALID, UNSUPPORTED, NOT_FUSED = 0, -1, -2, 1
NONE, MINMAX, HIST = 0, 1, 2
PARAMS = ('x w bias_a resid bias_b out n c h wd o stride relu sink_kind dst_a dst_r dst_out p0_a p1_a p0_r p1_r p0_out p1_out '
          'bins asym clip max_workgroups').split()
POINTERS = ('x', 'w', 'bias_a', 'resid', 'bias_b', 'out', 'dst_a', 'dst_r', 'dst_out')
# What a call is made of unless its case says otherwise: the P2b form on [1, 4, 2, 2] -> [1, 4, 2, 2] with three min/max sinks
DEFAULTS = dict(n=1, c=4, h=2, wd=2, o=4, stride=1, relu=1, sink_kind=MINMAX, p0_a=0.01, p1_a=0.0, p0_r=0.01, p1_r=0.0, p0_out=0.01,
                p1_out=0.0, bins=2048, asym=0, clip=1, max_workgroups=0)
P1 = dict(resid=None, bias_b=None, dst_a=None, dst_r=None)
SIZE, NULL, BINS = 'non-positive size', 'null pointer', 'histogram is empty or too large'
SHARED, OVERLAP = 'two sinks share one accumulator', 'an output overlaps an input'
R_SINK, B_SINK = 'without a residual only out has a sink', 'without bias_b, the residual is only read: it has no sink'
LARGE = 'more than 2^31 - 1 elements in x, w or out'

# (what differs from DEFAULTS -- 'x+1': pointer x one byte on, 'x=y': pointer x is pointer y -- , status, text)
CASES = [
    (dict(c=0), INVALID, SIZE), (dict(n=-1), INVALID, SIZE), (dict(o=0), INVALID, SIZE), (dict(h=0), INVALID, SIZE),
    (dict(stride=3), UNSUPPORTED, 'stride must be 1 or 2'), (dict(stride=0), UNSUPPORTED, 'stride must be 1 or 2'),
    (dict(max_workgroups=-1), INVALID, 'max_workgroups is negative'),
    (dict(sink_kind=3), INVALID, 'unknown sink kind'), (dict(sink_kind=-1), INVALID, 'unknown sink kind'),
    (dict(n=0), OK, None), (dict(n=0, x=None), OK, None),
    (dict(x=None), INVALID, NULL), (dict(w=None), INVALID, NULL), (dict(bias_a=None), INVALID, NULL), (dict(out=None), INVALID, NULL),
    (dict(resid=None, dst_a=None, dst_r=None), INVALID, 'bias_b without a residual'),
    (dict(n=1 << 20, c=1 << 12, h=1, wd=1), INVALID, LARGE), (dict(o=1 << 20, c=1 << 12), INVALID, LARGE),
    (dict(P1, dst_a=1), INVALID, R_SINK), (dict(P1, dst_r=1), INVALID, R_SINK),
    (dict(bias_b=None), INVALID, B_SINK),
    (dict(sink_kind=HIST, bins=0), INVALID, BINS), (dict(sink_kind=HIST, bins=1 << 31), INVALID, BINS),
    (dict(sink_kind=HIST, bins=-1), INVALID, BINS), (dict(P1, sink_kind=HIST, bins=0), INVALID, BINS),
    ({'dst_r=dst_a': 1}, INVALID, SHARED), ({'dst_out=dst_a': 1}, INVALID, SHARED), ({'dst_out=dst_r': 1}, INVALID, SHARED),
    ({'out=x': 1}, INVALID, OVERLAP), ({'out=resid': 1}, INVALID, OVERLAP), ({'out=bias_b': 1}, INVALID, OVERLAP),
    ({'out=w': 1}, INVALID, OVERLAP),
    # nothing is wrong, nothing is launched
    ({'x+1': 1}, NOT_FUSED, None), ({'w+1': 1}, NOT_FUSED, None), ({'bias_a+1': 1}, NOT_FUSED, None), ({'resid+1': 1}, NOT_FUSED, None),
    ({'bias_b+1': 1}, NOT_FUSED, None), ({'out+1': 1}, NOT_FUSED, None),
    (dict(sink_kind=NONE), NOT_FUSED, None), (dict(dst_a=None, dst_r=None, dst_out=None), NOT_FUSED, None),
    (dict(P1, dst_out=None), NOT_FUSED, None),
    (dict(sink_kind=HIST, bins=2049), NOT_FUSED, None),                        # three sinks: 6147 counters
    (dict(P1, sink_kind=HIST, bins=6145), NOT_FUSED, None),
    # two refusals at once: which one wins
    (dict(c=0, stride=3), INVALID, SIZE), (dict(stride=3, x=None), UNSUPPORTED, 'stride must be 1 or 2'),
    (dict(sink_kind=3, x=None), INVALID, 'unknown sink kind'), (dict(n=0, sink_kind=3), INVALID, 'unknown sink kind'),
    (dict(x=None, bias_b=None), INVALID, NULL), (dict(n=1 << 20, c=1 << 12, h=1, wd=1, bias_b=None), INVALID, LARGE),
    (dict(P1, dst_a=1, sink_kind=HIST, bins=0), INVALID, R_SINK), (dict(bias_b=None, sink_kind=HIST, bins=0), INVALID, B_SINK),
    ({'dst_r=dst_a': 1, 'sink_kind': HIST, 'bins': 0}, INVALID, BINS), ({'dst_r=dst_a': 1, 'out=x': 1}, INVALID, SHARED),
    ({'out=x': 1, 'w+1': 1}, INVALID, OVERLAP), ({'dst_r=dst_a': 1, 'sink_kind': HIST, 'bins': 2049}, INVALID, SHARED),
    ({'x+1': 1, 'sink_kind': NONE}, NOT_FUSED, None),
]
SENTINEL = np.float32(-12345.5)


def _call(over):
    """(status, text or None, whether `out` still holds its sentinel) of one call that must not reach a launch."""
    lib = _lib.lib
    bufs = {name: np.zeros(64 + 4, np.float32) for name in POINTERS}           # [1, 4, 2, 2] operands and room to step one byte on
    bufs['out'][:] = SENTINEL
    values = dict(DEFAULTS, **{name: b.ctypes.data for name, b in bufs.items()})
    for key, v in over.items():
        if key.endswith('+1'): values[key[:-2]] += 1
        elif '=' in key: values[key.split('=')[0]] = values[key.split('=')[1]]
        elif key in POINTERS and v is not None: pass                              # (1: keep the default address)
        else: values[key] = v
    assert lib.ppqhip_bias_act(None, None, -7, 1, 1, 0, None) == INVALID         # the sentinel: a text no case gives
    sentinel = _lib.last_error()
    assert sentinel.startswith('bias_act: n=-7 ')
    status = lib.ppqhip_conv1x1_epilogue(*[values[name] for name in PARAMS], None)
    text = _lib.last_error()
    return status, (None if text == sentinel else text), bool((bufs['out'] == SENTINEL).all())


def test_the_prototype_matches():
    assert len(PARAMS) + 1 == len(_lib.PROTOTYPES['ppqhip_conv1x1_epilogue'][1])   # (the stream is the last argument)


@pytest.mark.parametrize('case', range(len(CASES)), ids=lambda k: f'{k}-{"-".join(CASES[k][0])}'[:60])
def test_refusal(case):
    over, status, text = CASES[case]
    assert status != OK or over.get('n') == 0                                    # a table of refusals: none may reach a launch
    assert _call(over) == (status, None if text is None else f'conv1x1_epilogue: {text}', True)
