"""Host test of what the convolution epilogue entry points refuse (csrc/epilogue.hip: run_epilogue): every case below is turned
away on the host, before anything touches the device, so the pointers are host addresses that are never dereferenced.  The
table pins the status, the text of ``ppqhip_last_error()`` and, where two refusals apply, which one wins -- as the eleven entry
points gave them when each did its own checks.  ``None`` for the text: PPQHIP_NOT_FUSED sets none (the previous one stays)."""
import numpy as np
import pytest

from ppq_amd import _lib

INVALID, NOT_FUSED = -1, 1

_SINGLE = 'y bias n C epc relu'
_RESID = 'a bias_a b bias_b out n C epc relu'
_POOL = 'y bias pool n C H W relu kernel stride pad dilation ceil_mode'
_ROWS3 = ' rows_a p0_a p1_a rows_b p0_b p1_b rows_out p0_out p1_out bins asym clip'
PARAMS = {name: names.split() for name, names in {
    'bias_act': _SINGLE,
    'bias_add_act': _RESID,
    'bias_act_stats': _SINGLE + ' slots_y',
    'bias_add_act_stats': _RESID + ' slots_a slots_b slots_out',
    'bias_add_act_stats2': _RESID + ' slots_a slots_b slots_out elide',
    'bias_act_hist': _SINGLE + ' rows_y p0_y p1_y bins asym clip',
    'bias_add_act_hist': _RESID + _ROWS3 + ' elide',
    'bias_act_pool': _POOL,
    'bias_act_pool_stats': _POOL + ' slots_y store_relu',
    'bias_act_pool_hist': _POOL + ' rows_y p0_y p1_y bins asym clip store_relu',
}.items()}
POINTERS = ('y', 'bias', 'pool', 'a', 'bias_a', 'b', 'bias_b', 'out', 'slots_y', 'slots_a', 'slots_b', 'slots_out',
            'rows_y', 'rows_a', 'rows_b', 'rows_out')
# What a call is made of unless its case says otherwise: a fusable 2^21-element tensor [512, 8 channels, 512] (pooled:
# 16 x 16 planes under a 3 / 2 / 1 window), a distinct 16-B aligned address per pointer, ReLU, 2048 symmetric bins.
DEFAULTS = dict(n=1 << 21, C=8, epc=512, relu=1, elide=0, bins=2048, asym=0, clip=1, H=16, W=16, kernel=3, stride=2, pad=1,
                dilation=1, ceil_mode=0, store_relu=1, p0_y=0.01, p1_y=0.0, p0_a=0.01, p1_a=0.0, p0_b=0.01, p1_b=0.0,
                p0_out=0.01, p1_out=0.0)
G = 'n=%d is not [outer, %d channels, %d elem/channel]'
NULL, NEEDS_SINK = 'null pointer', 'a tensor that is not stored needs a sink'
B_SINK, BINS = 'without bias_b, b is only read: it has no sink', 'histogram is empty or too large'

# (entry point, what differs from DEFAULTS -- 'x+4': pointer x four bytes on, 'x=y': pointer x is pointer y -- , status, text)
CASES = [
    # bad geometry
    ('bias_act', dict(n=0), INVALID, 'n=0 is empty or has more than 2^31 - 1 elements'),
    ('bias_add_act_hist', dict(n=0), INVALID, 'n=0 is empty or has more than 2^31 - 1 elements'),
    ('bias_act_pool', dict(n=0), INVALID, 'n=0 is empty or has more than 2^31 - 1 elements'),
    ('bias_add_act', dict(n=12, C=5, epc=2), INVALID, G % (12, 5, 2)),
    ('bias_add_act_stats2', dict(n=12, C=5, epc=2), INVALID, G % (12, 5, 2)),
    ('bias_act_hist', dict(n=12, C=5, epc=2), INVALID, G % (12, 5, 2)),
    ('bias_act_pool_stats', dict(n=12, C=5, H=2, W=1), INVALID, G % (12, 5, 2)),
    # a null operand
    ('bias_act', dict(bias=None), INVALID, NULL),
    ('bias_add_act', dict(out=None), INVALID, NULL),
    ('bias_act_stats', dict(y=None), INVALID, NULL),
    ('bias_add_act_stats', dict(b=None), INVALID, NULL),
    ('bias_act_hist', dict(bias=None), INVALID, NULL),
    ('bias_add_act_hist', dict(a=None), INVALID, NULL),
    ('bias_act_pool', dict(pool=None), INVALID, NULL),
    ('bias_act_pool_hist', dict(bias=None), INVALID, NULL),
    # a sink for b without bias_b
    ('bias_add_act_stats', dict(bias_b=None), INVALID, B_SINK),
    ('bias_add_act_stats2', dict(bias_b=None), INVALID, B_SINK),
    ('bias_add_act_hist', dict(bias_b=None), INVALID, B_SINK),
    # elide
    ('bias_add_act_stats2', dict(elide=4), INVALID, 'elide has unknown bits'),
    ('bias_add_act_hist', dict(elide=4), INVALID, 'elide has unknown bits'),
    ('bias_add_act_stats2', dict(elide=1, slots_a=None), INVALID, NEEDS_SINK),
    ('bias_add_act_hist', dict(elide=1, rows_a=None), INVALID, NEEDS_SINK),
    ('bias_add_act_stats2', dict(elide=2, slots_b=None), INVALID, NEEDS_SINK),
    ('bias_add_act_stats2', dict(elide=2, bias_b=None), INVALID, B_SINK),
    ('bias_add_act_hist', dict(elide=2, bias_b=None), INVALID, B_SINK),
    ('bias_add_act_stats2', dict(elide=2, bias_b=None, slots_b=None), INVALID, NEEDS_SINK),
    # histogram
    ('bias_act_hist', dict(bins=0), INVALID, BINS),
    ('bias_add_act_hist', dict(bins=1 << 31), INVALID, BINS),
    ('bias_act_pool_hist', dict(bins=-1), INVALID, BINS),
    ('bias_act_hist', dict(bins=6145), NOT_FUSED, None),
    ('bias_add_act_hist', dict(bins=6145), NOT_FUSED, None),
    ('bias_add_act_hist', dict(bins=2049), NOT_FUSED, None),                      # three sinks: 6147 counters
    ('bias_act_pool_hist', dict(bins=6145), NOT_FUSED, None),
    ('bias_add_act_hist', {'rows_b=rows_a': 1}, INVALID, 'two sinks share one rows accumulator'),
    ('bias_add_act_hist', {'rows_out=rows_a': 1}, INVALID, 'two sinks share one rows accumulator'),
    ('bias_add_act_hist', {'rows_out=rows_b': 1}, INVALID, 'two sinks share one rows accumulator'),
    # nothing is wrong, nothing is launched
    ('bias_act_stats', dict(slots_y=None), NOT_FUSED, None),
    ('bias_add_act_stats', dict(slots_a=None, slots_b=None, slots_out=None), NOT_FUSED, None),
    ('bias_act_hist', dict(rows_y=None), NOT_FUSED, None),
    ('bias_add_act_hist', dict(rows_a=None, rows_b=None, rows_out=None), NOT_FUSED, None),
    ('bias_act_stats', {'y+4': 1}, NOT_FUSED, None),
    ('bias_add_act_stats', {'b+4': 1}, NOT_FUSED, None),
    ('bias_add_act_stats2', {'out+4': 1}, NOT_FUSED, None),
    ('bias_act_hist', {'y+4': 1}, NOT_FUSED, None),
    ('bias_add_act_hist', {'a+4': 1}, NOT_FUSED, None),
    ('bias_act_stats', dict(n=2, C=1, epc=1), NOT_FUSED, None),
    ('bias_add_act_stats', dict(n=3, C=3, epc=1), NOT_FUSED, None),
    ('bias_act_hist', dict(n=1 << 20), NOT_FUSED, None),
    ('bias_add_act_hist', dict(n=1 << 20), NOT_FUSED, None),
    ('bias_act_hist', dict(relu=0), NOT_FUSED, None),
    ('bias_add_act_hist', dict(relu=0), NOT_FUSED, None),
    # the pooled form
    ('bias_act_pool', dict(H=0), INVALID, 'the plane 0 x 16 is empty or too large'),
    ('bias_act_pool_stats', dict(W=1 << 31), INVALID, 'the plane 16 x 2147483648 is empty or too large'),
    ('bias_act_pool_hist', dict(H=1 << 16, W=1 << 16), INVALID, 'the plane 65536 x 65536 is empty or too large'),
    ('bias_act_pool', dict(kernel=4), NOT_FUSED, None),
    ('bias_act_pool_stats', dict(kernel=4), NOT_FUSED, None),
    ('bias_act_pool', dict(dilation=2), NOT_FUSED, None),
    ('bias_act_pool_hist', dict(dilation=2), NOT_FUSED, None),
    ('bias_act_pool', dict(ceil_mode=1), NOT_FUSED, None),
    ('bias_act_pool', dict(pad=2), NOT_FUSED, None),
    ('bias_act_pool', dict(stride=0), NOT_FUSED, None),
    ('bias_act_pool', dict(H=7, W=9, n=8 * 63), NOT_FUSED, None),                   # 63 % 4 != 0
    ('bias_act_pool', dict(H=128, W=128), NOT_FUSED, None),                         # 64 KB: no room for the staging lines
    ('bias_act_pool_stats', dict(H=128, W=128), NOT_FUSED, None),
    ('bias_act_pool_hist', dict(H=120, W=120, n=8 * 14400 * 4), NOT_FUSED, None),   # fits without the 2048 counters only
    ('bias_act_pool', {'y+4': 1}, NOT_FUSED, None),
    ('bias_act_pool_stats', {'pool+4': 1}, NOT_FUSED, None),
    ('bias_act_pool_stats', dict(store_relu=0, slots_y=None), INVALID, NEEDS_SINK),
    ('bias_act_pool_hist', dict(store_relu=0, rows_y=None), INVALID, NEEDS_SINK),
    ('bias_act_pool_stats', dict(slots_y=None), NOT_FUSED, None),
    ('bias_act_pool_hist', dict(rows_y=None), NOT_FUSED, None),
    ('bias_act_pool_hist', dict(relu=0), NOT_FUSED, None),
    # two refusals at once: which one wins
    ('bias_add_act', dict(n=12, C=5, epc=2, a=None), INVALID, G % (12, 5, 2)),
    ('bias_act_pool', dict(n=12, C=5, H=2, W=1, pool=None), INVALID, G % (12, 5, 2)),
    ('bias_act_pool', dict(n=0, H=0), INVALID, 'the plane 0 x 16 is empty or too large'),
    ('bias_act_hist', dict(n=12, C=5, epc=2, bins=0), INVALID, G % (12, 5, 2)),
    ('bias_act_hist', dict(y=None, bins=0), INVALID, NULL),
    ('bias_act_pool_hist', dict(bins=0, store_relu=0, rows_y=None), INVALID, BINS),
    ('bias_add_act_hist', dict(elide=4, bins=6145), INVALID, 'elide has unknown bits'),
    ('bias_add_act_hist', dict(elide=4, bins=0), INVALID, BINS),
    ('bias_add_act_hist', dict(bias_b=None, bins=0), INVALID, B_SINK),
    ('bias_add_act_hist', {'rows_b=rows_a': 1, 'elide': 4}, INVALID, 'elide has unknown bits'),
    ('bias_add_act_hist', {'rows_b=rows_a': 1, 'bins': 6145}, INVALID, 'two sinks share one rows accumulator'),
    ('bias_add_act_stats2', dict(elide=1, slots_a=None, slots_b=None, slots_out=None), INVALID, NEEDS_SINK),
    ('bias_act_pool_stats', dict(store_relu=0, slots_y=None, kernel=4), INVALID, NEEDS_SINK),
]


def _call(entry, over):
    """(status, text or None) of one refused call; the text None when the call left the sentinel error in place."""
    lib = _lib.lib
    buf = np.zeros(64 * len(POINTERS) + 16, np.uint8)
    base = (buf.ctypes.data + 15) & ~15
    values = dict(DEFAULTS, **{name: base + 64 * k for k, name in enumerate(POINTERS)})
    for key, v in over.items():
        if key.endswith('+4'): values[key[:-2]] += 4
        elif '=' in key: values[key.split('=')[0]] = values[key.split('=')[1]]
        else: values[key] = v
    assert lib.ppqhip_bias_act(None, None, -7, 1, 1, 0, None) == INVALID         # the sentinel: a text no case gives
    sentinel = _lib.last_error()
    assert sentinel.startswith('bias_act: n=-7 ')
    status = getattr(lib, 'ppqhip_' + entry)(*[values[name] for name in PARAMS[entry]], None)
    text = _lib.last_error()
    return status, (None if text == sentinel else text)


def test_the_table_covers_every_entry_point():
    assert {entry for entry, *_ in CASES} == set(PARAMS)
    for entry, names in PARAMS.items():                                          # (the stream is the last argument)
        assert len(names) + 1 == len(_lib.PROTOTYPES['ppqhip_' + entry][1]), entry


@pytest.mark.parametrize('case', range(len(CASES)), ids=lambda k: f'{CASES[k][0]}-{k}')
def test_refusal(case):
    entry, over, status, text = CASES[case]
    assert status in (INVALID, NOT_FUSED)                                        # a table of refusals: none may reach a launch
    assert _call(entry, over) == (status, None if text is None else f'{entry}: {text}')
