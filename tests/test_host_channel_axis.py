"""Host test of the shared (n, num_channel, elem_per_channel) validator (csrc/channel_axis.hpp): the entry points that take this
geometry refuse a bad one on the host, before anything is launched, with the same two messages -- `job k:` in front for the
job tables (AdaRound, round tuning), nothing in front for the convolution epilogues."""
import numpy as np

from ppq_amd import _lib, ffi

INVALID_VALUE = -1


def test_bad_geometry_is_refused_with_the_same_messages_everywhere():
    lib = _lib.lib
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data                                                          # never dereferenced: every call is refused

    def epilogue(n, C, epc):
        return [(lib.ppqhip_bias_act(p, p, n, C, epc, 1, None), _lib.last_error()),
                (lib.ppqhip_bias_add_act(p, p, p, None, p, n, C, epc, 1, None), _lib.last_error()),
                (lib.ppqhip_bias_act_stats(p, p, n, C, epc, 1, p, None), _lib.last_error()),
                (lib.ppqhip_bias_add_act_stats(p, p, p, None, p, n, C, epc, 1, p, None, p, None), _lib.last_error())]

    def tables(n, C, epc):
        """The bad geometry in job 1, behind a good job 0."""
        out = []
        for dtype, call in ((ffi._ROUNDTUNE_JOB, lambda t: lib.ppqhip_roundtune_fwd_multi(t, 2, None)),
                            (ffi._ADAROUND_JOB, lambda t: lib.ppqhip_adaround_fwd_multi(t, 2, None)),
                            (ffi._ADAROUND_JOB, lambda t: lib.ppqhip_adaround_bwd_multi(t, 2, p, None))):
            jobs = np.zeros(2, dtype=dtype)
            for name in dtype.names[:dtype.names.index('n')]: jobs[name] = p
            jobs['qmin'], jobs['qmax'] = -8, 7
            jobs['n'], jobs['num_channel'], jobs['elem_per_channel'] = (12, n), (3, C), (2, epc)
            out.append((call(jobs.ctypes.data), _lib.last_error()))
        return out

    names = ['bias_act', 'bias_add_act', 'bias_act_stats', 'bias_add_act_stats']
    tnames = ['roundtune_fwd_multi', 'adaround_fwd_multi', 'adaround_bwd_multi']
    for n in (0, -4, 1 << 31):
        text = f'n={n} is empty or has more than 2^31 - 1 elements'
        assert epilogue(n, 1, 1) == [(INVALID_VALUE, f'{w}: {text}') for w in names]
        assert tables(n, 1, 1) == [(INVALID_VALUE, f'{w}: job 1: {text}') for w in tnames]
    for n, C, epc in ((12, 5, 2), (12, 0, 2), (12, 3, 0), (12, -3, 2), (12, 1 << 31, 1), (12, 1, 1 << 31), (1 << 20, 1 << 40, 1 << 40)):
        text = f'n={n} is not [outer, {C} channels, {epc} elem/channel]'
        assert epilogue(n, C, epc) == [(INVALID_VALUE, f'{w}: {text}') for w in names]
        assert tables(n, C, epc) == [(INVALID_VALUE, f'{w}: job 1: {text}') for w in tnames]
