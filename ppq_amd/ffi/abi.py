"""The host-side job records: one numpy dtype per ``typedef struct ppqhip_*`` of include/ppq_hip.h, in the header's order, named as there in
``JOB_LAYOUTS``.  tests/test_host_abi_layout.py compiles the header, compares every size and offset, and fails for an unregistered struct."""
import numpy as np

FQ_JOB = np.dtype([('x', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('out', '<u8'), ('n', '<i8'),
                   ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('clip_min', '<i4'), ('clip_max', '<i4')])
LSQ_FINISH_JOB = np.dtype([('partial', '<u8'), ('grad_s', '<u8'), ('n', '<i8'), ('clip_min', '<i4'), ('clip_max', '<i4')])
LSQ_JOB = np.dtype([('x', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('grad_y', '<u8'), ('grad_x', '<u8'), ('grad_s', '<u8'),
                    ('n', '<i8'), ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('clip_min', '<i4'), ('clip_max', '<i4')])
FLOAT_SEARCH_JOB = np.dtype([('x', '<u8'), ('rows', '<i8'), ('row_len', '<i8'), ('exponent', '<i4'), ('mantissa', '<i4'),
                             ('clip_min', '<f4'), ('clip_max', '<f4')])
FQ_FLOAT_JOB = np.dtype([('x', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('out', '<u8'), ('n', '<i8'),
                         ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('exponent', '<i4'), ('mantissa', '<i4'),
                         ('clip_min', '<f4'), ('clip_max', '<f4')])
QUANTILE_JOB = np.dtype([('x', '<u8'), ('dest', '<u8'), ('hint', '<u8'), ('n', '<i8')])
MINMAX_C_JOB = np.dtype([('x', '<u8'), ('mins', '<u8'), ('maxs', '<u8'), ('n', '<i8'), ('num_channel', '<i8'),
                         ('elem_per_channel', '<i8'), ('fresh', '<i4'), ('reserved', '<i4')])
MINMAX_JOB = np.dtype([('x', '<u8'), ('slots', '<u8'), ('n', '<i8')])
HIST_JOB = np.dtype([('x', '<u8'), ('rows', '<u8'), ('n', '<i8'), ('p0', '<f4'), ('p1', '<f4')])
ADAROUND_JOB = np.dtype([('w', '<u8'), ('v', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('out', '<u8'), ('dy', '<u8'),
                         ('n', '<i8'), ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('qmin', '<i4'), ('qmax', '<i4')])
ROUNDTUNE_JOB = np.dtype([('w', '<u8'), ('r', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('out', '<u8'),
                          ('n', '<i8'), ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('qmin', '<i4'), ('qmax', '<i4')])
FETCH_JOB = np.dtype([('x', '<u8'), ('index', '<u8'), ('out', '<u8'), ('rows', '<i8'), ('row_len', '<i8'), ('count', '<i8')])
MEASURE_JOB = np.dtype([('p', '<u8'), ('r', '<u8'), ('index', '<u8'), ('sums', '<u8'), ('rows', '<i8'), ('row_len', '<i8'),
                        ('count', '<i8')])
FINISH_JOB = np.dtype([('sums', '<u8'), ('acc', '<u8'), ('row_out', '<u8'), ('rows', '<i8'), ('count', '<i8'),
                       ('method', '<i4'), ('reduce', '<i4')])
EQ_SEGMENT = np.dtype([('base', '<u8'), ('extent', '<i8'), ('div', '<i8'), ('a', '<i8'), ('b', '<i8'), ('outer', '<i8'),
                       ('stride', '<i8'), ('run', '<i8'), ('multiplier', '<f4'), ('downstream', '<i4')])
EQ_SCALE_JOB = np.dtype([('segments', '<u8'), ('scale', '<u8'), ('num_segments', '<i4'), ('num_channel', '<i4'),
                         ('value_threshold', '<f4'), ('reserved', '<i4')])
EQ_APPLY_JOB = np.dtype([('x', '<u8'), ('scale', '<u8'), ('n', '<i8'), ('run', '<i8'), ('inner', '<i8'), ('group_out', '<i8'),
                         ('num_scale', '<i8'), ('divide', '<i4'), ('reserved', '<i4')])
SPLIT_PLAN_JOB = np.dtype([('segments', '<u8'), ('src_of', '<u8'), ('count', '<u8'), ('num_segments', '<i4'), ('num_channel', '<i4'),
                           ('value_threshold', '<f4'), ('reserved', '<i4')])
SPLIT_APPLY_JOB = np.dtype([('x', '<u8'), ('out', '<u8'), ('src_of', '<u8'), ('n', '<i8'), ('run', '<i8'), ('num_channel', '<i4'),
                            ('count', '<i4')])
SSD_SCALES_JOB = np.dtype([('first', EQ_SEGMENT), ('last', EQ_SEGMENT), ('act_range', '<u8'), ('scales', '<u8'), ('ranges', '<u8'),
                           ('num_channel', '<i4'), ('channel_ratio', '<f4')])
SSD_APPLY_JOB = np.dtype([('x', '<u8'), ('out', '<u8'), ('scales', '<u8'), ('n', '<i8'), ('run', '<i8'), ('inner', '<i8'),
                          ('group_out', '<i8'), ('num_channel', '<i8'), ('divide', '<i4'), ('reserved', '<i4')])
FQ_MEASURE_JOB = np.dtype([('y', '<u8'), ('r', '<u8'), ('scale', '<u8'), ('offset', '<u8'), ('sums', '<u8'), ('rows', '<i8'),
                           ('count', '<i8'), ('num_channel', '<i8'), ('elem_per_channel', '<i8'), ('clip_min', '<i4'),
                           ('clip_max', '<i4'), ('rounding', '<i4'), ('reserved', '<i4')])
STAT_JOB = np.dtype([('p', '<u8'), ('r', '<u8'), ('rec', '<u8'), ('n', '<i8'), ('bins', '<i4'), ('reserved', '<i4')])
MX_JOB = np.dtype([('x', '<u8'), ('y', '<u8'), ('scale_codes', '<u8'), ('outer', '<i8'), ('axis_len', '<i8'), ('inner', '<i8'),
                   ('format', '<i4'), ('reserved', '<i4')])
MX_ROUND_SPLIT_JOB = np.dtype([('w', '<u8'), ('floored', '<u8'), ('rounding', '<u8'), ('scale_codes', '<u8'), ('outer', '<i8'),
                               ('axis_len', '<i8'), ('inner', '<i8'), ('format', '<i4'), ('reserved', '<i4')])
MX_ROUND_FWD_JOB = np.dtype([('floored', '<u8'), ('rounding', '<u8'), ('scale_codes', '<u8'), ('out', '<u8'), ('outer', '<i8'),
                             ('axis_len', '<i8'), ('inner', '<i8'), ('format', '<i4'), ('reserved', '<i4')])
MX_PACK_JOB = np.dtype([('x', '<u8'), ('elements', '<u8'), ('scales', '<u8'), ('outer', '<i8'), ('axis_len', '<i8'), ('inner', '<i8'),
                        ('format', '<i4'), ('reserved', '<i4')])
MX_UNPACK_JOB = np.dtype([('elements', '<u8'), ('scales', '<u8'), ('y', '<u8'), ('outer', '<i8'), ('axis_len', '<i8'), ('inner', '<i8'),
                          ('format', '<i4'), ('reserved', '<i4')])

# C struct name -> record, every ``typedef struct ppqhip_*`` of the header (``ppqhip_prof_entry`` is ``_lib.ProfEntry``)
JOB_LAYOUTS = {
    'ppqhip_fq_job': FQ_JOB, 'ppqhip_lsq_finish_job': LSQ_FINISH_JOB, 'ppqhip_lsq_job': LSQ_JOB,
    'ppqhip_float_search_job': FLOAT_SEARCH_JOB, 'ppqhip_fq_float_job': FQ_FLOAT_JOB, 'ppqhip_quantile_job': QUANTILE_JOB,
    'ppqhip_minmax_c_job': MINMAX_C_JOB, 'ppqhip_minmax_job': MINMAX_JOB, 'ppqhip_hist_job': HIST_JOB,
    'ppqhip_adaround_job': ADAROUND_JOB, 'ppqhip_roundtune_job': ROUNDTUNE_JOB, 'ppqhip_fetch_rows_job': FETCH_JOB,
    'ppqhip_measure_rows_job': MEASURE_JOB, 'ppqhip_measure_finish_job': FINISH_JOB, 'ppqhip_equalize_segment': EQ_SEGMENT,
    'ppqhip_equalize_scale_job': EQ_SCALE_JOB, 'ppqhip_equalize_apply_job': EQ_APPLY_JOB, 'ppqhip_split_plan_job': SPLIT_PLAN_JOB,
    'ppqhip_split_apply_job': SPLIT_APPLY_JOB, 'ppqhip_ssd_scales_job': SSD_SCALES_JOB, 'ppqhip_ssd_apply_job': SSD_APPLY_JOB,
    'ppqhip_fq_measure_rows_job': FQ_MEASURE_JOB, 'ppqhip_stat_job': STAT_JOB, 'ppqhip_mx_job': MX_JOB,
    'ppqhip_mx_round_split_job': MX_ROUND_SPLIT_JOB, 'ppqhip_mx_round_fwd_job': MX_ROUND_FWD_JOB, 'ppqhip_mx_pack_job': MX_PACK_JOB,
    'ppqhip_mx_unpack_job': MX_UNPACK_JOB,
}
