"""The weight-layout rules of the kernel arms, pinned: ``equalization.pair_jobs``, ``ssd.pair_geometry`` and
``channel_split.split_tensors`` return exactly the tuples recorded in tests/golden/pair_geometry.json (written by
tests/golden/make_pair_geometry.py before the three became compositions of ``equalization.endpoint_layout``)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import pair_geometry_cases as PG  # noqa: E402


def _book():
    with open(os.path.join(HERE, 'golden', 'pair_geometry.json')) as f: return json.load(f)


def _segments(book):
    for recs in list(book['equalization'].values()) + list(book['channel_split'].values()):
        for rec in recs: yield from rec['pair_jobs'][0][2]


def test_recorded_pairs_cover_every_layout_branch():
    """Gemm with transB 0 and 1 on both sides, a MatMul downstream, a grouped downstream Conv whose two key orders differ, a
    depthwise Conv, a biased upstream operation (bias and activation segments with their multipliers) and SSD's None."""
    book = _book()
    eq = {(n, tuple(r['up']), tuple(r['down'])): r for n, recs in book['equalization'].items() for r in recs}
    ssd = {(n, tuple(r['ops'])): r['pair_geometry'] for n, recs in book['ssd'].items() for r in recs}
    col, row = [1, 1, 0], [1]                                     # (div, a, b) of a column channel; div of a row channel
    gemm = {(tuple(r['up']), tuple(r['down'])): r['pair_jobs'][0][2] for (n, *_), r in eq.items() if n == 'gemm'}
    assert gemm[('fc1',), ('fc2',)][0][1:3] == [1, 10] and gemm[('fc2',), ('fc3',)][0][1:4] == col          # upstream transB 1, 0
    assert gemm[('fc1',), ('fc2',)][-1][1:3] == [1, 12] and gemm[('fc2',), ('fc3',)][-1][1:4] == col        # downstream transB 0, 1
    assert eq['gemm_0_to_1', ('fc1',), ('fc2',)]['split_tensors'] == [[{'var': 'fc1_w', 'shape': [5, 8]}, 1], [{'var': 'fc1_b', 'shape': [8]}, 0],
                                                                      [{'var': 'fc2_w', 'shape': [6, 8]}, 1]]
    mm = eq['matmul_down', ('fc1',), ('mm',)]
    assert mm['pair_jobs'][0][2][-1] == [{'var': 'mm_w', 'shape': [8, 3]}, 1, 3, 0, 1, 0, 3, 1.0, True] and mm['split_tensors'][-1][1] == 0
    assert [s[7] for s in mm['pair_jobs'][0][2]] == [1.0, PG.BIAS_MULTIPLIER, PG.ACT_MULTIPLIER, 1.0]       # weight, bias, activation, weight
    g2 = {'var': 'g2_w', 'shape': [12, 4, 3, 3]}
    assert eq['grouped', ('dw',), ('g2',)]['pair_jobs'][0][2][-1] == [g2, 2, 9, 216, 6, 36, 9, 1.0, True]   # (cin_local, group) rows
    assert ssd['depthwise', ('dw', 'r2', 'g2')][2] == [g2, 4, 216, 9, 6, 36, 9]                             # (group, cin_local) rows
    assert eq['grouped', ('c1',), ('dw',)]['pair_jobs'][1][-1] == [{'var': 'dw_w', 'shape': [8, 1, 3, 3]}, {'var': 'scale', 'shape': [8]}, 9, 1, 1, True]
    assert 'split_tensors' not in eq['grouped', ('dw',), ('g2',)]
    assert ssd['flat', ('c1', 'r1', 'gap', 'fc')] is not None and ssd['flat_wide', ('c1', 'r1', 'gap', 'fc')] is None
    assert ssd['gemm_0_to_1', ('fc1', 'fc2')][1][1:4] == col and ssd['gemm_0_to_1', ('fc1', 'fc2')][2][1:4] == col
    assert ssd['gemm', ('fc1', 'r1', 'fc2')][1][1:2] == row and ssd['gemm', ('fc1', 'r1', 'fc2')][2][1:2] == row
    assert any(s[8] for s in _segments(book)) and any(not s[8] for s in _segments(book))


def test_the_three_functions_return_the_recorded_tuples():
    want, got = _book(), json.loads(json.dumps(PG.record()))
    assert sorted(got) == sorted(want)
    for arm in want:
        assert sorted(got[arm]) == sorted(want[arm]), arm
        for name in want[arm]: assert got[arm][name] == want[arm][name], (arm, name)
