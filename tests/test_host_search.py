"""CPU only: pins the references of the clipping-search tests to each other, and checks the conditions tests/test_gpu_search.py relies
on, so that its comparisons cannot pass vacuously.

Three statements of the KL search meet here: tests/search_reference.py's ``kl_contract`` (the arithmetic search.hip documents: exact
sums rounded to float32 once), its bin-by-bin twin ``kl_contract_scalar`` (must be bit-equal) and ``oracle.kl_search`` (the
reference's float32 tensors summed in NumPy's order).

The contract and the oracle differ only in the ORDER of float32 sums.  Over the 153 cases below (9 histogram families x 17 (bins,
bits)) the worst |oracle - contract| measured here is 4.174e-7 (huge-2048-b2); it is recorded as search_reference.ORACLE_ABS_MEASURED
= 4.18e-7, and the bound a kernel test may use against the oracle is 4 x that, 1.672e-6: the reference's own torch reductions are a
third float32 order, and the factor covers it.  Both numbers come from these two CPU references; no kernel result went into them.

Ambiguity: tol_j = 2^-38 * A_j (unit round-off 2^-53, at most 2^14 terms in any order, a few ulp from each log10; derived, not
measured).  A case is ambiguous when more than one candidate lies within 2 * tol of the contract's minimum, unless those candidates
are exact zeros whose every term vanishes identically (p_i == 0 or p_i == q_i as float32: `zero` with A_j == 0, and `spike`, where p
== q holds but log10(p) != 0) -- those are 0.0 in any order, and the first must win.  With the seeds of search_reference no case is
ambiguous; AMBIGUOUS names them, and the test holds the list to what the references say."""
import numpy as np
import pytest

import search_reference as R
from oracle import ppq_oracle as O

AMBIGUOUS = ()                      # kl_case_id()s whose arg-min another summation order may move; admissible = the near-minimum set
assert AMBIGUOUS == R.KL_AMBIGUOUS  # the copy tests/test_gpu_search.py reads


@pytest.fixture(scope='module')
def kl_table():
    """id -> (bins, bits, family, contract losses, A, Z, oracle losses, oracle's best bin_range); computed once, never modified."""
    table = {}
    for bins, bits in R.KL_CASES:
        for family in R.KL_FAMILIES:
            hist = R.histogram(family, bins)
            losses, A, Z = R.kl_contract_detail(hist, bits)
            with np.errstate(all='ignore'):
                _, _, records, best = O.kl_search(hist, R.HIST_SCALE, bits, False, return_losses=True)
            assert [r['bin_range'] for r in records] == [(j + 1) << (bits - 1) for j in range(losses.size)]
            for a in (losses, A, Z): a.setflags(write=False)
            table[R.kl_case_id(bins, bits, family)] = (bins, bits, family, losses, A, Z, np.array([r['kl'] for r in records]), best)
    return table


@pytest.fixture(scope='module')
def mse_table():
    """(bins, qmin, qmax, symmetric, row name) -> (start, end, step, cell, losses, cells) of the oracle's first minimum."""
    table = {}
    for bins, qmin, qmax, families, modes in R.MSE_CASES:
        for mode in modes:
            for name, hist, hs, mn in R.mse_rows(bins, families, mode == 's'):
                table[(bins, qmin, qmax, mode == 's', name)] = R.mse_first_minimum(O, hist, hs, mn, qmin, qmax, mode == 's')
    return table


def test_histogram_families_are_what_they_claim():
    for bins in sorted({b for b, _ in R.KL_CASES}):
        hs = {f: R.histogram(f, bins) for f in R.KL_FAMILIES}
        assert all(h.dtype == np.int32 and h.shape == (bins,) and h.min() >= 0 for h in hs.values())
        assert np.count_nonzero(hs['spike']) == 1 and hs['spike'][bins // 3] > 0
        assert np.flatnonzero(hs['ends']).tolist() == [0, bins - 1]
        assert not hs['zero'].any() and np.all(hs['flat'] == hs['flat'][0]) and hs['flat'][0] > 0
        assert hs['huge'][0] == R.INT32_MAX and np.all(np.diff(hs['huge'].astype(np.int64)) <= 0)
        assert bins / 20 <= np.count_nonzero(hs['sparse']) <= bins / 16 + 1
        assert hs['relu_hot'][0] >= hs['relu_hot'][1:].sum()
        assert hs['longtail'][-1] == 3 and not hs['longtail'][int(bins * 1500 / 2048):-1].any()
        assert np.array_equal(hs['halfnormal'], R.histogram('halfnormal', bins))          # seeded
    assert np.all(R.histogram('huge', 96, mse=True) == R.INT32_MAX)


def test_longtail_is_the_golden_histogram_at_2048(golden_dir):
    import os
    z = np.load(os.path.join(golden_dir, 'observers.npz'))
    assert np.array_equal(R.histogram('longtail', 2048), z[f'kl_{int(z["kl_n"]) - 1}_hist'])


def test_case_lists():
    assert len(R.KL_CASES) == 17 and {b for _, b in R.KL_CASES} == {2, 3, 4, 5, 6, 7, 8, 11}
    assert all(bins % (1 << (bits - 1)) == 0 and bins <= 16384 for bins, bits in R.KL_CASES)
    assert (64, -128, 127) in [c[:3] for c in R.MSE_CASES]
    for bins, qmin, qmax, families, modes in R.MSE_CASES:
        levels = qmax - qmin + 1
        if (bins, qmin, qmax) == (2048, 0, 15):       # grid-stride path: more cells than 64 workgroups of 256 lanes
            assert 1 + ((bins + 7) // 8) * (bins // levels) > 64 * 256 and modes == 'a' and families == ('normal', 'spike')
        if bins == 16384: assert modes == 's' and families == ('normal',)
    for bins in (64, 512):                            # several starts stay valid under the negative min_value
        mn = R.mse_min_values(bins)[0]
        assert sum((s * R.HIST_SCALE) + mn <= 0 for s in range(0, bins, R.MSE_INTERVAL)) >= 5
    assert (296 * R.HIST_SCALE) + R.mse_min_values(512)[0] == 0.0          # a start exactly on the `> 0` boundary (range.py:477)


def test_scalar_and_vector_contract_are_bit_equal():
    for bins, bits in ((128, 2), (128, 5), (128, 8), (192, 4), (192, 7)):
        for family in R.KL_FAMILIES:
            hist = R.histogram(family, bins)
            vector, scalar = R.kl_contract(hist, bits)[0], R.kl_contract_scalar(hist, bits)
            assert np.array_equal(vector.view(np.uint64), scalar.view(np.uint64)), (bins, bits, family)


def test_single_rounding_of_the_sums_matters():
    """Teeth of the bit-equality above: in some case q_sum and hist_sum are NOT float32 values before their one rounding, so a
    restatement that skipped it (or rounded partial sums) would compute other bits."""
    hist = R.histogram('huge', 128)
    hf = R._edited(hist).astype(np.float64)
    assert float(np.float32(hf.sum())) != hf.sum()
    g = hf[:128].reshape(64, 2)
    qg = (g.sum(axis=1).astype(np.float32) / np.float32(2)).astype(np.float64)
    assert float(np.float32(2 * qg.sum())) != 2 * qg.sum()


def test_contract_against_oracle(kl_table):
    worst, worst_id = 0.0, None
    for cid, (bins, bits, family, losses, A, Z, want, best) in kl_table.items():
        assert np.array_equal(np.isnan(losses), np.isnan(want)), cid
        assert not np.isinf(losses).any() and not np.isinf(want).any(), cid
        finite = np.isfinite(want)
        delta = float(np.max(np.abs(losses[finite] - want[finite]))) if finite.any() else 0.0
        if delta > worst: worst, worst_id = delta, cid
        assert delta <= R.ORACLE_ABS_BOUND, (cid, delta)
        if not R.kl_ambiguous(losses, A, Z):
            assert R.pick(losses, 1 << (bits - 1)) == best, cid
    print(f'worst |oracle - contract| = {worst:.4e} at {worst_id}; recorded {R.ORACLE_ABS_MEASURED:.3e}, '
          f'bound {R.ORACLE_ABS_FACTOR} x = {R.ORACLE_ABS_BOUND:.3e}')
    # NumPy's float32 summation order depends on the CPU's vector width, so the worst case is held to the bound (every case, above) and
    # the record to being neither stale nor loose, not to one figure
    assert R.ORACLE_ABS_MEASURED / 4 <= worst <= R.ORACLE_ABS_BOUND, (worst, worst_id)
    assert R.ORACLE_ABS_BOUND == 4 * R.ORACLE_ABS_MEASURED


def test_ambiguous_cases_are_the_named_ones(kl_table):
    found = []
    for cid, (bins, bits, family, losses, A, Z, want, best) in kl_table.items():
        near = R.kl_near_minimum(losses, A)
        if R.kl_ambiguous(losses, A, Z):
            found.append(cid)
        elif near.size > 1:                           # identically-zero ties: the first candidate must win, in both references
            assert np.all(losses[near] == 0.0) and np.all(Z[near]), cid
            if not np.isnan(losses).any():
                first = (int(near[0]) + 1) << (bits - 1)
                assert R.pick(losses, 1 << (bits - 1)) == first == best, cid
        assert np.all(A[Z] >= 0) and np.all(losses[Z] == 0.0), cid
    assert sorted(found) == sorted(AMBIGUOUS)
    assert len(found) * 10 <= len(kl_table)
    assert any(cid.startswith('spike-') for cid, c in kl_table.items() if R.kl_near_minimum(c[3], c[4]).size > 1)
    assert any(cid.startswith('zero-') and np.all(c[4] == 0) for cid, c in kl_table.items())


def test_pick_is_the_first_minimum_and_python_sort_on_nan():
    assert R.pick([3.0, 1.0, 2.0, 1.0], 4) == 8                           # first of the tied minima
    assert R.pick([0.0, 0.0, 0.0], 2) == 2
    nan = float('nan')
    assert R.pick([nan, nan, 5.0, 1.0], 2) == 2                           # the reference's sorted() leaves a leading NaN in front
    assert R.pick([5.0, nan, 1.0], 2) == sorted([(5.0, 2), (nan, 4), (1.0, 6)], key=lambda t: t[0])[0][1]


def test_kl_teeth(kl_table):
    with_nan = [cid for cid, c in kl_table.items() if np.isnan(c[3]).any()]
    assert with_nan and all(cid.endswith('-2048-b2') for cid in with_nan)
    for cid in with_nan:                                                  # int(2048 * .002) = 4 >= bin_range 2, 4: q_sum == 0
        bins, bits, family, losses, A, Z, want, best = kl_table[cid]
        assert np.flatnonzero(np.isnan(losses)).tolist() == [0, 1]
        assert best == 2 == R.pick(losses, 2)                             # and the reference's sort returns the NaN candidate
    # losses small enough that a relative tolerance says nothing (the reason the oracle comparison is absolute)
    assert any(0 < np.nanmin(np.abs(c[3][c[3] != 0])) < 1e-3 for c in kl_table.values() if np.any(c[3] != 0))
    # bits 11 fills the kernel's 1024 per-group slots
    assert any(bits == 11 for _, bits in R.KL_CASES)


def test_mse_teeth(mse_table):
    tied_far = all_nan = single = s_zero = 0
    for (bins, qmin, qmax, sym, name), (start, end, step, cell, losses, cells) in mse_table.items():
        levels = qmax - qmin + 1
        assert cells[0] == 0 and len(set(cells.tolist())) == cells.size and np.all(np.diff(cells) > 0)   # enumeration order == cell order
        if np.isnan(losses).all():
            all_nan += 1
            assert (start, end, step, cell) == (0, levels * (bins // levels + 1), bins // levels + 1, 0)
        else:
            assert not np.isnan(losses).any()
            ties = np.flatnonzero(losses == losses.min())
            assert cell == cells[ties[0]]                                 # the first minimum
            if ties.size >= 5 and cells[ties[-1]] - cells[ties[0]] > 256: tied_far += 1
        if losses.size == 1: single += 1
        if bins < levels:
            s_zero += 1
            assert (start, end, step, cell) == (0, levels, 1, 0) and losses.size == 1
    assert tied_far >= 1 and all_nan >= 1 and single >= 1 and s_zero >= 1
    assert O.mse_candidates(64, .1, -3.2, -128, 127, True) == [(0, 1, 256)]
