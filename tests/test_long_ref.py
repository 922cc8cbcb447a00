"""The directed long-read inputs and their plain reference (tests/long_ref.py) against the C oracle, without a
GPU: what tests/test_gpu_long_directed.py expects of the device is right, and every input has the property
it was built for."""
import numpy as np
import pytest

import long_ref as R
from oracle import oracle as O


def _main_pair(case):
    """The ranks (lower, higher) of reads r0 / r1 and their lists as (list1, list2)."""
    rk = R.rank_of(case.data())
    a, b = sorted((rk[0], rk[1]))
    lists = R.read_lists(case.data().csr())
    return a, b, lists[a], lists[b]


@pytest.mark.parametrize('overlap', [0.8, 0.5, 0.0, -0.5])
@pytest.mark.parametrize('case', R.CASES, ids=repr)
def test_long_ref_equals_the_oracle(case, overlap):
    """Edges with I and U, forward degrees and components, at both cutoff lists of the input; the cap does not
    bind, so the capped oracle (the reference program's own loop) gives the same.  overlap <= 0, where every
    same-chromosome cell matches, is what the device's general evaluator is held against."""
    csr = case.data().csr()
    for cuts in case.cuts + [[0.3]]:
        want = case.ref(overlap, cuts)
        for use_cap in (False, True):
            o = O.run_core(R.oracle_from_csr(csr), overlap=overlap, cutoffs=cuts, use_cap=use_cap)
            got = sorted(zip(o['edge_a'].tolist(), o['edge_b'].tolist(), o['edge_I'].tolist(), o['edge_U'].tolist()))
            assert got == want.edges
            np.testing.assert_array_equal(o['fwd'], want.fwd)
            np.testing.assert_array_equal(o['comp'], want.comp)
        assert want.fwd.max() <= 10


@pytest.mark.parametrize('case', R.CASES, ids=repr)
def test_input_has_its_length_and_its_pair(case):
    csr = case.data().csr()
    assert int(np.diff(csr.read_off).max()) == case.max_len
    if case.pair is not None:
        a, b, _, _ = _main_pair(case)
        scores = {(x, y): (i, u) for x, y, i, u in R.pair_scores(csr, case.overlap)}
        assert scores[(a, b)] == case.pair


def test_both_outcomes_occur():
    """Over the inputs and their cutoff lists r0 / r1 are an edge in some and none in others, so a wrong I
    or U can show in the edge set; where they are an edge the test of the device compares I and U."""
    seen = {}
    for case in R.CASES:
        if (case.pair is None and not case.gadget) or case.name == 'many_chromosomes':     # 193 / 207: always one
            continue
        a, b, _, _ = _main_pair(case)
        for cuts in case.cuts:
            seen.setdefault(case.name.split('_')[0], set()).add(
                any(e[:2] == (a, b) for e in case.ref(case.overlap, cuts).edges))
    assert all(v == {True, False} for v in seen.values()), seen
    for case in R.CASES:                              # the 4096 inputs and the seam gadgets each show as an edge
        if case.max_len == R.MAX_READ or case.gadget:
            a, b, _, _ = _main_pair(case)
            assert any(e[:2] == (a, b) for e in case.ref(case.overlap, case.cuts[0]).edges), case


def test_diagonal_lengths_and_ranks():
    """(la, lb) are the lengths of the lower and the higher rank."""
    for la, lb in [(64, 65), (65, 64), (1, 65), (65, 1), (4095, 4096)]:
        c = R.CASE[f'diag_{la}_{lb}']
        rk = R.rank_of(c.data())
        L = np.diff(c.data().csr().read_off)
        assert rk[0] < rk[1] and (L[rk[0]], L[rk[1]]) == (la, lb)


@pytest.mark.parametrize('case', [c for c in R.CASES if c.gadget], ids=repr)
def test_gadget_first_fit_is_below_the_maximum(case):
    """A condition on the input: first-fit's I is the maximum matching less one per gadget, in the
    orientation the loop uses (list1 = the lower rank) and in the other one.  First-fit gives the same I in
    both orientations for every pattern up to 4 x 4, so the swapped inputs are about ranks and index
    bookkeeping, not about another I."""
    a, b, l1, l2 = _main_pair(case)
    n_gadgets = len(R.GADGET_PLACES[case.name.replace('_swapped', '')][2])
    cells = R.matching_cells(l1, l2, case.overlap)
    assert R.first_fit(l1, l2, case.overlap) == R.first_fit_cells(cells) == R.max_matching(cells) - n_gadgets
    back = [(j, i) for i, j in cells]
    assert R.first_fit(l2, l1, case.overlap) == R.first_fit_cells(back) == R.first_fit_cells(cells)
    # the read listed first ranks lower: A, which holds the gadget rows r0 and r1, unless swapped
    rk = R.rank_of(case.data())
    assert rk[0] < rk[1]
    la, lb = R.GADGET_PLACES[case.name.replace('_swapped', '')][:2]
    assert (len(l1), len(l2)) == ((lb, la) if case.name.endswith('_swapped') else (la, lb))


def test_gadget_cells_sit_on_the_seams():
    """The named gadget of each input: r0 matches {c0, c1}, r1 matches {c0} alone."""
    for name, (_, _, places) in R.GADGET_PLACES.items():
        _, _, l1, l2 = _main_pair(R.CASE[name])
        cells = set(R.matching_cells(l1, l2, 0.5))
        for r0, r1, c0, c1 in places:
            assert {(i, j) for i, j in cells if i in (r0, r1) or j in (c0, c1)} == {(r0, c0), (r0, c1), (r1, c0)}


def test_first_fit_orientation_brute_force():
    """Every 0/1 pattern up to 4 x 4: first-fit's I does not depend on which list gives the rows."""
    for nr in range(1, 5):
        for nc in range(1, 5):
            for bits in range(1 << (nr * nc)):
                cells = [(k // nc, k % nc) for k in range(nr * nc) if bits >> k & 1]
                assert R.first_fit_cells(cells) == R.first_fit_cells([(j, i) for i, j in cells])


def test_gate_inputs_decide_at_the_boundary():
    for name, want in [('gate_fail', {(0, 2)}), ('gate_equal', {(0, 1), (0, 2), (1, 2)}), ('gate_below', {(1, 2)})]:
        c = R.CASE[name]
        rk = R.rank_of(c.data())
        assert [rk[k] for k in range(3)] == [0, 1, 2]
        scored = {(a, b) for a, b, _, _ in R.pair_scores(c.data().csr(), 0.8) if b < 3}
        assert scored == want
    q = R.GATES['gate_equal']
    assert q[1][0] / q[0][0] >= 1 - R.QLEN_DIFF and not (q[1][0] - 1) / q[0][0] >= 1 - R.QLEN_DIFF
    assert q[2][1] / q[0][1] >= 1 - R.NAL_DIFF and not (q[2][1] - 1) / q[0][1] >= 1 - R.NAL_DIFF


def test_max_matching_small():
    assert R.max_matching([]) == 0
    assert R.max_matching([(0, 0), (0, 1), (1, 0)]) == 2 and R.first_fit_cells([(0, 0), (0, 1), (1, 0)]) == 1
    assert R.max_matching([(0, 0), (1, 0), (2, 0)]) == 1
    assert R.max_matching([(i, j) for i in range(5) for j in range(3)]) == 3
