"""tests/containment_ref.py, the plain statement of fslr_cluster_path_containment, on hand-worked cases (no device).
Tokens are t = locus * 2 + rev; rows are written in their canonical direction, as fslr_cluster_paths stores them."""
import numpy as np

import containment_ref as cr


def run(*clusters):
    res = cr.containment(cr.paths_of_rows([list(c) for c in clusters]))
    for k in cr.NAMES:
        assert res[k].dtype == cr.DTYPES[k], k
    return res


def pairs_of(res):
    inner = np.repeat(np.arange(len(res['coff']) - 1), np.diff(res['coff'])).tolist()
    return list(zip(inner, res['outer'].tolist(), res['offset'].tolist(), res['rev'].tolist(), res['n_occ'].tolist()))


def test_three_chains_in_a_five_chain_at_offset_0_in_the_middle_and_at_the_end():
    # ascending rows: 0 = (0,2,4), 1 = (0,2,4,6,8), 2 = (2,4,6), 3 = (4,6,8)
    res = run([((0, 2, 4, 6, 8), 10), ((0, 2, 4), 1), ((2, 4, 6), 2), ((4, 6, 8), 3)])
    assert pairs_of(res) == [(0, 1, 0, 0, 1), (2, 1, 1, 0, 1), (3, 1, 2, 0, 1)]
    assert res['coff'].tolist() == [0, 1, 1, 2, 3]
    assert res['n_inner'].tolist() == [0, 3, 0, 0] and res['support'].tolist() == [1, 16, 2, 3]
    assert res['collapse_to'].tolist() == [1, 1, 1, 1] and res['collapsed_reads'].tolist() == [0, 16, 0, 0]


def test_the_reverse_direction():
    # rc((4,6,8)) = (9,7,5) lies in (0,2,9,7,5) at offset 2; (4,6,8) itself does not
    res = run([((0, 2, 9, 7, 5), 4), ((4, 6, 8), 1)])
    assert pairs_of(res) == [(1, 0, 2, 1, 1)]
    assert res['support'].tolist() == [5, 1] and res['collapse_to'].tolist() == [0, 0]


def test_forward_and_reverse_occurrences_of_one_pair_the_smaller_offset_wins():
    # (4,6) forward at offset 3, its reverse complement (7,5) at offset 1
    res = run([((0, 7, 5, 4, 6), 1), ((4, 6), 1)])
    assert pairs_of(res) == [(1, 0, 1, 1, 2)]
    res = run([((0, 4, 6, 7, 5), 1), ((4, 6), 1)])
    assert pairs_of(res) == [(1, 0, 1, 0, 2)]


def test_a_palindromic_inner_is_not_counted_twice():
    # (2,3): reversed and flipped it is (3 ^ 1, 2 ^ 1) = (2,3) again
    assert tuple(t ^ 1 for t in reversed((2, 3))) == (2, 3)
    res = run([((0, 2, 3, 6), 1), ((2, 3), 1)])
    assert pairs_of(res) == [(1, 0, 1, 0, 1)]


def test_a_repeated_token_gives_three_occurrences():
    res = run([((2, 4, 2, 6, 2), 2), ((2,), 5)])
    assert pairs_of(res) == [(0, 1, 0, 0, 3)]
    assert res['support'].tolist() == [5, 7] and res['n_inner'].tolist() == [0, 1]


def test_equal_lengths_are_never_contained():
    res = run([((0, 2, 4), 1), ((0, 2, 6), 1), ((2, 4, 6), 3)])
    assert pairs_of(res) == [] and res['coff'].tolist() == [0, 0, 0, 0]
    assert res['collapse_to'].tolist() == [0, 1, 2] and res['collapsed_reads'].tolist() == [1, 1, 3]
    assert res['support'].tolist() == [1, 1, 3]


def test_three_nested_rows_transitivity_and_collapse_skips_the_middle_one():
    # ascending rows: 0 = (0,2,4), 1 = (0,2,4,6), 2 = (2,4)
    res = run([((2, 4), 7), ((0, 2, 4), 5), ((0, 2, 4, 6), 1)])
    assert pairs_of(res) == [(0, 1, 0, 0, 1), (2, 0, 1, 0, 1), (2, 1, 1, 0, 1)]
    assert res['support'].tolist() == [12, 13, 7] and res['n_inner'].tolist() == [1, 2, 0]
    # the middle row has the larger n_reads, but it is contained itself: (2,4) collapses to the full-length row
    assert res['collapse_to'].tolist() == [1, 1, 1] and res['collapsed_reads'].tolist() == [0, 13, 0]


def test_a_tie_on_support_goes_to_the_smaller_row():
    # ascending rows: 0 = (0,4), 1 = (2,4), 2 = (4,)
    res = run([((0, 4), 3), ((2, 4), 3), ((4,), 2)])
    assert res['support'].tolist() == [5, 5, 2] and res['collapse_to'].tolist() == [0, 1, 0]
    assert res['collapsed_reads'].tolist() == [5, 3, 0]
    res = run([((0, 4), 3), ((2, 4), 4), ((4,), 2)])
    assert res['collapse_to'].tolist() == [0, 1, 1] and res['collapsed_reads'].tolist() == [3, 6, 0]


def test_two_clusters_of_the_same_shapes_never_pair_across():
    # (the device's tokens differ between clusters; the statement does not rely on that)
    one = [((0, 2), 1), ((0, 2, 4), 2)]
    res = run(one, one)
    assert pairs_of(res) == [(0, 1, 0, 0, 1), (2, 3, 0, 0, 1)]
    assert res['collapsed_reads'].tolist() == [0, 3, 0, 3] and res['collapse_to'].tolist() == [1, 1, 3, 3]


def test_no_rows():
    res = run()
    assert res['coff'].tolist() == [0] and all(res[k].size == 0 for k in cr.NAMES[1:])
