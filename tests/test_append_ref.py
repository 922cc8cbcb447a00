"""The numpy statement of fslr_append_reads' merged data order (append_ref) against a stable argsort of
resident-then-new starts: with ties inside and across the lists, at empty sides, and as the CSR of a union."""
import numpy as np
import pytest

import append_ref as ar
import match_ref as mr


def check(a, b):
    a, b = np.sort(np.asarray(a, np.int64)), np.sort(np.asarray(b, np.int64))
    pos_res, pos_new = ar.merged_positions(a, b)
    order = np.argsort(np.concatenate([a, b]), kind='stable')        # merged position -> source element
    want = np.empty(order.size, np.int64)
    want[order] = np.arange(order.size)
    np.testing.assert_array_equal(pos_res, want[:a.size])
    np.testing.assert_array_equal(pos_new, want[a.size:])
    both = np.concatenate([pos_res, pos_new])
    assert sorted(both.tolist()) == list(range(a.size + b.size))     # a permutation
    return pos_res, pos_new


@pytest.mark.parametrize('seed', range(4))
def test_merged_order_is_the_stable_argsort(seed):
    rng = np.random.default_rng(seed)
    check(rng.integers(0, 10 ** 6, 3000), rng.integers(0, 10 ** 6, 400))


@pytest.mark.parametrize('values', [1, 2, 8])
def test_ties_inside_and_across_the_lists(values):
    rng = np.random.default_rng(values)
    pos_res, pos_new = check(rng.integers(0, values, 500), rng.integers(0, values, 300))
    if values == 1:                                                  # one run: every resident element first
        np.testing.assert_array_equal(pos_res, np.arange(500))
        np.testing.assert_array_equal(pos_new, 500 + np.arange(300))


def test_empty_sides():
    pos_res, pos_new = check([], [3, 3, 5])
    assert pos_res.size == 0 and pos_new.tolist() == [0, 1, 2]
    pos_res, pos_new = check([1, 2, 2], [])
    assert pos_new.size == 0 and pos_res.tolist() == [0, 1, 2]
    check([], [])


def test_indexes_that_do_not_append_say_so():
    from fslr_amd import cluster
    data = mr.resident_data([[(1, 5, 60, 55)], [(1, 7, 66, 59)]], [1000, 1000], [3, 3])
    with pytest.raises(NotImplementedError, match='multi-GPU index .* does not append'):
        cluster.MultiGpuIndex(data, 2).append(data)
    rows = cluster.RowsIndex.__new__(cluster.RowsIndex)               # (its constructor needs a device)
    with pytest.raises(NotImplementedError, match='fslr_set_reads_rows.* does not append'):
        rows.append(data)


def test_concat_csr_is_the_csr_of_the_union():
    """The concatenated CSR keeps the resident rows, bases the new rows behind them, and its data_pos sorts
    the union by start with the resident interval first on ties."""
    rng = np.random.default_rng(5)
    reads = [[(int(c), int(s), int(s) + 50, 50) for c, s in zip(rng.integers(1, 3, L), rng.integers(0, 40, L))]
             for L in rng.integers(1, 6, 60)]
    res = mr.resident_data(reads[:45], np.full(45, 1000), np.full(45, 3), shuffle_seed=1).csr()
    new = mr.resident_data(reads[45:], np.full(15, 1000), np.full(15, 3), shuffle_seed=2).csr()
    u = ar.concat_csr(res, new)
    assert u.n_reads == 60 and u.n_intervals == res.n_intervals + new.n_intervals
    np.testing.assert_array_equal(u.read_off[:46], res.read_off)
    np.testing.assert_array_equal(np.diff(u.read_off)[45:], np.diff(new.read_off))
    assert sorted(u.data_pos.tolist()) == list(range(u.n_intervals))
    by_pos = np.empty(u.n_intervals, np.int64)
    by_pos[u.data_pos] = np.arange(u.n_intervals)                    # data position -> CSR interval
    s = u.iv_start[by_pos]
    assert (np.diff(s) >= 0).all()
    tie = np.flatnonzero(np.diff(s) == 0)
    is_new = by_pos >= res.n_intervals
    assert tie.size > 20 and not (is_new[tie] & ~is_new[tie + 1]).any()      # never new before resident in a run
    # inside either list the order is the list's own
    for sel, own in ((~is_new, res.data_pos), (is_new, new.data_pos)):
        k = by_pos[sel] - (res.n_intervals if sel is is_new else 0)
        np.testing.assert_array_equal(np.asarray(own)[k], np.arange(k.size))
