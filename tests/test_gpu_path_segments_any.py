"""Path segments for reads of more than 64 intervals (fslr_cluster_path_segments_any) against tests/segments_ref.py on
the real CSR, which states the contract for lists of any length (tests/test_segments_any_ref.py pins it beyond 64).
Hand-built inputs of a handful of reads; all nine columns are compared exactly, dtypes included.  The golden fixture
with long reads goes through the wrapper and the command line."""
import os

import numpy as np
import pytest

import chain_any_cases as cc
import fixtures as fx
import segments_ref as sg
from fslr_amd import _lib, cluster
from test_gpu_loci import fixture_membership, query, run_cli
from test_gpu_path_segments import HEADER, blob, expected_lines, get_rows, resident_equals, same

pytestmark = pytest.mark.gpu

STATE = f'fslr error {_lib.FSLR_ERR_STATE}'
INVALID = f'fslr error {_lib.FSLR_ERR_INVALID}'
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
LENS = (64, 65, 128, 129, 1000, 4096, 3, 2, 1, 70, 17)
ALONE = 9                                            # the read of 70 intervals


def device(c, qkey, qend=None, rev=None, labels=None, loci=True, paths=True):
    if labels is not None:
        c.cluster_table(labels)
    if loci:
        c.cluster_loci()
    if paths:
        c.cluster_paths_any(qkey, rev)
    return dict(zip(sg.NAMES, c.cluster_path_segments_any(qkey, qend)))


def check(idx, labels, qkey, qend=None, rev=None):
    p, want = sg.segments_of_csr(idx.csr, labels, qkey, qend, rev)
    same(device(idx.ctx, qkey, qend, rev, labels), want)
    last = np.asarray(p['tok_off'][1:], np.int64) - 1                     # the last slot of every row holds no gap
    assert not any(want[k][last].any() for k in sg.NAMES[6:])
    return p, want


def ends_near(qkey, rng):
    return np.clip(qkey.astype(np.int64) + rng.integers(-30, 30, qkey.size), I32_MIN, I32_MAX).astype(np.int32)


@pytest.fixture(scope='module')
def mixed():
    """One cluster of all of LENS but the read of 70 intervals."""
    c = _lib.Context(0)
    idx = cc.index_of_lens(c, LENS, seed=5)
    yield idx, cc.one_cluster(idx.csr, alone=(ALONE,))
    c.close()


# ------------------------------------------------------------------ 1. lengths and key orders
@pytest.mark.parametrize('with_qend', [True, False])
@pytest.mark.parametrize('mode', cc.KEY_MODES)
def test_lengths_in_one_cluster_under_every_key_order(mixed, mode, with_qend):
    idx, lab = mixed
    csr = idx.csr
    assert idx.long is not None and idx.ctx.n_reads > csr.n_reads
    rng = np.random.default_rng(len(mode))
    key = cc.keys_of(csr, mode)
    rev = (rng.integers(0, 2, csr.n_intervals).astype(np.uint8), None)[mode == 'equal']
    p, want = check(idx, lab, key, ends_near(key, rng) if with_qend else None, rev)
    alone = cc.rank_of_walk(csr, ALONE)
    assert p['path_of_read'][alone] == -1 and (np.delete(p['path_of_read'], alone) >= 0).all()
    assert sorted(np.diff(p['tok_off']).tolist()) == sorted(n for k, n in enumerate(LENS) if k != ALONE)
    assert len(want['start_med']) == sum(LENS) - LENS[ALONE]
    assert any(want[k].any() for k in sg.NAMES[6:]) == with_qend


# ------------------------------------------------------------------ 2. gaps
def test_gaps_at_the_seam_at_the_last_link_and_saturated_both_ways(mixed):
    """Keys j - 60: the chain is the list order, the keys are negative up to position 59.  The gap of link j is
    (j + 1 - 60) - qend[j]: -4 by default; 101 at the chunk seam (63 -> 64); 7 at the last link of every read;
    -49 - INT32_MAX, saturated to INT32_MIN, at link 10 and 11 - INT32_MIN, saturated to INT32_MAX, at link 70."""
    idx, lab = mixed
    csr = idx.csr
    j = cc.place(csr).astype(np.int64)
    length = np.repeat(np.diff(np.asarray(csr.read_off, np.int64)), np.diff(np.asarray(csr.read_off, np.int64)))
    key = j - 60
    qend = key + 5
    qend[j == 63] = 64 - 60 - 101
    qend[j == length - 2] = length[j == length - 2] - 1 - 60 - 7
    qend[j == 10] = I32_MAX
    qend[j == 70] = I32_MIN
    p, want = check(idx, lab, key.astype(np.int32), qend.astype(np.int32))
    for place, n in enumerate(LENS):
        if place == ALONE:
            continue
        r = cc.rank_of_walk(csr, place)
        base, flipped = int(p['tok_off'][p['path_of_read'][r]]), bool(p['flipped'][r])
        gap = lambda link: {int(want[k][base + (n - 2 - link if flipped else link)]) for k in sg.NAMES[6:]}
        assert {int(want[k][base + n - 1]) for k in sg.NAMES[6:]} == {0}          # the last slot, of 4096 too
        if n >= 2:
            assert gap(n - 2) == {7}
        if n > 65:                                                                # (at 65 the seam is the last link)
            assert gap(63) == {101}
        if n > 72:
            assert gap(10) == {I32_MIN} and gap(70) == {I32_MAX} and gap(20) == {-4}
    assert (want['gap_min'] == I32_MIN).any() and (want['gap_max'] == I32_MAX).any()


# ------------------------------------------------------------------ 3. rows of k equal long walks
def walk_of(rng, n):
    """n pieces, locus 0 forward first and loci >= 2 behind it: canonical as it stands."""
    return [(0, 0)] + [(int(a), int(v)) for a, v in zip(rng.integers(2, 8, n - 1), rng.integers(0, 2, n - 1))]


@pytest.fixture(scope='module')
def rows_of_walks():
    """One cluster: a walk of 65 pieces 17 times, another twice, a third once, and a short walk of 5 pieces 3 times."""
    rng = np.random.default_rng(31)
    a, b, d, s = walk_of(rng, 65), walk_of(rng, 65), walk_of(rng, 65), walk_of(rng, 5)
    walks = [a] * 17 + [b] * 2 + [d] + [s] * 3
    c = _lib.Context(0)
    idx, key, rev = cc.index_of_walks(c, walks)
    qend = (key.astype(np.int64) + rng.integers(-40, 40, key.size)).astype(np.int32)
    lab = np.zeros(len(walks), np.int32)
    yield idx, key, qend, rev, lab
    c.close()


def test_rows_of_one_two_and_seventeen_long_reads_under_moved_seams(rows_of_walks, monkeypatch):
    idx, key, qend, rev, lab = rows_of_walks
    monkeypatch.delenv('FSLR_SEGS_SMALL', raising=False)
    monkeypatch.delenv('FSLR_SEGS_LDS', raising=False)
    p, want = check(idx, lab, key, qend, rev)
    assert sorted(zip(p['n_reads'].tolist(), np.diff(p['tok_off']).tolist())) == [(1, 65), (2, 65), (3, 5), (17, 65)]
    assert (want['gap_min'] < want['gap_med']).any() and (want['gap_med'] < want['gap_max']).any()
    blobs = [blob(want)]
    # (1, 2): the row of 2 goes to the LDS tier, those of 3 and 17 to the select tier; (4, 8): 17 to the select tier
    for small, lds in (('1', '2'), ('4', '8')):
        monkeypatch.setenv('FSLR_SEGS_SMALL', small)
        monkeypatch.setenv('FSLR_SEGS_LDS', lds)
        got = device(idx.ctx, key, qend, loci=False, paths=False)
        same(got, want)
        blobs.append(blob(got))
    assert all(b == blobs[0] for b in blobs)


# ------------------------------------------------------------------ 4. flipped reads
def test_a_long_read_and_its_reverse_complement_leave_the_same_gap_on_every_link():
    """Walks: W (65 pieces), W from the other strand, and a palindrome of 80 pieces twice.  qend is made so that both
    W reads leave g(t) on link t of the row, the one that walks it backwards too."""
    rng = np.random.default_rng(40)
    W = walk_of(rng, 65)
    other = [(a, 1 - v) for a, v in reversed(W)]
    X = walk_of(rng, 40)
    pal = X + [(a, 1 - v) for a, v in reversed(X)]
    c = _lib.Context(0)
    try:
        idx, key, rev = cc.index_of_walks(c, [W, other, pal, list(pal)])
        csr = idx.csr
        walk = np.repeat(np.asarray(csr.read_qcode), np.diff(csr.read_off))
        g = lambda t: (t * 37) % 101 - 50
        t = key.astype(np.int64)                                          # the piece's place in its own walk
        qend = t + 3
        qend[walk == 0] = (t + 1 - g(t))[walk == 0]                       # link t of the row
        qend[walk == 1] = (t + 1 - g(63 - t))[walk == 1]                  # its link u lies at link 63 - u of the row
        lab = np.zeros(4, np.int32)
        p, want = check(idx, lab, key, qend.astype(np.int32), rev)
        r = [cc.rank_of_walk(csr, k) for k in range(4)]
        row = p['path_of_read']
        assert row[r[0]] == row[r[1]] and p['flipped'][r[0]] == 0 and p['flipped'][r[1]] == 1
        base = int(p['tok_off'][row[r[0]]])
        links = [g(x) for x in range(64)]
        for k in sg.NAMES[6:]:
            assert want[k][base:base + 64].tolist() == links and want[k][base + 64] == 0, k
        # the palindrome (80 pieces, two reads on its row) is not flipped
        assert row[r[2]] == row[r[3]] != row[r[0]] and p['flipped'][r[2]] == p['flipped'][r[3]] == 0
        assert int(p['tok_off'][row[r[2]] + 1] - p['tok_off'][row[r[2]]]) == 80
    finally:
        c.close()


# ------------------------------------------------------------------ 5. the shape of the clusters
def test_short_and_long_rows_together_unclustered_reads_and_no_clusters(mixed):
    idx, _ = mixed
    csr, n = idx.csr, idx.csr.n_reads
    rng = np.random.default_rng(9)
    key = cc.keys_of(csr, 'shuffled')
    qend = ends_near(key, rng)
    # clusters of three consecutive ranks, the last two reads alone
    lab = cc.groups_of(n, 3)
    lab[9:] = np.arange(9, n)
    p, _ = check(idx, lab, key, qend)
    assert (p['path_of_read'] == -1).sum() == n - 9 and len(p['off']) == 4
    # a cluster of short reads only: the workgroup kernel has nothing to do
    lab = np.arange(n, dtype=np.int32)
    short = [cc.rank_of_walk(csr, k) for k in (0, 6, 7, 8, 10)]          # 64, 3, 2, 1 and 17 intervals
    lab[short] = min(short)
    p, want = check(idx, lab, key, qend)
    assert len(want['start_med']) == 64 + 3 + 2 + 1 + 17
    # no clusters at all: zero tokens, and the getter succeeds
    got = device(idx.ctx, key, qend, None, np.arange(n, dtype=np.int32))
    assert all(got[k].shape == (0,) and got[k].dtype == np.int32 for k in sg.NAMES)
    assert idx.ctx._L.fslr_get_cluster_path_segments(idx.ctx._h, None, None, None, 0) == _lib.FSLR_OK


# ------------------------------------------------------------------ 6. contexts without long reads
def test_without_long_reads_the_bytes_are_the_plain_call_s():
    data, csr, cid, nc, kw = fixture_membership('cfg1_1k_x3')
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is None
        c = idx.ctx
        rng = np.random.default_rng(2)
        key, rev = rng.integers(-50, 50, csr.n_intervals).astype(np.int32), rng.integers(0, 2, csr.n_intervals).astype(np.uint8)
        qend = ends_near(key, rng)
        cluster.cluster_table(query(idx, data, kw), ctx=c)
        c.cluster_loci()
        c.cluster_paths(key, rev)
        plain = dict(zip(sg.NAMES, c.cluster_path_segments(key, qend)))
        assert len(plain['start_med']) > 10 and plain['gap_med'].any()
        got = dict(zip(sg.NAMES, c.cluster_path_segments_any(key, qend)))
        same(got, plain)
        resident_equals(c, plain)                                     # through the getter, after the _any call
        assert blob(got) == blob(plain)
        after = dict(zip(sg.NAMES, c.cluster_path_segments(key, qend)))         # the plain call still works
        assert blob(after) == blob(plain)
        n = csr.n_intervals
        a = idx.cluster_path_segments(np.arange(n), np.arange(n) + 3, None)
        b = idx.cluster_path_segments_any(np.arange(n), np.arange(n) + 3, None)
        assert b.paths is a.paths                                     # the resident path rows are reused
        assert [x.tobytes() for x in a.columns()] == [x.tobytes() for x in b.columns()]
    finally:
        idx.ctx.close()


# ------------------------------------------------------------------ 7. state
def test_state_failed_calls_keep_the_rows_and_a_stale_table_after_remove_any():
    c = _lib.Context(0, profiling=True)
    try:
        idx = cc.index_of_lens(c, (130, 5, 66, 2), seed=8)
        csr, n = idx.csr, idx.csr.n_reads
        rng = np.random.default_rng(6)
        key = cc.keys_of(csr, 'shuffled')
        qend = ends_near(key, rng)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*no cluster table'):
            c.cluster_path_segments_any(key, qend)
        lab = np.zeros(n, np.int32)
        c.cluster_table(lab)
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_loci first'):
            c.cluster_path_segments_any(key, qend)
        c.cluster_loci()
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_paths first'):
            c.cluster_path_segments_any(key, qend)
        assert get_rows(c, 0)[0] == _lib.FSLR_ERR_STATE
        p, want = check(idx, lab, key, qend)
        nt = len(want['start_med'])
        assert nt == 130 + 5 + 66 + 2
        assert c.cluster_path_segments_timings()['segments'] > 0
        # two runs give the same bytes
        again = device(c, key, qend, loci=False, paths=False)
        assert blob(again) == blob(want)
        # failed calls keep the rows: the plain call's refusal, a wrong count, NULL keys
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*more than 64'):
            c.cluster_path_segments(key, qend)
        resident_equals(c, want)
        with pytest.raises(_lib.FslrError, match=f'{INVALID}.*n_intervals'):
            c.cluster_path_segments_any(key[:-1], qend[:-1])
        resident_equals(c, want)
        cnt = _lib.ctypes.c_int64(-7)
        assert c._L.fslr_cluster_path_segments_any(c._h, None, _lib._ptr(qend), csr.n_intervals, _lib.ctypes.byref(cnt)) == \
            _lib.FSLR_ERR_INVALID
        assert cnt.value == -7 and 'NULL' in c._L.fslr_last_error(c._h).decode()
        resident_equals(c, want)
        # a successful paths call drops them; made again they are the same
        c.cluster_paths_any(key)
        assert get_rows(c, nt)[0] == _lib.FSLR_ERR_STATE
        same(device(c, key, qend, loci=False, paths=False), want)
        # remove_any leaves a stale table: refused, the rows made before still answer
        keep = np.ones(n, bool)
        keep[cc.rank_of_walk(csr, 1)] = False
        idx.remove_any(keep=keep)
        assert idx.csr.n_reads == n - 1 and idx.long is not None
        key2 = cc.keys_of(idx.csr, 'descending')
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_path_segments_any(key2)
        resident_equals(c, want)
        check(idx, np.zeros(n - 1, np.int32), key2, ends_near(key2, rng))
    finally:
        c.close()


def test_append_any_leaves_a_stale_table():
    data, csr, cid, nc, kw = fixture_membership('longreads_400')
    codes = np.unique(data.qcode)
    late = np.isin(data.qcode, codes[codes.size * 2 // 3:])
    idx = cluster.build_interval_trees(data.select(~late))
    try:
        c = idx.ctx
        assert idx.long is not None and ((np.diff(idx.csr.read_off) > 64).sum()) > 20
        rng = np.random.default_rng(14)
        key = cc.keys_of(idx.csr, 'shuffled')
        _, want = check(idx, cc.groups_of(idx.csr.n_reads, 5), key, ends_near(key, rng))
        idx.append_any(data.select(late))
        key = cc.keys_of(idx.csr, 'shuffled')
        with pytest.raises(_lib.FslrError, match=f'{STATE}.*fslr_cluster_table again'):
            c.cluster_path_segments_any(key)
        resident_equals(c, want)
        check(idx, cc.groups_of(idx.csr.n_reads, 5), key, ends_near(key, rng))
    finally:
        idx.ctx.close()


# ------------------------------------------------------------------ 8. the golden fixture with long reads
def test_wrapper_and_cli_on_the_long_read_fixture(tmp_path):
    name = 'longreads_400'
    p, want, lines, (data, kw, qstart, qend, rev) = expected_lines(name)
    long_rows = np.flatnonzero(np.diff(p['tok_off']) > 64)
    assert len(lines) > 1000 and long_rows.size > 10 and (p['n_reads'][long_rows] >= 1).all()
    idx = cluster.build_interval_trees(data)
    try:
        assert idx.long is not None and int(idx.long.max()) > 64
        got = idx.cluster_path_segments_any(qstart, qend, rev, query(idx, data, kw))   # makes the table, loci and paths
        assert isinstance(got, cluster.ClusterPathSegments) and len(got) == len(lines)
        same(dict(zip(sg.NAMES, got.columns())), want)
        np.testing.assert_array_equal(got.paths.tok_off, p['tok_off'])
        again = idx.cluster_path_segments_any(qstart, qend, rev)                       # on the resident path rows
        assert again.paths is got.paths
        same(dict(zip(sg.NAMES, again.columns())), want)
        made = idx.cluster_paths_any(qstart, rev)                                      # its return value is ClusterPaths
        assert isinstance(made, cluster.ClusterPaths)
        third = idx.cluster_path_segments_any(qstart, None, rev)
        assert third.paths is made and not third.gap_med.any()
        np.testing.assert_array_equal(third.start_med, want['start_med'])
        with pytest.raises(ValueError, match='intervals'):
            idx.cluster_path_segments_any(qstart, qend[:-1])
        with pytest.raises(NotImplementedError, match='more than 64'):                 # the plain wrapper still refuses
            idx.cluster_path_segments(qstart, qend, rev)
    finally:
        idx.ctx.close()
    text = HEADER + ''.join('\t'.join(map(str, r)) + '\n' for r in lines)
    for io_flag in ('--native-io', '--pandas-io'):
        out = tmp_path / io_flag.strip('-')
        out.mkdir()
        res = run_cli(name, str(out), io_flag, '--cluster-path-segments-any')
        assert res.exit_code == 0, (res.output, res.exception)
        assert 'file is written' not in res.output
        assert open(os.path.join(str(out), 'fx.mappings.cluster_path_segments.bed')).read() == text
        for which in ('cluster', 'representative'):
            assert open(os.path.join(str(out), f'fx.mappings.{which}.bed')).read() == fx.expected_text(name, which), which


def test_cli_flag_writes_the_plain_flag_s_bytes_without_long_reads(tmp_path):
    texts = []
    for flag in ('--cluster-path-segments', '--cluster-path-segments-any'):
        tmp = tmp_path / flag.strip('-')
        tmp.mkdir()
        res = run_cli('cfg1_1k_x3', str(tmp), flag)
        assert res.exit_code == 0, (res.output, res.exception)
        texts.append(open(os.path.join(str(tmp), 'fx.mappings.cluster_path_segments.bed')).read())
    assert texts[0] == texts[1] and texts[0].count('\n') > 10
