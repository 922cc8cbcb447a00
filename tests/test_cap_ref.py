"""tests/cap_ref.py pinned on the CPU: its loop to the C oracle (edges, I, U, forward degrees, components),
its closure and visit lists to tests/sweep_emu.py, on every directed input of tests/cap_cases.py and on
the capbind_1500, zdcap_skip and zdcap_raise fixtures.  And each directed input's premise, asserted from
the reference alone: an input that no longer reaches its seam fails here instead of passing quietly on
the device."""
import functools

import numpy as np
import pytest

import cap_cases as C
import cap_ref as R
import fixtures as fx
from host_pipeline import host_prepare
from oracle import oracle as O
from sweep_emu import EmuSweepContext
from fslr_amd.prep import fold_overlap_threshold

ALL = C.loop_cases() + C.list_cases()
IDS = [c[0] for c in ALL]


def oracle_csr(c):
    cnt = np.diff(c.read_off)
    return O.OracleCSR(c.read_off, c.iv_chrom, c.iv_start, c.iv_end, c.iv_aln, np.repeat(c.read_qlen2, cnt),
                       np.repeat(c.read_nal, cnt), c.data_pos)


def run_oracle(csr, p, thr, use_cap):
    return O.run_core(oracle_csr(csr), p['overlap'], p['cutoffs'], p['qlen_diff'], p['nal_diff'], edge_threshold=thr,
                      use_cap=use_cap)


def same_graph(rep, o, n):
    r = R.as_oracle(rep, n)
    oe = sorted(zip(o['edge_a'].tolist(), o['edge_b'].tolist(), o['edge_I'].tolist(), o['edge_U'].tolist()))
    assert sorted(rep['edges']) == oe
    np.testing.assert_array_equal(r['fwd'], o['fwd'])
    np.testing.assert_array_equal(r['comp'], o['comp'])
    assert r['stats']['max_fwd'] == o['stats']['max_fwd']


def pinned(csr, p, thr):
    """replay == the oracle (capped and E*); closure and visit lists == sweep_emu's."""
    e = R.expected(csr, p, thr)
    same_graph(e['cap'], run_oracle(csr, p, thr, True), csr.n_reads)
    same_graph(e['star'], run_oracle(csr, p, thr, False), csr.n_reads)
    emu = EmuSweepContext(csr, fold_overlap_threshold(csr.iv_aln, p['overlap']))
    rows = np.array(e['rows'], np.int64).reshape(-1, 2)
    assert emu._candidates(thr, rows, e['star']['formed']) == e['T']
    assert emu._hit_lists(e['T'], None) == e['lists']
    return e


@pytest.mark.parametrize('cid,builder,args', ALL, ids=IDS)
def test_reference_equals_oracle_and_emulator(cid, builder, args):
    case = C.case(builder, *args)
    e = pinned(case.csr, case.params, case.thr)
    assert e is not None and case.exp['stats'] == e['stats']
    assert np.asarray(e['star']['formed']).max() <= 256          # the sweep keeps one run per read
    assert np.asarray(e['star']['formed']).max() > case.thr      # the cap binds: the device replays


@functools.lru_cache(maxsize=None)
def fixture_csr(name):
    data, _, kw = host_prepare(name)
    p = dict(overlap=kw['overlap'], cutoffs=tuple(float(x) for x in kw['jaccard_cutoffs'].split(',')),
             qlen_diff=kw['qlen_diff'], nal_diff=kw['n_alignment_diff'])
    return data.csr(), p


@pytest.mark.parametrize('name', ['capbind_1500', 'zdcap_skip', 'zdcap_raise'])
def test_reference_equals_oracle_on_fixtures(name):
    csr, p = fixture_csr(name)
    if fx.meta(name)['exception']:
        with pytest.raises(ZeroDivisionError):
            R.replay(csr, p, 10)
        with pytest.raises(ZeroDivisionError):
            run_oracle(csr, p, 10, True)
        return
    rep = R.replay(csr, p, 10)
    same_graph(rep, run_oracle(csr, p, 10, True), csr.n_reads)
    assert rep['breaks']
    if name == 'capbind_1500':                                   # E* raises on the zdcap inputs
        pinned(csr, p, 10)


# ------------------------------------------------------------------------------------ closure shapes
@pytest.mark.parametrize('name', list(C.closure_shapes()))
def test_closure_shape_premises(name):
    thr, n, rows = C.closure_shapes()[name]
    fwd = np.bincount([a for a, _ in rows], minlength=n)
    T, rounds = R.closure(n, rows, fwd, thr)
    assert fwd.max() > thr                                      # fslr_cap_local wants a binding cap
    emu = EmuSweepContext(C.witness_reads(2), [1, 1, 1, 1])
    emu.n_reads = n
    assert emu._candidates(thr, np.array(rows), fwd) == T
    for order in ('sorted', 'reversed', 'shuffled'):
        assert R.closure(n, C.ordered(rows, order), fwd, thr) == (T, rounds)
    if name.startswith('ladder'):
        d = int(name[6:])
        assert R.depth(rounds) == d and T == list(range(d + 1))
        assert all(rounds[k] == k and (fwd[k] == thr - 1 or k == 0) for k in T)
    if name == 'fan129':
        assert R.depth(rounds) == 1 and sum(r == 1 for r in rounds.values()) == 129 and fwd[0] == 130
    if name == 'two_rounds':
        assert rounds == {0: 0, 1: 1, 5: 2} and fwd[5] == 0
    if name == 'only_seeds':
        assert rounds == {0: 0, 4: 0}
    if name == 'everyone':
        assert T == list(range(n)) and fwd[n - 1] == 0 and R.depth(rounds) == 1


def test_closure_row_orders_differ():
    rows = C.closure_shapes()['ladder17'][2]
    s, r, h = (C.ordered(rows, o) for o in ('sorted', 'reversed', 'shuffled'))
    assert s != r and s != h and r != h and sorted(r) == s and sorted(h) == s
    assert [a for a, _ in s] == sorted(a for a, _ in s)
    assert [a for a, _ in r] != sorted(a for a, _ in r) and [a for a, _ in h] != sorted(a for a, _ in h)


# ------------------------------------------------------------------------------------ premises: lists
def interval_lists(case, name):
    """The visit lists (as interval indices) of read `name`'s intervals."""
    return R.visit_lists(case.csr, [case.rank[name]], with_intervals=True)


@pytest.mark.parametrize('count', C.TIE_COUNTS)
@pytest.mark.parametrize('ends', C.TIE_ENDS)
def test_tie_run_premises(count, ends):
    case = C.case('tie_run', count, ends)
    csr, rank = case.csr, case.rank
    x = rank['x']
    assert x in case.exp['T']
    first = interval_lists(case, 'x')[0]
    st, en = csr.iv_start[first], csr.iv_end[first]
    run = np.flatnonzero(st == 50_020)
    assert run.size == count                                    # this tie run has `count` members ...
    assert run[0] == 9 and run[0] < 64 <= run[-1]               # ... and straddles the 64-hit chunk seam
    assert np.array_equal(run, np.arange(run[0], run[0] + count))
    e = en[run]
    assert {'distinct': np.unique(e).size == count, 'equal': np.unique(e).size == 1,
            'mixed': 1 < np.unique(e).size < count}[ends]
    assert (np.diff(e) >= 0).all()                              # ends ascend inside a run; equal ends: position descends
    dp = csr.data_pos[np.array(first)[run]]
    assert all(dp[k] > dp[k + 1] for k in range(count - 1) if e[k] == e[k + 1])
    # x's own second interval lies inside the run in data order and is not listed
    own = csr.data_pos[csr.read_off[x] + 1]
    assert csr.iv_start[csr.read_off[x] + 1] == 50_020 and dp.min() < own < dp.max()
    reads_first = R.visit_lists(csr, [x])[0]
    assert x not in reads_first and rank['touch'] in reads_first and rank['miss'] not in reads_first
    assert csr.iv_end[csr.read_off[rank['touch']]] == csr.iv_start[csr.read_off[x]]
    assert csr.iv_end[csr.read_off[rank['miss']]] == csr.iv_start[csr.read_off[x]] - 1


def test_directions_premises():
    case = C.case('directions')
    csr, rank, T = case.csr, case.rank, case.exp['T']
    assert {rank['x'], rank['p'], rank['q']} <= set(T)
    lists = interval_lists(case, 'x')
    k0 = csr.read_off[rank['x']]
    pos = csr.data_pos
    assert len(lists[0]) == 3 and all(pos[p] < pos[k0] for p in lists[0])          # all backward
    assert len(lists[1]) == 3 and all(pos[p] > pos[k0 + 1] for p in lists[1])      # all forward
    assert lists[2] == []
    assert csr.iv_start[csr.read_off[rank['p']]] == csr.iv_start[csr.read_off[rank['q']]]


# ------------------------------------------------------------------------------------ premises: loops
@pytest.mark.parametrize('thr', C.BREAK_THR)
def test_break_position_premise(thr):
    case = C.case('one_locus', thr)
    e = case.exp
    assert e['cap']['breaks'][0] == (0, thr - 1)                # read 0 breaks at list index thr - 1 of interval 0
    assert e['lists'][0] == list(range(199, 0, -1)) and e['T'][0] == 0


@pytest.mark.parametrize('kind', ['edge', 'counted'])
@pytest.mark.parametrize('k', C.FILLERS)
def test_walk_premise(k, kind):
    case = C.case('walks', k, kind)
    e, rank = case.exp, case.rank
    assert e['T'][0] == 0 and e['cap']['breaks'][0] == (0, case.thr - 1)
    # interval 1's walk passes k uncounted hits and stops on z; interval 2's runs off the end; interval 3's
    # passes one filler and stops on the counted non-edge z2
    assert e['cap']['walks'][0] == [(1, k, kind), (2, None, None), (3, 1, 'counted')]
    lst = e['lists'][1]
    assert lst[:k] == [rank[f'f{f}'] for f in range(k - 1, -1, -1)] and lst[k] == rank['z']
    pred = R.Pairs(case.csr, case.params)
    assert all(pred(0, y) == (False, False, 0, 0) for y in lst[:k])
    assert pred(0, rank['z'])[:2] == (True, kind == 'edge')
    if kind == 'counted':
        assert pred(0, rank['z'])[2] == 1 and np.diff(case.csr.read_off)[rank['z']] == 3
    assert len(e['lists'][2]) > 0
    formed = set(map(tuple, np.array(e['cap']['edges'])[:, :2].tolist()))
    assert ((0, rank['z']) in formed) == (kind == 'edge') and (0, rank['z2']) not in formed


def test_empty_segment_premise():
    case = C.case('empty_segments')
    e = case.exp
    n_hits = [len(x) for x in e['lists']]
    assert e['T'] == list(range(6))
    assert n_hits[:5] == [0, 4, 0, 5, 0]                        # read 0: empty before and after the break's interval
    assert e['cap']['breaks'][0] == (1, case.thr - 1)
    assert e['cap']['walks'][0] == [(2, None, None), (3, 0, 'edge'), (4, None, None)]
    assert n_hits[-1] == 0                                      # the last read of T ends in an empty segment


def test_eval_mix_premise():
    case = C.case('eval_mix')
    e = case.exp
    L = np.diff(case.csr.read_off)
    assert set(L.tolist()) == {1, 16, 17, 64} and len(e['T']) == case.n
    seen = {(L[min(a, b)], L[max(a, b)]) for a, b, _, _ in e['cap']['edges']}
    assert {(16, 16), (16, 17), (17, 16), (17, 17)} <= seen
    assert any(1 in s for s in seen) and any(64 in s and 17 in s for s in seen)
    # sorted by (t, partner), 64 consecutive slots hold lane-decided and wavefront-decided pairs
    slots = sorted({(t, y) for t in e['T'] for y in range(case.n) if y != t})
    first = [max(L[t], L[y]) <= 16 for t, y in slots[:64]]
    assert any(first) and not all(first)
    I = np.array(e['cap']['edges'])[:, 2]
    assert np.unique(I).size >= 4


def test_left_behind_premise():
    case = C.case('left_behind')
    e, r = case.exp, case.rank
    T = set(e['T'])
    star = set(e['rows'])
    edges = {(a, b) for a, b, _, _ in e['cap']['edges']}
    assert r['u'] not in T and {r['y'], r['x'], r['x2']} <= T
    assert (r['y'], r['x']) in star and (r['x'], r['y']) in edges and (r['y'], r['x']) not in edges
    assert (r['y'], r['x2']) in star and (r['y'], r['x2']) not in edges and (r['x2'], r['y']) not in edges
    assert (r['u'], r['y']) in edges
    assert e['stats']['backward'] == 1 and e['stats']['dropped'] == 1


@pytest.mark.parametrize('where', ['end', 'start'])
def test_hole_fill_premise(where):
    case = C.case('hole_fill', where)
    e = case.exp
    lower = np.array([a for a, _ in sorted(e['rows'])])          # one run per read in rank order
    inT = np.isin(lower, e['T'])
    k = int(inT.sum())
    assert 0 < k < lower.size
    assert inT[-k:].all() if where == 'end' else inT[:k].all()
    if where == 'start':
        assert e['stats']['dropped'] > lower.size - k            # more holes than surviving tail rows
    assert e['stats']['dropped'] > 0


@pytest.mark.parametrize('thr', [0, -1])
def test_threshold_zero_premise(thr):
    case = C.case('threshold_zero', thr)
    e = case.exp
    assert e['T'] == list(range(60))                             # every read is a seed, those without hits too
    per_read = np.add.reduceat([len(x) for x in e['lists']], case.csr.read_off[:-1])
    assert (per_read == 0).sum() == 20
    assert e['stats']['dropped'] > 0
    # a loop breaks on its first new counted pair; one that meets only seen pairs (b0: a0 came first) does not
    assert case.rank['a0'] in e['cap']['breaks'] and case.rank['b0'] not in e['cap']['breaks']
    # a counted pair that is no edge breaks a loop too: edges >= thr holds from the start
    assert e['cap']['breaks'][case.rank['c0']] == (0, 0) and e['cap']['formed'][case.rank['c0']] == 0
    assert e['cap']['edges'] == C.case('threshold_zero', 0).exp['cap']['edges']
