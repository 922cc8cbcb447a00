"""The query's host/device protocols against the CPU oracle (oracle.oracle.run_core), bit for bit.

A. a query that overflows its edge buffer counts every edge, is refused by every reader and gives the
   oracle's graph after fslr_reserve_edges at the exact count and a rerun (fslr_query with both engines,
   Context.run_query, the short-pair part of fslr_long_query, fslr_sweep_evaluate);
B. the same for the walk engine's deferred list;
C. a sweep query on resident reads after every change its reuse state is keyed on (thresholds, either
   cut, the pass table, a walk query in between, another input), with fslr_set_query_reuse on and off,
   each queried twice (the second takes the sync-free path when reuse is on), bench.py's step loop, and
   fslr_sweep_partition again after a change of either cut (where the kept length-gate ranges are live);
D. the sticky word of fslr_edge_cap_deferred / fslr_edge_cap_deferred_read.

Edges with I and U, forward degrees, max_fwd and components are compared exactly (and the walk engine's
evaluated_pairs / jaccard_evals): no tolerance anywhere.

The input ("the sensitive input") is built so that every setting changes the oracle's edge set: the
synthetic generator's reads pass the length gate and the overlap test at any setting, so a query that
reused stale gate ranges or thresholds would still match the oracle on them.  The tests without the gpu
mark check that from the oracle alone.

Left out: a sweep query over a read sub-range.  The sweep engine takes no read range (sweep.hip never
reads SweepArgs::a_begin / a_end: a forced FSLR_ENGINE_SWEEP covers every read, include/fslr_hip.h), so
there is no half-range result to compare.
"""
import dataclasses
import functools

import numpy as np
import pytest

import fixtures as fx  # noqa: F401  (tests/golden on the path, as test_gpu_parity)
from host_pipeline import host_prepare
from fslr_amd import _lib, synth
from fslr_amd.prep import fold_overlap_threshold, pass_table, umax_table
from oracle import oracle as O
from test_gpu_parity import _squeezed, compare_capped_with_oracle, compare_with_oracle, oracle_from_csr

gpu = pytest.mark.gpu
ENGINES = ['walk', 'sweep']
CUTS = (1, 1, 0.66, 0.66, 0.66, 0.5)
# name -> (overlap, cutoffs, qlen_diff, n_alignment_diff)
SETTINGS = {
    'default': (0.8, CUTS, 0.04, 0.25),
    'overlap95': (0.95, CUTS, 0.04, 0.25),
    'overlap50': (0.5, CUTS, 0.04, 0.25),
    'qlen01': (0.8, CUTS, 0.01, 0.25),
    'nal0': (0.8, CUTS, 0.04, 0.0),
    'cut1': (0.8, (1.0,), 0.04, 0.25),
    'cut03': (0.8, (0.3,), 0.04, 0.25),
}
# the oracle's counts on the sensitive input (seed 7): edges, max_fwd, jaccard_evals (None: not quoted)
EXPECTED = {'default': (11566, 25, 69522), 'overlap95': (3141, None, None), 'overlap50': (33003, None, None),
            'qlen01': (10068, None, 60375), 'nal0': (10421, None, None), 'cut1': (4224, None, None),
            'cut03': (26077, None, None)}
# group C's settings in the order of its steps (the walk query of step 9 leaves the default again)
SEQUENCE = ['default', 'overlap95', 'overlap50', 'default', 'qlen01', 'nal0', 'cut1', 'cut03', 'default']
# the settings of the partition path's test, in its order
PARTITION_SEQUENCE = ['default', 'qlen01', 'nal0', 'default']


@functools.lru_cache(maxsize=None)
def sensitive(seed=7):
    """3000 reads in dense events; qlen2 within 8 % and n_alignments within 3..5 of each other (both
    gates cut at the tested settings) and 40 % of the intervals shortened to 55..100 % of their aligned
    size (the overlap test cuts between 0.5 and 0.95).  The starts are untouched: still start-sorted."""
    csr = _squeezed(3000, 16, 47, 100, 'uniform', cluster_cap=30, size_p=0.05)
    n, n_iv = csr.n_reads, csr.n_intervals
    rng = np.random.default_rng(seed)
    qlen2 = 1000 + rng.integers(0, 80, n)
    nal = rng.integers(3, 6, n)
    pick = rng.random(n_iv) < 0.4
    u = rng.uniform(0.55, 1.0, n_iv)
    start = csr.iv_start.astype(np.int64)
    length = csr.iv_end.astype(np.int64) - start
    end = np.where(pick, start + np.maximum(1, (length * u).astype(np.int64)), csr.iv_end)
    return dataclasses.replace(csr, read_qlen2=qlen2.astype(np.int32), read_nal=nal.astype(np.int32),
                               iv_end=end.astype(np.int32))


@functools.lru_cache(maxsize=None)
def oracle(setting='default', seed=7, use_cap=False):
    """The oracle's result, computed once per (setting, input) and shared; the callers only read it."""
    overlap, cuts, qd, nd = SETTINGS[setting]
    return O.run_core(oracle_from_csr(sensitive(seed)), overlap, cuts, qd, nd, 10, use_cap=use_cap)


def edge_set(o):
    return set(zip(o['edge_a'].tolist(), o['edge_b'].tolist(), o['edge_I'].tolist(), o['edge_U'].tolist()))


# ------------------------------------------------------------------ the input's conditions (CPU)
def test_sensitive_input_oracle_counts():
    for name, (ne, max_fwd, jacc) in EXPECTED.items():
        o = oracle(name)
        assert len(o['edge_a']) == ne, name
        assert max_fwd is None or o['stats']['max_fwd'] == max_fwd, name
        assert jacc is None or o['stats']['jaccard_evals'] == jacc, name
        assert 23 <= o['stats']['max_fwd'] <= 29, name          # an edge cap of 10 binds at every setting
    assert oracle('default', use_cap=True)['stats']['max_fwd'] > 10


def test_consecutive_settings_differ_in_5_percent_of_the_edges():
    """A condition, not a measurement: were two consecutive steps of group C to share (nearly) one edge
    set, a query that kept the earlier step's state would pass the later step's comparison."""
    for seq in (SEQUENCE, PARTITION_SEQUENCE):
        sets = [edge_set(oracle(name)) for name in seq]
        if seq is SEQUENCE:
            sets.append(edge_set(oracle('default', seed=8)))
        for k in range(1, len(sets)):
            assert 20 * len(sets[k - 1] ^ sets[k]) >= max(len(sets[k - 1]), len(sets[k])), (seq, k)
    other = sensitive(8)
    assert (other.n_reads, other.n_intervals) == (sensitive().n_reads, sensitive().n_intervals)


# ------------------------------------------------------------------ helpers (GPU)
@pytest.fixture
def ctx():
    """A context of its own for every test: a shared context's buffers only grow."""
    c = _lib.Context(0)
    yield c
    c.close()


def params(setting):
    overlap, cuts, qd, nd = SETTINGS[setting]
    return 1 - qd, 1 - nd, pass_table(cuts)


def thresholds(setting, seed=7):
    return fold_overlap_threshold(sensitive(seed).iv_aln, SETTINGS[setting][0])


def result(c, st):
    a, b, I, U = c.edges(st['n_edges'])
    return dict(stats=st, labels=c.labels(), fwd=c.fwd_degree(), a=a, b=b, I=I, U=U)


def query_equals_oracle(c, setting, engine, seed=7):
    """query, components, stats, then the comparison; returns the stats."""
    c.query(*params(setting), 10, engine=engine)
    c.components()
    st = c.stats()
    assert st['engine'] == engine
    compare_with_oracle(result(c, st), oracle(setting, seed), c.n_reads)
    return st


def assert_overflowed_query_is_refused(c, n_edges, cap_and_table=True):
    """Every reader of an overflowed query's results raises FslrError (and the process lives on)."""
    with pytest.raises(_lib.FslrError):
        c.stats()
    with pytest.raises(_lib.FslrError):
        c.edges(n_edges)
    c.components()                 # async: the union-find flags the lost edges for the label readers
    with pytest.raises(_lib.FslrError):
        c.labels()
    if cap_and_table:
        with pytest.raises(_lib.FslrError):
            c.cluster_table()
        with pytest.raises(_lib.FslrError):
            c.apply_edge_cap(10)


# ------------------------------------------------------------------ A. edge-buffer overflow and rerun
@gpu
@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('below', [None, 1, 0], ids=['cap64', 'capE-1', 'capE'])
def test_edge_overflow_counts_refuses_and_reruns(ctx, engine, below):
    csr, o = sensitive(), oracle()
    E = len(o['edge_a'])
    cap = 64 if below is None else E - below
    ctx.load_csr(csr, thresholds('default'))
    ctx.reserve_edges(cap)
    ctx.build_index()
    ctx.query(*params('default'), 10, engine=engine)
    st = ctx.stats(check=False)
    assert st['edge_capacity'] == cap
    if cap < E:
        assert st['n_edges'] == E                     # the count does not stop at the capacity
        assert st['max_fwd'] == o['stats']['max_fwd']
        assert_overflowed_query_is_refused(ctx, E)
        ctx.reserve_edges(E)                          # the last edge lands at k == cap - 1
        ctx.query(*params('default'), 10, engine=engine)
    ctx.components()
    st = ctx.stats()
    assert st['edge_capacity'] == E and st['engine'] == engine
    compare_with_oracle(result(ctx, st), o, csr.n_reads)


@gpu
@pytest.mark.parametrize('engine', ENGINES)
def test_run_query_grows_both_buffers_and_stops(ctx, engine):
    """Context.run_query from 64 edges and 64 deferred entries.  Its loop reruns while a buffer was too
    small, so it issues at least 2 queries here (E > 64).  Both counts are taken before the capacity
    check, so the deferred count of query 1 is exact whatever the capacities, and the edge count of a
    query whose deferred list fitted is exact too.  Hence: 2 queries when query 1's deferred list fitted
    (the sweep engine defers nothing) - query 1 reports E, query 2 fits; otherwise query 1's edge count
    lacks the lost deferred pairs' edges, query 2's is exact and may exceed 1.25 x query 1's + 4096, and
    query 3 fits: at most 3."""
    csr, o = sensitive(), oracle()
    ctx.load_csr(csr, thresholds('default'))
    ctx.reserve_edges(64)
    ctx.reserve_deferred(64)
    ctx.build_index()
    seen = []
    inner_query, inner_stats = ctx.query, ctx.stats
    queries = []

    def counting_query(*a, **kw):
        queries.append(1)
        return inner_query(*a, **kw)

    def recording_stats(check=True):
        s = inner_stats(check=check)
        if not check:
            seen.append(s)
        return s

    ctx.query, ctx.stats = counting_query, recording_stats
    st = ctx.run_query(*params('default'), 10, engine=engine)
    ctx.query, ctx.stats = inner_query, inner_stats
    first_deferred_fitted = seen[0]['deferred'] <= 64
    print(f'run_query[{engine}]: {len(queries)} queries, deferred of query 1: {seen[0]["deferred"]}')
    assert engine != 'sweep' or first_deferred_fitted
    assert len(queries) == 2 or (not first_deferred_fitted and len(queries) == 3)
    assert st['n_edges'] == len(o['edge_a']) <= st['edge_capacity']
    ctx.components()
    compare_with_oracle(result(ctx, ctx.stats()), o, csr.n_reads)


@functools.lru_cache(maxsize=None)
def long_input():
    """Short reads and reads of more than 64 intervals (test_gpu_long's first input) and its oracle."""
    csr = synth.generate(3000, 150, 3, lmin=1).interval_data().csr()
    return csr, O.run_core(oracle_from_csr(csr), 0.8, CUTS, 0.04, 0.25, 10, use_cap=False)


def test_long_input_has_short_pairs_beyond_64_edges():
    csr, o = long_input()
    L = np.diff(csr.read_off)
    short = (L[o['edge_a']] <= 64) & (L[o['edge_b']] <= 64)
    assert L.max() > 64 and short.sum() > 64 and (~short).sum() > 0


@gpu
def test_long_query_short_pairs_overflow_and_rerun(ctx):
    """fslr_long_query writes the pairs of two short reads into the context's edge buffer (the sweep's
    pair stage, through fslr_sweep_evaluate): the same count, refusals and rerun."""
    csr, o = long_input()
    n, L = csr.n_reads, np.diff(csr.read_off)
    want = sorted(edge_set(o))
    want_short = [e for e in want if L[e[0]] <= 64 and L[e[1]] <= 64]
    Es = len(want_short)
    q = (*params('default'), 10)
    ctx.load_csr_any(csr, np.zeros(csr.n_intervals, np.int32))
    ctx.build_index()
    ctx.set_thresholds(fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.set_long_cutoffs(umax_table(CUTS, int(L.max())))
    ctx.reserve_edges(64)
    ctx.long_query(*q)
    st = ctx.stats(check=False)
    assert st['n_edges'] == Es and st['edge_capacity'] == 64
    assert_overflowed_query_is_refused(ctx, Es, cap_and_table=False)
    ctx.reserve_edges(Es)
    n_long = ctx.long_query(*q)
    st = ctx.stats()
    assert st['n_edges'] == Es == st['edge_capacity']
    la, lb, lI, lU = ctx.long_edges(n_long)
    sa, sb, sI, sU = ctx.edges(Es)
    assert sorted(zip(sa.tolist(), sb.tolist(), sI.tolist(), sU.tolist())) == want_short
    got = sorted(zip(np.r_[sa, la].tolist(), np.r_[sb, lb].tolist(), np.r_[sI, lI].tolist(), np.r_[sU, lU].tolist()))
    assert got == want
    np.testing.assert_array_equal(np.bincount(np.r_[sa, la], minlength=n), o['fwd'])
    ctx.components()
    ctx.union_pairs(la, lb, n_long, on_device=False)
    ctx.finalize_labels()
    lab = ctx.labels()[:n]
    sizes = np.bincount(lab, minlength=n)
    rid = np.full(n, -1)
    rid[np.flatnonzero(sizes >= 2)] = np.arange((sizes >= 2).sum())
    np.testing.assert_array_equal(np.where(sizes[lab] >= 2, rid[lab], -1), o['comp'])


@gpu
def test_sweep_evaluate_overflow_and_rerun(ctx):
    """fslr_sweep_partition with one destination feeding fslr_sweep_evaluate on the same context (the
    multi-GPU sweep at world size 1)."""
    import torch
    csr, o = sensitive(), oracle()
    E = len(o['edge_a'])
    q = params('default')
    ctx.load_csr(csr, thresholds('default'))
    ctx.reserve_edges(64)                             # before the partition, whose first call sizes the buffers
    ctx.build_index()
    buf = torch.empty(1 << 16, dtype=torch.int64, device=torch.device('cuda', 0))
    ok, counts = ctx.sweep_partition(*q, 1, 6, buf)
    if not ok:
        buf = torch.empty(int(counts.sum()) + 16, dtype=torch.int64, device=torch.device('cuda', 0))
        ok, counts = ctx.sweep_partition(*q, 1, 6, buf)
    assert ok and counts.sum() > 0
    ctx.sweep_evaluate(*q, buf, int(counts[0]))
    st = ctx.stats(check=False)
    assert st['n_edges'] == E and st['edge_capacity'] == 64 and st['max_fwd'] == o['stats']['max_fwd']
    assert_overflowed_query_is_refused(ctx, E)
    ctx.reserve_edges(E)
    ctx.sweep_evaluate(*q, buf, int(counts[0]))
    ctx.components()
    st = ctx.stats()
    assert st['edge_capacity'] == E
    compare_with_oracle(result(ctx, st), o, csr.n_reads)


# ------------------------------------------------------------------ B. deferred-list overflow (walk)
@gpu
def test_deferred_overflow_counts_refuses_and_reruns(ctx, monkeypatch):
    """300 reads on one interval with one partner partition (FSLR_PASS_RECORDS=0): the first reads have
    more matching partners than their match lists hold, and the rest goes through the deferred list."""
    monkeypatch.setenv('FSLR_PASS_RECORDS', '0')
    n = 300
    off = np.arange(n + 1, dtype=np.int64)
    chrom = np.zeros(n, np.int32)
    start = np.sort(np.full(n, 5000, np.int32) + (np.arange(n) % 7).astype(np.int32))
    end = start + 1000
    aln = np.full(n, 1000, np.int64)
    qlen2, nal = np.full(n, 100, np.int32), np.full(n, 3, np.int32)
    o = O.run_core(O.OracleCSR(off, chrom, start, end, aln, qlen2, nal, np.arange(n)), 0.8, (1.0,), 0.04, 0.25,
                   use_cap=False)
    q = (1 - 0.04, 1 - 0.25, pass_table([1.0]))
    ctx.set_reads(off, qlen2, nal, chrom, start, end, fold_overlap_threshold(aln, 0.8), 1, iv_data_pos=np.arange(n))
    ctx.reserve_edges(n * n)
    ctx.reserve_deferred(64)
    ctx.build_index()
    ctx.query(*q, 10, engine='walk')
    st = ctx.stats(check=False)
    print(f'deferred entries of the one-locus input (n = {n}): {st["deferred"]}')
    assert st['deferred'] > st['deferred_capacity'] == 64
    assert st['overflow_flags'] & 1
    with pytest.raises(_lib.FslrError):
        ctx.stats()
    ctx.components()
    with pytest.raises(_lib.FslrError):
        ctx.labels()
    ctx.reserve_deferred(st['deferred'])              # the last entry lands at k == cap - 1
    ctx.query(*q, 10, engine='walk')
    ctx.components()
    st2 = ctx.stats()
    assert st2['deferred'] == st['deferred'] == st2['deferred_capacity'] and st2['overflow_flags'] == 0
    compare_with_oracle(result(ctx, st2), o, n)


# ------------------------------------------------------------------ C. repeat and reuse (sweep)
def twice_equals_oracle(c, setting, seed=7):
    """The step's query, then the same query again (the sync-free path when reuse is on): both equal the
    oracle and count the same entries and pairs."""
    first = query_equals_oracle(c, setting, 'sweep', seed)
    second = query_equals_oracle(c, setting, 'sweep', seed)
    assert (second['match_entries'], second['matched_pairs']) == (first['match_entries'], first['matched_pairs'])
    return first


@gpu
@pytest.mark.parametrize('reuse', [True, False], ids=['reuse', 'full'])
def test_sweep_requery_after_every_change_of_its_state(ctx, reuse):
    csr = sensitive()
    n = csr.n_reads
    ctx.set_query_reuse(reuse)
    ctx.load_csr(csr, thresholds('default'))
    ctx.reserve_edges(1 << 16)
    ctx.build_index()
    entries = [twice_equals_oracle(ctx, 'default')['match_entries']]                  # 1
    for setting in ('overlap95', 'overlap50', 'default'):                             # 2, 3, 4: thresholds
        ctx.set_thresholds(thresholds(setting))
        entries.append(twice_equals_oracle(ctx, setting)['match_entries'])
    assert entries[2] > max(entries[:2])              # more entries than any step before it
    for setting in ('qlen01', 'nal0', 'cut1', 'cut03'):                               # 5, 6: a cut; 7, 8: the table
        twice_equals_oracle(ctx, setting)
    # 9: a walk query of a sub-range under another cut overwrites that part of the gate ranges
    ctx.query(*params('qlen01'), 10, a_begin=n // 3, a_end=2 * n // 3, engine='walk')
    twice_equals_oracle(ctx, 'default')
    # (10, a sweep query over a sub-range, is left out: see the module docstring)
    # 11: another input of the same size
    ctx.load_csr(sensitive(8), thresholds('default', 8))
    ctx.build_index()
    twice_equals_oracle(ctx, 'default', seed=8)


def partition_equals_oracle(c, buf, setting):
    """fslr_sweep_partition with one destination, fslr_sweep_evaluate of its entries, components."""
    q = params(setting)
    ok, counts = c.sweep_partition(*q, 1, 6, buf)
    assert ok
    c.sweep_evaluate(*q, buf, int(counts[0]))
    c.components()
    compare_with_oracle(result(c, c.stats()), oracle(setting), c.n_reads)


@gpu
@pytest.mark.parametrize('reuse', [True, False], ids=['reuse', 'full'])
def test_partition_again_after_a_change_of_either_cut(ctx, reuse):
    """The kept length-gate ranges (keyed on the input generation and both cuts) are live on the
    partition path: fslr_query marks them stale on every call (the walk engine writes its own part of
    them), fslr_sweep_partition does not.  Each setting is partitioned twice; the gate is applied where
    the entries are written, so stale ranges give the earlier setting's edges."""
    import torch
    ctx.set_query_reuse(reuse)
    ctx.load_csr(sensitive(), thresholds('default'))
    ctx.reserve_edges(1 << 16)
    ctx.build_index()
    buf = torch.empty(1 << 20, dtype=torch.int64, device=torch.device('cuda', 0))
    for setting in PARTITION_SEQUENCE:
        partition_equals_oracle(ctx, buf, setting)
        partition_equals_oracle(ctx, buf, setting)


@gpu
@pytest.mark.parametrize('reuse', [True, False], ids=['reuse', 'full'])
def test_bench_shaped_steps_without_host_reads(ctx, reuse):
    """bench.py's timed loop: 8 steps of index, query, components and the deferred cap check with no
    host read in between, then one stats() and the comparison."""
    csr = sensitive()
    ctx.set_query_reuse(reuse)
    ctx.load_csr(csr, thresholds('default'))
    ctx.reserve_edges(1 << 16)
    for _ in range(8):
        ctx.build_index()
        ctx.query(*params('default'), 10, engine='sweep')
        ctx.components()
        ctx.edge_cap_deferred(10_000)
    st = ctx.stats()
    compare_with_oracle(result(ctx, st), oracle(), csr.n_reads)
    assert ctx.edge_cap_deferred_read() == 0


# ------------------------------------------------------------------ D. the deferred cap word
def cap_steps(c, engine, thresholds_, setting='default'):
    for t in thresholds_:
        c.build_index()
        c.query(*params(setting), 10, engine=engine)
        c.components()
        c.edge_cap_deferred(t)


@gpu
def test_deferred_cap_before_any_query_is_a_state_error(ctx):
    with pytest.raises(_lib.FslrError, match=f'fslr error {_lib.FSLR_ERR_STATE}'):
        ctx.edge_cap_deferred(10)
    assert ctx.edge_cap_deferred_read() == 0


@gpu
@pytest.mark.parametrize('engine', ENGINES)
def test_deferred_cap_word_stays_clear_when_nothing_binds(ctx, engine):
    csr = synth.generate(3000, 16, 2).interval_data().csr()
    o = O.run_core(oracle_from_csr(csr), use_cap=False)
    assert o['stats']['max_fwd'] == 9
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    cap_steps(ctx, engine, [10, 10, 10])
    assert ctx.edge_cap_deferred_read() == 0
    compare_with_oracle(result(ctx, ctx.stats()), o, csr.n_reads)


@gpu
@pytest.mark.parametrize('engine', ENGINES)
def test_deferred_cap_word_on_a_binding_input(ctx, engine):
    csr, o = sensitive(), oracle()
    max_fwd = o['stats']['max_fwd']
    ctx.load_csr(csr, thresholds('default'))
    ctx.reserve_edges(1 << 16)
    cap_steps(ctx, engine, [10, 10, 10])
    assert ctx.edge_cap_deferred_read() == 1          # bit 0 alone: the cap binds, no ZeroDivisionError pair
    assert ctx.edge_cap_deferred_read() == 0          # the read cleared it
    cap_steps(ctx, engine, [10_000, 10, 10_000])
    assert ctx.edge_cap_deferred_read() == 1          # sticky across the queries, which reset the error words
    cap_steps(ctx, engine, [max_fwd])
    assert ctx.edge_cap_deferred_read() == 0          # max_fwd > threshold is strict
    cap_steps(ctx, engine, [max_fwd - 1])
    assert ctx.edge_cap_deferred_read() == 1
    # the word fired: the step again with the synchronous cap, as bench.py does
    ctx.build_index()
    ctx.query(*params('default'), 10, engine=engine)
    ctx.components()
    cap = ctx.apply_edge_cap(10)
    assert cap['applied'] == 1
    ctx.components()
    st = ctx.stats()
    st['max_fwd'] = cap['max_fwd']
    compare_capped_with_oracle(result(ctx, st), oracle(use_cap=True), csr.n_reads)


@gpu
def test_deferred_cap_word_zero_division_fixture(ctx):
    """An aln_size == 0 interval (the walk engine's input): the listed pair sets bit 1."""
    csr = host_prepare('zerodiv')[0].csr()
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    cap_steps(ctx, 'walk', [10])
    assert ctx.edge_cap_deferred_read() & 2
    with pytest.raises(ZeroDivisionError):
        ctx.stats()


@gpu
@pytest.mark.parametrize('engine', ENGINES)
def test_deferred_cap_word_zero_qlen2_pair(ctx, engine):
    """Two overlapping reads with qlen2 == 0 (test_zero_qlen2_pair_raises' input, which the sweep takes
    too): bit 1, and bit 0 clear (one edge at most)."""
    start = np.array([5000, 5010], np.int32)
    ctx.set_reads(np.array([0, 1, 2], np.int64), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32),
                  start, start + 1000, fold_overlap_threshold(np.full(2, 1000, np.int64), 0.8), 1,
                  iv_data_pos=np.arange(2))
    for t in (10, 10):
        ctx.build_index()
        ctx.query(1 - 0.04, 1 - 0.25, pass_table([1.0]), 10, engine=engine)
        ctx.components()
        ctx.edge_cap_deferred(t)
    assert ctx.edge_cap_deferred_read() == 2
