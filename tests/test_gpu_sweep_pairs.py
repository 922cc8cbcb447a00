"""Directed tests of the sweep engine's pair kernel (sweep.hip k_sweep_pairs) through
fslr_sweep_evaluate: hand-built match entries against the plain reference of tests/pairs_ref.py, bit
for bit, and stacked pile-ups through the whole query on both engines against the CPU oracle.

The entries of a case are built so that their positions after the grouping by A are known: small
consecutive A's with known entry counts (a run = the entries of one A).  The kernel's constants the
docstrings refer to: a wave owns the runs that start in its chunk of kChunk2 = 512 sorted entries;
it takes whole runs in groups of at most kStageE = 128 entries, sorted by (run, B, i, j) in a
bitonic network of 32, 64 or 128 elements; a run of more than 128 entries goes alone, either
bucketed (P = ceil(len / 96) <= 64 hash buckets of partners, none above 128 entries) or in
ceil(len / kPerPass) partner partitions (kPerPass = 40) of at most kPairLimit = 64 partners; edges
are staged 256 per wave.  `paths()` restates the bucket and partition hashes only to assert, on the
CPU, that a case's input reaches the branch its docstring names.
"""
import functools

import numpy as np
import pytest
import torch

import pairs_ref as pr
import test_gpu_parity as parity
from fslr_amd import _lib
from fslr_amd.prep import fold_overlap_threshold, pass_table
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CUTS = ((0.0,), (1, 1, 0.66, 0.66, 0.66, 0.5))
KINDS = ('perm', 'row', 'col', 'both')
N_DIR = 4096                                                   # reads of the directed cases
L_DIR = np.array([64, 8, 5, 3], np.int64)[np.arange(N_DIR) % 4]   # ranks = 0 mod 4 have 64 intervals, the rest few:
#                                                                  pairs of short reads pass the default cuts


class Dev:
    def __init__(self):
        self.ctx = _lib.Context(0)
        self.L = None

    def upload(self, L):
        """Reads of L[r] short intervals at private, disjoint coordinates (only L matters to
        fslr_sweep_evaluate: the 1-byte lengths)."""
        L = np.asarray(L, dtype=np.int64)
        if self.L is not None and np.array_equal(self.L, L):
            return
        ni = int(L.sum())
        off = np.concatenate([[0], np.cumsum(L)])
        start = (100 * np.arange(ni)).astype(np.int32)
        self.ctx.set_reads(off, np.full(L.size, 100, np.int32), np.full(L.size, 3, np.int32), np.zeros(ni, np.int32),
                           start, start + 50, fold_overlap_threshold(np.full(ni, 50, np.int64), 0.8), 1)
        self.L = L


@pytest.fixture(scope='module')
def dev():
    d = Dev()
    yield d
    d.ctx.close()


def evaluate(dev, L, ent, cut):
    """One fslr_sweep_evaluate of `ent` and its comparison with the reference; returns the reference's
    edges.  stats() checks: an overflow flag raises."""
    ctx = dev.ctx
    dev.upload(L)
    edges, fwd, n_pairs = pr.evaluate_entries(ent, L, cut)
    t = torch.from_numpy(np.ascontiguousarray(ent)).to('cuda:0') if ent.size else None
    ctx.reserve_edges(n_pairs + 64)
    ctx.sweep_evaluate(1.0, 1.0, pass_table(cut), t, ent.size)
    st = ctx.stats()
    assert st['engine'] == 'sweep'
    a, b, I, U = ctx.edges(st['n_edges'])
    got = sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist()))
    assert st['matched_pairs'] == n_pairs                       # every run evaluated exactly once
    assert st['n_edges'] == len(edges)
    assert got == edges
    np.testing.assert_array_equal(ctx.fwd_degree(), fwd)
    assert st['max_fwd'] == (int(fwd.max()) if fwd.size else 0)
    # a read's forward edges are one run of the edge list (reads of up to 256 edges: one stage)
    if a.size:
        u, c = np.unique(a[np.r_[True, a[1:] != a[:-1]]], return_counts=True)
        assert all(fwd[x] > 256 for x in u[c > 1].tolist()), u[c > 1][:8]
    return edges


def check(dev, L, ent):
    for cut in CUTS:
        evaluate(dev, L, ent, cut)


# ------------------------------------------------------------------------------ building runs
def split_even(total, k):
    k = max(1, min(k, total))
    return [total // k + (x < total % k) for x in range(k)]


def run_desc(rng, L, A, parts, b0=None, step=1):
    """One run: read A with partners b0, b0 + step, ... (default A + 1 ...), one per item of `parts`:
    m | (m, kind) | (m, kind, box) | (m, kind, box, B); kinds cycle through KINDS where not given."""
    desc = []
    B = A + 1 if b0 is None else b0
    for k, p in enumerate(parts):
        p = (p,) if isinstance(p, (int, np.integer)) else tuple(p)
        m = int(p[0])
        kind = p[1] if len(p) > 1 and p[1] is not None else KINDS[k % 4]
        box = p[2] if len(p) > 2 and p[2] else {}
        if len(p) > 3:
            B = p[3]
        if not isinstance(kind, str):
            c = np.asarray(kind)                                # explicit cells
        else:
            lim = {'perm': min(L[A], L[B]), 'row': L[B], 'col': L[A]}.get(kind)
            if lim is not None and m > lim and not box:
                kind = 'both'
            c = pr.cells(rng, int(L[A]), int(L[B]), m, kind, **box)
        desc.append((A, B, c))
        B += step
    return desc


def runs_desc(rng, L, lengths, sizes=(1, 2, 3, 4, 5, 6), a0=0):
    """Consecutive runs A = a0, a0 + 1, ... of the given lengths, each spread over partners of
    1..6 entries (sizes cycling, the last partner taking the rest)."""
    desc = []
    for r, n in enumerate(lengths):
        parts, left, k = [], n, r
        while left > 0:
            m = min(left, sizes[k % len(sizes)])
            parts.append(m)
            left -= m
            k += 1
        desc += run_desc(rng, L, a0 + r, parts, b0=a0 + len(lengths) + r)
    return desc


def layout(ent):
    """[(A, first sorted position, length)] of the runs after the grouping by A."""
    a = np.sort(pr.unpack(ent)[0])
    heads = np.flatnonzero(np.r_[True, a[1:] != a[:-1]])
    return [(int(a[h]), int(h), int(e - h)) for h, e in zip(heads, np.r_[heads[1:], a.size])]


def paths(ent):
    """{A: 'group' | 'buckets' | 'partition'}: how k_sweep_pairs takes each run (restated from its
    constants to check the cases' inputs); asserts the partition path's documented limit of 64
    partners per pass."""
    a, b, _, _ = pr.unpack(ent)
    out = {}
    for A in np.unique(a).tolist():
        B = b[a == A]
        n = B.size
        if n <= 128:
            out[A] = 'group'
            continue
        P = (n + 95) // 96
        cnt = np.bincount((((B * 0x9E3779B1) & 0xFFFFFFFF) >> 8) % P, minlength=P)
        if P <= 64 and cnt.max() <= 128:
            out[A] = 'buckets'
            continue
        npass = (n + 39) // 40
        part = (((np.unique(B) * 0x85EBCA6B) & 0xFFFFFFFF) >> 8) % npass
        assert np.bincount(part).max() <= 64
        out[A] = 'partition'
    return out


def bucketed_parts(rng, length, A, sizes=(1, 2, 3, 4, 5, 6), cap=120, pool=range(8, N_DIR)):
    """Partners (m, None, None, B) summing to `length` whose hash buckets all stay at or below `cap`
    entries, so long_run_buckets accepts the run."""
    P = (length + 95) // 96
    cnt = np.zeros(P, np.int64)
    parts, left, k = [], length, 0
    for B in pool:
        if left == 0:
            break
        if B <= A:
            continue
        m = min(left, sizes[k % len(sizes)])
        bk = (((B * 0x9E3779B1) & 0xFFFFFFFF) >> 8) % P
        if cnt[bk] + m > cap:
            continue
        cnt[bk] += m
        parts.append((m, None, None, B))
        left -= m
        k += 1
    assert left == 0
    return parts


# ------------------------------------------------------------------------------ network sizes
@pytest.mark.parametrize('n', [1, 2, 31, 32, 33, 63, 64, 65, 127, 128])
def test_one_run_at_the_network_sizes(dev, n):
    """A single run of n entries is one group (n <= kStageE, last_done since it ends the array): the
    32-element network for n <= 32, 64 for n <= 64, else 128, at both sides of each threshold.  The
    run is spread over min(n, 3 + n % 7) partners with permutation, shared-row, shared-column and
    mixed patterns in turn; the highest partner, the last segment of the sorted group (it ends at
    position n: PH[nseg] = gend closes it), has shared rows and columns."""
    rng = np.random.default_rng(n)
    sizes = [2] if n == 2 else split_even(n, 3 + n % 7)
    parts = [(m, KINDS[k % 4]) for k, m in enumerate(sizes)]
    parts[-1] = (sizes[-1], 'both' if sizes[-1] >= 4 else 'row')     # both guarantee a shared row from 2 entries on
    desc = run_desc(rng, L_DIR, 0, parts, b0=4, step=4)
    ent = pr.build_entries(desc, L_DIR, seed=n)
    assert layout(ent) == [(0, 0, n)] and paths(ent) == {0: 'group'}
    if n > 1:
        I, m = pr.pair_intersections(ent)[desc[-1][:2]]
        assert I < m
    check(dev, L_DIR, ent)


# ------------------------------------------------------------------------------ the lane 63 / 64 seam
SEAM_ROW = [(0, 0), (1, 1), (2, 2), (3, 3), (3, 4), (4, 5), (5, 6), (6, 7)]       # sorted entries 3 and 4 share row 3
SEAM_COL = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 3), (5, 5), (6, 6), (7, 7)]       # sorted entries 3 and 4 share column 3
SEAM_HEAD = [(0, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 4), (5, 6), (6, 7)]      # entries 0 and 1 share row 0


@pytest.mark.parametrize('first,cells,want', [(60, SEAM_ROW, 7), (60, SEAM_COL, 7), (64, SEAM_HEAD, 6),
                                              (63, SEAM_HEAD, 6)])
def test_segment_across_the_lane_seam(dev, first, cells, want):
    """A 128-entry group holds its sorted keys two per lane: positions 0..63 in the first register,
    64..127 in the second, and position 64 compares with position 63 through a shuffle of its own
    (q1 of lane 0 = k0 of lane 63).  Partners 4, 8, 12 of read 0 have `first`, 8 and 120 - `first`
    entries, so partner 8's segment lies at sorted positions first .. first + 7.  first = 60: the
    repeated row (its columns all differ: only the adjacent-row flag sends the segment to first-fit)
    or the shared column is exactly the position pair (63, 64).  first = 64: the segment's head is
    position 64 and its repeated row is (64, 65); first = 63: the head is lane 63 and the repeated
    row crosses the seam."""
    rng = np.random.default_rng(first)
    desc = run_desc(rng, L_DIR, 0, [(first, 'perm'), (8, np.array(cells)), (120 - first, 'perm')], b0=4, step=4)
    ent = pr.build_entries(desc, L_DIR, seed=first)
    assert layout(ent) == [(0, 0, 128)]
    b = np.sort(ent) >> 14 & pr.RANK_MASK
    assert np.flatnonzero(b == 8).tolist() == list(range(first, first + 8))
    assert pr.pair_intersections(ent)[(0, 8)] == (want, 8)
    check(dev, L_DIR, ent)


# ------------------------------------------------------------------------------ row / column bit ranges
BOXES = {'low': dict(ihi=32, jhi=32), 'high': dict(ilo=32, jlo=32), 'across': dict(ilo=27, jlo=29),
         'rows_high': dict(ilo=32, jhi=32), 'cols_high': dict(ihi=32, jlo=32)}


def box_parts(m=12):
    return [(m, kind, box) for box in BOXES.values() for kind in ('row', 'col', 'both')]


def test_group_row_and_column_ranges(dev):
    """Group path: conflicting pairs whose rows / columns lie in 0..31 only, in 32..63 only, and
    across both (the segment's column mask PJ is one 64-bit word, `used` of the first-fit another).
    15 partners of 8 entries per run, two runs: 120 entries each, one group per run."""
    rng = np.random.default_rng(7)
    desc = run_desc(rng, L_DIR, 0, box_parts(8), b0=4, step=4) + run_desc(rng, L_DIR, 4, box_parts(8), b0=8, step=4)
    ent = pr.build_entries(desc, L_DIR, seed=7)
    assert [x[1:] for x in layout(ent)] == [(0, 120), (120, 120)] and set(paths(ent).values()) == {'group'}
    check(dev, L_DIR, ent)


@pytest.mark.parametrize('others', [False, True])
def test_full_block_pair(dev, others):
    """The full 64 x 64 block of one pair: 4096 entries, I = 64.  Alone in its run: P = 43 buckets but
    the pair's bucket holds all 4096 > 128, so long_run_buckets declines and the run takes 103 partner
    partitions with one partner, whose conflict flag sends it through ordered_I with every row mask
    full in both halves.  With `others` the same block is one of six partners of the run."""
    rng = np.random.default_rng(11)
    parts = [(4096, 'full', None, 4)]
    if others:
        parts += [(20, 'perm', None, 8), (30, 'both', None, 12), (10, 'row', None, 16), (64, 'perm', None, 20),
                  (9, 'col', None, 24)]
    ent = pr.build_entries(run_desc(rng, L_DIR, 0, parts), L_DIR, seed=11)
    assert paths(ent) == {0: 'partition'}
    assert pr.pair_intersections(ent)[(0, 4)] == (64, 4096)
    check(dev, L_DIR, ent)


# ------------------------------------------------------------------------------ groups of several runs
@pytest.mark.parametrize('lengths', [
    [3] * 40,                      # 40 runs in one group of 120 entries (RUNA / RUNF slots 0..39)
    [3] * 50,                      # 150 entries: the window holds 42 whole runs and two entries of the 43rd
    [50, 78, 30, 98, 128, 5],      # a run ends exactly at window position 128, twice; then a run of 128
    [128, 1],                      # a full-window run, then the array's last entry as its own group
    [1], [60, 67], [60, 68], [60, 69], [100] * 5 + [12], [100] * 5 + [13], [128] * 5,
], ids=lambda x: '-'.join(map(str, x)) if len(x) < 7 else f'{len(x)}x{x[0]}')
def test_groups_of_runs_and_window_ends(dev, lengths):
    """A window is the next 128 entries; the group is its whole runs.  Its end `gend` is the first head
    after the last owned head, or the window's end when the entry after the window starts a new run
    (last_done) or the array ends there.  [50, 78, ...]: run 1 ends at window position 128 and run 2
    begins there; [98, 128]: a run of exactly 128 right after a group.  The last run ends at
    n = 1, 127, 128, 129, 512, 513 and 640 (the window past n is padding)."""
    rng = np.random.default_rng(len(lengths) + lengths[0])
    ent = pr.build_entries(runs_desc(rng, L_DIR, lengths), L_DIR, seed=sum(lengths))
    assert [x[2] for x in layout(ent)] == lengths and set(paths(ent).values()) == {'group'}
    check(dev, L_DIR, ent)


# ------------------------------------------------------------------------------ chunk ownership
@pytest.mark.parametrize('lengths,starts', [
    ([100] * 5 + [40, 60, 30], {5: 500}),                # a run over [500, 540): it crosses 512, chunk 0 owns it
    ([100] * 5 + [11, 30, 60], {6: 511}),                # a run starting at 511, the chunk's last entry
    ([100] * 5 + [12, 30, 60], {6: 512}),                # at 512: the first entry of chunk 1 is a head
    ([100] * 5 + [13, 30, 60], {6: 513}),                # at 513: chunk 1 skips the entry of chunk 0's last run
    ([100] * 3 + [1000, 7, 90, 128, 3], {3: 300}),       # [300, 1300): chunk 1 = [512, 1024) has no run start
    ([100, 1500] + [20] * 12, {1: 100, 2: 1600}),        # chunk 0 to chunk 3, then short runs chunk 3 owns
])
def test_chunk_ownership(dev, lengths, starts):
    """A wave owns the runs that start in its 512-entry chunk: it skips the run in progress at the
    chunk's first entry (next_run from a_at(c0 - 1)) and finishes its own last run beyond the chunk's
    end.  Each run must be evaluated exactly once: matched_pairs equals the reference's pair count and
    every edge appears once."""
    rng = np.random.default_rng(lengths[5] if len(lengths) > 5 else 1)
    desc = []
    for r, n in enumerate(lengths):
        if n > 128:
            desc += run_desc(rng, L_DIR, r, bucketed_parts(rng, n, r, pool=range(100, N_DIR)))
        else:
            desc += runs_desc(rng, L_DIR, [n], a0=r)
    ent = pr.build_entries(desc, L_DIR, seed=lengths[-1])
    lay = layout(ent)
    assert [x[2] for x in lay] == lengths
    assert {r: lay[r][1] for r in starts} == starts
    check(dev, L_DIR, ent)


# ------------------------------------------------------------------------------ bucketed long runs
@pytest.mark.parametrize('n,single', [(129, False), (192, False), (193, False), (1000, False), (6144, False),
                                      (1000, True)])
def test_bucketed_long_runs(dev, n, single):
    """A run of n > 128 entries goes alone (gend = 0).  P = ceil(n / 96) = 2, 2, 3, 11, 64 buckets, the
    partners chosen so that no bucket exceeds 120 entries: long_run_buckets takes it, sorts each
    bucket by (B, i, j) (a network size per bucket count) and runs the same segment first-fit with
    the keys shifted by 7 bits (i at bit 14, j at bit 7).  Partners of 1..6 entries with every
    pattern in turn; `single`: one entry per partner, the pile-up shape, as the control.  A short run
    before and after it shares the wave's edge stage."""
    rng = np.random.default_rng(n + single)
    parts = bucketed_parts(rng, n, 1, sizes=(1,) if single else (1, 2, 3, 4, 5, 6), cap=128 if n == 6144 else 120)
    desc = runs_desc(rng, L_DIR, [30], a0=0) + run_desc(rng, L_DIR, 1, parts) + runs_desc(rng, L_DIR, [17], a0=2)
    ent = pr.build_entries(desc, L_DIR, seed=n)
    assert [x[2] for x in layout(ent)] == [30, n, 17]
    assert paths(ent) == {0: 'group', 1: 'buckets', 2: 'group'}
    if not single:
        assert sum(I != m for I, m in pr.pair_intersections(ent).values()) > n // 8
    check(dev, L_DIR, ent)


def test_bucketed_row_and_column_ranges(dev):
    """The bit-range patterns of test_group_row_and_column_ranges inside a bucketed run (15 partners
    of 12 entries = 180 entries, P = 2)."""
    rng = np.random.default_rng(3)
    pool = [B for B in range(4, N_DIR, 4)]
    parts, cnt = [], [0, 0]
    it = iter(pool)
    for m, kind, box in box_parts(12):
        B = next(it)
        while cnt[(((B * 0x9E3779B1) & 0xFFFFFFFF) >> 8) % 2] + m > 120:
            B = next(it)
        cnt[(((B * 0x9E3779B1) & 0xFFFFFFFF) >> 8) % 2] += m
        parts.append((m, kind, box, B))
    ent = pr.build_entries(run_desc(rng, L_DIR, 0, parts), L_DIR, seed=3)
    assert paths(ent) == {0: 'buckets'}
    check(dev, L_DIR, ent)


# ------------------------------------------------------------------------------ partition-path long runs
@pytest.mark.parametrize('big', [129, 300])
def test_partition_run_with_one_heavy_partner(dev, big):
    """One partner with `big` > 128 conflicting entries: its bucket exceeds kStageE, long_run_buckets
    declines (having written nothing) and the run takes ceil(len / 40) partner partitions over the
    LDS hash.  The 20 small partners alternate conflict-free patterns (I = the entry count: the
    popcount path) and the bit-range conflict patterns (the conflict flag: ordered_I over RR's row
    masks, low and high halves); some pass holds both kinds."""
    rng = np.random.default_rng(big)
    small = []
    for k, (m, kind, box) in enumerate(box_parts(6)[:10]):
        small += [(m, kind, box), (3 + k % 5, 'perm', None)]
    parts = [(big, 'both', None, 8)] + [(m, kind, box, 12 + 4 * k) for k, (m, kind, box) in enumerate(small)]
    desc = runs_desc(rng, L_DIR, [40], a0=0) + run_desc(rng, L_DIR, 4, parts)
    ent = pr.build_entries(desc, L_DIR, seed=big)
    assert paths(ent) == {0: 'group', 4: 'partition'}
    n = layout(ent)[1][2]
    npass = (n + 39) // 40
    pi = pr.pair_intersections(ent)
    by_pass = {}
    for (a, b), (I, m) in pi.items():
        if a == 4:
            by_pass.setdefault((((b * 0x85EBCA6B) & 0xFFFFFFFF) >> 8) % npass, set()).add(I != m)
    assert any(v == {True, False} for v in by_pass.values())
    check(dev, L_DIR, ent)


def test_partition_run_beyond_64_buckets(dev):
    """A run of 6200 entries over 40 partners: P = 65 > 64 buckets, so the partition path, in 155
    passes; with 40 partners no pass can exceed kPairLimit = 64.  Eight partners are full
    permutations (no conflict: popcount), 32 have 128..213 entries with shared rows and columns
    (ordered_I)."""
    rng = np.random.default_rng(6200)
    parts = [(64, 'perm', None, 8 + 4 * k) for k in range(8)]
    left = 6200 - 64 * 8
    parts += [(m, 'both', None, 40 + 4 * k) for k, m in enumerate(split_even(left, 32))]
    ent = pr.build_entries(run_desc(rng, L_DIR, 0, parts) + runs_desc(rng, L_DIR, [9, 100], a0=1), L_DIR, seed=6200)
    assert [x[2] for x in layout(ent)] == [6200, 9, 100]
    assert paths(ent) == {0: 'partition', 1: 'group', 2: 'group'}
    check(dev, L_DIR, ent)


# ------------------------------------------------------------------------------ the edge stage
@pytest.mark.parametrize('lengths,single_long', [
    ([100, 100, 100, 100, 100], 0),          # 500 single-entry pairs in chunk 0: > 256 edges, a flush every second group
    ([100, 100, 100], 0),                    # 200 staged, the third group's 100 segments do not fit: the early flush
    ([100] * 5, 300),                        # 500 staged edges, then a bucketed run of 300 partners: > 512 edges on one wave
    ([90], 400),                             # a long run right after a partly filled stage
])
def test_edge_stage_flushes(dev, lengths, single_long):
    """Runs of single-entry pairs: under the cut (0.0,) every pair is an edge, so a group of g entries
    stages g edges.  The stage holds 256: a group whose segments would not fit flushes it first
    (es.n + nseg > 256), a long run flushes it before its first edge and then every 256 (its read has
    more than 256 forward edges, the one case where a read's edges may be split).  Under the default
    cuts a single match of two reads of 3..64 intervals never passes, so the stage stays empty and the
    same layout must leave no edge behind."""
    rng = np.random.default_rng(sum(lengths) + single_long)
    desc = []
    for r, n in enumerate(lengths):
        desc += run_desc(rng, L_DIR, r, [(1, 'perm')] * n, b0=50 + r)
    if single_long:
        A = len(lengths)
        desc += run_desc(rng, L_DIR, A, bucketed_parts(rng, single_long, A, sizes=(1,), pool=range(60, N_DIR)))
    desc += runs_desc(rng, L_DIR, [25], a0=len(lengths) + 1)
    ent = pr.build_entries(desc, L_DIR, seed=7)
    assert [x[2] for x in layout(ent)] == lengths + ([single_long] if single_long else []) + [25]
    edges = evaluate(dev, L_DIR, ent, CUTS[0])
    assert len(edges) == len(pr.pair_intersections(ent)) > 256
    evaluate(dev, L_DIR, ent, CUTS[1])


def test_edge_stage_partly_filled_by_the_cuts(dev):
    """Short reads (2..5 intervals) under the default cuts: about a fifth of the pairs pass (11..25 per
    group of 100), so the stage fills unevenly across 12 groups and a long run of 200 partners, 57 of
    them edges, starts on a partly filled stage."""
    rng = np.random.default_rng(21)
    L = rng.integers(2, 6, 1200)
    desc = []
    for r in range(12):
        for k in range(100):
            B = 20 + (r * 37 + k * 11) % 1100
            m = int(rng.integers(1, min(L[r], L[B]) + 1))
            desc.append((r, B, pr.cells(rng, int(L[r]), int(L[B]), m, 'perm')))
    for k in range(200):
        B = 20 + 5 * k
        desc.append((12, B, pr.cells(rng, int(L[12]), int(L[B]), int(min(L[12], L[B])), 'perm')))
    ent = pr.build_entries(desc, L, seed=21)
    edges, _, n_pairs = pr.evaluate_entries(ent, L, CUTS[1])
    assert 200 < len(edges) < n_pairs - 200
    check(dev, L, ent)


# ------------------------------------------------------------------------------ grouping by A
@pytest.mark.parametrize('n_reads', [2, 65, 4097, 70000])
def test_grouping_by_a_lowest_and_highest_ranks(dev, n_reads):
    """The grouping's counting sort splits A into hb high and lo low bits from n_reads: 1, 7, 13 and
    17 bits here.  The same entry pattern sits on the four lowest and the four highest ranks (the
    first and last bins of both passes); every other read has one interval and no entry: its forward
    degree must read 0."""
    rng = np.random.default_rng(n_reads)
    L = np.ones(n_reads, np.int64)
    groups = [[0, 1]] if n_reads == 2 else [[0, 1, 2, 3], list(range(n_reads - 4, n_reads))]
    desc = []
    for g in groups:
        L[g] = [64, 56, 48, 40][:len(g)]
    for g in groups:
        pairs = [(g[0], g[1])] if len(g) == 2 else [(g[0], g[1]), (g[0], g[2]), (g[0], g[3]), (g[1], g[3]), (g[2], g[3])]
        for k, (a, b) in enumerate(pairs):
            desc.append((a, b, pr.cells(rng, int(L[a]), int(L[b]), 9 + 5 * k, KINDS[(k + 1) % 4])))
    ent = pr.build_entries(desc, L, seed=n_reads)
    check(dev, L, ent)


# ------------------------------------------------------------------------------ context reuse
def test_context_reuse(dev):
    """One context, three entry sets in a row: a large one (group, bucketed and partition runs), a
    small one on other reads, and none.  No edge or forward degree of an earlier set may remain
    (evaluate compares fwd_degree() of every read), and components() after each equals a union-find
    over the reference's edges."""
    rng = np.random.default_rng(99)
    big = runs_desc(rng, L_DIR, [100, 128, 3, 77] * 6, a0=0) + \
        run_desc(rng, L_DIR, 24, bucketed_parts(rng, 700, 24, pool=range(200, N_DIR))) + \
        run_desc(rng, L_DIR, 28, [(200, 'both', None, 32), (5, 'perm', None, 36), (7, 'row', None, 40)])
    small = runs_desc(rng, L_DIR, [5, 9], a0=3000)
    sets = [pr.build_entries(big, L_DIR, seed=1), pr.build_entries(small, L_DIR, seed=2), np.zeros(0, np.int64)]
    assert set(paths(sets[0]).values()) == {'group', 'buckets', 'partition'}
    for ent in sets + sets[:1]:
        for cut in CUTS:
            edges = evaluate(dev, L_DIR, ent, cut)
            dev.ctx.components()
            np.testing.assert_array_equal(dev.ctx.labels(), pr.union_find_labels(N_DIR, edges))
    st = dev.ctx.stats()
    assert st['n_edges'] > 0


# ------------------------------------------------------------------------------ randomised
SEEDS = [101, 102, 103, 104, 105, 106, 107, 108]


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """300 reads of 1..64 intervals; each A has 0..60 partners; a pair has one entry (70 %), a sparse
    random subset of its L_A x L_B matrix (about 1/128 of it, 29 %), half of it (0.4 %) or all of it (0.2 %)."""
    rng = np.random.default_rng(seed)
    n = 300
    L = rng.integers(1, 65, n)
    desc = []
    for a in range(n - 1):
        k = min(n - 1 - a, int(rng.integers(0, 61)))
        for b in np.sort(rng.choice(np.arange(a + 1, n), size=k, replace=False)).tolist():
            box = int(L[a] * L[b])
            u = rng.random()
            m = 1 if u < 0.70 else max(2, box // 128) if u < 0.994 else box // 2 if u < 0.998 else box
            m = max(1, min(m, box))
            flat = rng.permutation(box)[:m]
            desc.append((a, b, np.stack(np.divmod(flat, int(L[b])), axis=1)))
    return L, pr.build_entries(desc, L, seed)


@pytest.mark.parametrize('seed', SEEDS)
def test_random_entry_sets(dev, seed):
    """Random entry sets with every density.  Conditions on the input, asserted before the device is
    touched: 5k..80k entries, at least 1000 pairs whose I differs from their entry count, and a run
    longer than 128 entries."""
    L, ent = random_case(seed)
    assert 5_000 <= ent.size <= 80_000, ent.size
    assert sum(I != m for I, m in pr.pair_intersections(ent).values()) >= 1000
    assert max(x[2] for x in layout(ent)) > 128
    paths(ent)
    check(dev, L, ent)


# ------------------------------------------------------------------------------ stacked pile-ups, both engines
PILEUPS = [(3, 16, 400, 14), (40, 8, 400, 1), (12, 24, 400, 1), (200, 2, 300, 1), (3, 64, 400, 34)]     # n, L, jit, seed


@functools.lru_cache(maxsize=None)
def pileup(n, L, jit, seed):
    """n reads of L intervals each, all on one locus: start = 5000 + U[0, jit], end = start + 1000 +
    U[0, jit], aln = end - start.  A read's intervals in start order, the reads ranked by their first
    start, data_pos each interval's position in the stable start order: what prepare_data gives."""
    rng = np.random.default_rng(seed)
    start = 5000 + rng.integers(0, jit + 1, (n, L))
    end = start + 1000 + rng.integers(0, jit + 1, (n, L))
    o = np.argsort(start, axis=1, kind='stable')
    start, end = np.take_along_axis(start, o, 1), np.take_along_axis(end, o, 1)
    r = np.argsort(start[:, 0], kind='stable')
    start, end = start[r].reshape(-1), end[r].reshape(-1)
    dp = np.empty(n * L, np.int64)
    dp[np.argsort(start, kind='stable')] = np.arange(n * L)
    return dict(n=n, off=np.arange(n + 1, dtype=np.int64) * L, chrom=np.zeros(n * L, np.int32),
                start=start.astype(np.int32), end=end.astype(np.int32), aln=(end - start).astype(np.int64),
                q=np.full(n, 100, np.int32), m=np.full(n, 3, np.int32), dp=dp)


@functools.lru_cache(maxsize=None)
def pileup_oracle(shape, cutoffs, cap):
    p = pileup(*shape)
    per = np.repeat
    oc = O.OracleCSR(p['off'], p['chrom'], p['start'], p['end'], p['aln'], per(p['q'], shape[1]), per(p['m'], shape[1]),
                     p['dp'])
    if cap is None:
        return O.run_core(oc, 0.8, cutoffs, 0.04, 0.25, use_cap=False)
    return O.run_core(oc, 0.8, cutoffs, 0.04, 0.25, edge_threshold=cap, use_cap=True)


def pileup_run(ctx, p, cutoffs, engine, cap=None):
    ctx.set_reads(p['off'], p['q'], p['m'], p['chrom'], p['start'], p['end'], fold_overlap_threshold(p['aln'], 0.8), 1,
                  iv_data_pos=p['dp'])
    ctx.reserve_edges(p['n'] * p['n'])
    ctx.build_index()
    if engine == 'sweep':            # no rerun: a fallback to the walk engine or an overflow fails here
        ctx.query(1 - 0.04, 1 - 0.25, pass_table(cutoffs), engine='sweep')
        st = ctx.stats()
    else:
        st = ctx.run_query(1 - 0.04, 1 - 0.25, pass_table(cutoffs), engine=engine)
    assert st['engine'] == engine
    if cap is not None:
        st['cap'] = ctx.apply_edge_cap(cap)
        st['n_edges'] = ctx.stats()['n_edges']
        st['max_fwd'] = st['cap']['max_fwd']
    ctx.components()
    a, b, I, U = ctx.edges(st['n_edges'])
    return dict(stats=st, labels=ctx.labels(), fwd=ctx.fwd_degree(), a=a, b=b, I=I, U=U)


@pytest.mark.parametrize('engine', parity.ENGINES)
@pytest.mark.parametrize('cutoffs', CUTS, ids=['cut0', 'default'])
@pytest.mark.parametrize('shape', PILEUPS, ids=lambda s: f'{s[0]}x{s[1]}')
def test_stacked_pileup_vs_oracle(dev, shape, cutoffs, engine):
    """Reads whose intervals all stack on one locus: a read pair's matches share rows and columns
    because of the geometry, so k_sweep<2> must emit the conflicting entries and the walk engine
    must reach the same I through its match list, slow path and deferred path.  The oracle's I
    takes at least two values below L (asserted on the CPU first; with L = 2 only I = 1 lies below
    L, and both 1 and 2 must occur)."""
    o0 = pileup_oracle(shape, CUTS[0], None)
    assert np.unique(o0['edge_I'][o0['edge_I'] < shape[1]]).size >= min(2, shape[1] - 1)
    assert np.unique(o0['edge_I']).size >= 2
    dev.L = None
    g = pileup_run(dev.ctx, pileup(*shape), cutoffs, engine)
    parity.compare_with_oracle(g, pileup_oracle(shape, cutoffs, None), shape[0])


@pytest.mark.parametrize('engine', parity.ENGINES)
def test_stacked_pileup_capped_vs_oracle(dev, engine):
    """(40, 8): every pair is an edge under (0.0,), forward degrees up to 39, so the cap of 10 binds."""
    shape = PILEUPS[1]
    o = pileup_oracle(shape, CUTS[0], 10)
    assert pileup_oracle(shape, CUTS[0], None)['fwd'].max() == 39
    dev.L = None
    g = pileup_run(dev.ctx, pileup(*shape), CUTS[0], engine, cap=10)
    assert g['stats']['cap']['applied'] == 1 and g['stats']['cap']['capped'] > 0
    parity.compare_capped_with_oracle(g, o, shape[0])


def test_stacked_pileup_score_pairs(dev):
    """fslr_score_pairs on all 780 pairs of the (40, 8) pile-up: the oracle's I and U."""
    shape = PILEUPS[1]
    p, o = pileup(*shape), pileup_oracle(shape, CUTS[0], None)
    assert o['edge_a'].size == 780
    dev.L = None
    dev.ctx.set_reads(p['off'], p['q'], p['m'], p['chrom'], p['start'], p['end'], fold_overlap_threshold(p['aln'], 0.8),
                      1, iv_data_pos=p['dp'])
    I, U, flags = dev.ctx.score_pairs(o['edge_a'], o['edge_b'], 1 - 0.04, 1 - 0.25, pass_table(CUTS[0]))
    np.testing.assert_array_equal(I, o['edge_I'])
    np.testing.assert_array_equal(U, o['edge_U'])
    assert (flags & _lib.SCORE_EDGE).all()
