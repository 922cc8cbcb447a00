"""A plain reference of the edge cap (cluster.py:197-224) that shows its intermediate steps.  TEST
INFRASTRUCTURE ONLY: pure Python / numpy, written from the text of the reference loop and the
documented stand-in order of the interval search (hits are end-inclusive; a list is in descending
(start, -end, data position) order; the query read's own intervals are dropped).  It shares no code
with oracle/fslr_oracle.c or cap.hip; tests/test_cap_ref.py pins it to the oracle and to
tests/sweep_emu.py.

  closure(n, rows, fwd, thr)     T and each member's Kleene round
  visit_lists(csr, reads)        per interval of each listed read: the partner reads in search order
  replay(csr, params, thr)       the loop with its seen-set: edges, breaks, walks
  expected(csr, params, thr)     E*, T, the capped graph and the counts fslr_cap_stats reports
"""
from __future__ import annotations

import numpy as np

DEFAULT = dict(overlap=0.8, cutoffs=(1, 1, 0.66, 0.66, 0.66, 0.5), qlen_diff=0.04, nal_diff=0.25)


# ------------------------------------------------------------------------------------ closure
def closure(n, rows, fwd, thr):
    """T by the rank-ordered definition: x joins when fwd(x) + #{y in T, y < x, (y, x) in rows} >= thr.
    Returns (T sorted, {member: round}): round 0 are the seeds (fwd >= thr), round r the reads that
    reach thr with the back counts of the members of the rounds below r (Kleene iteration); the
    largest round is the closure's depth.  Both constructions must give the same set."""
    adj = {}
    for a, b in np.asarray(rows, dtype=np.int64).reshape(-1, 2).tolist():
        assert 0 <= a < b < n, (a, b)
        adj.setdefault(a, []).append(b)
    back = [0] * n
    T = []
    for x in range(n):
        if fwd[x] + back[x] >= thr:
            T.append(x)
            for y in adj.get(x, ()):
                back[y] += 1
    rnd = {x: 0 for x in range(n) if fwd[x] >= thr}
    cnt = [0] * n
    frontier, r = sorted(rnd), 0
    while frontier:
        r += 1
        touched = set()
        for x in frontier:
            for y in adj.get(x, ()):
                cnt[y] += 1
                touched.add(y)
        frontier = sorted(y for y in touched if y not in rnd and fwd[y] + cnt[y] >= thr)
        for y in frontier:
            rnd[y] = r
    assert sorted(rnd) == T
    return T, rnd


def depth(rounds):
    return max(rounds.values()) if rounds else -1


# ------------------------------------------------------------------------------------ visit lists
def _columns(csr):
    off = np.asarray(csr.read_off, np.int64)
    read_of = np.repeat(np.arange(off.size - 1), np.diff(off))
    return (off, read_of, np.asarray(csr.iv_chrom, np.int64), np.asarray(csr.iv_start, np.int64),
            np.asarray(csr.iv_end, np.int64), np.asarray(csr.data_pos, np.int64))


def visit_lists(csr, reads, with_intervals=False):
    """For each interval (CSR order) of each read of `reads`: the partner reads of its hits in search
    order.  A hit of interval k is an interval p of the same chromosome with start_p <= end_k and
    end_p >= start_k (both ends inclusive); the list descends by (start, -end, data position); the
    intervals of k's own read are left out (cluster.py:203-204)."""
    off, read_of, ch, st, en, dp = _columns(csr)
    out = []
    for x in reads:
        for k in range(off[x], off[x + 1]):
            h = np.flatnonzero((ch == ch[k]) & (st <= en[k]) & (en >= st[k]) & (read_of != x))
            h = h[np.lexsort((dp[h], -en[h], st[h]))[::-1]]
            out.append(h.tolist() if with_intervals else read_of[h].tolist())
    return out


# ------------------------------------------------------------------------------------ the pair predicate
def lengths_differ(q1, q2, n1, n2, qlen_diff, nal_diff):
    """cluster.py:178-183 (raises ZeroDivisionError as the reference does)."""
    if min(q1, q2) / max(q1, q2) >= 1 - qlen_diff:
        return False
    if min(n1, n2) / max(n1, n2) >= 1 - nal_diff:
        return False
    return True


def jaccard(l1, l2, overlap):
    """cluster.py:140-170 on two lists of (chrom, start, end, aln): rows of l1 in order, each takes the
    first unused element of l2 it matches; returns (I, U)."""
    used = [False] * len(l2)
    I = 0
    for c1, s1, e1, a1 in l1:
        for j, (c2, s2, e2, a2) in enumerate(l2):
            if used[j]:
                continue
            if c1 != c2:
                continue
            o = max(0, min(e1, e2) - max(s1, s2))
            if min(o / a1, o / a2) >= overlap:
                used[j] = True
                I += 1
                break
    return I, len(l1) + len(l2) - I


def is_edge(I, U, cutoffs):
    if I == 0:
        return False
    target = cutoffs[I - 1] if I - 1 < len(cutoffs) else cutoffs[-1]
    return I / U >= target


class Pairs:
    """The predicate of a read pair (query read first), cached: (counted, edge, I, U); counted = the
    pair passes the length gate with I > 0 (the pairs after which :223 checks the cap)."""

    def __init__(self, csr, params):
        off, _, ch, st, en, _ = _columns(csr)
        aln = np.asarray(csr.iv_aln, np.int64)
        self.items = [[(int(ch[k]), int(st[k]), int(en[k]), int(aln[k])) for k in range(off[x], off[x + 1])]
                      for x in range(off.size - 1)]
        self.q = np.asarray(csr.read_qlen2, np.int64).tolist()
        self.m = np.asarray(csr.read_nal, np.int64).tolist()
        self.p = params
        self.memo = {}

    def __call__(self, x, y):
        got = self.memo.get((x, y))
        if got is None:
            p = self.p
            if lengths_differ(self.q[x], self.q[y], self.m[x], self.m[y], p['qlen_diff'], p['nal_diff']):
                got = (False, False, 0, 0)
            else:
                I, U = jaccard(self.items[x], self.items[y], p['overlap'])
                got = (I > 0, is_edge(I, U, p['cutoffs']), I, U)
            self.memo[(x, y)] = got
        return got


# ------------------------------------------------------------------------------------ the loop
def replay(csr, params=DEFAULT, thr=10, use_cap=True):
    """cluster.py:197-224.  Returns a dict:
      edges   [(former, partner, I, U)] in the order the loops add them
      formed  edges added per read's own loop
      breaks  {read: (interval index, list index)} of each read's first break (:223-224)
      walks   {read: [(interval index, list index | None, 'edge' | 'counted' | None)]}: for each
              interval after the break, where its walk stopped (None: it ran off the end) and whether
              the pair it stopped at became an edge or was only counted
    use_cap False never breaks (E*: every candidate pair from its lower read)."""
    n = int(np.asarray(csr.read_off).size - 1)
    lists = visit_lists(csr, range(n))
    off = np.asarray(csr.read_off, np.int64)
    pred = Pairs(csr, params)
    seen = set()
    edges, formed, breaks, walks = [], [0] * n, {}, {}
    for x in range(n):
        count = 0
        for ii, k in enumerate(range(off[x], off[x + 1])):
            stop = None
            for pos, y in enumerate(lists[k]):
                b = (x, y) if x < y else (y, x)
                if b in seen:
                    continue
                seen.add(b)
                counted, edge, I, U = pred(x, y)
                if not counted:
                    continue
                if edge:
                    edges.append((x, y, I, U))
                    count += 1
                if use_cap and count >= thr:
                    stop = (pos, 'edge' if edge else 'counted')
                    break
            if stop is not None and x not in breaks:
                breaks[x] = (ii, stop[0])
                walks[x] = []
            elif x in breaks:
                walks[x].append((ii,) + (stop if stop is not None else (None, None)))
        formed[x] = count
    return dict(edges=edges, formed=np.array(formed, np.int64), breaks=breaks, walks=walks)


def components(n, edges):
    """Component index per read as the reference numbers them (by first member, singletons -1)."""
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    for e in edges:
        a, b = find(e[0]), find(e[1])
        if a != b:
            par[max(a, b)] = min(a, b)
    root = [find(x) for x in range(n)]
    size = np.bincount(root, minlength=n)
    ids = {}
    return np.array([ids.setdefault(r, len(ids)) if size[r] >= 2 else -1 for r in root], np.int64)


def expected(csr, params=DEFAULT, thr=10):
    """Everything the device reports for one input: E* (the loop without the cap), T over E*, T's visit
    lists, the capped loop and the fslr_cap_stats counts."""
    n = int(np.asarray(csr.read_off).size - 1)
    star = replay(csr, params, thr, use_cap=False)
    rows = [(a, b) for a, b, _, _ in star['edges']]
    assert all(a < b for a, b in rows)
    T, rounds = closure(n, rows, star['formed'], thr)
    cap = replay(csr, params, thr)
    lists = visit_lists(csr, T)
    off = np.asarray(csr.read_off, np.int64)
    owner = np.repeat(np.arange(len(T)), [off[x + 1] - off[x] for x in T]) if T else np.zeros(0, np.int64)
    pairs = len({(int(t), y) for t, lst in zip(owner, lists) for y in lst})
    got = {(min(a, b), max(a, b)) for a, b, _, _ in cap['edges']}
    assert got <= set(rows) and set(cap['breaks']) <= set(T)
    stats = dict(applied=1, max_fwd=int(cap['formed'].max()) if n else 0, candidates=len(T), capped=len(cap['breaks']),
                 hits=sum(len(x) for x in lists), pairs=pairs, dropped=len(rows) - len(cap['edges']),
                 backward=sum(a > b for a, b, _, _ in cap['edges']))
    return dict(star=star, rows=rows, T=T, rounds=rounds, cap=cap, lists=lists, stats=stats)


def as_oracle(rep, n):
    """A replay result in the shape of oracle.run_core's (for the suite's comparison helpers)."""
    e = np.array(rep['edges'], np.int64).reshape(-1, 4)
    return dict(edge_a=e[:, 0], edge_b=e[:, 1], edge_I=e[:, 2], edge_U=e[:, 3], fwd=np.asarray(rep['formed']),
                comp=components(n, rep['edges']),
                stats=dict(n_edges=len(e), max_fwd=int(np.max(rep['formed'])) if n else 0))
