"""The expected result of the index's batched search (fslr_search), by brute force in numpy, and the
small inputs the search tests share."""
import numpy as np

from fslr_amd.prep import IntervalData


def brute_force(chrom, start, end, qc, qs, qe):
    """Per query (qc, qs, qe): a boolean mask of the predicate ``chrom == qc and start <= qe and end >=
    qs`` over the `data` list's columns, then np.lexsort on (data position, -end, start), reversed.
    Returns ``(offsets int64[nq + 1], data positions int64[total])``."""
    chrom, start, end = (np.asarray(x) for x in (chrom, start, end))
    start, end = start.astype(np.int64), end.astype(np.int64)
    out, off = [], [0]
    by_chrom = {}
    for c, s, e in zip(list(qc), list(qs), list(qe)):
        if c not in by_chrom:
            by_chrom[c] = np.flatnonzero(chrom == c)
        cand = by_chrom[c]
        m = cand[(start[cand] <= e) & (end[cand] >= s)]
        o = np.lexsort((m, -end[m], start[m]))
        out.append(m[o][::-1])
        off.append(off[-1] + m.size)
    return np.asarray(off, np.int64), (np.concatenate(out) if out else np.zeros(0)).astype(np.int64)


def make_data(chrom, start, end, qcode=None, shuffle_seed=None) -> IntervalData:
    """An IntervalData (the `data` list) of the given intervals in non-decreasing start order; ties of
    equal start keep the given order (or a seeded shuffle of it).  ``qcode`` None: one read per
    interval."""
    chrom, start, end = (np.asarray(x, np.int64) for x in (chrom, start, end))
    n = start.size
    first = np.arange(n) if shuffle_seed is None else np.random.default_rng(shuffle_seed).permutation(n)
    order = first[np.argsort(start[first], kind='stable')]
    q = np.arange(n, dtype=np.int64) if qcode is None else np.asarray(qcode, np.int64)
    aln = np.maximum(end - start, 1)
    return IntervalData(chrom=chrom[order], start=start[order], end=end[order], aln_size=aln[order], qcode=q[order],
                        qnames=np.asarray([f'q{k}' for k in range(int(q.max(initial=-1)) + 1)], dtype=object),
                        n_alignments=np.full(n, 3, np.int64), qlen2=np.full(n, 1000, np.int64),
                        middle=(aln // 2 + start)[order], index=np.arange(n, dtype=np.int64))


def tie_input(seed=5):
    """Runs of equal (chrom, start) of lengths 2, 63, 64, 65, 257 and 1100 among singletons, on two
    chromosomes; ends shuffled, several equal inside a run (so the data position decides).  Returns
    (data, queries) with the queries cutting each run at every distinct end."""
    rng = np.random.default_rng(seed)
    chrom, start, end = [], [], []
    pos = 1000
    for c, runs in ((7, (2, 63, 1100)), (9, (64, 65, 257))):
        for run in runs:
            for _ in range(int(rng.integers(3, 40))):            # singletons between the runs
                chrom.append(c), start.append(pos), end.append(pos + int(rng.integers(1, 400)))
                pos += int(rng.integers(1, 30))
            ends = pos + rng.integers(1, max(3, run // 3), run)   # ~3 intervals per distinct end
            chrom += [c] * run
            start += [pos] * run
            end += ends.tolist()
            pos += int(rng.integers(1, 30))
    data = make_data(chrom, start, end, shuffle_seed=seed)
    qc, qs, qe = [], [], []
    s_arr, e_arr, c_arr = np.asarray(start), np.asarray(end), np.asarray(chrom)
    for c in (7, 9):
        for s in np.unique(s_arr[c_arr == c]):
            sel = (c_arr == c) & (s_arr == s)
            if sel.sum() < 2:
                continue
            for e in np.unique(e_arr[sel]):
                qc += [c, c, c]
                qs += [int(e), int(e) + 1, int(s)]                # at the end, just past it, at the start
                qe += [int(e) + 50, int(e) + 50, int(s)]
    return data, (np.asarray(qc), np.asarray(qs, np.int64), np.asarray(qe, np.int64))
