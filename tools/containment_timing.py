#!/usr/bin/env python3
"""Path containment: the device call's time against a host composition of the same rows, in one process on one box:

    python tools/containment_timing.py [--configs cfg3,long] [--out profiles/containment/timing.jsonl]

``cfg3`` (tools/segments_timing.py's input: synth.generate(1000000, 16, 11), no long reads; labels from the device
query, the path rows from fslr_cluster_paths) and ``long`` (tools/chain_any_timing.py's input of that name, with its
generator, seeds and labels; the path rows from fslr_cluster_paths_any).  Timed, after --warmup, over --repeats:

* ``event``: the HIP-event time of the call (fslr_cluster_path_containment_timings);
* ``wall``: Context.cluster_path_containment() (the call, the getter and the wrapper; nothing is uploaded);
* ``host``: a Python composition from the downloaded path rows: per cluster every ordered pair of rows of different
  length, the shorter searched in the longer in both directions with bytes.find on the rows' int32 tokens, then the
  per-row columns.  It runs on every ``--sample``-th cluster that has two or more rows (1: all of them) and its time
  is reported for those clusters alone, with their share of the rows; the device's rows of the sampled clusters are
  asserted equal to it.

The line also holds the pair and occurrence counts and the candidates the probes visit (the occurrences of each inner
row's anchor tokens: its first token, and its last token ^ 1 unless the row is palindromic), counted on the host from
the path rows.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))

import chain_any_timing as cat          # noqa: E402  (long_input, CONFIGS)

CONFIGS = cat.CONFIGS
NAMES = ('coff', 'outer', 'offset', 'rev', 'n_occ', 'n_inner', 'support', 'collapse_to', 'collapsed_reads')


def note(text):
    print(text, file=sys.stderr, flush=True)


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def find_all(hay, needle):
    """The token offsets at which the int32 tokens ``needle`` (bytes) stand in ``hay`` (bytes)."""
    out, at = [], hay.find(needle)
    while at >= 0:
        if at % 4 == 0:
            out.append(at // 4)
        at = hay.find(needle, at + 1)
    return out


def host_cluster(lo, toks, n_reads):
    """One cluster whose rows are lo .. lo + len(toks) - 1: ``toks`` their tokens (int32 arrays).  Returns the pairs
    {(inner, outer): (offset, rev, n_occ)} and the per-row columns {row: (n_inner, support, collapse_to, collapsed)}."""
    fw = [t.tobytes() for t in toks]
    bw = [(t[::-1] ^ 1).tobytes() for t in toks]
    pairs = {}
    for i, a in enumerate(toks):
        for j, b in enumerate(toks):
            if a.size >= b.size:
                continue
            occ = [(o, 0) for o in find_all(fw[j], fw[i])]
            if bw[i] != fw[i]:
                occ += [(o, 1) for o in find_all(fw[j], bw[i])]
            if occ:
                pairs[(lo + i, lo + j)] = (*min(occ), len(occ))
    n_inner, support = {}, {lo + i: int(n_reads[lo + i]) for i in range(len(toks))}
    for (a, b) in pairs:
        n_inner[b] = n_inner.get(b, 0) + 1
        support[b] += int(n_reads[a])
    inner = {a for a, _ in pairs}
    to = {}
    for r in support:
        best = [b for (a, b) in pairs if a == r and b not in inner]
        to[r] = min(best, key=lambda b: (-support[b], b)) if best else r
    collapsed = dict.fromkeys(support, 0)
    for r in support:
        collapsed[to[r]] += int(n_reads[r])
    return pairs, {r: (n_inner.get(r, 0), support[r], to[r], collapsed[r]) for r in support}


def host_check(paths, got, sample):
    """The host composition on every ``sample``-th cluster of two or more rows, asserted against ``got``; returns its
    time (ms), the clusters and rows it covered and the clusters and rows it could have."""
    off, tok_off, n_reads, _, locus, trev = paths[:6]
    tok = (locus.astype(np.int32) * 2 + trev).astype(np.int32)
    multi = np.flatnonzero(np.diff(off) >= 2)
    take = multi[::sample]
    res = dict(zip(NAMES, got))
    inner_of = np.repeat(np.arange(len(n_reads)), np.diff(res['coff']))
    t0 = time.perf_counter()
    made = [host_cluster(int(off[c]), [tok[tok_off[r]:tok_off[r + 1]] for r in range(int(off[c]), int(off[c + 1]))], n_reads)
            for c in take.tolist()]
    ms = (time.perf_counter() - t0) * 1e3
    rows = 0
    for c, (pairs, cols) in zip(take.tolist(), made):
        lo, hi = int(off[c]), int(off[c + 1])
        rows += hi - lo
        p0, p1 = int(res['coff'][lo]), int(res['coff'][hi])
        dev = {(int(inner_of[k]), int(res['outer'][k])): (int(res['offset'][k]), int(res['rev'][k]), int(res['n_occ'][k]))
               for k in range(p0, p1)}
        assert dev == pairs, f'cluster {c}: the pairs differ'
        for r, want in cols.items():
            have = (int(res['n_inner'][r]), int(res['support'][r]), int(res['collapse_to'][r]), int(res['collapsed_reads'][r]))
            assert have == want, f'row {r}: {have} != {want}'
    return ms, int(take.size), rows, int(multi.size), int(np.diff(off)[multi].sum())


def candidates_visited(paths):
    """The occurrence records the probes read: per row the occurrences of its first token, and of its last token ^ 1
    unless the row is palindromic."""
    _, tok_off, _, _, locus, trev = paths[:6]
    tok = locus.astype(np.int64) * 2 + trev
    if not tok.size:
        return 0
    count = np.bincount(tok, minlength=int(tok.max()) + 2)
    first, last = tok[tok_off[:-1]], tok[tok_off[1:] - 1] ^ 1
    lens = np.diff(tok_off)
    pal = np.zeros(lens.size, bool)
    for n in np.unique(lens[lens % 2 == 0]).tolist():          # a palindrome has an even length
        rows = np.flatnonzero(lens == n)
        m = tok[tok_off[rows][:, None] + np.arange(n)[None, :]]
        pal[rows] = (m == (m[:, ::-1] ^ 1)).all(axis=1)
    return int(count[first].sum() + count[last][~pal].sum())


def measure(name, cfg, ctx, paths, extra, repeats, warmup, sample):
    t = {'wall': [], 'event': []}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        got = ctx.cluster_path_containment()
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            t['wall'].append(wall)
            t['event'].append(ctx.cluster_path_containment_timings()['containment'])
    note(f'{name}: device rows made')
    host_ms, h_clusters, h_rows, m_clusters, m_rows = host_check(paths, got, sample)
    res = dict(zip(NAMES, got))
    lens, k = np.diff(paths[1]), paths[2]
    maximal = np.diff(res['coff']) == 0
    print(json.dumps({'config': name, **cfg, **extra, 'rows': int(k.size), 'tokens': int(paths[4].size),
                      'rows_of_one_read': int((k == 1).sum()), 'rows_longer_than_64': int((lens > 64).sum()),
                      'clusters_of_two_or_more_rows': m_clusters, 'rows_in_them': m_rows,
                      'pairs': int(res['outer'].size), 'occurrences': int(res['n_occ'].sum()),
                      'candidates_visited': candidates_visited(paths), 'maximal_rows': int(maximal.sum()),
                      'rows_of_one_read_after_collapse': int(((res['collapsed_reads'] == 1) & maximal).sum()),
                      'largest_support': int(res['support'].max(initial=0)), 'repeats': repeats, 'warmup': warmup,
                      'host_sample': {'every': sample, 'clusters': h_clusters, 'rows': h_rows, 'equal': True},
                      'ms': {**{kk: stats(v) for kk, v in t.items()}, 'host_on_the_sample': host_ms}}), flush=True)


def run_plain(name, cfg, repeats, warmup, sample):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    bed = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'])
    data = bed.interval_data()
    csr = data.csr()
    pos = np.asarray(csr.data_pos, np.int64)
    rows = np.asarray(data.index, np.int64)
    qkey = np.asarray(bed.qstart, np.int64)[rows][pos].astype(np.int32)
    rev = np.random.default_rng(17).integers(0, 2, csr.n_intervals).astype(np.uint8)
    note(f'{name}: input made')
    ctx = _lib.Context(0, profiling=True)
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.reserve_edges(max(1 << 16, 12 * csr.n_reads))
    ctx.build_index()
    ctx.run_query(0.96, 0.75, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10)
    ctx.apply_edge_cap(10)
    ctx.components()
    info = ctx.cluster_table()
    ctx.cluster_loci()
    paths = ctx.cluster_paths(qkey, rev)
    note(f'{name}: path rows made')
    measure(name, cfg, ctx, paths, {'n_intervals': csr.n_intervals, 'n_clusters': info['n_clusters']}, repeats, warmup, sample)
    ctx.close()


def run_long(name, cfg, repeats, warmup, sample):
    from fslr_amd import _lib, cluster
    data, n_long = cat.long_input(cfg)
    note(f'{name}: input made')
    ctx = _lib.Context(0, profiling=True)
    idx = cluster.build_interval_trees(data, ctx=ctx)
    csr = idx.csr
    assert idx.long is not None
    n = csr.n_reads
    labels = ((np.arange(n) // 4) * 4).astype(np.int32)
    rng = np.random.default_rng(17)
    qkey = rng.integers(0, 1 << 20, csr.n_intervals).astype(np.int32)
    rev = rng.integers(0, 2, csr.n_intervals).astype(np.uint8)
    info = ctx.cluster_table(labels)
    ctx.cluster_loci()
    paths = ctx.cluster_paths_any(qkey, rev)
    note(f'{name}: path rows made')
    measure(name, cfg, ctx, paths, {'n_real': n, 'n_intervals': csr.n_intervals, 'lengthened_reads': n_long,
                                    'n_clusters': info['n_clusters']}, repeats, warmup, sample)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help='(child) measure this config in this process')
    ap.add_argument('--configs', default='cfg3,long')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sample', type=int, default=8, help='the host composition takes every n-th cluster of two or more rows')
    ap.add_argument('--limit', type=int, default=420, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'containment', 'timing.jsonl'))
    args = ap.parse_args()
    if args.child:
        cfg = CONFIGS[args.child]
        (run_plain if cfg['kind'] == 'plain' else run_long)(args.child, cfg, args.repeats, args.warmup, max(args.sample, 1))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.configs.split(','):
        # a fresh child under its own limit (its notes go straight to stderr); a failure writes nothing and ends the run
        r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child',
                            name, '--repeats', str(args.repeats), '--warmup', str(args.warmup), '--sample', str(args.sample)],
                           stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')]
        for ln in lines:
            print(ln, flush=True)
        if r.returncode != 0 or not lines:
            print(f'{name}: exit status {r.returncode}; nothing written', file=sys.stderr)
            return r.returncode or 1
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
