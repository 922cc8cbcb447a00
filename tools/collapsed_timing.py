#!/usr/bin/env python3
"""Collapsed path segments: the device call's time against a host composition of the same rows from the downloaded
results, in one process on one box:

    python tools/collapsed_timing.py [--configs cfg3,long,cfg3_trunc] [--out profiles/collapsed/timing.jsonl]

``cfg3`` and ``long`` are tools/containment_timing.py's inputs of those names (random strand bits: cfg3 holds no
contained pair, so it times the path without containment).  ``cfg3_trunc`` is cfg3's synthetic input in which
containment is common: the labels come from the device query on the full input, then every second clustered read of
two or more intervals loses an end piece (the piece with the smallest query start and the one with the largest, in
turn: tests/containment_cases.py's truncation), the index is built again on what is left, a truncated read stays in
its cluster, and every strand bit is 0.  ``small_trunc`` is the same on 20,000 reads, a quick check of the tool
itself.  Timed, after --warmup, over --repeats:

* ``event``: the HIP-event time of the call (fslr_cluster_collapsed_segments_timings), the uploads excluded;
* ``wall``: Context.cluster_collapsed_segments_any(qkey, qend) (two columns up, eleven down, the wrapper);
* ``host``: a Python composition of the same rows from the downloaded path rows and containment rows and the two
  columns: per read of a sampled cluster the chain, the row it collapses to and the slots, then the order statistics
  per slot.  It runs on every ``--sample``-th cluster of two or more reads' rows and its time is reported for those
  clusters alone; the device's columns on the slots of the sampled clusters are asserted equal to it.
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

CONFIGS = dict(cat.CONFIGS, cfg3_trunc=dict(cat.CONFIGS['cfg3'], kind='trunc'),
               small_trunc=dict(cat.CONFIGS['small'], kind='trunc'))
NAMES = ('n_cov', 'n_link', 'start_min', 'start_med', 'start_max', 'end_min', 'end_med', 'end_max', 'gap_min', 'gap_med',
         'gap_max')
CT = ('coff', 'outer', 'offset', 'rev', 'n_occ', 'n_inner', 'support', 'collapse_to', 'collapsed_reads')
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def note(text):
    print(text, file=sys.stderr, flush=True)


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def three(v):
    v = sorted(v)
    return v[0], v[(len(v) - 1) // 2], v[-1]


def host_check(csr, paths, ct, qkey, qend, got, sample):
    """The host composition on every ``sample``-th cluster, asserted against ``got``; returns its time (ms) and the
    clusters, reads and slots it covered."""
    off, tok_off = paths[0], paths[1]
    por, flipped = paths[6], paths[7]
    res = dict(zip(CT, ct))
    take = np.arange(len(off) - 1)[::sample]
    in_take = np.zeros(len(off) - 1, bool)
    in_take[take] = True
    row_cluster = np.repeat(np.arange(len(off) - 1), np.diff(off))
    reads = np.flatnonzero((por >= 0) & in_take[row_cluster[np.maximum(por, 0)]])
    read_off, ivs, ive = np.asarray(csr.read_off, np.int64), np.asarray(csr.iv_start), np.asarray(csr.iv_end)
    t0 = time.perf_counter()
    starts, ends, gaps, links = {}, {}, {}, {}
    for r in reads.tolist():
        A = int(por[r])
        ks = sorted(range(int(read_off[r]), int(read_off[r + 1])), key=lambda k: (int(qkey[k]), k))
        a, B, o, d = len(ks), int(res['collapse_to'][A]), 0, 0
        if B != A:
            p0, p1 = int(res['coff'][A]), int(res['coff'][A + 1])
            at = p0 + int(np.searchsorted(res['outer'][p0:p1], B))
            o, d = int(res['offset'][at]), int(res['rev'][at])
        base = int(tok_off[B])
        q = []
        for t in range(a):
            p = a - 1 - t if flipped[r] else t
            q.append(base + (o + (a - 1 - p) if d else o + p))
        for t, k in enumerate(ks):
            starts.setdefault(q[t], []).append(int(ivs[k]))
            ends.setdefault(q[t], []).append(int(ive[k]))
            if t + 1 < a:
                s = min(q[t], q[t + 1])
                links[s] = links.get(s, 0) + 1
                gaps.setdefault(s, []).append(max(I32_MIN, min(I32_MAX, int(qkey[ks[t + 1]]) - int(qend[k]))))
    want = {}
    for s, v in starts.items():
        want[s] = (len(v), links.get(s, 0)) + three(v) + three(ends[s]) + (three(gaps[s]) if s in gaps else (0, 0, 0))
    ms = (time.perf_counter() - t0) * 1e3
    dev = dict(zip(NAMES, got))
    slots = 0
    for c in take.tolist():
        for s in range(int(tok_off[off[c]]), int(tok_off[off[c + 1]])):
            slots += 1
            have = tuple(int(dev[k][s]) for k in NAMES)
            assert have == want.get(s, (0,) * 11), f'slot {s}: {have} != {want.get(s)}'
    return ms, int(take.size), int(reads.size), slots


def measure(name, cfg, ctx, csr, paths, qkey, qend, extra, repeats, warmup, sample):
    ct = ctx.cluster_path_containment()
    t = {'wall': [], 'event': []}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        got = ctx.cluster_collapsed_segments_any(qkey, qend)
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            t['wall'].append(wall)
            t['event'].append(ctx.cluster_collapsed_segments_timings()['collapsed'])
    note(f'{name}: device rows made')
    host_ms, h_clusters, h_reads, h_slots = host_check(csr, paths, ct, qkey, qend, got, sample)
    res, dev = dict(zip(CT, ct)), dict(zip(NAMES, got))
    lens, k = np.diff(paths[1]), paths[2]
    maximal = res['collapse_to'] == np.arange(k.size)
    print(json.dumps({'config': name, **cfg, **extra, 'rows': int(k.size), 'tokens': int(paths[4].size),
                      'clustered_reads': int((paths[6] >= 0).sum()), 'rows_longer_than_64': int((lens > 64).sum()),
                      'pairs': int(res['outer'].size), 'rows_that_collapse_onto_another': int((~maximal).sum()),
                      'reads_on_them': int(k[~maximal].sum()), 'slots_of_maximal_rows': int(lens[maximal].sum()),
                      'largest_n_cov': int(dev['n_cov'].max(initial=0)),
                      'slots_with_fewer_links_than_intervals_behind_a_link': int(((dev['n_link'] > 0) & (dev['n_link'] < dev['n_cov'])).sum()),
                      'repeats': repeats, 'warmup': warmup,
                      'host_sample': {'every': sample, 'clusters': h_clusters, 'reads': h_reads, 'slots': h_slots, 'equal': True},
                      'ms': {**{kk: stats(v) for kk, v in t.items()}, 'host_on_the_sample': host_ms}}), flush=True)


def query_labels(ctx, csr):
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.reserve_edges(max(1 << 16, 12 * csr.n_reads))
    ctx.build_index()
    ctx.run_query(0.96, 0.75, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10)
    ctx.apply_edge_cap(10)
    ctx.components()


def columns(bed, data, csr):
    pos = np.asarray(csr.data_pos, np.int64)
    rows = np.asarray(data.index, np.int64)
    return (np.asarray(bed.qstart, np.int64)[rows][pos].astype(np.int32), np.asarray(bed.qend, np.int64)[rows][pos].astype(np.int32))


def run_plain(name, cfg, repeats, warmup, sample):
    from fslr_amd import _lib, synth
    bed = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'])
    data = bed.interval_data()
    csr = data.csr()
    qkey, qend = columns(bed, data, csr)
    rev = np.random.default_rng(17).integers(0, 2, csr.n_intervals).astype(np.uint8)
    note(f'{name}: input made')
    ctx = _lib.Context(0, profiling=True)
    query_labels(ctx, csr)
    info = ctx.cluster_table()
    ctx.cluster_loci()
    paths = ctx.cluster_paths(qkey, rev)
    note(f'{name}: path rows made')
    measure(name, cfg, ctx, csr, paths, qkey, qend, {'n_intervals': csr.n_intervals, 'n_clusters': info['n_clusters']},
            repeats, warmup, sample)
    ctx.close()


def run_trunc(name, cfg, repeats, warmup, sample):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import fold_overlap_threshold
    bed = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'])
    data = bed.interval_data()
    csr = data.csr()
    qkey, _ = columns(bed, data, csr)
    ctx = _lib.Context(0, profiling=True)
    query_labels(ctx, csr)
    labels = np.asarray(ctx.labels(), np.int64)
    ctx.close()
    # the truncation: every second clustered read of two or more intervals loses the piece with the smallest query
    # start or the one with the largest, in turn
    n = csr.n_reads
    read_off = np.asarray(csr.read_off, np.int64)
    lens = np.diff(read_off)
    clustered = np.bincount(labels, minlength=n)[labels] >= 2
    chosen = np.flatnonzero(clustered & (lens >= 2))[::2]
    read_of = np.repeat(np.arange(n), lens)
    order = np.lexsort((qkey, read_of))                 # per read ascending query start
    first, last = order[read_off[:-1]], order[read_off[1:] - 1]
    drop_csr = np.where(np.arange(chosen.size) % 2 == 0, first[chosen], last[chosen])
    keep = np.ones(csr.n_intervals, bool)
    keep[np.asarray(csr.data_pos, np.int64)[drop_csr]] = False
    code_of_rank = np.asarray(csr.read_qcode, np.int64)
    group_of_code = np.full(int(code_of_rank.max()) + 1, -1, np.int64)
    group_of_code[code_of_rank] = labels
    data2 = data.select(keep)
    csr2 = data2.csr()
    qkey2, qend2 = columns(bed, data2, csr2)
    g = group_of_code[np.asarray(csr2.read_qcode, np.int64)]
    low = np.full(n, csr2.n_reads, np.int64)
    np.minimum.at(low, g, np.arange(csr2.n_reads))
    lab2 = low[g].astype(np.int32)
    rev = np.zeros(csr2.n_intervals, np.uint8)
    note(f'{name}: input made, {chosen.size} reads truncated')
    ctx = _lib.Context(0, profiling=True)
    ctx.load_csr(csr2, fold_overlap_threshold(csr2.iv_aln, 0.8))
    ctx.build_index()
    info = ctx.cluster_table(lab2)
    ctx.cluster_loci()
    paths = ctx.cluster_paths(qkey2, rev)
    note(f'{name}: path rows made')
    measure(name, cfg, ctx, csr2, paths, qkey2, qend2, {'n_intervals': csr2.n_intervals, 'n_clusters': info['n_clusters'],
                                                         'truncated_reads': int(chosen.size)}, repeats, warmup, sample)
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
    qend = (qkey.astype(np.int64) + rng.integers(1, 400, csr.n_intervals)).astype(np.int32)
    info = ctx.cluster_table(labels)
    ctx.cluster_loci()
    paths = ctx.cluster_paths_any(qkey, rev)
    note(f'{name}: path rows made')
    measure(name, cfg, ctx, csr, paths, qkey, qend, {'n_real': n, 'n_intervals': csr.n_intervals, 'lengthened_reads': n_long,
                                                     'n_clusters': info['n_clusters']}, repeats, warmup, sample)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help='(child) measure this config in this process')
    ap.add_argument('--configs', default='cfg3,long,cfg3_trunc')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sample', type=int, default=8, help='the host composition takes every n-th cluster')
    ap.add_argument('--limit', type=int, default=420, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'collapsed', 'timing.jsonl'))
    args = ap.parse_args()
    if args.child:
        cfg = CONFIGS[args.child]
        {'plain': run_plain, 'long': run_long, 'trunc': run_trunc}[cfg['kind']](args.child, cfg, args.repeats, args.warmup,
                                                                              max(args.sample, 1))
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
