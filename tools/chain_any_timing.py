#!/usr/bin/env python3
"""Cluster junctions and paths for reads of any length: the _any calls' time against the plain calls', and on an
input with reads of more than 64 intervals against a host composition, in one process per line on one box:

    python tools/chain_any_timing.py [--configs cfg3,long] [--out profiles/chain_any/timing.jsonl]

``cfg3`` (synth.generate(1000000, 16, 11), no long reads): labels from the normal device query, table from the resident
labels, loci rows from fslr_cluster_loci, ``qstart`` the generator's query positions, strand bits random (seed 17).
The plain call and the _any call alternate in one process; per call the HIP-event times as median / min / max.  They
run the same kernels, so the _any median should lie inside the plain call's min-max spread.

``long`` (and ``long_small``): synth.generate(n, 16, 11) with a share of the reads lengthened to 65..4096 intervals
(lengths log-uniform, seed 23, the first of them exactly 4096): a lengthened read takes copies of random rows of the
input, shifted by up to 50 bases, as its further intervals.  Labels: clusters of four consecutive ranks (a host vector;
a query is not part of what is timed).  Query keys random int32 below 2^20 with ties, strand bits random (seed 17).
Recorded: the event time of both _any calls, the wall time of the wrapper calls (permutation, uploads, call, getters),
the sort passes and sum ceil(len / p) against m * ceil(Lmax / p), and the same rows from a host composition (numpy
lexsort and searchsorted for the junctions, sorted tuples for the paths), asserted equal, with its wall time.
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

CONFIGS = {'cfg3': dict(kind='plain', n_reads=1_000_000, lmax=16, seed=11),
           'small': dict(kind='plain', n_reads=20_000, lmax=16, seed=11),
           'long': dict(kind='long', n_reads=200_000, lmax=16, seed=11, share=0.002),
           'long_small': dict(kind='long', n_reads=5_000, lmax=16, seed=11, share=0.004)}


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def run_plain(name, cfg, repeats, warmup):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    bed = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'])
    data = bed.interval_data()
    csr = data.csr()
    pos = np.asarray(csr.data_pos, np.int64)
    qkey = np.asarray(bed.qstart, np.int64)[np.asarray(data.index, np.int64)][pos].astype(np.int32)
    rev = np.random.default_rng(17).integers(0, 2, csr.n_intervals).astype(np.uint8)
    ctx = _lib.Context(0, profiling=True)
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.reserve_edges(max(1 << 16, 12 * csr.n_reads))
    ctx.build_index()
    ctx.run_query(0.96, 0.75, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10)
    ctx.apply_edge_cap(10)
    ctx.components()
    info = ctx.cluster_table()
    loci = ctx.cluster_loci()
    base = {'config': name, **cfg, 'n_intervals': csr.n_intervals, 'n_clusters': info['n_clusters'],
            'n_nodes': info['n_nodes'], 'loci_rows': int(loci[1].size), 'repeats': repeats, 'warmup': warmup}
    calls = {'junctions': (ctx.cluster_junctions, ctx.cluster_junctions_timings),
             'junctions_any': (ctx.cluster_junctions_any, ctx.cluster_junctions_timings),
             'paths': (ctx.cluster_paths, ctx.cluster_paths_timings),
             'paths_any': (ctx.cluster_paths_any, ctx.cluster_paths_timings)}
    ev, blobs = {k: [] for k in calls}, {}
    for k in range(warmup + repeats):                        # alternated: plain, _any, plain, _any ...
        for line, (call, timing) in calls.items():
            got = call(qkey, rev)
            if k >= warmup:
                ev[line].append(next(iter(timing().values())))
            blobs[line] = [a.tobytes() for a in got]
    assert blobs['junctions'] == blobs['junctions_any'] and blobs['paths'] == blobs['paths_any']
    for line in calls:
        print(json.dumps({**base, 'line': line, 'ms': {'event': stats(ev[line])}}), flush=True)
    ctx.close()
    return len(calls)


def long_input(cfg):
    """The IntervalData of the ``long`` configs and the number of lengthened reads."""
    from fslr_amd import synth
    from fslr_amd.prep import IntervalData
    d = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed']).interval_data()
    rng = np.random.default_rng(23)
    codes = np.unique(d.qcode)
    chosen = rng.choice(codes, max(1, int(round(codes.size * cfg['share']))), replace=False)
    want = np.exp(rng.uniform(np.log(65), np.log(4096), chosen.size)).astype(np.int64)
    want[0] = 4096
    have = np.bincount(d.qcode, minlength=int(codes.max()) + 1)[chosen]
    extra = np.maximum(want - have, 0)
    src = rng.integers(0, len(d.start), int(extra.sum()))
    shift = rng.integers(0, 50, src.size)
    first = np.asarray([np.flatnonzero(d.qcode == c)[0] for c in chosen.tolist()], np.int64)   # a row of each chosen read
    own = np.repeat(first, extra)
    cols = {'chrom': np.concatenate([d.chrom, d.chrom[src]]), 'start': np.concatenate([d.start, d.start[src] + shift]),
            'end': np.concatenate([d.end, d.end[src] + shift]), 'aln_size': np.concatenate([d.aln_size, d.aln_size[src]]),
            'qcode': np.concatenate([d.qcode, np.repeat(chosen, extra)]),
            'n_alignments': np.concatenate([d.n_alignments, d.n_alignments[own]]),
            'qlen2': np.concatenate([d.qlen2, d.qlen2[own]]), 'middle': np.concatenate([d.middle, d.middle[src] + shift])}
    order = np.argsort(cols['start'], kind='stable')
    return IntervalData(qnames=d.qnames, index=np.arange(order.size, dtype=np.int64),
                        **{k: v[order] for k, v in cols.items()}), int(chosen.size)


def host_rows(csr, cid, loci, qkey, rev):
    """(junction rows, path rows) of the contract from numpy on the host; ``loci`` = cluster_loci's columns."""
    loff, lchrom, lstart = loci[0], loci[1].astype(np.int64), loci[2].astype(np.int64)
    off = np.asarray(csr.read_off, np.int64)
    lens = np.diff(off)
    read = np.repeat(np.arange(csr.n_reads), lens)
    j = np.arange(csr.n_intervals) - np.repeat(off[:-1], lens)
    c_iv = cid[read].astype(np.int64)
    keep = np.flatnonzero(c_iv >= 0)
    ch, st, en = (np.asarray(x, np.int64) for x in (csr.iv_chrom, csr.iv_start, csr.iv_end))
    nch = int(max(lchrom.max(initial=0), ch.max(initial=0))) + 1
    row_key = (np.repeat(np.arange(loff.size - 1), np.diff(loff)) * nch + lchrom) * (1 << 31) + lstart
    locus = np.searchsorted(row_key, (c_iv[keep] * nch + ch[keep]) * (1 << 31) + st[keep], 'right') - 1
    order = np.lexsort((j[keep], qkey[keep].astype(np.int64), read[keep]))       # chain order inside each read
    k, locus = keep[order], locus[order]
    r, rv = read[k], rev[k].astype(np.int64)
    # junctions: consecutive pairs inside a read
    a = np.flatnonzero(r[1:] == r[:-1])
    ea, ba = locus[a] * 2 + (1 - rv[a]), np.where(rv[a] == 1, st[k[a]], en[k[a]])
    eb, bb = locus[a + 1] * 2 + rv[a + 1], np.where(rv[a + 1] == 1, en[k[a + 1]], st[k[a + 1]])
    swap = (ea > eb) | ((ea == eb) & (ba > bb))
    ea, eb, ba, bb = np.where(swap, eb, ea), np.where(swap, ea, eb), np.where(swap, bb, ba), np.where(swap, ba, bb)
    o = np.lexsort((r[a], eb, ea))
    ea, eb, ba, bb, ro = ea[o], eb[o], ba[o], bb[o], r[a][o]
    head = np.flatnonzero(np.r_[True, (ea[1:] != ea[:-1]) | (eb[1:] != eb[:-1])]) if ea.size else np.zeros(0, np.int64)
    newread = np.r_[True, (ro[1:] != ro[:-1])] if ea.size else np.zeros(0, bool)
    newread[head] = True
    red = lambda f, v: f.reduceat(v, head) if head.size else v[:0]
    junction = [ea[head] >> 1, ea[head] & 1, eb[head] >> 1, eb[head] & 1, np.diff(np.r_[head, ea.size]),
                red(np.add, newread.astype(np.int64)), red(np.minimum, ba), red(np.maximum, ba), red(np.minimum, bb),
                red(np.maximum, bb)]
    # paths: the canonical tuple of each clustered read
    tok = (locus * 2 + rv).tolist()
    bounds = np.flatnonzero(np.r_[True, r[1:] != r[:-1], True]).tolist()
    path = {}
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        F = tuple(tok[lo:hi])
        B = tuple(t ^ 1 for t in reversed(F))
        path[int(r[lo])] = (min(F, B), B < F)
    rows = sorted(set(p for p, _ in path.values()))
    row_of = {p: i for i, p in enumerate(rows)}
    por, flipped = np.full(csr.n_reads, -1, np.int32), np.zeros(csr.n_reads, np.uint8)
    for rr, (p, f) in path.items():
        por[rr], flipped[rr] = row_of[p], f
    return junction, (np.bincount(por[por >= 0], minlength=len(rows)), [t for p in rows for t in p], por, flipped)


def run_long(name, cfg, repeats, warmup):
    from fslr_amd import _lib, cluster
    data, n_long = long_input(cfg)
    ctx = _lib.Context(0, profiling=True)
    idx = cluster.build_interval_trees(data, ctx=ctx)
    csr = idx.csr
    assert idx.long is not None
    n = csr.n_reads
    lens = np.diff(np.asarray(csr.read_off, np.int64))
    labels = ((np.arange(n) // 4) * 4).astype(np.int32)
    rng = np.random.default_rng(17)
    qkey = rng.integers(0, 1 << 20, csr.n_intervals).astype(np.int32)
    rev = rng.integers(0, 2, csr.n_intervals).astype(np.uint8)
    info = ctx.cluster_table(labels)
    loci = ctx.cluster_loci()
    cid = ctx.cluster_ids()[0]
    clen = lens[cid >= 0]
    kbits = max(1, int(2 * loci[1].size).bit_length())
    p = max(1, 64 // kbits)
    base = {'config': name, **cfg, 'n_real': n, 'n_virtual': int(ctx.n_reads), 'n_intervals': csr.n_intervals,
            'lengthened_reads': n_long, 'longest_read': int(lens.max()), 'clustered_reads': int(clen.size),
            'clustered_long_reads': int((clen > 64).sum()), 'n_clusters': info['n_clusters'],
            'loci_rows': int(loci[1].size), 'tokens_per_key': p, 'sort_passes': int(-(-clen.max() // p)),
            'keys_sorted_suffix_scheme': int((-(-clen // p)).sum()),
            'keys_sorted_full_passes': int(clen.size * -(-clen.max() // p)), 'repeats': repeats, 'warmup': warmup}
    t = {'junctions_any': {'wall': [], 'event': []}, 'paths_any': {'wall': [], 'event': []}}
    for k in range(warmup + repeats):
        for line, call, timing in (('junctions_any', ctx.cluster_junctions_any, ctx.cluster_junctions_timings),
                                   ('paths_any', ctx.cluster_paths_any, ctx.cluster_paths_timings)):
            w0 = time.perf_counter()
            got = call(qkey, rev)
            wall = (time.perf_counter() - w0) * 1e3
            if k >= warmup:
                t[line]['wall'].append(wall)
                t[line]['event'].append(next(iter(timing().values())))
            if line == 'junctions_any':
                junction = got
            else:
                paths = got
    w0 = time.perf_counter()
    hj, hp = host_rows(csr, cid, loci, qkey, rev)
    host_ms = (time.perf_counter() - w0) * 1e3
    for a, b in zip(junction[1:], hj):
        np.testing.assert_array_equal(np.asarray(a, np.int64), b)
    np.testing.assert_array_equal(paths[2], hp[0])
    np.testing.assert_array_equal(paths[4].astype(np.int64) * 2 + paths[5], hp[1])
    np.testing.assert_array_equal(paths[6], hp[2])
    np.testing.assert_array_equal(paths[7], hp[3])
    print(json.dumps({**base, 'line': 'junctions_any', 'rows': int(junction[1].size),
                      'ms': {k: stats(v) for k, v in t['junctions_any'].items()}}), flush=True)
    print(json.dumps({**base, 'line': 'paths_any', 'rows': int(paths[2].size), 'tokens': int(paths[4].size),
                      'ms': {k: stats(v) for k, v in t['paths_any'].items()}}), flush=True)
    print(json.dumps({**base, 'line': 'host_composition', 'equal': True, 'ms': {'wall': host_ms}}), flush=True)
    ctx.close()
    return 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help='(child) measure this config in this process')
    ap.add_argument('--configs', default='cfg3,long')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=420, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'chain_any', 'timing.jsonl'))
    args = ap.parse_args()
    if args.child:
        cfg = CONFIGS[args.child]
        (run_plain if cfg['kind'] == 'plain' else run_long)(args.child, cfg, args.repeats, args.warmup)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.configs.split(','):
        # a fresh child under its own limit; a failure writes nothing and ends the run
        r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child',
                            name, '--repeats', str(args.repeats), '--warmup', str(args.warmup)],
                           capture_output=True, text=True)
        sys.stderr.write(r.stderr[-3000:])
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
