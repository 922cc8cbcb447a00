#!/usr/bin/env python3
"""Cluster loci, device call against the host composition it replaces, in one process on one box:

    python tools/loci_timing.py [--configs cfg3] [--out profiles/loci/loci_timing.jsonl]

For cfg3 (synth.generate(1000000, 16, 11)) the labels come from the normal device query (sweep, edge cap,
components) and the table from those resident labels.  Timed, after --warmup, over --repeats:

* ``device``: Context.cluster_loci() = fslr_cluster_loci + fslr_get_cluster_loci and the Python wrapper (wall
  time), and the library's HIP-event time of fslr_cluster_loci (fslr_cluster_loci_timings).
* ``host``: what a caller does without the call: fslr_get_cluster_ids + fslr_get_csr (the D2H copies), a numpy
  lexsort of the clustered intervals by (cluster, chrom, start), and a vectorised segmented sweep (running
  maximum per segment, heads, row reductions, distinct reads through one more sort).  The phases are timed
  apart.

Each line carries median / min / max; both must give the same rows.  The ratio is a description, not a pass
mark.
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

CONFIGS = {'cfg3': dict(n_reads=1_000_000, lmax=16, seed=11, dist='uniform'),
           'cfg5': dict(n_reads=10_000_000, lmax=64, seed=13, dist='zipf')}
COLUMNS = ('off', 'chrom', 'start', 'end', 'n_intervals', 'n_reads')


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def segmented_running_max(seg_head, end):
    """Inclusive running maximum of ``end`` inside the segments that begin where ``seg_head`` is set (ends
    are below 2**30, so adding the segment number << 31 makes one global running maximum do it)."""
    key = (np.cumsum(seg_head, dtype=np.int64) << 31) + end
    return (np.maximum.accumulate(key) & ((1 << 31) - 1)).astype(np.int64)


def host_loci(cid, n_clusters, csr):
    """The rows from the cluster ids and the CSR, vectorised numpy: (columns, seconds of the sort, of the sweep)."""
    t0 = time.perf_counter()
    read_off = np.asarray(csr['read_off'], np.int64)
    read_of = np.repeat(np.arange(read_off.size - 1, dtype=np.int64), np.diff(read_off))
    c_iv = cid[read_of]
    sel = np.flatnonzero(c_iv >= 0)
    c, ch = c_iv[sel].astype(np.int64), csr['iv_chrom'][sel].astype(np.int64)
    s, e, r = csr['iv_start'][sel].astype(np.int64), csr['iv_end'][sel].astype(np.int64), read_of[sel]
    order = np.lexsort((s, ch, c))
    c, ch, s, e, r = c[order], ch[order], s[order], e[order], r[order]
    t1 = time.perf_counter()
    m = c.size
    off = np.zeros(n_clusters + 1, np.int64)
    if m == 0:
        z = np.zeros(0, np.int32)
        return (off, z, z, z, z, z), t1 - t0, 0.0
    seg = (c << 32) | ch
    seg_head = np.ones(m, bool)
    seg_head[1:] = seg[1:] != seg[:-1]
    rmax = segmented_running_max(seg_head, e)
    head = seg_head.copy()
    head[1:] |= s[1:] > rmax[:-1]
    hp = np.flatnonzero(head)
    last = np.append(hp[1:], m) - 1
    lid = np.cumsum(head) - 1
    n_reads = np.bincount(np.unique(lid * np.int64(read_off.size) + r) // np.int64(read_off.size), minlength=hp.size)
    np.cumsum(np.bincount(c[hp], minlength=n_clusters), out=off[1:])
    cols = (off, ch[hp].astype(np.int32), s[hp].astype(np.int32), rmax[last].astype(np.int32),
            (last - hp + 1).astype(np.int32), n_reads.astype(np.int32))
    return cols, t1 - t0, time.perf_counter() - t1


def run(name, repeats, warmup):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import pass_table
    cfg = CONFIGS[name]
    data = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'], dist=cfg['dist']).interval_data()
    csr = data.csr()
    n = csr.n_reads
    ctx = _lib.Context(0, profiling=True)
    # the reads from rows (the columnar CLI's upload): fslr_get_csr answers on such a context.  The `data` list
    # is start-sorted already, so its own order is the start order
    rows = dict(chrom=data.chrom, start=data.start, end=data.end, aln=data.aln_size, qcode=data.qcode,
                nal=data.n_alignments, qlen2=data.qlen2)
    ctx.rows_upload(rows, int(np.asarray(data.qcode).max()) + 1, int(np.asarray(data.chrom).max()) + 1)
    made = ctx.set_reads_rows(np.arange(len(data), dtype=np.int64), None, 0.8)
    assert (made['n_reads'], made['n_intervals'], made['n_chroms']) == (n, csr.n_intervals, csr.n_chroms)
    ctx.reserve_edges(max(1 << 16, 12 * n))
    ctx.build_index()
    st = ctx.run_query(0.96, 0.75, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10)
    ctx.apply_edge_cap(10)
    ctx.components()
    info = ctx.cluster_table()
    base = {'config': name, **cfg, 'n_intervals': csr.n_intervals, 'edges': int(st['n_edges']),
            'n_clusters': info['n_clusters'], 'n_nodes': info['n_nodes'], 'repeats': repeats, 'warmup': warmup}

    t = {'wall': [], 'event': []}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        got = ctx.cluster_loci()
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            t['wall'].append(wall)
            t['event'].append(ctx.cluster_loci_timings()['loci'])
    dev = stats(t['wall'])
    clustered = int(got[4].sum())
    print(json.dumps({**base, 'line': 'device', 'rows': int(got[1].size), 'clustered_intervals': clustered,
                      'ms': {k: stats(v) for k, v in t.items()}}), flush=True)

    h = {'wall': [], 'copies': [], 'lexsort': [], 'sweep': []}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        cid, _ = ctx.cluster_ids()
        d = ctx.device_csr(csr.n_intervals, csr.n_chroms)
        w1 = time.perf_counter()
        want, sort_s, sweep_s = host_loci(cid, info['n_clusters'], d)
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            h['wall'].append(wall)
            h['copies'].append((w1 - w0) * 1e3)
            h['lexsort'].append(sort_s * 1e3)
            h['sweep'].append(sweep_s * 1e3)
    for a, b, col in zip(got, want, COLUMNS):
        assert a.dtype == b.dtype and np.array_equal(a, b), col
    hs = stats(h['wall'])
    print(json.dumps({**base, 'line': 'host', 'rows': int(want[1].size), 'ms': {k: stats(v) for k, v in h.items()},
                      'host_over_device': hs['median'] / dev['median']}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help='(child) measure this config in this process')
    ap.add_argument('--configs', default='cfg3')
    ap.add_argument('--repeats', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--limit', type=int, default=540, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'loci', 'loci_timing.jsonl'))
    args = ap.parse_args()
    if args.child:
        run(args.child, args.repeats, args.warmup)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.configs.split(','):
        # a fresh child under its own limit; a failure writes nothing and ends the run
        r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child',
                            name, '--repeats', str(args.repeats), '--warmup', str(args.warmup)],
                           capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')]
        for ln in lines:
            print(ln, flush=True)
        if r.returncode != 0 or len(lines) != 2:
            print(f'{name}: exit status {r.returncode}; nothing written', file=sys.stderr)
            return r.returncode or 1
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
