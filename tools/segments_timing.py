#!/usr/bin/env python3
"""Path segments: the device call's time against a host composition of the same rows, in one process on one box:

    python tools/segments_timing.py [--configs cfg3] [--out profiles/segments/timing.jsonl]

For cfg3 (synth.generate(1000000, 16, 11)) the labels come from the normal device query (sweep, edge cap,
components), the table from those resident labels, the loci rows from fslr_cluster_loci and the path rows from
fslr_cluster_paths.  ``qstart`` / ``qend`` are the generator's query span of each filling; the strand bits are random
with a fixed seed.  Timed, after --warmup, over --repeats:

* ``event``: the HIP-event time of the call (fslr_cluster_path_segments_timings);
* ``wall``: Context.cluster_path_segments() (the two columns' upload, the call, the getter and the wrapper);
* ``host``: a numpy composition from the downloaded path rows (chain ranks by lexsort, slots, a lexsort of
  (slot, value) per stream, the three order statistics by offsets), asserted equal to the device's rows.

The line also holds the tier populations: the path rows with k = 1, 2..64, 65..4096 and more than 4096 reads.
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
           'small': dict(n_reads=20_000, lmax=16, seed=11, dist='uniform')}
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def three(slot, value, n_tokens):
    """min, lower median, max of ``value`` per ``slot`` (zeros where a slot has none)."""
    order = np.lexsort((value, slot))
    v = value[order]
    k = np.bincount(slot, minlength=n_tokens)
    first = np.cumsum(k) - k
    has = k > 0
    out = np.zeros((3, n_tokens), np.int32)
    out[0, has] = v[first[has]]
    out[1, has] = v[first[has] + (k[has] - 1) // 2]
    out[2, has] = v[first[has] + k[has] - 1]
    return out


def host_rows(csr, paths, qkey, qend):
    """The nine columns by numpy from the downloaded path rows."""
    off, tok_off, n_reads, first_read, locus, trev, por, flipped = paths
    read_off = np.asarray(csr.read_off, np.int64)
    lens = np.diff(read_off)
    read = np.repeat(np.arange(lens.size), lens)
    keep = por[read] >= 0
    at = np.flatnonzero(keep)
    r = read[at]
    order = np.lexsort((at, qkey[at], r))                                  # by read, then (query key, CSR position)
    at, r = at[order], r[order]
    # the rank in the chain: the place within the read's run of the sorted list
    run_first = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    t = np.arange(at.size) - np.repeat(run_first, np.diff(np.r_[run_first, at.size]))
    L = lens[r]
    flip = flipped[r] != 0
    p = np.where(flip, L - 1 - t, t)
    slot = tok_off[por[r]] + p
    nt = int(tok_off[-1])
    start = three(slot, np.asarray(csr.iv_start, np.int64)[at], nt)
    end = three(slot, np.asarray(csr.iv_end, np.int64)[at], nt)
    link = np.flatnonzero(t + 1 < L)
    gap = np.clip(qkey[at[link + 1]].astype(np.int64) - qend[at[link]].astype(np.int64), I32_MIN, I32_MAX)
    gslot = tok_off[por[r[link]]] + np.where(flip[link], L[link] - 2 - t[link], t[link])
    return (*start, *end, *three(gslot, gap, nt))


def run(name, repeats, warmup):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    cfg = CONFIGS[name]
    bed = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'], dist=cfg['dist'])
    data = bed.interval_data()
    csr = data.csr()
    n = csr.n_reads
    pos = np.asarray(csr.data_pos, np.int64)
    rows = np.asarray(data.index, np.int64)
    qkey = np.asarray(bed.qstart, np.int64)[rows][pos].astype(np.int32)
    qend = np.asarray(bed.qend, np.int64)[rows][pos].astype(np.int32)
    rev = np.random.default_rng(17).integers(0, 2, csr.n_intervals).astype(np.uint8)
    ctx = _lib.Context(0, profiling=True)
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.reserve_edges(max(1 << 16, 12 * n))
    ctx.build_index()
    st = ctx.run_query(0.96, 0.75, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10)
    ctx.apply_edge_cap(10)
    ctx.components()
    info = ctx.cluster_table()
    loci = ctx.cluster_loci()
    paths = ctx.cluster_paths(qkey, rev)
    k = paths[2]
    t = {'wall': [], 'event': []}
    for i in range(warmup + repeats):
        w0 = time.perf_counter()
        got = ctx.cluster_path_segments(qkey, qend)
        wall = (time.perf_counter() - w0) * 1e3
        if i >= warmup:
            t['wall'].append(wall)
            t['event'].append(ctx.cluster_path_segments_timings()['segments'])
    h0 = time.perf_counter()
    want = host_rows(csr, paths, qkey, qend)
    host_ms = (time.perf_counter() - h0) * 1e3
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    print(json.dumps({'config': name, **cfg, 'n_intervals': csr.n_intervals, 'edges': int(st['n_edges']),
                      'n_clusters': info['n_clusters'], 'n_nodes': info['n_nodes'], 'loci_rows': int(loci[1].size),
                      'rows': int(k.size), 'tokens': int(paths[4].size), 'largest_k': int(k.max(initial=0)),
                      'rows_by_k': {'1': int((k == 1).sum()), '2..64': int(((k >= 2) & (k <= 64)).sum()),
                                    '65..4096': int(((k > 64) & (k <= 4096)).sum()), '>4096': int((k > 4096).sum())},
                      'gaps_nonzero': int((got[7] != 0).sum()), 'repeats': repeats, 'warmup': warmup,
                      'ms': {**{kk: stats(v) for kk, v in t.items()}, 'host': host_ms}}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help='(child) measure this config in this process')
    ap.add_argument('--configs', default='cfg3')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=540, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'segments', 'timing.jsonl'))
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
        if r.returncode != 0 or len(lines) != 1:
            print(f'{name}: exit status {r.returncode}; nothing written', file=sys.stderr)
            return r.returncode or 1
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
