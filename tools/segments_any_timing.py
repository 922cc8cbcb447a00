#!/usr/bin/env python3
"""Path segments for reads of any length: the _any call's time against the plain call's, and on an input with reads
of more than 64 intervals against a host composition, one process per config on one box:

    python tools/segments_any_timing.py [--configs cfg3,long] [--out profiles/segments_any/timing.jsonl]

``cfg3`` (tools/segments_timing.py's input: synth.generate(1000000, 16, 11), no long reads; labels from the device
query, path rows from fslr_cluster_paths): fslr_cluster_path_segments and fslr_cluster_path_segments_any alternate in
one process, the bytes asserted equal; per call the HIP-event times as median / min / max.  They run the same
kernels, so the _any median should lie inside the plain call's own min-max spread; ``any_inside_plain_spread`` says
whether it does.

``long`` (and ``long_small``): tools/chain_any_timing.py's input of that name, with its generator, seeds and labels
(clusters of four consecutive ranks), its query keys and strand bits; the query end of an interval is its key plus
a random length below 2^10 (seed 29).  The path rows come from fslr_cluster_paths_any.  Recorded: the HIP-event time
of fslr_cluster_path_segments_any, the wall time of Context.cluster_path_segments_any() (the permuted uploads, the
call, the getter and the wrapper), and tools/segments_timing.py's numpy host composition of the same rows, asserted
equal, with its wall time.
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
import segments_timing as sgt           # noqa: E402  (host_rows, stats)

CONFIGS = cat.CONFIGS


def note(text):
    print(text, file=sys.stderr, flush=True)


def rows_by_k(k, lens):
    return {'rows': int(k.size), 'largest_k': int(k.max(initial=0)), 'rows_k1': int((k == 1).sum()),
            'rows_k2_64': int(((k >= 2) & (k <= 64)).sum()), 'rows_k_over_64': int((k > 64).sum()),
            'rows_longer_than_64': int((lens > 64).sum()),
            'rows_longer_than_64_of_k2_or_more': int(((lens > 64) & (k >= 2)).sum())}


def run_plain(name, cfg, repeats, warmup):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    bed = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'])
    data = bed.interval_data()
    csr = data.csr()
    pos = np.asarray(csr.data_pos, np.int64)
    rows = np.asarray(data.index, np.int64)
    qkey = np.asarray(bed.qstart, np.int64)[rows][pos].astype(np.int32)
    qend = np.asarray(bed.qend, np.int64)[rows][pos].astype(np.int32)
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
    calls = {'segments': ctx.cluster_path_segments, 'segments_any': ctx.cluster_path_segments_any}
    ev, blobs = {k: [] for k in calls}, {}
    for k in range(warmup + repeats):                        # alternated: plain, _any, plain, _any ...
        for line, call in calls.items():
            got = call(qkey, qend)
            if k >= warmup:
                ev[line].append(ctx.cluster_path_segments_timings()['segments'])
            blobs[line] = [a.tobytes() for a in got]
    assert blobs['segments'] == blobs['segments_any']
    plain, anyl = sgt.stats(ev['segments']), sgt.stats(ev['segments_any'])
    base = {'config': name, **cfg, 'n_intervals': csr.n_intervals, 'n_clusters': info['n_clusters'],
            'tokens': int(paths[4].size), **rows_by_k(paths[2], np.diff(paths[1])), 'same_bytes': True,
            'any_inside_plain_spread': bool(plain['min'] <= anyl['median'] <= plain['max']), 'repeats': repeats,
            'warmup': warmup}
    for line in calls:
        print(json.dumps({**base, 'line': line, 'ms': {'event': sgt.stats(ev[line])}}), flush=True)
    ctx.close()


def run_long(name, cfg, repeats, warmup):
    from fslr_amd import _lib, cluster
    data, n_long = cat.long_input(cfg)
    note(f'{name}: input made')
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
    qend = (qkey + np.random.default_rng(29).integers(0, 1 << 10, csr.n_intervals)).astype(np.int32)
    info = ctx.cluster_table(labels)
    ctx.cluster_loci()
    paths = ctx.cluster_paths_any(qkey, rev)
    note(f'{name}: path rows made')
    por = paths[6]
    t = {'wall': [], 'event': []}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        got = ctx.cluster_path_segments_any(qkey, qend)
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            t['wall'].append(wall)
            t['event'].append(ctx.cluster_path_segments_timings()['segments'])
    h0 = time.perf_counter()
    want = sgt.host_rows(csr, paths, qkey, qend)
    host_ms = (time.perf_counter() - h0) * 1e3
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    base = {'config': name, **cfg, 'n_real': n, 'n_virtual': int(ctx.n_reads), 'n_intervals': csr.n_intervals,
            'lengthened_reads': n_long, 'longest_read': int(lens.max()), 'clustered_reads': int((por >= 0).sum()),
            'clustered_long_reads': int(((por >= 0) & (lens > 64)).sum()), 'n_clusters': info['n_clusters'],
            'tokens': int(paths[4].size), **rows_by_k(paths[2], np.diff(paths[1])),
            'gaps_nonzero': int((got[7] != 0).sum()), 'repeats': repeats, 'warmup': warmup}
    print(json.dumps({**base, 'line': 'segments_any', 'ms': {k: sgt.stats(v) for k, v in t.items()}}), flush=True)
    print(json.dumps({**base, 'line': 'host_composition', 'equal': True, 'ms': {'wall': host_ms}}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help='(child) measure this config in this process')
    ap.add_argument('--configs', default='cfg3,long')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=420, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'segments_any', 'timing.jsonl'))
    args = ap.parse_args()
    if args.child:
        cfg = CONFIGS[args.child]
        (run_plain if cfg['kind'] == 'plain' else run_long)(args.child, cfg, args.repeats, args.warmup)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.configs.split(','):
        # a fresh child under its own limit (its notes go straight to stderr); a failure writes nothing and ends the run
        r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--child',
                            name, '--repeats', str(args.repeats), '--warmup', str(args.warmup)],
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
