#!/usr/bin/env python3
"""Cluster paths: the device call's time, and whether packing several tokens per sort key earns its code, in one
process on one box:

    python tools/paths_timing.py [--configs cfg3] [--out profiles/paths/paths_timing.jsonl]

For cfg3 (synth.generate(1000000, 16, 11)) the labels come from the normal device query (sweep, edge cap,
components), the table from those resident labels and the loci rows from fslr_cluster_loci.  ``qstart`` is the
generator's cumulative query position of each filling; the strand bits are random with a fixed seed.  Timed, after
--warmup, over --repeats, once per line:

* ``packed``: FSLR_PATHS_PACK unset, as many tokens per 64-bit sort key as fit;
* ``pack1``: FSLR_PATHS_PACK=1, one token per key, one sort pass per chain position;
* ``junctions``: fslr_cluster_junctions on the same state, for scale.

Per line: the HIP-event time of the call (fslr_cluster_paths_timings), the wall time of Context.cluster_paths() (the
two columns' upload, the call, fslr_get_cluster_paths and the wrapper), the rows, tokens and sort passes, each time as
median / min / max.  Both packings must give the same bytes.
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


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def passes(loci_rows, longest, pack_cap):
    """The sort passes of a call: ceil(longest / p), p = tokens per key (include/fslr_hip.h, paths.hip)."""
    kbits = max(1, int(2 * loci_rows).bit_length())
    p = max(1, min(64 // kbits, pack_cap or 64))
    return p, -(-longest // p)


def run(name, repeats, warmup):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    cfg = CONFIGS[name]
    bed = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'], dist=cfg['dist'])
    data = bed.interval_data()
    csr = data.csr()
    n = csr.n_reads
    pos = np.asarray(csr.data_pos, np.int64)
    qkey = np.asarray(bed.qstart, np.int64)[np.asarray(data.index, np.int64)][pos].astype(np.int32)
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
    cid, _ = ctx.cluster_ids()
    longest = int(np.diff(csr.read_off)[cid >= 0].max()) if (cid >= 0).any() else 0
    base = {'config': name, **cfg, 'n_intervals': csr.n_intervals, 'edges': int(st['n_edges']),
            'n_clusters': info['n_clusters'], 'n_nodes': info['n_nodes'], 'loci_rows': int(loci[1].size),
            'longest_clustered_read': longest, 'repeats': repeats, 'warmup': warmup}
    ev = []
    for k in range(warmup + repeats):
        ctx.cluster_junctions(qkey, rev)
        if k >= warmup:
            ev.append(ctx.cluster_junctions_timings()['junctions'])
    junction_line = json.dumps({**base, 'line': 'junctions', 'ms': {'event': stats(ev)}})
    blobs = {}
    for line, pack in (('packed', None), ('pack1', 1), ('packed_again', None)):
        if pack is None:
            os.environ.pop('FSLR_PATHS_PACK', None)
        else:
            os.environ['FSLR_PATHS_PACK'] = str(pack)
        t = {'wall': [], 'event': []}
        for k in range(warmup + repeats):
            w0 = time.perf_counter()
            got = ctx.cluster_paths(qkey, rev)
            wall = (time.perf_counter() - w0) * 1e3
            if k >= warmup:
                t['wall'].append(wall)
                t['event'].append(ctx.cluster_paths_timings()['paths'])
        blobs[line] = [a.tobytes() for a in got]
        p, n_pass = passes(int(loci[1].size), longest, pack)
        print(json.dumps({**base, 'line': line, 'rows': int(got[2].size), 'tokens': int(got[4].size),
                          'tokens_per_key': p, 'sort_passes': n_pass, 'ms': {k: stats(v) for k, v in t.items()}}), flush=True)
    os.environ.pop('FSLR_PATHS_PACK', None)
    assert blobs['packed'] == blobs['pack1'] == blobs['packed_again']
    assert int(got[2].sum()) == info['n_nodes']
    print(junction_line, flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help='(child) measure this config in this process')
    ap.add_argument('--configs', default='cfg3')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=540, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'paths', 'paths_timing.jsonl'))
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
        if r.returncode != 0 or len(lines) != 4:
            print(f'{name}: exit status {r.returncode}; nothing written', file=sys.stderr)
            return r.returncode or 1
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
