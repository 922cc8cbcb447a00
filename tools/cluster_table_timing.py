#!/usr/bin/env python3
"""The stages after the connected components, host against device, in one process on one box:

    python tools/cluster_table_timing.py [--configs cfg3,cfg5] [--out profiles/r08/cluster_table_timing.jsonl]

For cfg3 (synth.generate(1000000, 16, 11)) and the cfg5 generator (synth.generate(10000000, 64, 13,
dist='zipf')) the labels come from the normal device query (sweep, edge cap, components).  The code space
is the CLI's: one qname code per read (csr.read_qcode), every code present, a qname-grouped file with two
rows more than the read has intervals, seeded int64 scores.  Timed, after --warmup, over --repeats:

* ``host``: fastcli._assign_host + fastcli._choose_host, the numpy block the columnar CLI ran before the
  device calls existed and still runs where they do not apply (wall time).
* ``device``: Context.cluster_table() on the labels resident in the context (the CLI's case), then
  assign_clusters and choose_representatives: wall time with every H2D / D2H copy and the Python wrappers,
  and the library's HIP-event times (fslr_cluster_timings).
* ``device_host_labels``: the same with the labels uploaded from the host (the multi-GPU / long-read case).

Each line carries median / min / max; the two paths must choose the same codes.  The ratio is a
description, not a pass mark.
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


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def run(name, repeats, warmup):
    from fslr_amd import _lib, fastcli, synth
    from fslr_amd.prep import fold_overlap_threshold, pass_table
    cfg = CONFIGS[name]
    t0 = time.perf_counter()
    csr = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'], dist=cfg['dist']).interval_data().csr()
    prep_s = time.perf_counter() - t0
    n = csr.n_reads
    ctx = _lib.Context(0, profiling=True)
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, 0.8))
    ctx.reserve_edges(max(1 << 16, 12 * n))
    ctx.build_index()
    st = ctx.run_query(0.96, 0.75, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10)
    ctx.apply_edge_cap(10)
    ctx.components()
    labels = ctx.labels()
    # the CLI's code space
    rng = np.random.default_rng(5)
    read_qcode = np.asarray(csr.read_qcode, np.int64)
    n_q = int(read_qcode.max()) + 1
    rows_of = np.full(n_q, 2, np.int64)
    rows_of[read_qcode] += np.diff(np.asarray(csr.read_off, np.int64))
    qc = np.repeat(np.arange(n_q, dtype=np.int64), rows_of)
    present = np.ones(n_q, bool)
    keys = np.arange(n_q)
    sums = rng.integers(0, 3000, n_q) * rows_of + rng.integers(0, 3, n_q)        # many tied means
    avg = sums.astype(np.float64) / rows_of
    first_row = np.concatenate(([0], np.cumsum(rows_of)[:-1]))

    def host():
        q_cid, q_size, k, n_cl = fastcli._assign_host(labels, read_qcode, present, n_q)
        return q_cid, k, n_cl, fastcli._choose_host(q_cid, keys, avg, first_row, qc, qc.size, n_q)

    def device(lab):
        n_cl = ctx.cluster_table(lab)['n_clusters']
        q_cid, q_size, k = ctx.assign_clusters(present, read_qcode)
        avg_d, win = ctx.choose_representatives(q_cid, sums, rows_of, first_row, n_cl + k)
        chosen = np.zeros(n_q, bool)
        chosen[win[win >= 0]] = True
        return q_cid, k, n_cl, chosen, avg_d

    base = {'config': name, **cfg, 'n_codes': n_q, 'rows': int(qc.size), 'edges': int(st['n_edges']),
            'repeats': repeats, 'warmup': warmup, 'host_prep_s': prep_s}
    want = host()
    out = {}
    for mode, lab in (('device', None), ('device_host_labels', labels)):
        t = {k: [] for k in ('wall', 'table', 'assign', 'choose')}
        for k in range(warmup + repeats):
            w0 = time.perf_counter()
            got = device(lab)
            wall = (time.perf_counter() - w0) * 1e3
            if k >= warmup:
                t['wall'].append(wall)
                for key, v in ctx.cluster_timings().items():
                    t[key].append(v)
        assert np.array_equal(got[0], want[0]) and got[1:3] == want[1:3] and np.array_equal(got[3], want[3]), mode
        assert got[4].tobytes() == avg.tobytes(), mode
        out[mode] = stats(t['wall'])
        print(json.dumps({**base, 'line': mode, 'n_clusters': got[2], 'singletons': got[1],
                          'ms': {k: stats(v) for k, v in t.items()}}), flush=True)
    t = []
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        host()
        if k >= warmup:
            t.append((time.perf_counter() - w0) * 1e3)
    hs = stats(t)
    print(json.dumps({**base, 'line': 'host', 'ms': {'wall': hs},
                      'host_over_device': hs['median'] / out['device']['median'],
                      'host_over_device_host_labels': hs['median'] / out['device_host_labels']['median']}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None, help='(child) measure this config in this process')
    ap.add_argument('--configs', default='cfg3,cfg5')
    ap.add_argument('--repeats', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--limit', type=int, default=540, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'r08', 'cluster_table_timing.jsonl'))
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
        if r.returncode != 0 or len(lines) != 3:
            print(f'{name}: exit status {r.returncode}; nothing written', file=sys.stderr)
            return r.returncode or 1
        with open(args.out, 'a') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
