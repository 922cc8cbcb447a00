#!/usr/bin/env python3
"""Cluster junctions, device call against the host composition it replaces, in one process on one box:

    python tools/junctions_timing.py [--configs cfg3] [--out profiles/junctions/junctions_timing.jsonl]

For cfg3 (synth.generate(1000000, 16, 11)) the labels come from the normal device query (sweep, edge cap,
components), the table from those resident labels and the loci rows from fslr_cluster_loci.  ``qstart`` is the
generator's cumulative query position of each filling; the strand bits are random with a fixed seed.  Timed,
after --warmup, over --repeats:

* ``device``: Context.cluster_junctions() = the two columns' upload, fslr_cluster_junctions,
  fslr_get_cluster_junctions and the Python wrapper (wall time), and the library's HIP-event time of
  fslr_cluster_junctions (fslr_cluster_junctions_timings: the device work behind the upload).
* ``host``: what a caller does without the call: fslr_get_cluster_ids + fslr_get_csr + fslr_get_cluster_loci (the
  D2H copies), then vectorised numpy: every interval's locus by a search in the rows, the chains by a lexsort on
  (read, key, position), the ends and breakpoints of the adjacent pairs, a stable sort on the pair of ends and
  segment reductions.  The phases are timed apart.

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
           'small': dict(n_reads=20_000, lmax=16, seed=11, dist='uniform')}
COLUMNS = ('off', 'locus_a', 'side_a', 'locus_b', 'side_b', 'n_obs', 'n_reads', 'bp_a_min', 'bp_a_max', 'bp_b_min',
           'bp_b_max')


def stats(v):
    return {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}


def host_junctions(cid, n_clusters, csr, loci, qkey, rev):
    """The rows from the cluster ids, the CSR, the loci rows and the two columns, vectorised numpy: (columns,
    seconds of the locus search and the chain sort, of the pair sort and the reductions)."""
    t0 = time.perf_counter()
    read_off = np.asarray(csr['read_off'], np.int64)
    lens = np.diff(read_off)
    read_of = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    c_iv = cid[read_of].astype(np.int64)
    sel = np.flatnonzero((c_iv >= 0) & (lens[read_of] >= 2))
    off = np.zeros(n_clusters + 1, np.int64)
    if sel.size == 0:
        z, zb = np.zeros(0, np.int32), np.zeros(0, np.uint8)
        return (off, z, zb, z, zb, z, z, z, z, z, z), time.perf_counter() - t0, 0.0
    l_off, l_chrom, l_start = loci[0], loci[1].astype(np.int64), loci[2].astype(np.int64)
    cl_of_row = np.repeat(np.arange(n_clusters, dtype=np.int64), np.diff(l_off))
    nch = int(l_chrom.max()) + 1
    row_key = ((cl_of_row * nch + l_chrom) << 31) + l_start
    s, e = csr['iv_start'][sel].astype(np.int64), csr['iv_end'][sel].astype(np.int64)
    row = np.searchsorted(row_key, ((c_iv[sel] * nch + csr['iv_chrom'][sel].astype(np.int64)) << 31) + s, side='right') - 1
    r, rv = read_of[sel], rev[sel].astype(bool)
    order = np.lexsort((sel, qkey[sel], r))
    r, rv, row, s, e = r[order], rv[order], row[order], s[order], e[order]
    pair = np.flatnonzero(r[1:] == r[:-1])
    x, y = pair, pair + 1
    ea, ba = row[x] * 2 + ~rv[x], np.where(rv[x], s[x], e[x])
    eb, bb = row[y] * 2 + rv[y], np.where(rv[y], e[y], s[y])
    swap = (ea > eb) | ((ea == eb) & (ba > bb))
    ea, eb, ba, bb = np.where(swap, eb, ea), np.where(swap, ea, eb), np.where(swap, bb, ba), np.where(swap, ba, bb)
    rd = r[x]
    t1 = time.perf_counter()
    key = (ea << 31) | eb
    o = np.argsort(key, kind='stable')
    key, ba, bb, rd = key[o], ba[o], bb[o], rd[o]
    head = np.ones(key.size, bool)
    head[1:] = key[1:] != key[:-1]
    hp = np.flatnonzero(head)
    new_read = head.copy()
    new_read[1:] |= rd[1:] != rd[:-1]
    ka, kb = key[hp] >> 31, key[hp] & ((1 << 31) - 1)
    np.cumsum(np.bincount(cl_of_row[ka >> 1], minlength=n_clusters), out=off[1:])
    i32 = lambda a: a.astype(np.int32)
    cols = (off, i32(ka >> 1), (ka & 1).astype(np.uint8), i32(kb >> 1), (kb & 1).astype(np.uint8),
            i32(np.diff(np.append(hp, key.size))), i32(np.add.reduceat(new_read.astype(np.int64), hp)),
            i32(np.minimum.reduceat(ba, hp)), i32(np.maximum.reduceat(ba, hp)),
            i32(np.minimum.reduceat(bb, hp)), i32(np.maximum.reduceat(bb, hp)))
    return cols, t1 - t0, time.perf_counter() - t1


def run(name, repeats, warmup):
    from fslr_amd import _lib, synth
    from fslr_amd.prep import pass_table
    cfg = CONFIGS[name]
    bed = synth.generate(cfg['n_reads'], cfg['lmax'], cfg['seed'], dist=cfg['dist'])
    data = bed.interval_data()
    csr = data.csr()
    n = csr.n_reads
    pos = np.asarray(csr.data_pos, np.int64)
    qkey = np.asarray(bed.qstart, np.int64)[np.asarray(data.index, np.int64)][pos].astype(np.int32)
    rev = np.random.default_rng(17).integers(0, 2, csr.n_intervals).astype(np.uint8)
    ctx = _lib.Context(0, profiling=True)
    # the reads from rows (the columnar CLI's upload): fslr_get_csr answers on such a context.  The `data` list
    # is start-sorted already, so its own order is the start order
    rows = dict(chrom=data.chrom, start=data.start, end=data.end, aln=data.aln_size, qcode=data.qcode,
                nal=data.n_alignments, qlen2=data.qlen2)
    ctx.rows_upload(rows, int(np.asarray(data.qcode).max()) + 1, int(np.asarray(data.chrom).max()) + 1)
    made = ctx.set_reads_rows(np.arange(len(data), dtype=np.int64), None, 0.8)
    assert (made['n_reads'], made['n_intervals'], made['n_chroms']) == (n, csr.n_intervals, csr.n_chroms)
    d = ctx.device_csr(csr.n_intervals, csr.n_chroms)
    assert np.array_equal(d['data_pos'], pos)                   # the device's CSR order is the host's
    ctx.reserve_edges(max(1 << 16, 12 * n))
    ctx.build_index()
    st = ctx.run_query(0.96, 0.75, pass_table([1, 1, 0.66, 0.66, 0.66, 0.5]), 10)
    ctx.apply_edge_cap(10)
    ctx.components()
    info = ctx.cluster_table()
    loci = ctx.cluster_loci()
    base = {'config': name, **cfg, 'n_intervals': csr.n_intervals, 'edges': int(st['n_edges']),
            'n_clusters': info['n_clusters'], 'n_nodes': info['n_nodes'], 'loci_rows': int(loci[1].size),
            'repeats': repeats, 'warmup': warmup}

    t = {'wall': [], 'event': []}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        got = ctx.cluster_junctions(qkey, rev)
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            t['wall'].append(wall)
            t['event'].append(ctx.cluster_junctions_timings()['junctions'])
    dev = stats(t['wall'])
    print(json.dumps({**base, 'line': 'device', 'rows': int(got[1].size), 'observations': int(got[5].sum()),
                      'ms': {k: stats(v) for k, v in t.items()}}), flush=True)

    h = {'wall': [], 'copies': [], 'chains': [], 'reduce': []}
    for k in range(warmup + repeats):
        w0 = time.perf_counter()
        cid, _ = ctx.cluster_ids()
        d = ctx.device_csr(csr.n_intervals, csr.n_chroms)
        lrows = ctx.cluster_loci_rows()
        w1 = time.perf_counter()
        want, chain_s, reduce_s = host_junctions(cid, info['n_clusters'], d, lrows, qkey, rev)
        wall = (time.perf_counter() - w0) * 1e3
        if k >= warmup:
            h['wall'].append(wall)
            h['copies'].append((w1 - w0) * 1e3)
            h['chains'].append(chain_s * 1e3)
            h['reduce'].append(reduce_s * 1e3)
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
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--limit', type=int, default=540, help='seconds per config')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'junctions', 'junctions_timing.jsonl'))
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
