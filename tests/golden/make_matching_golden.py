#!/usr/bin/env python3
"""Record the reference's own first-fit matching for about 300 read pairs of the committed golden inputs.

    python tests/golden/make_matching_golden.py

Runs on the CPU where the reference is present (refharness.load()) and writes
``tests/golden/matching/pairs.npz``, which holds indices only.

The reference's overall_jaccard_similarity (cluster.py:140-170) returns the count, not the matching, but its
scratch array marks the taken columns, and a row's choice depends on the earlier rows alone.  So the column
newly marked between the calls on ``l1[:i]`` and ``l1[:i + 1]`` is row i's column; no new mark means the row
is unmatched; a raise ends the pair (tests/matching_ref.py prefix_matching, here on the reference's function
and its own IntervalItem lists from its own prepare_data).

Per source fixture ``s`` (``sources``): ``<s>_a``, ``<s>_b`` read ranks (reads rank by first appearance in the
prepare_data list, a read's intervals keep list order: the product's CSR order, which this script checks
against the product's host stages), ``<s>_raised`` (the reference raised ZeroDivisionError for the pair: no
rows), ``<s>_off`` / ``<s>_i`` / ``<s>_j`` the rows, and ``<s>_pct`` the overlap cutoff.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)

PCT = 0.8


def reference_lists(ref, name):
    """The reference's prepare_data list of fixture ``name`` (main.py:209-237), grouped per read in order of
    first appearance: (qnames, lists of the reference's IntervalItem)."""
    import pandas as pd

    import fixtures as fx
    kw = fx.cli_options(name)
    bed = pd.read_csv(os.path.join(fx.input_dir(name), 'input.mappings.bed.gz'), sep='\t')
    mask = {m for m in kw['cluster_mask'].split(',') if m in set(bed['chrom']) or m == 'subtelomere'}
    lengths = ref.get_chromosome_lengths(fx.input_bam(name))
    bed, chr_lengths, mask, _ = ref.rename_chromosomes(bed, lengths, mask)
    data = ref.prepare_data(ref.keep_fillings(bed), mask, chr_lengths, threshold=500_000)
    lists = {}
    for it in data:
        lists.setdefault(it.qname, []).append(it)
    return list(lists), list(lists.values())


def product_lists(name):
    import host_pipeline as hp
    from fslr_amd import cluster
    data, _, _ = hp.host_prepare(name)
    csr = cluster.IntervalData.from_items(data).csr() if not hasattr(data, 'csr') else data.csr()
    dp = np.asarray(csr.data_pos, np.int64)
    names = data.qnames[csr.read_qcode]
    out = []
    for r in range(csr.n_reads):
        k = dp[csr.read_off[r]:csr.read_off[r + 1]]
        out.append(list(zip(data.chrom[k].tolist(), data.start[k].tolist(), data.end[k].tolist(),
                            data.aln_size[k].tolist())))
    return list(names), out


def shape(rows):
    """(a row took a column above a free one, an unmatched row lies between matched ones)"""
    taken, skipped = set(), False
    for i, j in rows:
        skipped |= any(c not in taken for c in range(j))
        taken.add(j)
    got = [i for i, _ in rows]
    return skipped, bool(got) and got != list(range(got[0], got[0] + len(got)))


def choose_pairs(name, qnames, lists, plain, rng):
    import fixtures as fx
    from matching_ref import matching_or_raise
    n = len(lists)
    rank = {q: r for r, q in enumerate(qnames)}
    # the rarer shapes first, found among rank neighbours with the plain statement (the recording below is
    # the reference's)
    odd = [[], []]
    for x, y in [(r, r + d) for d in (1, 2, 3, -1, -2) for r in range(max(0, -d), min(n, n - d))]:
        for k, hit in enumerate(shape(matching_or_raise(plain[x], plain[y], PCT)[0])):
            if hit and len(odd[k]) < 10 and (x, y) not in odd[0]:
                odd[k].append((x, y))
    pairs = odd[0] + odd[1]
    st = fx.stage(name)
    if st:                                             # the reference's own edges, both orientations
        e = [(rank[x[0]], rank[x[1]]) for x in st['edges']]
        for k in rng.choice(len(e), min(50, len(e)), replace=False).tolist():
            pairs.append(e[k] if k % 3 else e[k][::-1])
    has_zero = [r for r in range(n) if any(it.aln_size == 0 for it in lists[r])]
    for r in has_zero:                                 # reads around an aln_size == 0 interval, both ways
        for d in (-2, -1, 1, 2):
            if 0 <= r + d < n:
                pairs += [(r, r + d), (r + d, r)]
        pairs.append((r, r))
    near = rng.integers(0, n - 1, 25)
    pairs += [(int(r), int(r) + 1) for r in near]
    pairs += [(int(x), int(y)) for x, y in rng.integers(0, n, (20, 2))]
    pairs += [(int(r), int(r)) for r in rng.integers(0, n, 5)]
    return pairs


def main():
    import refharness
    from matching_ref import matching_or_raise, prefix_matching
    ref, _ = refharness.load()
    rng = np.random.default_rng(20241021)
    out, total = {'sources': np.array(['mixed_2k_l8', 'ties_600', 'zerodiv'])}, 0
    seen = dict(zero=0, raised=0, not_lowest=0, unmatched_between=0)
    for name in out['sources'].tolist():
        qnames, lists = reference_lists(ref, name)
        pq, pl = product_lists(name)
        assert pq == qnames, 'the product ranks the reads as the reference lists them'
        assert pl == [[(it.chrom, it.start, it.end, it.aln_size) for it in l] for l in lists]
        pairs = choose_pairs(name, qnames, lists, pl, rng)
        off, ii, jj, raised = [0], [], [], []
        scratch = np.zeros(max(len(l) for l in lists), np.int8)
        for a, b in pairs:
            try:
                rows = prefix_matching(ref.overall_jaccard_similarity, lists[a], lists[b], PCT, scratch)
                _, n_i = ref.overall_jaccard_similarity(lists[a], lists[b], scratch, PCT, 0.5)
                assert n_i == len(rows)
                raised.append(False)
            except ZeroDivisionError:
                rows = []
                raised.append(True)
            # the plain statement agrees with the recording
            assert matching_or_raise(pl[a], pl[b], PCT) == (rows, raised[-1]), (name, a, b)
            seen['zero'] += not rows and not raised[-1]
            seen['raised'] += raised[-1]
            skipped, gap = shape(rows)
            seen['not_lowest'] += skipped
            seen['unmatched_between'] += gap
            ii += [r[0] for r in rows]
            jj += [r[1] for r in rows]
            off.append(len(ii))
        a, b = np.array(pairs, np.int32).T
        out.update({f'{name}_a': a, f'{name}_b': b, f'{name}_raised': np.array(raised),
                    f'{name}_off': np.array(off, np.int64), f'{name}_i': np.array(ii, np.int32),
                    f'{name}_j': np.array(jj, np.int32), f'{name}_pct': np.array(PCT)})
        total += len(pairs)
    assert 250 <= total <= 400 and min(seen.values()) >= 3, (total, seen)
    path = os.path.join(HERE, 'matching', 'pairs.npz')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', total, 'pairs;', seen)


if __name__ == '__main__':
    main()
