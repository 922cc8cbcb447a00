"""A short numpy / Python restatement of the three host stages that follow the connected components:
get_subgraphs (cluster.py:230-234), assign_clusters (main.py:251-342) and choose_alignment
(cluster.py:237-254), over read ranks and qname codes.  tests/test_cluster_table_host.py pins it to the
reference's own outputs; the GPU tests compare the device calls with it."""
import numpy as np


def labels_from_components(components, rank_of, n):
    """Min-rank labels of ``n`` reads from a list of components (collections of names; ``rank_of`` maps a
    name to its read rank): every read of a component gets the component's smallest rank, the others their own."""
    lab = np.arange(n, dtype=np.int32)
    for comp in components:
        r = np.asarray(sorted(rank_of[q] for q in comp), np.int32)
        lab[r] = r[0]
    return lab


def labels_from_edges(n, a, b):
    """Min-rank labels from an edge list, by a plain union-find."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.asarray([find(x) for x in range(n)], np.int32)


def valid_labels(labels):
    """The first r with labels[r] outside [0, r] or labels[labels[r]] != labels[r], or -1."""
    lab = np.asarray(labels, np.int64)
    r = np.arange(lab.size)
    bad = (lab < 0) | (lab > r)
    bad[~bad] = lab[lab[~bad]] != lab[~bad]
    return int(np.argmax(bad)) if bad.any() else -1


def table(labels):
    """cid, size per rank; roots, off, members of the components of two or more reads, in ascending root
    order (the reference's networkx order), members ascending in rank."""
    lab = np.asarray(labels, np.int64)
    n = lab.size
    counts = np.bincount(lab, minlength=n) if n else np.zeros(0, np.int64)
    size = counts[lab] if n else np.zeros(0, np.int64)
    roots = np.flatnonzero(counts >= 2)
    rid = np.full(n, -1, np.int64)
    rid[roots] = np.arange(roots.size)
    cid = np.where(size >= 2, rid[lab], -1) if n else np.zeros(0, np.int64)
    nodes = np.flatnonzero(cid >= 0)
    members = nodes[np.argsort(cid[nodes], kind='stable')]
    off = np.concatenate(([0], np.cumsum(counts[roots]))).astype(np.int64)
    return {'cid': cid.astype(np.int32), 'size': size.astype(np.int32), 'roots': roots.astype(np.int32), 'off': off,
            'members': members.astype(np.int32), 'n_clusters': int(roots.size), 'n_nodes': int(nodes.size),
            'max_size': int(counts.max()) if roots.size else 0}


def assign(t, present, code_of_rank=None):
    """main.py:334-342 over qname codes: (cluster, n_reads, n_singletons).  A present code whose rank is
    clustered gets the rank's cid and size, every other present code n_clusters + k in ascending code order
    and 1, an absent code -1 and 0."""
    present = np.asarray(present, bool)
    nc = present.size
    cor = np.arange(t['cid'].size) if code_of_rank is None else np.asarray(code_of_rank, np.int64)
    cl = np.full(nc, -1, np.int64)
    nr = np.zeros(nc, np.int64)
    node = t['cid'] >= 0
    cl[cor[node]] = t['cid'][node]
    nr[cor[node]] = t['size'][node]
    single = present & (cl < 0)
    k = int(single.sum())
    cl[single] = t['n_clusters'] + np.arange(k)
    nr[single] = 1
    cl[~present] = -1
    nr[~present] = 0
    return cl, nr, k


def choose(cluster, score_sum, score_cnt, first_row, n_out):
    """cluster.py:237-254 over qname codes: (avg, winner_code).  Python's own float division and a plain
    loop: the largest mean of each cluster, ties to the smallest first_row."""
    cluster, score_sum, score_cnt, first_row = (np.asarray(x, np.int64).tolist()
                                                for x in (cluster, score_sum, score_cnt, first_row))
    avg = np.full(len(cluster), np.nan)
    best = {}
    for c, (g, s, q, fr) in enumerate(zip(cluster, score_sum, score_cnt, first_row)):
        if g < 0 or q == 0:
            continue
        a = float(s) / float(q)
        avg[c] = a
        if g not in best or (a, -fr) > (best[g][0], -best[g][1]):
            best[g] = (a, fr, c)
    win = np.full(n_out, -1, np.int64)
    for g, (_, _, c) in best.items():
        win[g] = c
    return avg, win


def golden_fixtures():
    """The fixtures with expected CLI outputs."""
    import fixtures as fx
    return [n for n in fx.FIXTURES if fx.expected_text(n, 'cluster') is not None]


def fixture_case(name):
    """A golden fixture as the stages see it: min-rank labels from the reference's get_subgraphs list
    (stage.json 'components'), the qname of each read rank, the reference's two output frames, and the code
    space of the cluster frame (codes by first appearance, their score sums, counts and first rows)."""
    import io

    import fixtures as fx
    import pandas as pd
    from host_pipeline import host_prepare
    data, _, _ = host_prepare(name)
    csr = data.csr()
    names = np.asarray(data.qnames, dtype=object)[np.asarray(csr.read_qcode)]
    rank_of = {q: r for r, q in enumerate(names.tolist())}
    comps = fx.stage(name)['components']
    lab = labels_from_components(comps, rank_of, len(names))
    exp = pd.read_csv(io.StringIO(fx.expected_text(name, 'cluster')), sep='\t')
    rep = pd.read_csv(io.StringIO(fx.expected_text(name, 'representative')), sep='\t', float_precision='round_trip')
    codes, uniq = pd.factorize(exp['qname'])
    code_of = {q: c for c, q in enumerate(uniq.tolist())}
    score = exp['alignment_score'].to_numpy().astype(np.int64)
    first_row = np.full(len(uniq), -1, np.int64)
    first_row[codes[::-1]] = np.arange(len(codes) - 1, -1, -1)
    return {'labels': lab, 'names': names, 'components': comps, 'rank_of': rank_of, 'cluster_bed': exp,
            'representative_bed': rep, 'codes': codes, 'n_codes': len(uniq),
            'code_of_rank': np.asarray([code_of[q] for q in names.tolist()], np.int64),
            'score_sum': np.bincount(codes, weights=score.astype(np.float64), minlength=len(uniq)).astype(np.int64),
            'score_cnt': np.bincount(codes, minlength=len(uniq)).astype(np.int64), 'first_row': first_row}


def check_fixture_outputs(case, cl, nr, k, avg, win):
    """The assign columns and the representatives (per code) against the reference's output frames."""
    exp, rep, codes = case['cluster_bed'], case['representative_bed'], case['codes']
    dtype = np.float64 if k else np.int64
    assert exp['cluster'].dtype == dtype and exp['n_reads'].dtype == dtype
    np.testing.assert_array_equal(cl[codes].astype(dtype), exp['cluster'].to_numpy())
    np.testing.assert_array_equal(nr[codes].astype(dtype), exp['n_reads'].to_numpy())
    chosen = np.zeros(case['n_codes'], bool)
    chosen[win[win >= 0]] = True
    rows = chosen[codes]
    assert exp['qname'][rows].tolist() == rep['qname'].tolist()
    np.testing.assert_array_equal(exp[rows].index.to_numpy(), np.flatnonzero(rows))
    assert avg[codes][rows].view(np.int64).tolist() == rep['avg_alignment_score'].to_numpy().view(np.int64).tolist()
