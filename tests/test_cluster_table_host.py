"""tests/cluster_ref.py (the numpy restatement of get_subgraphs, assign_clusters and choose_alignment the
GPU tests compare the device with) against the reference's own outputs on every golden fixture, and against
networkx on random graphs."""
import networkx as nx
import numpy as np
import pytest

import cluster_ref as cr


@pytest.mark.parametrize('name', cr.golden_fixtures())
def test_restatement_reproduces_the_reference_outputs(name):
    case = cr.fixture_case(name)
    lab = case['labels']
    assert cr.valid_labels(lab) == -1
    t = cr.table(lab)
    # the reference's get_subgraphs list, in its order: ascending smallest rank
    comps = case['components']
    assert t['n_clusters'] == len(comps)
    got = [set(case['names'][t['members'][t['off'][k]:t['off'][k + 1]]].tolist()) for k in range(len(comps))]
    assert got == [set(c) for c in comps]
    assert t['roots'].tolist() == [min(case['rank_of'][q] for q in c) for c in comps]
    assert t['n_nodes'] == sum(len(c) for c in comps) and t['max_size'] == max(len(c) for c in comps)
    cl, nr, k = cr.assign(t, np.ones(case['n_codes'], bool), case['code_of_rank'])
    avg, win = cr.choose(cl, case['score_sum'], case['score_cnt'], case['first_row'], t['n_clusters'] + k)
    cr.check_fixture_outputs(case, cl, nr, k, avg, win)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_table_matches_networkx_on_random_graphs(seed):
    rng = np.random.default_rng(seed)
    n = 3000
    m = int(rng.integers(600, 1500))
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = a != b
    a, b = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    order = np.lexsort((b, a))
    G = nx.Graph()
    G.add_edges_from(zip(a[order].tolist(), b[order].tolist()))
    comps = list(nx.connected_components(G))
    lab = cr.labels_from_edges(n, a, b)
    assert cr.valid_labels(lab) == -1
    t = cr.table(lab)
    assert [set(t['members'][t['off'][k]:t['off'][k + 1]].tolist()) for k in range(t['n_clusters'])] == comps
    assert t['roots'].tolist() == [min(c) for c in comps] == sorted(min(c) for c in comps)
    assert t['n_nodes'] == G.number_of_nodes()
    for k, c in enumerate(comps):
        members = sorted(c)
        assert t['members'][t['off'][k]:t['off'][k + 1]].tolist() == members
        assert (t['cid'][members] == k).all() and (t['size'][members] == len(c)).all()
    alone = np.setdiff1d(np.arange(n), np.fromiter(G.nodes, int))
    assert (t['cid'][alone] == -1).all() and (t['size'][alone] == 1).all()


def test_valid_labels_reports_the_first_offender():
    assert cr.valid_labels([0, 0, 2, 2]) == -1
    assert cr.valid_labels([0, 2, 2]) == 1
    assert cr.valid_labels([0, -1, 1]) == 1
    assert cr.valid_labels([0, 0, 1, 2]) == 2
    assert cr.valid_labels([]) == -1
