"""Directed tests of the edge-cap replay (cap.hip) against the plain reference tests/cap_ref.py, exactly.
The inputs are the hand-built ones of tests/cap_cases.py; tests/test_cap_ref.py asserts on the CPU that
each reaches the seam it is built for and pins the reference to the C oracle.

A  the closure T on arbitrary graphs, read back through witness reads, on every route reachable in-process
B  the visit lists (fslr_cap_local + fslr_cap_copy_local) after a real query
C  whole loops: query (both engines), fslr_apply_edge_cap, components
D  the environment-selected alternatives, each in a fresh child process

FSLR_CAP_REPLAY=dag is left out on purpose: its ready queue waits across wavefronts, so a defect there
would show as a hang, not as a failed assertion.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cap_cases as C
import cap_ref as R
import test_gpu_parity as parity
from fslr_amd import _lib
from fslr_amd.prep import fold_overlap_threshold, pass_table

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to('cuda:0')


def load(ctx, csr, overlap=0.8):
    ctx.load_csr(csr, fold_overlap_threshold(csr.iv_aln, overlap))
    ctx.reserve_edges(1 << 16)
    ctx.build_index()


def query(ctx, p, engine):
    args = (1 - p['qlen_diff'], 1 - p['nal_diff'], pass_table(p['cutoffs']))
    if engine == 'sweep':                  # no rerun: a fallback to the walk engine or an overflow fails here
        ctx.query(*args, engine='sweep')
        st = ctx.stats()
    else:
        st = ctx.run_query(*args, engine=engine)
    assert st['engine'] == engine
    return st


def edge_list(ctx):
    return ctx.edges(ctx.stats()['n_edges'])


def copy_local(ctx, nti, nh):
    counts = torch.full((max(nti, 1),), -7, dtype=torch.int32, device='cuda:0')
    hits = torch.full((max(nh, 1),), -7, dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    ctx.cap_copy_local(counts, hits)
    ctx.sync()
    return counts.cpu().numpy()[:nti], hits.cpu().numpy()[:nh]


# ------------------------------------------------------------------------------------ A: closure
ROUTES = ('context', 'gathered_sorted', 'gathered')
ORDERS = ('sorted', 'reversed', 'shuffled')


def device_closure(ctx, rows, thr, route):
    """T of the installed rows (graph read x = rank 2x) and the closure the route takes.
    context: fslr_cap_install_edges, fslr_cap_local over the context's edge list: k_cap_init, then
      k_cap_back + k_cap_join in batches of 8 rounds, k_cap_tpack / k_cap_tlist ('rounds').
    gathered_sorted: fslr_sort_edges, the (a, b) rows (with three padding rows) through
      fslr_cap_install_pairs at world 1: k_cap_runs finds one run per read, so fslr_cap_local takes
      k_cap_seed, k_cap_frontier_w<true> in batches of 16 rounds with k_cap_fcnt_roll between batches,
      and k_cap_tfin ('frontier').
    gathered: the same without the sort: rows that are not grouped by lower read make k_cap_runs flag
      them, forward degrees come from k_cap_gfwd and the closure is 'rounds' over the gathered rows;
      rows that happen to be grouped take 'frontier'."""
    m = len(rows)
    r4 = np.zeros((m, 4), np.int32)
    r4[:, :2] = 2 * np.asarray(rows, np.int64).reshape(-1, 2)
    r4[:, 2] = 1 | (1 << 8)
    t4 = dev(r4.reshape(-1))
    ctx.cap_install_edges(t4, m)
    kind = 'rounds'
    keep = None
    if route != 'context':
        if route == 'gathered_sorted':
            ctx.sort_edges()
        a, b, _, _ = ctx.edges(m)
        assert sorted(zip(a.tolist(), b.tolist())) == sorted(map(tuple, r4[:, :2].tolist()))
        if (np.diff(a) >= 0).all():
            kind = 'frontier'
        assert route != 'gathered_sorted' or kind == 'frontier'
        keep = torch.zeros(2 * (m + 3), dtype=torch.int32, device='cuda:0')
        torch.cuda.synchronize()
        ctx.edges_into(keep, m + 3)
        ctx.cap_install_pairs(keep, m + 3, 1, 0)
    nti, nh = ctx.cap_local(thr)
    nt = ctx.cap_sizes()[0]
    counts, hits = copy_local(ctx, nti, nh)
    assert nt == nti == nh and (counts == 1).all()           # one interval, one witness per member
    assert (hits % 2 == 1).all()
    del keep
    return ((hits - 1) // 2).tolist(), kind


@pytest.mark.parametrize('name', list(C.closure_shapes()))
def test_closure_on_every_route(ctx, name):
    """Each shape in three row orders through the three routes of device_closure(): T equals
    cap_ref.closure exactly, and the routes cover both closure implementations."""
    thr, n, rows = C.closure_shapes()[name]
    fwd = np.bincount([a for a, _ in rows], minlength=n)
    T, _ = R.closure(n, rows, fwd, thr)
    csr = C.witness_reads(n)
    load(ctx, csr)
    query(ctx, R.DEFAULT, 'sweep')
    kinds = set()
    for route in ROUTES:
        for order in ORDERS:
            got, kind = device_closure(ctx, C.ordered(rows, order), thr, route)
            assert got == T, (name, route, order)
            kinds.add(kind)
            if route == 'gathered' and order != 'sorted':
                assert kind == 'rounds'
    assert kinds == {'rounds', 'frontier'}


# ------------------------------------------------------------------------------------ B: visit lists
@pytest.mark.parametrize('cid,builder,args', C.list_cases(), ids=[c[0] for c in C.list_cases()])
def test_visit_lists(ctx, cid, builder, args):
    """fslr_cap_local after a full query: |T|, the T-intervals' hit counts and the partner reads in
    search order equal cap_ref.visit_lists (tie runs across the 64-hit chunk seam, the inclusive end, the
    read's own interval inside a run, backward-only / forward-only / empty intervals, two T reads of equal
    start)."""
    case = C.case(builder, *args)
    e = case.exp
    load(ctx, case.csr)
    st = query(ctx, case.params, 'sweep')
    assert st['n_edges'] == len(e['rows'])
    nti, nh = ctx.cap_local(case.thr)
    assert ctx.cap_sizes() == (len(e['T']), nti, nh)
    counts, hits = copy_local(ctx, nti, nh)
    assert counts.tolist() == [len(x) for x in e['lists']]
    assert hits.tolist() == [y for x in e['lists'] for y in x]


# ------------------------------------------------------------------------------------ C: loops
def run_loops(ctx, case, engine, thr=None, loaded=False):
    """query, fslr_apply_edge_cap, components; everything compared with cap_ref.  Returns the cap stats."""
    thr = case.thr if thr is None else thr
    e = case.exp if thr == case.thr else R.expected(case.csr, case.params, thr)
    if not loaded:
        load(ctx, case.csr)
    st = query(ctx, case.params, engine)
    a, b, I, U = ctx.edges(st['n_edges'])
    assert sorted(zip(a.tolist(), b.tolist(), I.tolist(), U.tolist())) == sorted(e['star']['edges'])
    cap = ctx.apply_edge_cap(thr)
    ctx.components()
    a, b, I, U = edge_list(ctx)
    g = dict(stats=dict(st, cap=cap, max_fwd=cap['max_fwd']), labels=ctx.labels(), fwd=ctx.fwd_degree(), a=a, b=b,
             I=I, U=U)
    parity.compare_capped_with_oracle(g, R.as_oracle(e['cap'], case.n), case.n)
    assert {k: cap[k] for k in e['stats']} == e['stats']
    return cap


LOOPS = [c for c in C.loop_cases() if not c[0].startswith('holes')]


@pytest.mark.parametrize('engine', parity.ENGINES)
@pytest.mark.parametrize('cid,builder,args', LOOPS, ids=[c[0] for c in LOOPS])
def test_loops(ctx, cid, builder, args, engine):
    """Edges (former, partner, I, U), forward degrees, labels and the fslr_cap_stats counts of: the break
    at list index thr - 1 (lanes 0, 1, 62, 63, lane 0 of chunks 2 and 3), post-break walks behind 0 .. 128
    gate-failing fillers that stop on an edge or on a counted pair or run off the end, empty segments
    around the break and at the end of T, the kLaneL = 16 mix, left-behind pairs, and thresholds 0 and -1
    (replayed like any other: fslr_hip.h)."""
    run_loops(ctx, C.case(builder, *args), engine)


@pytest.mark.parametrize('where', ['end', 'start'])
def test_hole_fill(ctx, where):
    """The sweep's edge list is one run per read, so the replay classifies T's runs in place and fills the
    dropped rows' holes from the list's tail: T's runs at the very end (no survivor behind the new end),
    at the very start, and with more holes than surviving tail rows."""
    case = C.case('hole_fill', where)
    e = case.exp
    load(ctx, case.csr)
    st = query(ctx, case.params, 'sweep')
    a = ctx.edges(st['n_edges'])[0]
    heads = a[np.r_[True, a[1:] != a[:-1]]]
    assert np.unique(heads).size == heads.size                # one run per read
    inT = np.isin(a, e['T'])
    k = int(inT.sum())
    assert (inT[-k:] if where == 'end' else inT[:k]).all() and 0 < k < a.size
    run_loops(ctx, case, 'sweep')


def test_reuse_one_context(ctx):
    """thr = 64, a new query, thr = 1 on one context (the arenas shrink and grow), then
    fslr_apply_edge_cap again without a query: the graph stays and the call reports applied = 0."""
    case = C.case('one_locus', 64)
    load(ctx, case.csr)
    run_loops(ctx, case, 'sweep', loaded=True)
    cap = run_loops(ctx, case, 'sweep', thr=1, loaded=True)
    assert cap['applied'] == 1
    before = [x.copy() for x in edge_list(ctx)] + [ctx.fwd_degree()]
    again = ctx.apply_edge_cap(1)
    assert again['applied'] == 0 and again['max_fwd'] == cap['max_fwd']
    after = list(edge_list(ctx)) + [ctx.fwd_degree()]
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------ D: alternatives
CHILD_CASES = (('one_locus', (64,)), ('walks', (64, 'edge')), ('eval_mix', ()))
SETTINGS = [('FSLR_CAP_SLOTSORT', 'lds'), ('FSLR_CAP_SLOTSORT', 'global'), ('FSLR_CAP_CLOSURE', 'frontier')]


def child_main():
    """One fresh process: the three inputs through both engines (and, for the closure switch, one ladder
    through the context route, which then builds an adjacency and walks k_cap_frontier_w<false>)."""
    ctx = _lib.Context(0)
    for builder, args in CHILD_CASES:
        for engine in parity.ENGINES:
            run_loops(ctx, C.case(builder, *args), engine)
    thr, n, rows = C.closure_shapes()['ladder17']
    T, _ = R.closure(n, rows, np.bincount([a for a, _ in rows], minlength=n), thr)
    load(ctx, C.witness_reads(n))
    query(ctx, R.DEFAULT, 'sweep')
    assert device_closure(ctx, C.ordered(rows, 'shuffled'), thr, 'context')[0] == T
    ctx.close()
    print('cap child ok')


@pytest.mark.parametrize('var,value', SETTINGS, ids=[f'{k}={v}' for k, v in SETTINGS])
def test_environment_alternatives(var, value):
    """FSLR_CAP_SLOTSORT=lds | global and FSLR_CAP_CLOSURE=frontier (the non-default closure) are read once
    per process: each runs in a child of its own, which compares with the reference like the tests above."""
    env = dict(os.environ, **{var: value})
    env['PYTHONPATH'] = os.pathsep.join([HERE, os.path.dirname(HERE), os.path.join(HERE, 'golden'),
                                         env.get('PYTHONPATH', '')])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and 'cap child ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == '__main__':
    torch.cuda.init()
    child_main()
