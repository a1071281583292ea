"""The multigraph fixtures of tests/multi_graphs.py have the properties they are named for, and
tests/multi_ref.py is a reference worth comparing with -- checked without the engine, so that
test_multi_gpu.py cannot pass vacuously on inputs that drifted back to simple graphs:

  * multi_ref's distances and min-key parent edges equal OracleGraph.dijkstra(s, TIE_MINKEY)
    exactly (two independent statements of the header's tie rule);
  * the tie rule's edge id decides numbers: at least 5% of the parents are chosen among two or
    more tight parallel edges of differing reliability, at least 5% are an added (higher-id)
    edge, and the mutant that takes the highest tight edge id changes rel in every source row;
  * the reference's igraph_get_eid replay (OracleGraph.source_row) yields other latencies than
    the distance: hazard H3, and the reason oracle_rows is not the reference here.
"""
import dataclasses

import numpy as np
import pytest

from tests import multi_graphs as mg
from tests.multi_ref import Ref

_REF = {}


def ref_of(name, tie="low"):
    if (name, tie) not in _REF:
        _REF[name, tie] = Ref(mg.get(name), tie)
    return _REF[name, tie]


@pytest.mark.parametrize("name", list(mg.SUITE))
def test_ref_equals_the_oracle_min_key_tree(oracle_mod, name):
    g = mg.get(name)
    og = oracle_mod.OracleGraph(g)
    ref = ref_of(name)
    for s in mg.sources(name):
        d, pe, _, _ = ref.dijkstra(int(s))
        od, op = og.dijkstra(int(s), oracle_mod.TIE_MINKEY)
        assert np.array_equal(d, od) and np.array_equal(pe, op), (name, s)
    assert ref.complete == og.is_complete()


@pytest.mark.parametrize("name", mg.PARALLEL)
def test_parallel_edges_decide_parents(name):
    g, ref = mg.get(name), ref_of(name)
    S = mg.sources(name)
    first = mg.added_from(name)
    total = par = added = 0
    for s in S:
        _, pe, _, p = ref.dijkstra(int(s))
        total += int((pe >= 0).sum()); par += int(p.sum()); added += int((pe >= first).sum())
    print(name, "parents", total, "among tight parallel edges of differing reliability", par, "added edges", added)
    assert total == len(S) * (g.n - 1)
    assert par >= 0.05 * total and added >= 0.05 * total


def test_frac_has_near_misses():
    """multi389_frac: a vertex with a parallel arc that is not tight, within 0.01 ms of a tight
    one from the same neighbour (two candidates in a key interval, one tight arc)."""
    g, ref = mg.get("multi389_frac"), ref_of("multi389_frac")
    assert np.all(np.rint(g.latency * 100.0) / 100.0 == g.latency) and np.any(np.rint(g.latency * 100.0) % 10 != 0)
    assert np.rint(g.latency * 100.0).max() <= 65535
    near = equal = 0
    for s in (0, 7, 200, 388):
        d, pe, pu, _ = ref.dijkstra(s)
        cand = d[ref.U] + ref.W
        tight = (cand == d[ref.V]) & (ref.V != s)
        key = ref.V * g.n + ref.U
        tk = set(key[tight].tolist())
        miss = ~tight & (ref.V != s) & (cand - d[ref.V] <= 0.0100001) & (cand > d[ref.V])
        near += sum(1 for k in key[miss].tolist() if k in tk)
        uk, c = np.unique(key[tight], return_counts=True)
        equal += int((c >= 2).sum())
    assert near > 0 and equal > 0, (near, equal)


@pytest.mark.parametrize("name", mg.PARALLEL)
def test_highest_edge_id_mutant_changes_rel(name):
    g = mg.get(name)
    ref, mut = ref_of(name), ref_of(name, "high")
    T = np.arange(g.n)
    rows = 0
    for s in mg.sources(name):
        lat, rel, hops = ref.row(int(s))
        ml, mr, mh = mut.row(int(s))
        assert np.array_equal(lat, ml, equal_nan=True) and np.array_equal(hops, mh)
        changed = int((rel[T != s] != mr[T != s]).sum())
        rows += changed > 0
        assert changed > 0, (name, s)
    assert rows > 0


@pytest.mark.parametrize("name", mg.PARALLEL)
def test_get_eid_replay_is_not_the_distance(oracle_mod, name):
    """OracleGraph.source_row walks the same vertex paths but asks get_eid for each hop's edge."""
    g, ref = mg.get(name), ref_of(name)
    og = oracle_mod.OracleGraph(g)
    wrong = total = 0
    for s in mg.sources(name)[:8]:
        T = np.array([t for t in range(g.n) if t != s], np.int32)
        lat = ref.row(int(s))[0][T]
        ol = og.source_row(int(s), T, oracle_mod.TIE_MINKEY)[0]
        assert np.all(ol >= lat)
        wrong += int((ol != lat).sum()); total += len(T)
    print(name, "entries where the get_eid replay is not the distance:", wrong, "of", total)
    assert wrong > 0


def nrel(g):
    nl = g.src != g.dst
    return len(np.unique(1.0 - g.packetloss[nl]))


def test_named_properties():
    for name in ("multi389", "multi389_dir", "multi389_frac", "multi389_vloss", "multi8000"):
        assert nrel(mg.get(name)) <= 254, name
    assert nrel(mg.get("multi389_manyrel")) > 254
    for name in mg.SUITE:                     # strongly connected: every distance is finite
        d = ref_of(name).dijkstra(0)[0]
        assert np.isfinite(d).all(), name
        if mg.get(name).directed:
            g = mg.get(name)
            rev = Ref(dataclasses.replace(g, src=g.dst, dst=g.src))
            assert np.isfinite(rev.dijkstra(0)[0]).all(), name
    for name in ("multi389", "multi389_frac", "multi389_manyrel", "multi389_vloss", "multi8000"):
        g = mg.get(name)
        assert not g.directed and np.all(g.latency == np.floor(g.latency)) == (name != "multi389_frac")
    assert mg.get("multi389_dir").directed
    vl = mg.get("multi389_vloss").vertex_packetloss
    assert 0 < np.isnan(vl).sum() < len(vl) and np.nanmax(vl) > 0
    assert all(mg.get(n).vertex_packetloss is None for n in ("multi389", "multi389_dir", "multi389_frac"))


def test_self_loops():
    """A third of the vertices have no self-loop, a share has two, and the lower id is not always
    the cheaper one."""
    for name in ("multi389", "multi389_dir", "loops_only", "count_complete"):
        g = mg.get(name)
        lp = np.flatnonzero(g.src == g.dst)
        cnt = np.bincount(g.src[lp], minlength=g.n)
        assert (cnt == 0).any() and (cnt == 1).any() and (cnt == 2).any(), name
        cheaper = dearer = 0
        for v in np.flatnonzero(cnt == 2):
            a, b = lp[g.src[lp] == v]
            assert g.packetloss[a] != g.packetloss[b]
            cheaper += g.latency[b] < g.latency[a]; dearer += g.latency[b] >= g.latency[a]
        assert cheaper > 0 and dearer > 0, name


def test_loops_only_is_simple_but_for_its_loops():
    g = mg.get("loops_only")
    nl = g.src != g.dst
    pairs = {(min(a, b), max(a, b)) for a, b in zip(g.src[nl].tolist(), g.dst[nl].tolist())}
    assert len(pairs) == int(nl.sum())
    s = mg.without_second_loops(g)
    assert s.m < g.m and np.bincount(s.src[s.src == s.dst], minlength=s.n).max() == 1
    assert np.array_equal(s.src[s.src != s.dst], g.src[nl])


def test_multi_k24_pairs():
    """Added edges that are lighter than their twin, and equal ones with another loss."""
    g = mg.get("multi_k24")
    first = mg.added_from("multi_k24")
    ref = ref_of("multi_k24")
    lighter = equal = 0
    for e in range(first, g.m):
        e0 = ref.first[int(g.src[e]), int(g.dst[e])]
        assert e0 < first
        lighter += g.latency[e] < g.latency[e0]
        equal += g.latency[e] == g.latency[e0] and g.packetloss[e] != g.packetloss[e0]
    assert lighter > 10 and equal > 10
    assert ref.complete


def test_count_complete(oracle_mod):
    g, ref = mg.get("count_complete"), ref_of("count_complete")
    assert ref.complete and oracle_mod.OracleGraph(g).is_complete()
    missing = [(a, b) for a in range(g.n) for b in range(g.n) if a != b and (a, b) not in ref.first]
    assert len(missing) == g.n * 5
    deg = np.bincount(np.concatenate([g.src, g.dst]), minlength=g.n)
    assert deg.min() >= g.n
