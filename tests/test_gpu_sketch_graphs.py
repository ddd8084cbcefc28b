"""The graph stages on hand-built minimizer-space graphs (tests/sketch_graphs.py): every case goes in through Mdbg.ingest_sketch as per-read hashes and positions,
and the node table, the edges, the unitigs, every schedule of tips, bubbles and small components, and the components must equal the plain model, the two edge
references and the restatements exactly.  The CPU side (the model's pin, the recorded figures, what each case is there for) is tests/test_sketch_graphs_cpu.py."""
import numpy as np
import pytest

import components_restatement as CR
import sketch_graphs as G
import unitig_restatement as U
from oracle import oracle as O
from test_gpu_components import assert_simplify_equals_restatement, check_components
from test_gpu_edges import as_rows
from test_gpu_parity import _mdbg, assert_nodes_equal
from test_gpu_simplify import assert_equals_restatement as assert_simplify_without_components, same_list
from test_gpu_unitigs import assert_equals_restatement as assert_unitigs_equal_restatement

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in G.CASES}


def feed(m, reads, split=None):
    """the reads as one ingest_sketch batch, or as two with consecutive first ordinals; then the insertion of everything resident"""
    import torch
    dev = torch.device("cuda", 0)
    cuts = [0, len(reads)] if split is None else [0, split, len(reads)]
    keep = []
    for a, b in zip(cuts, cuts[1:]):
        h, p, o = G.sketch_arrays(reads[a:b])
        # (torch has no uint64 / uint32 arithmetic: the bits travel as int64 / int32)
        t = [torch.from_numpy(h.view(np.int64)).to(dev), torch.from_numpy(p.view(np.int32)).to(dev), torch.from_numpy(o.view(np.int64)).to(dev)]
        torch.cuda.synchronize()
        m.ingest_sketch(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), b - a, a)
        keep.append(t)
    m.insert_resident()
    return keep


def check_nodes(got, exp):
    assert_nodes_equal(got, exp)
    for f in ("src_read", "src_start", "src_end", "reversed"):
        assert np.array_equal(got[f], exp[f]), f


def check_edges(m, nodes, presimp):
    """the shape of tests/test_gpu_edges.py: the host emitter row for row, the oracle's emitter as a sorted multiset, twice"""
    from rust_mdbg_amd import emit as E
    got = m.graph_edges(presimp)
    again = m.graph_edges(presimp)
    host = E.Emitter().edges(nodes, presimp)
    assert as_rows(got) == as_rows(host) == as_rows(again)
    assert got["presimp_removed"] == host["presimp_removed"] == again["presimp_removed"]
    rows, removed = O.edges_from_nodes(nodes, presimp)
    assert sorted(as_rows(got)) == rows and got["presimp_removed"] == removed
    return got


def check_unitigs(R, m, nodes, edges, reads):
    got = m.graph_unitigs()
    same_list(got, m.graph_unitigs(), R)
    return got, assert_unitigs_equal_restatement(got, nodes, edges, reads)


@pytest.mark.parametrize("name", G.CASE_IDS)
def test_gpu_stages_on_hand_built_graphs(name):
    R = _mdbg()
    c = BY_NAME[name]
    exp_nodes = G.nodes_from_sketch(c.reads, c.k, G.L, c.A)
    reads = G.fake_bases(c.reads, G.L, 1) if c.strings else None
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        feed(m, c.reads, c.split)
        nodes = m.finalize()
        check_nodes(nodes, exp_nodes)
        assert nodes["n_nodes"] == c.expect["nodes"]
        for p in reversed(c.presimps):                                            # presimps[0] last: the schedules run on its edges
            edges = check_edges(m, nodes, p)
            if p in c.expect.get("edges", {}):
                assert (len(edges["n1"]), edges["presimp_removed"]) == c.expect["edges"][p]
            got, cur = check_unitigs(R, m, nodes, edges, reads)
            if reads is None:                                                     # no strings: walks, orientations, circular, kc_sum and the edges' ends only
                continue
            check_components(R, m, cur)
        if reads is None:
            return
        if "unitigs" in c.expect:
            assert list(zip(np.diff(got["offsets"].astype(np.int64)).tolist(), got["length"].tolist())) == c.expect["unitigs"]
        for steps in c.schedules:
            simp = m.graph_simplify(steps)
            again = m.graph_simplify(steps)
            assert simp["stats"] == again["stats"]
            same_list(simp, again, R)
            if all(kind != CR.COMPONENTS for kind, _, _ in steps):
                log, left = assert_simplify_without_components(simp, nodes, edges, reads, steps)
            else:
                log, left = assert_simplify_equals_restatement(simp, nodes, edges, reads, steps)
            assert simp["stats"]["nodes_removed"] == [len(st["nodes"]) for st in log] and simp["stats"]["unitigs_removed"] == [len(st["unitigs"]) for st in log]
            if tuple(steps) in c.expect.get("removed", {}):
                assert [sorted(st["nodes"]) for st in log] == c.expect["removed"][tuple(steps)]
                assert sorted(simp["node"].tolist()) == sorted(set(nodes["index"].tolist()) - {n for st in c.expect["removed"][tuple(steps)] for n in st})
            check_components(R, m, left)                                          # the simplified list is the current one
        same_list(m.graph_unitigs(), got, R)                                      # and the plain list is what it was


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_gpu_stages_on_random_minimizer_space_graphs(seed):
    """dense repeats, palindromes and hubs: nodes, edges and unitigs (tests/test_sketch_graphs_cpu.py shows that the restatement accepts every seed)"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    exp_nodes = G.nodes_from_sketch(reads, k, G.L, A)
    strings = G.fake_bases(reads, G.L, seed)
    with R.Mdbg(k, G.L, G.D, A) as m:
        feed(m, reads, len(reads) // 3)
        nodes = m.finalize()
        check_nodes(nodes, exp_nodes)
        edges = check_edges(m, nodes, presimp)
        check_unitigs(R, m, nodes, edges, strings)
