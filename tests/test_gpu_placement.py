"""The placement scratch that the read paths, the junction support, the transits and an EDGES step share on one context (csrc/placement.hip): what one call sized
or filled, the next call must not trust.  The stages themselves are checked in test_gpu_read_paths.py, test_gpu_junctions.py and test_gpu_transits.py."""
import numpy as np
import pytest

import sketch_graphs as G
import test_gpu_junctions as JX
import test_gpu_transits as TX
from test_gpu_parity import _mdbg
from test_gpu_read_paths import check_paths, distinct_hashes, feed_batches
from test_gpu_sketch_graphs import BY_NAME, feed
from test_read_paths_cpu import hashes

pytestmark = pytest.mark.gpu

EDGES = 8


def assert_same(a, b, where=""):
    """two results of the Python API, column by column"""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for f in a:
            assert_same(a[f], b[f], where + "/" + f)
    else:
        assert np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype, where


def test_interleaved_stages_over_ranges_of_different_sizes():
    """seed 6 has explained and missing crossings, and an EDGES step removes records of it.  Every call of the sequence gives what it gives as the FIRST call on a
    context of its own: small ranges in front of large ones, stages with records round one without, a list with fewer records in between"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(6)
    cut = len(reads) // 3

    def fresh():
        m = R.Mdbg(k, G.L, G.D, A)
        feed_batches(m, [(reads[:cut], 0), (reads[cut:], cut)])
        m.finalize()
        m.graph_edges(presimp)
        return m, m.graph_unitigs()

    calls = [("transits [1, 3)", lambda m: m.graph_transits(1, 2, 1)),
             ("read paths", lambda m: m.graph_read_paths()),
             ("junctions [1, 3)", lambda m: m.graph_junctions(1, 2)),
             ("simplify EDGES", lambda m: m.graph_simplify([(EDGES, 1, 0)])),
             ("unitigs", lambda m: m.graph_unitigs()),
             ("transits", lambda m: m.graph_transits(0, 0, 1)),
             ("junctions", lambda m: m.graph_junctions())]
    m, plain = fresh()
    with m:
        got = [call(m) for _, call in calls]
    assert got[0]["n_reads"] == got[2]["n_reads"] == 2 and got[1]["n_reads"] == len(reads) and got[3]["stats"]["edges_removed"][0] > 0
    assert got[6]["n_records"] == len(plain["edges"]["n1"]) > len(got[3]["edges"]["n1"]) and got[6]["n_explained"] > 0 and got[6]["n_missing"] > 0
    for (name, call), g in zip(calls, got):
        m, ul = fresh()
        with m:
            assert_same(g, ul if name == "unitigs" else call(m), name)


def test_a_list_without_records_after_a_list_with_records():
    """the fork (15 rows, 88 minimizer indices, 3 unitigs, 4 records), then on the same context one linear path seen twice (6 rows, 16 indices, 1 unitig, no
    record): nothing of the larger graph's sorted keys or maps is read"""
    R = _mdbg()
    c = BY_NAME["fork"]
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        feed(m, c.reads, c.split)
        nodes = m.finalize()
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        assert len(ul["edges"]["n1"]) == 4 and len(nodes["index"]) == 15
        check_paths(R, m, c.reads, c.k, nodes, ul)
        jx, _ = JX.check(R, m, c.reads, c.k, nodes, ul)
        tx, _ = TX.check(R, m, hashes(c.reads), c.k, nodes, ul)
        assert jx["n_records"] == 4 and jx["n_explained"] > 0 and tx["n_explained"] > 0
        m.reset(0)
        reads = [G.mread(distinct_hashes(31, 8))] * 2
        feed(m, reads)
        nodes = m.finalize()
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        assert (ul["n_unitigs"], len(ul["edges"]["n1"]), len(nodes["index"])) == (1, 0, 6)
        rp, _ = check_paths(R, m, reads, c.k, nodes, ul)
        jx, _ = JX.check(R, m, reads, c.k, nodes, ul)
        tx, _ = TX.check(R, m, hashes(reads), c.k, nodes, ul)
        assert rp["n_steps"] == 2 and rp["n_placed"] == 12
        assert (jx["n_records"], jx["n_explained"], jx["n_crossings"], jx["n_missing"], jx["n_links"]) == (0, 0, 0, 0, 10)
        assert (tx["n_explained"], tx["n_crossings"], tx["n_transits"], tx["n_passes"], tx["n_repeats"]) == (0, 0, 0, 0, 0)
