"""The junction restatement (tests/junctions_restatement.py) pinned without a GPU: hand-written supports, the recorded figures of the catalogue of
tests/sketch_graphs.py, the invariants of include/mdbg_hip.h (mdbg_graph_junctions) and the identity against the read paths on every case, a simplified list,
the text of the .junctions.tsv, and the Python mirror of mdbg_junction_list.  The GPU side is tests/test_gpu_junctions.py."""
import functools
import os

import numpy as np
import pytest

import junctions_restatement as J
import read_paths_restatement as RP
import simplify_restatement as S
import sketch_graphs as G
import unitig_restatement as U
from conftest import ROOT
from test_read_paths_cpu import hashes
from test_sketch_graphs_cpu import BY_NAME, case_strings, host_edges, model_nodes, random_graph


def on_list(nodes, reads, k, walks, circular, edges):
    """-> (junctions, read paths) of one list; the junction invariants and the identity against the read paths are asserted on the way"""
    keys, index = nodes["keys"].tolist(), nodes["index"].tolist()
    j = J.junctions(hashes(reads), k, keys, index, walks, [e[:4] for e in edges])
    r = RP.read_paths(hashes(reads), k, keys, index, walks, circular)
    assert j["n_explained"] + j["n_missing_crossings"] == j["n_crossings"] and j["n_links"] + j["n_crossings"] == j["n_adjacent"]
    assert j["n_missing_crossings"] == sum(j["missing"].values()) and j["n_missing"] == len(j["missing"]) and j["n_records"] == len(edges) == len(j["support"])
    by_key = {}
    for key, sup in zip(j["keys"], j["support"]):                                       # records with equal keys carry equal counts
        assert by_key.setdefault(key, sup) == sup
    assert sum(by_key.values()) == j["n_explained"]
    wraps = 0                                                                           # ring wraps inside steps, from the step records alone
    for st in r["steps"]:
        for _, n, u, j0, s in st:
            if circular[u]:
                m = len(walks[u])
                wraps += (j0 + n - 1) // m if s == 0 else (m - 1 - j0 + n - 1) // m
    assert j["n_adjacent"] - j["n_crossings"] + wraps == r["n_placed"] - r["n_steps"]
    return j, r


@functools.lru_cache(maxsize=None)
def plain(name, presimp=0.0):
    c, nodes = BY_NAME[name], model_nodes(name)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    return u, on_list(nodes, c.reads, c.k, u["walks"], u["circular"], u["edges"])[0]


def by_record(u, j):
    return {e[:4]: s for e, s in zip(u["edges"], j["support"])}


# ---- hand-written, from the definition --------------------------------------------------------------------------------------------------------------------
def test_fork_two_junction_keys():
    """the trunk's first unitig (4 entries) ends where the long read (5 times) goes on into the trunk and the short read (2 times) into the arm"""
    u, j = plain("fork")
    assert by_record(u, j) == {(0, "+", 1, "+"): 5, (1, "-", 0, "-"): 5, (0, "+", 2, "+"): 2, (2, "-", 0, "-"): 2}
    assert sorted(set(j["keys"])) == [((0, 3, 0), (1, 0, 0)), ((0, 3, 0), (2, 0, 0))]
    assert (j["n_adjacent"], j["n_links"], j["n_crossings"], j["n_explained"], j["n_missing"]) == (67, 60, 7, 7, 0) and j["missing"] == {}


def test_bubble_the_other_strand_read_exercises_the_mirror_rule():
    """read `two` walks u2 backwards from its last entry, its own branch u3 forwards, then u0 backwards: its crossings (u2, 0, 1) -> (u3, 0, 0) and
    (u3, 3, 0) -> (u0, 3, 1); the second is the larger of itself and its mirror (u0, 3, 0) -> (u3, 3, 1), so it is counted under the mirror"""
    u, j = plain("bubble 7/3")
    sup = by_record(u, j)
    assert sup[(0, "+", 1, "+")] == sup[(1, "-", 0, "-")] == sup[(1, "+", 2, "+")] == sup[(2, "-", 1, "-")] == 7
    assert sup[(2, "-", 3, "+")] == sup[(3, "-", 2, "+")] == sup[(3, "+", 0, "-")] == sup[(0, "+", 3, "-")] == 3 and len(sup) == 8
    assert J.key_of(((3, 3, 0), (0, 3, 1))) == ((0, 3, 0), (3, 3, 1)) and J.key_of(((2, 0, 1), (3, 0, 0))) == ((2, 0, 1), (3, 0, 0)) == J.key_of(((3, 0, 1), (2, 0, 0)))
    assert (j["n_links"], j["n_crossings"], j["n_missing"]) == (90, 20, 0)


def test_islands_the_closing_record_of_the_ring_gets_its_wraps():
    """the two ring reads go once round and one window more, against the walk: one wrap 0 -> 5 each, which is the key of the closing record and of its mirror"""
    u, j = plain("islands")
    assert u["circular"] == [False, False, False, True] and by_record(u, j) == {(3, "+", 3, "+"): 2, (3, "-", 3, "-"): 2}
    assert set(j["keys"]) == {((3, 0, 1), (3, 5, 1))} and (j["n_links"], j["n_crossings"], j["n_missing"]) == (29, 2, 0)


def test_mirror_is_an_involution_and_a_link_is_never_a_record_key():
    pair = ((4, 2, 0), (1, 7, 1))
    assert J.mirror(J.mirror(pair)) == pair and J.key_of(pair) == J.key_of(J.mirror(pair)) == ((1, 7, 0), (4, 2, 1))
    assert J.is_link((0, 1, 0), (0, 2, 0)) and J.is_link((0, 2, 1), (0, 1, 1)) and not J.is_link((0, 5, 0), (0, 0, 0)) and not J.is_link((0, 1, 0), (0, 2, 1))
    assert not J.is_link((0, 1, 0), (1, 2, 0))


# ---- recorded figures ---------------------------------------------------------------------------------------------------------------------------------------
def figures(j):
    return (j["n_records"], len(set(j["keys"])), sum(1 for s in j["support"] if s == 0), j["n_links"], j["n_crossings"], j["n_missing"])


def test_recorded_figures_of_the_catalogue():
    assert figures(plain("islands")[1])[:2] + figures(plain("islands")[1])[3:] == (2, 1, 29, 2, 0) and plain("islands")[1]["support"] == [2, 2]
    assert figures(plain("hub")[1]) == (3200, 1600, 3120, 160, 40, 0)
    assert figures(plain("odd k=3 5-5-5-5-5-5")[1]) == (16, 3, 8, 0, 6, 0)
    j = plain("presimp 200/1 at 0.01")[1]
    assert (j["n_records"], j["n_links"], j["n_crossings"], j["n_missing"]) == (4, 804, 201, 0)
    j = plain("presimp 200/1 at 0.01", 0.01)[1]                                         # the one read that took the removed branch leaves the trunk at an interior entry
    assert (j["n_records"], j["n_links"], j["n_crossings"]) == (0, 1004, 1) and j["missing"] == {((0, 2, 0), (1, 0, 0)): 1}
    assert plain("presimp 5/2 at 0.5", 0.5)[1]["missing"] == {((0, 2, 0), (1, 0, 0)): 2}


# seed -> (records, distinct keys, records with support 0, links, crossings, missing keys, missing crossings); None = not pinned
RANDOM = {0: (7778, 3653, 7084, 0, 3302, 0, 0), 6: (5392, 2512, 4830, None, 3612, 64, 570)}


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_graphs(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    j, _ = on_list(nodes, reads, k, u["walks"], u["circular"], u["edges"])
    if presimp == 0.0:
        assert j["n_missing"] == 0
    if seed in RANDOM:
        got = figures(j) + (j["n_missing_crossings"],)
        assert all(w is None or g == w for g, w in zip(got, RANDOM[seed])), got


# ---- the catalogue --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_catalogue_invariants(name):
    c, nodes = BY_NAME[name], model_nodes(name)
    for p in c.presimps:
        u = U.unitigs(nodes, host_edges(nodes, p))
        j, _ = on_list(nodes, c.reads, c.k, u["walks"], u["circular"], u["edges"])     # the invariants and the identity are asserted inside
        if p == 0.0:
            assert j["n_missing"] == 0, p                                               # consecutive windows share a (k-1)-mer: their arc exists
        assert j["missing_rows"] == sorted(j["missing_rows"])


def test_fork_after_clipping_the_arm():
    """[(TIPS, 3, 0)] leaves the trunk as ONE unitig of 12 nodes without edge records: the long read is all links; the short read's windows on the arm are
    unplaced, so it leaves no crossing either"""
    c, nodes = BY_NAME["fork"], model_nodes("fork")
    log, left = S.simplify(nodes, host_edges(nodes, 0.0), [(G.TIPS, 3, 0)], case_strings("fork"), None)
    assert [len(w) for w in left["walks"]] == [12]
    j, r = on_list(nodes, c.reads, c.k, left["walks"], left["circular"], left["edges"])
    assert (j["n_records"], j["n_adjacent"], j["n_links"], j["n_crossings"], j["n_missing"]) == (len(left["edges"]), 61, 61, 0, 0)


# ---- the text -------------------------------------------------------------------------------------------------------------------------------------------------
FORK_TSV = ("L\tutg0000001l\t+\tutg0000002l\t+\t102M\t5\n" "L\tutg0000001l\t+\tutg0000003l\t+\t102M\t2\n" "L\tutg0000002l\t-\tutg0000001l\t-\t102M\t5\n"
            "L\tutg0000003l\t-\tutg0000001l\t-\t102M\t2\n")


def as_library_result(u, j):
    """a restatement result in the shape of Mdbg.graph_unitigs()["edges"] and Mdbg.graph_junctions()"""
    from rust_mdbg_amd import api
    col = lambda i, t, f=int: np.array([f(e[i]) for e in u["edges"]], dtype=t)
    edges = dict(n1=col(0, np.uint32), o1=col(1, np.uint8, ord), n2=col(2, np.uint32), o2=col(3, np.uint8, ord), overlap=col(4, np.uint32))
    missing = {f: np.array([row[i] for row in j["missing_rows"]], dtype=t) for i, (f, t, _) in enumerate(api.JUNCTION_FIELDS[1:])}
    return edges, np.array(j["support"], np.uint64), missing


def test_tsv_text_character_for_character():
    from rust_mdbg_amd import api
    u, j = plain("fork")
    assert J.tsv_text(u["edges"], j, u["circular"]) == FORK_TSV
    edges, support, missing = as_library_result(u, j)
    assert api.junction_text(edges, support, missing, np.array(u["circular"], np.uint8)) == FORK_TSV
    u, j = plain("presimp 200/1 at 0.01", 0.01)
    text = J.tsv_text(u["edges"], j, u["circular"])
    assert text == "X\tutg0000001l\t+\t2\tutg0000002l\t+\t0\t1\n"
    assert api.junction_text(*as_library_result(u, j), u["circular"]) == text
    u, j = plain("islands")
    assert J.tsv_text(u["edges"], j, u["circular"]).split("\n")[0] == "L\tutg0000004c\t-\tutg0000004c\t-\t102M\t2"


def test_merge_of_ranges_is_the_whole_call():
    """api.merge_junctions on the restatement's results of three ranges of reads of random seed 6 (which has missing keys): what run_file does with the chunks"""
    from rust_mdbg_amd import api
    k, A, presimp, reads, nodes = random_graph(6)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    run = lambda rd: J.junctions(hashes(rd), k, nodes["keys"].tolist(), nodes["index"].tolist(), u["walks"], [e[:4] for e in u["edges"]])

    def shaped(j, first, n):
        _, support, missing = as_library_result(u, j)
        return dict(missing, support=support, first_read=first, n_reads=n, n_records=j["n_records"], n_missing=j["n_missing"],
                    **{f: j[f] for f in api.JUNCTION_COUNTS if f != "n_reads"})
    whole = shaped(run(reads), 0, len(reads))
    parts = [shaped(run(reads[a:b]), a, b - a) for a, b in ((0, 1), (1, 50), (50, len(reads)))]
    merged = api.merge_junctions(parts)
    assert sorted(merged) == sorted(whole)
    for f in whole:
        assert np.array_equal(merged[f], whole[f]) and np.asarray(merged[f]).dtype == np.asarray(whole[f]).dtype, f
    assert whole["n_missing"] == 64 and whole["n_missing_crossings"] == 570


# ---- the columns of the result (its layout and prototypes: tests/test_abi_exports.py) -------------------------------------------------------------------------------
def test_the_column_table_follows_the_result_struct():
    from rust_mdbg_amd import api
    fields = [f for f, _ in api.JunctionList._fields_]
    assert fields == ["first_read", "n_reads", "n_adjacent", "n_links", "n_crossings", "n_explained", "n_missing_crossings", "n_records", "n_missing", "support",
                      "missing_unitig1", "missing_entry1", "missing_strand1", "missing_unitig2", "missing_entry2", "missing_strand2", "missing_count"]
    assert [f for f, _, _ in api.JUNCTION_FIELDS] == fields[9:]
    L = api.load_library()
    for f in ("mdbg_graph_junctions", "mdbg_graph_junctions_device", "mdbg_junctions_ms"):
        assert hasattr(L, f) and f in api.EXPORTS
