"""The edge-pruning restatement (tests/edge_prune_restatement.py: the EDGES step of include/mdbg_hip.h, mdbg_graph_simplify) pinned without a GPU: three
hand-written cases round one repeat of k - 1 minimizers, the recorded figures of the catalogue of tests/sketch_graphs.py and of its random graphs, the
observation that a second step with the same threshold finds nothing, and the C side of the new step kind.  The GPU side is tests/test_gpu_edge_prune.py."""
import functools
import os
import subprocess

import pytest

import edge_prune_restatement as EP
import sketch_graphs as G
import unitig_restatement as U
from conftest import ROOT
from test_read_paths_cpu import hashes
from test_sketch_graphs_cpu import BY_NAME, case_strings, host_edges, model_nodes, random_graph

EDGES = EP.EDGES


# ---- one repeat of k - 1 = 2 minimizers shared by two contexts (k = 3, A = 2) ---------------------------------------------------------------------------------
def hand_reads():
    h = G.fresh(7, 40)
    a, b, rep = h[:6], h[6:12], h[12:14]
    r1, r2, r3 = G.mread(a[:3] + rep + a[3:]), G.mread(b[:3] + rep + b[3:]), G.mread(a[:3] + rep + b[3:])
    return {"repeat": [r1] * 3 + [r2] * 3, "repeat + span": [r1] * 3 + [r2] * 3 + [r3] * 2, "one exit only": [r1] * 3 + [G.mread(b[:3] + rep)] * 3}


HAND_K, HAND_A = 3, 2
# (case, min_support) -> (weak unitig edge records, records removed, entries of the unitigs that are left)
HAND = {("repeat", 1): (4, 4, [6, 6]), ("repeat", 3): (4, 4, [6, 6]), ("repeat", 4): (8, 0, [3, 3, 3, 3]),
        ("repeat + span", 1): (2, 2, [3, 3, 3, 3]), ("repeat + span", 3): (4, 4, [6, 6]), ("repeat + span", 4): (8, 0, [3, 3, 3, 3]),
        ("one exit only", 1): (2, 0, [3, 3, 3])}


@functools.lru_cache(maxsize=None)
def hand_graph(name):
    reads = hand_reads()[name]
    nodes = G.nodes_from_sketch(reads, HAND_K, G.L, HAND_A)
    return reads, nodes, host_edges(nodes, 0.0), G.fake_bases(reads, G.L, 1)


def run(nodes, edges, steps, reads, k, strings, length_of=None):
    return EP.simplify(nodes, edges, steps, hashes(reads), k, strings, length_of)


@pytest.mark.parametrize("name,T", sorted(HAND))
def test_hand_cases(name, T):
    reads, nodes, edges, strings = hand_graph(name)
    weak, removed, left = HAND[(name, T)]
    log, final = run(nodes, edges, [(EDGES, T, 0), (EDGES, T, 0)], reads, HAND_K, strings)
    assert (log[0]["weak"], log[0]["edges"], [len(w) for w in final["walks"]]) == (weak, removed, left)
    assert log[0]["nodes"] == set() and log[0]["unitigs"] == [] and log[1]["edges"] == 0
    assert sum(len(w) for w in final["walks"]) == nodes["n_nodes"]                      # the step removes no node


def test_the_repeat_in_detail():
    """12 nodes, 24 records, four unitigs of three entries that meet in a full 2 x 2 cross; the reads take the two straight ways only"""
    reads, nodes, edges, strings = hand_graph("repeat")
    plain = U.unitigs(nodes, edges, strings)
    assert (nodes["n_nodes"], len(edges["n1"]), [len(w) for w in plain["walks"]], len(plain["edges"])) == (12, 24, [3, 3, 3, 3], 8)
    log, final = run(nodes, edges, [(EDGES, 1, 0)], reads, HAND_K, strings)
    assert log[0]["support"] == [3, 0, 3, 0, 0, 3, 0, 3]
    assert final["edges"] == [] and len(final["seqs"]) == 2
    gone = [e[:4] for e, s in zip(plain["edges"], log[0]["support"]) if s == 0]
    mirror = lambda e: (e[2], U.flip(e[3]), e[0], U.flip(e[1]))
    assert sorted(gone) == sorted(mirror(e) for e in gone)                                # a record and its mirror record fall together
    # the spanning reads make one of the two crossed ways a supported one: its records stay at min_support 1 and 2, and go at 3 with the rest
    reads, nodes, edges, strings = hand_graph("repeat + span")
    log, final = run(nodes, edges, [(EDGES, 1, 0)], reads, HAND_K, strings)
    assert log[0]["support"] == [3, 2, 3, 0, 0, 3, 2, 3] and len(final["edges"]) == 6


def test_a_weak_edge_that_is_the_only_way_out_stays():
    """the second context ends inside the repeat: its unitig has no way on but the two unsupported records, so the dead-end side has no strong exit"""
    reads, nodes, edges, strings = hand_graph("one exit only")
    plain = U.unitigs(nodes, edges, strings)
    log, final = run(nodes, edges, [(EDGES, 1, 0)], reads, HAND_K, strings)
    assert log[0]["support"] == [3, 3, 0, 0] and log[0]["edges"] == 0 and final["edges"] == plain["edges"] and final["walks"] == plain["walks"]


def test_no_resident_read_means_nothing_is_strong():
    reads, nodes, edges, strings = hand_graph("repeat")
    log, final = EP.simplify(nodes, edges, [(EDGES, 1, 0)], [], HAND_K, strings)
    assert log[0]["weak"] == 8 and log[0]["edges"] == 0 and len(final["edges"]) == 8


def test_the_checker_refuses_what_the_library_refuses():
    reads, nodes, edges, strings = hand_graph("repeat")
    for bad in ([(EDGES, 0, 0)], [(EDGES, 1, 1)], [(4, 1, 0)]):
        with pytest.raises(AssertionError):
            run(nodes, edges, bad, reads, HAND_K, strings)


# ---- the catalogue at min_support 1: figures of the committed checker ----------------------------------------------------------------------------------------
CATALOGUE_REMOVED = {"odd k=3 5-5-5-5-5-5": 8, "odd k=3 1-2-1-2-1-2-1-3": 16, "odd k=2 1-2-1-3-1-4-1-1": 40, "hub": 3120}      # every other case: 0


@pytest.mark.parametrize("name", G.CASE_IDS)
def test_catalogue_at_min_support_one(name):
    c, nodes, strings = BY_NAME[name], model_nodes(name), case_strings(name)
    edges = host_edges(nodes, c.presimps[0])
    length_of = None if strings is not None else G.length_of_walk(nodes)
    log, final = run(nodes, edges, [(EDGES, 1, 0), (EDGES, 1, 0)], c.reads, c.k, strings, length_of)
    assert log[0]["edges"] == CATALOGUE_REMOVED.get(name, 0)
    assert log[1]["edges"] == 0                                                          # observed on these inputs, not a law
    if name == "hub":
        assert len(U.unitigs(nodes, edges)["walks"]) == 80 and len(final["walks"]) == 40
    if log[0]["edges"] == 0:
        assert final["walks"] == U.unitigs(nodes, edges)["walks"]


# ---- the random graphs: seed -> per min_support 1, 2, 3 (weak records, records removed, unitigs left); records and unitigs of the plain list ---------------------
RANDOM = {0: ((7778, 246), [(7084, 7054, 110), (7094, 6774, 132), (7098, 6670, 143)]),
          1: ((518, 96), [(242, 238, 19), (242, 238, 19), (242, 238, 19)]),
          2: ((60, 11), [(40, 40, 1), (40, 40, 1), (40, 40, 1)]),
          3: ((7530, 243), [(6856, 6856, 121), (6872, 6818, 123), (6884, 6514, 136)]),
          4: ((558, 101), [(208, 208, 30), (228, 228, 27), (244, 198, 28)]),
          5: ((34, 7), [(22, 20, 1), (22, 20, 1), (22, 20, 1)]),
          6: ((5392, 250), [(4830, 4028, 165), (4842, 4016, 168), (4852, 4026, 166)]),
          7: ((508, 101), [(248, 246, 18), (254, 234, 24), (268, 214, 27)])}
PROTECTED = (0, 1, 5, 6, 7)                    # seeds on which the step removes strictly fewer records than are weak: the protection of dead-end sides is exercised
MIXED = [(EDGES, 1, 0), (EP.TIPS, 3, 0), (EP.BUBBLES, 0, 0), (EDGES, 2, 0), (EP.TIPS, 0, 0)]


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_graphs(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    edges = host_edges(nodes, presimp)
    strings = G.fake_bases(reads, G.L, seed)
    plain = U.unitigs(nodes, edges, strings)
    assert (len(plain["edges"]), len(plain["walks"])) == RANDOM[seed][0]
    for T, want in zip((1, 2, 3), RANDOM[seed][1]):
        log, final = run(nodes, edges, [(EDGES, T, 0), (EDGES, T, 0)], reads, k, strings)
        assert (log[0]["weak"], log[0]["edges"], len(final["walks"])) == want
        assert 20 <= log[0]["edges"] <= 7054 and log[0]["edges"] <= log[0]["weak"]
        assert (log[0]["edges"] < log[0]["weak"]) or seed not in PROTECTED
        assert log[1]["edges"] == 0                                                      # observed on these inputs, not a law
        assert len(final["edges"]) <= len(plain["edges"]) - log[0]["edges"]              # (a record that became an interior link is no unitig edge either)


def test_tips_and_bubbles_decide_on_a_graph_with_dead_arcs():
    """the mixed schedule of the GPU test: some seed's later steps remove something, so the state (alive, dead_arcs) is carried through"""
    later_edges = later_nodes = 0
    for seed in (1, 3, 4, 7):
        k, A, presimp, reads, nodes = random_graph(seed)
        log, final = run(nodes, host_edges(nodes, presimp), MIXED, reads, k, G.fake_bases(reads, G.L, seed))
        assert log[0]["edges"] == RANDOM[seed][1][0][1]
        later_edges += log[3]["edges"]
        later_nodes += sum(len(st["nodes"]) for st in log[1:])
        assert sum(len(w) for w in final["walks"]) == nodes["n_nodes"] - sum(len(st["nodes"]) for st in log)
    assert later_edges > 0 and later_nodes > 0


# ---- the C side ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_python_mirror_and_the_c99_header(tmp_path):
    from rust_mdbg_amd import api
    assert api.MDBG_SIMPLIFY_EDGES == EDGES == 8 and "mdbg_simplify_edges_removed" in api.EXPORTS and hasattr(api.load_library(), "mdbg_simplify_edges_removed")
    arr, n = api.simplify_steps([(api.MDBG_SIMPLIFY_EDGES, 2, 0)])
    assert n == 1 and (arr[0].kind, arr[0].max_nodes, arr[0].max_bases) == (8, 2, 0)
    assert len(api.MAGIC_SIMPLIFY_STEPS) == 14 and all(kind in (1, 2) for kind, _, _ in api.MAGIC_SIMPLIFY_STEPS)
    src = tmp_path / "edges_step.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mdbg_hip.h"\n'
                   "int main(void) {\n    mdbg_simplify_step st = {MDBG_SIMPLIFY_EDGES, 2, 0};\n    const uint64_t* per_step = NULL; uint64_t total = 0;\n"
                   "    int rc = mdbg_simplify_edges_removed(NULL, &per_step, &total);\n"
                   '    printf("%u %d %u\\n", st.kind, rc, (unsigned)MDBG_ABI_VERSION);\n    return 0;\n}\n')
    exe = str(tmp_path / "edges_step")
    lib = os.path.join(ROOT, "rust_mdbg_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lmdbg_hip", "-Wl,-rpath," + lib,
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["8", "-1", "3"]      # a null context is MDBG_E_PARAM (the layouts: tests/test_abi_exports.py)
