"""The read-path restatement (tests/read_paths_restatement.py) pinned without a GPU: hand-written paths, the recorded figures of the catalogue of
tests/sketch_graphs.py, the invariant support_windows == kc_sum, a simplified list, the text of the .read_paths.tsv, and the Python mirror of
mdbg_read_path_list.  The GPU side is tests/test_gpu_read_paths.py."""
import os

import numpy as np
import pytest

import read_paths_restatement as RP
import simplify_restatement as S
import sketch_graphs as G
import unitig_restatement as U
from conftest import ROOT
from test_sketch_graphs_cpu import BY_NAME, case_strings, host_edges, model_nodes, random_graph

# the u16 abundance of the hub's nodes saturates at 65535 + 656 / 655 sightings or wraps to 0 at 65536: an abundance is a count of windows only below that
WRAPPED = ("presimp 65535/656 at 0.01", "presimp 65535/655 at 0.01", "presimp 65535/1 at 0.01")


def hashes(reads):
    return [h for h, _ in reads]


def paths_on(nodes, reads, k, walks, circular):
    return RP.read_paths(hashes(reads), k, nodes["keys"].tolist(), nodes["index"].tolist(), walks, circular)


def plain(name, presimp=0.0):
    c, nodes = BY_NAME[name], model_nodes(name)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    return c, u, paths_on(nodes, c.reads, c.k, u["walks"], u["circular"])


# ---- hand-written paths --------------------------------------------------------------------------------------------------------------------------------
def test_fork_every_step():
    """the long read walks the trunk's two unitigs (nodes 0..3, 4..11), the short read the first of them and the arm (12..14); every walk lies in the
    reads' direction.  Steps are (first_window, n_windows, unitig, first_entry, strand)."""
    c, u, r = plain("fork")
    assert [len(w) for w in u["walks"]] == [4, 8, 3]
    long_read, short_read = [(0, 4, 0, 0, 0), (4, 8, 1, 0, 0)], [(0, 4, 0, 0, 0), (4, 3, 2, 0, 0)]
    assert r["steps"] == [long_read] * 5 + [short_read] * 2
    assert r["windows"] == [12] * 5 + [7] * 2 and r["placed"] == r["windows"]
    assert (r["n_windows"], r["n_placed"], r["n_steps"]) == (74, 74, 14) and max(len(s) for s in r["steps"]) == 2
    assert r["support_windows"] == [28, 40, 6] == u["kc_sum"] and r["support_steps"] == [7, 5, 2]


def test_bubble_with_a_branch_from_the_other_strand():
    """read `two` is sequenced from the other strand: it enters the shared ends at their LAST entry and walks them backwards (strand 1, first_entry 3),
    its own branch lies in its direction"""
    c, u, r = plain("bubble 7/3")
    assert [len(w) for w in u["walks"]] == [4, 4, 4, 4]
    one, two = [(0, 4, 0, 0, 0), (4, 4, 1, 0, 0), (8, 4, 2, 0, 0)], [(0, 4, 2, 3, 1), (4, 4, 3, 0, 0), (8, 4, 0, 3, 1)]
    assert r["steps"] == [one] * 7 + [two] * 3
    assert r["support_windows"] == [40, 28, 40, 12] == u["kc_sum"] and r["support_steps"] == [10, 7, 10, 3]
    assert (r["n_windows"], r["n_placed"], r["n_steps"]) == (120, 120, 30)


def test_islands_ring_is_one_step_longer_than_the_ring():
    c, u, r = plain("islands")
    assert u["circular"] == [False, False, False, True] and [len(w) for w in u["walks"]] == [7, 3, 2, 6]
    assert r["steps"] == [[(0, 7, 0, 0, 0)]] * 2 + [[(0, 3, 1, 0, 0)]] * 2 + [[(0, 2, 2, 0, 0)]] * 3 + [[(0, 7, 3, 0, 1)]] * 2
    ring = r["steps"][-1][0]
    assert ring[1] == 7 > len(u["walks"][3])                                           # once round and one window more: ONE step
    assert {s[4] for st in r["steps"] for s in st} == {0, 1}
    assert r["support_windows"] == [14, 6, 6, 14] == u["kc_sum"] and r["support_steps"] == [2, 2, 3, 2]
    # the same ring cut open: a linear unitig never continues onto itself
    cut = paths_on(model_nodes("islands"), c.reads, c.k, u["walks"], [False] * 4)
    assert cut["steps"][-1] == [(0, 1, 3, 0, 1), (1, 6, 3, 5, 1)]


def test_a_linear_one_node_unitig_never_continues_onto_itself():
    c, u, r = plain("odd k=3 5-5-5-5-5-5")
    assert len(u["walks"]) == 1 and len(u["walks"][0]) == 1 and not u["circular"][0]
    assert r["n_windows"] == 8 and r["steps"] == [[(w, 1, 0, 0, 1) for w in range(4)]] * 2


def test_partition_is_asserted():
    nodes = model_nodes("fork")
    with pytest.raises(AssertionError):
        paths_on(nodes, BY_NAME["fork"].reads, 3, [[(0, "+")], [(0, "-")]], [False, False])


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------------------------
FIGURES = {"fork": (74, 74), "hub": (240, 240), "islands": (40, 40), "odd k=3 5-5-5-5-5-5": (8, 8)}


@pytest.mark.parametrize("name", G.CASE_IDS)
def test_catalogue_invariant_and_figures(name):
    c, nodes = BY_NAME[name], model_nodes(name)
    for p in c.presimps:
        u = U.unitigs(nodes, host_edges(nodes, p))
        r = paths_on(nodes, c.reads, c.k, u["walks"], u["circular"])
        assert r["n_windows"] == sum(len(h) - c.k + 1 for h, _ in c.reads if len(h) > c.k) and r["n_placed"] <= r["n_windows"]
        assert sum(r["support_windows"]) == r["n_placed"] and sum(r["support_steps"]) == r["n_steps"]
        if name in WRAPPED:
            assert r["support_windows"] != u["kc_sum"]                                 # the u16 abundance saturated or wrapped: no longer a count of windows
            assert r["n_placed"] == r["n_windows"]
        else:
            assert r["support_windows"] == u["kc_sum"]
        if name in FIGURES:
            assert (r["n_windows"], r["n_placed"]) == FIGURES[name]
        for st, W in zip(r["steps"], r["windows"]):                                    # steps lie inside the read, in order, without overlap
            assert all(a[0] + a[1] <= b[0] for a, b in zip(st, st[1:])) and (not st or st[-1][0] + st[-1][1] <= W)


RANDOM = {0: (3417, 3417, 3417), 1: (3405, 3405, 1246), 2: (3271, 3271, 210), 3: (3504, 3502, 3502), 4: (3451, 3449, 1392), 5: (3373, 3368, 184),
          6: (3725, 3725, 3725), 7: (3646, 3646, 1336)}


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_graph_figures(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    r = paths_on(nodes, reads, k, u["walks"], u["circular"])
    assert (r["n_windows"], r["n_placed"], r["n_steps"]) == RANDOM[seed]
    assert r["support_windows"] == u["kc_sum"]                                          # (A = 2 filters rows: their windows are unplaced AND in no kc_sum)


# ---- after a simplify schedule ---------------------------------------------------------------------------------------------------------------------------
def test_fork_after_clipping_the_arm():
    """[(TIPS, 3, 0)] removes nodes 12, 13, 14: the trunk is ONE unitig of 12 nodes, the windows of the two short reads that lay on the arm are unplaced"""
    c, nodes = BY_NAME["fork"], model_nodes("fork")
    log, left = S.simplify(nodes, host_edges(nodes, 0.0), [(G.TIPS, 3, 0)], case_strings("fork"), None)
    assert [sorted(st["nodes"]) for st in log] == [[12, 13, 14]] and [len(w) for w in left["walks"]] == [12]
    r = paths_on(nodes, c.reads, c.k, left["walks"], left["circular"])
    assert r["steps"] == [[(0, 12, 0, 0, 0)]] * 5 + [[(0, 4, 0, 0, 0)]] * 2
    assert r["windows"] == [12] * 5 + [7] * 2 and r["placed"] == [12] * 5 + [4] * 2
    assert r["support_windows"] == [68] and r["support_steps"] == [7] and (r["n_windows"], r["n_placed"]) == (74, 68)


# ---- the text --------------------------------------------------------------------------------------------------------------------------------------------
SHORT_READS_TSV = ("0\t0\t0\t*\n" "1\t0\t0\t*\n" "2\t2\t2\t0:2:>utg0000001l:0\n" "3\t0\t0\t*\n" "4\t0\t0\t*\n" "5\t3\t3\t0:3:>utg0000001l:1\n" "6\t0\t0\t*\n" "7\t0\t0\t*\n")


def test_tsv_text_character_for_character():
    c, u, r = plain("short reads")
    assert RP.tsv_text(r, range(len(c.reads)), u["circular"]) == SHORT_READS_TSV
    c, u, r = plain("islands")
    text = RP.tsv_text(r, [100 + i for i in range(len(c.reads))], u["circular"])
    assert text.split("\n")[0] == "100\t7\t7\t0:7:>utg0000001l:0" and text.split("\n")[8] == "108\t7\t7\t0:7:<utg0000004c:0"
    c, u, r = plain("bubble 7/3")
    assert RP.tsv_text(r, range(10), u["circular"]).split("\n")[9] == "9\t12\t12\t0:4:<utg0000003l:3,4:4:>utg0000004l:0,8:4:<utg0000001l:3"


def as_library_result(r, ordinals):
    """a restatement result in the shape of Mdbg.graph_read_paths()"""
    flat = [s for st in r["steps"] for s in st]
    col = lambda i, t: np.array([s[i] for s in flat], dtype=t)
    return dict(ordinal=np.array(list(ordinals), np.uint64), read_windows=np.array(r["windows"], np.uint32),
                step_offsets=np.cumsum([0] + [len(st) for st in r["steps"]]).astype(np.uint64), first_window=col(0, np.uint32), step_windows=col(1, np.uint32),
                unitig=col(2, np.uint32), first_entry=col(3, np.uint32), strand=col(4, np.uint8))


def test_the_library_side_writer_prints_the_same_text():
    from rust_mdbg_amd import api
    c, u, r = plain("short reads")
    assert api.read_path_text(as_library_result(r, range(len(c.reads))), u["circular"]) == SHORT_READS_TSV
    c, u, r = plain("bubble 7/3")
    assert api.read_path_text(as_library_result(r, range(50, 60)), np.array(u["circular"], np.uint8)) == RP.tsv_text(r, range(50, 60), u["circular"])
