"""The transit restatement (tests/transits_restatement.py) pinned without a GPU: the hand-written expectations of tests/transit_graphs.py, the invariants of
include/mdbg_hip.h (mdbg_graph_transits) against the read paths and the junction support on every case of tests/sketch_graphs.py and every random graph, the
recorded figures of three random graphs, the text of the .transits.tsv, the host-side merge and verdict rule, and the Python mirror of mdbg_transit_list.
The GPU side is tests/test_gpu_transits.py."""
import functools
import os
from collections import Counter

import numpy as np
import pytest

import edge_prune_restatement as EP
import junctions_restatement as J
import read_paths_restatement as RP
import sketch_graphs as G
import transit_graphs as TG
import transits_restatement as T
import unitig_restatement as U
from conftest import ROOT
from test_read_paths_cpu import hashes
from test_sketch_graphs_cpu import BY_NAME, host_edges, model_nodes, random_graph


def restate(reads, k, nodes, walks, edges, min_support=1):
    return T.transits(hashes(reads), k, nodes["keys"].tolist(), nodes["index"].tolist(), walks, [e[:4] for e in edges], min_support)


@functools.lru_cache(maxsize=None)
def list_of(name):
    """a case of transit_graphs -> (nodes, the unitig restatement's list the case asks for: plain, or what its schedule leaves)"""
    c = TG.BY_NAME[name]
    nodes = G.nodes_from_sketch(c.reads, c.k, G.L, c.A)
    edges = host_edges(nodes, c.presimp)
    if c.steps is None:
        return nodes, U.unitigs(nodes, edges)
    return nodes, EP.simplify(nodes, edges, c.steps, hashes(c.reads), c.k, length_of=G.length_of_walk(nodes))[1]


def check_invariants(t, reads, k, nodes, walks, circular, edges):
    """the invariants of the header against the other two restatements, on one list over all reads.
    count <= support: a transit (c, c') names c' as its out-pair (s == 0) or mirror(c) (s == 1), so ONE crossing c1 serves a key's out-pair twice only as the
    second crossing of a transit with s == 0 and the first of one with s == 1 on the same key, which makes c1 == mirror(c1): the bound doubles for a pair that
    is its own mirror and for no other (likewise for the in-pair).  "odd k=4 1-2-3-2-1-2-3-2-1" has such a key: count 4 on an out-pair crossed twice."""
    keys, index = nodes["keys"].tolist(), nodes["index"].tolist()
    j = J.junctions(hashes(reads), k, keys, index, walks, [e[:4] for e in edges])
    r = RP.read_paths(hashes(reads), k, keys, index, walks, circular)
    assert sum(t["passes"]) == t["n_passes"] == sum(row[-1] for row in t["rows"]) and t["n_transits"] == len(t["rows"])
    assert (t["n_crossings"], t["n_explained"]) == (j["n_crossings"], j["n_explained"])
    assert all(p <= s for p, s, c in zip(t["passes"], r["support_steps"], circular) if not c)
    for row in t["rows"]:
        u, ri, ro, n = row[0], row[7], row[8], row[9]
        m = len(walks[u])
        own = lambda pair: 2 if J.mirror(pair) == pair else 1
        assert n <= min(j["support"][ri] * own((row[1:4], (u, 0, 0))), j["support"][ro] * own(((u, m - 1, 0), row[4:7])))
        assert j["keys"][ri] == J.key_of((row[1:4], (u, 0, 0))) and j["keys"][ro] == J.key_of(((u, m - 1, 0), row[4:7]))
        assert ri == j["keys"].index(j["keys"][ri]) and ro == j["keys"].index(j["keys"][ro])       # the smallest record number of the key
    assert t["rows"] == sorted(t["rows"])
    return j


# ---- the hand-built repeats ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TG.CASE_IDS)
def test_hand_built_repeats(name):
    c = TG.BY_NAME[name]
    nodes, u = list_of(name)
    e = c.expect
    for ms, n_resolved in e["resolved"].items():
        t = restate(c.reads, c.k, nodes, u["walks"], u["edges"], ms)
        assert (t["n_transits"], t["n_passes"], sorted(t["counts"].values()), t["n_repeats"], t["n_resolved"]) == (e["transits"], e["passes"], e["counts"], e["repeats"], n_resolved), ms
        tally = Counter(t["verdict"])
        assert tuple(tally[v] for v in (T.PLAIN, T.RESOLVED, T.UNRESOLVED, T.SELF)) == (len(u["walks"]) - e["repeats"], n_resolved, e["repeats"] - n_resolved, 0), ms
    if "walks" in e:
        assert sorted(len(w) for w in u["walks"]) == e["walks"]
    j = check_invariants(t, c.reads, c.k, nodes, u["walks"], u["circular"], u["edges"])
    assert (j["n_missing"] > 0) == bool(e.get("missing"))


def test_cross_keys_written_out():
    """cross r=3: the repeat is the one-entry unitig; the forward reads enter it from the last entry of A's unitig and leave for the first of B's, the reads
    of the other strand fall on the same kind of key: both ends at strand 0 after the canonical form, or both mirrored"""
    c = TG.BY_NAME["cross r=3"]
    nodes, u = list_of("cross r=3")
    t = restate(c.reads, c.k, nodes, u["walks"], u["edges"])
    rep = [i for i, w in enumerate(u["walks"]) if len(w) == 1]
    assert len(rep) == 1 and {row[0] for row in t["rows"]} == set(rep)
    assert (t["n_in"][rep[0]], t["n_out"][rep[0]], t["passes"][rep[0]], t["verdict"][rep[0]]) == (2, 2, 6, T.RESOLVED)
    for row in t["rows"]:
        (pu, pj, ps), (qu, qj, qs) = row[1:4], row[4:7]
        assert pj == (5 if ps == 0 else 0) and qj == (0 if qs == 0 else 5) and len({pu, qu, rep[0]}) == 3      # an end of a flank unitig, as the strand says
    assert {row[1] for row in t["rows"]} | {row[4] for row in t["rows"]} == set(range(5)) - set(rep)                # the four flanks, each once


def test_ring_is_entered_and_left_by_its_closing_record():
    c = TG.BY_NAME["ring"]
    nodes, u = list_of("ring")
    t = restate(c.reads, c.k, nodes, u["walks"], u["edges"])
    assert u["circular"] == [True] and len(t["rows"]) == 1
    row = t["rows"][0]
    assert row[:7] == (0, 0, 5, 0, 0, 0, 0) and row[7] == row[8] and t["verdict"] == [T.PLAIN] and (t["n_in"], t["n_out"]) == ([1], [1])
    r = RP.read_paths(hashes(c.reads), c.k, nodes["keys"].tolist(), nodes["index"].tolist(), u["walks"], u["circular"])
    assert t["passes"] == [4] and r["support_steps"] == [2]                         # the bound of the linear unitigs does not hold on a ring


def test_self_verdicts():
    c, nodes = BY_NAME[TG.SELF_CASE], model_nodes(TG.SELF_CASE)
    u = U.unitigs(nodes, host_edges(nodes, 0.0))
    t = restate(c.reads, c.k, nodes, u["walks"], u["edges"])
    assert t["verdict"] == [T.SELF] and (t["n_transits"], t["n_passes"], t["n_repeats"], t["n_resolved"]) == (1, 4, 1, 0)
    k, A, presimp, reads, nodes = random_graph(0)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    t = restate(reads, k, nodes, u["walks"], u["edges"])
    assert set(t["verdict"]) == {T.SELF} and t["n_repeats"] == len(u["walks"]) == 246 and t["n_resolved"] == 0


def test_the_verdict_rule_one_test_at_a_time():
    p1, p2, q1, q2 = (1, 5, 0), (2, 0, 1), (3, 0, 0), (4, 5, 1)
    both = {(p1, q1): 3, (p2, q2): 2}
    assert T.verdict_of(0, 1, 2, True, both, 1) == T.PLAIN and T.verdict_of(0, 2, 1, False, both, 1) == T.PLAIN      # PLAIN comes first, in front of SELF
    assert T.verdict_of(0, 2, 2, True, both, 1) == T.SELF
    assert T.verdict_of(0, 2, 2, False, both, 1) == T.verdict_of(0, 2, 2, False, both, 2) == T.RESOLVED
    assert T.verdict_of(0, 2, 2, False, both, 3) == T.UNRESOLVED                    # one strong key for two entrances
    assert T.verdict_of(0, 3, 2, False, both, 1) == T.verdict_of(0, 3, 3, False, both, 1) == T.UNRESOLVED
    assert T.verdict_of(0, 2, 2, False, {(p1, q1): 3, (p2, q1): 3}, 1) == T.UNRESOLVED      # two strong keys share their exit
    assert T.verdict_of(0, 2, 2, False, {(p1, q1): 3, (p1, q2): 3}, 1) == T.UNRESOLVED      # or their entrance
    weak_third = {**both, (p1, q2): 1}                                              # weak keys do not block
    assert T.verdict_of(0, 2, 2, False, weak_third, 2) == T.RESOLVED and T.verdict_of(0, 2, 2, False, weak_third, 1) == T.UNRESOLVED


# ---- the catalogue of sketch_graphs and the random graphs: the invariants, and three recorded graphs -----------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_invariants_on_the_catalogue(name):
    c, nodes = BY_NAME[name], model_nodes(name)
    for p in c.presimps:
        u = U.unitigs(nodes, host_edges(nodes, p))
        check_invariants(restate(c.reads, c.k, nodes, u["walks"], u["edges"]), c.reads, c.k, nodes, u["walks"], u["circular"], u["edges"])


# seed -> (transits, passes, (plain, resolved, unresolved, self) at min_support 1)
RANDOM = {1: (115, 1022, (1, 5, 77, 13)), 4: (131, 1177, (8, 12, 65, 16)), 7: (113, 1112, (9, 6, 71, 15))}


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_graphs(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    t = restate(reads, k, nodes, u["walks"], u["edges"])
    check_invariants(t, reads, k, nodes, u["walks"], u["circular"], u["edges"])
    tally = Counter(t["verdict"])
    assert t["n_repeats"] == len(u["walks"]) - tally[T.PLAIN] and t["n_resolved"] == tally[T.RESOLVED]
    if seed in RANDOM:
        assert (t["n_transits"], t["n_passes"], tuple(tally[v] for v in (T.PLAIN, T.RESOLVED, T.UNRESOLVED, T.SELF))) == RANDOM[seed]


def test_the_three_recorded_graphs_hold_all_four_verdicts():
    assert all(all(n > 0 for n in RANDOM[seed][2]) for seed in RANDOM)


# ---- the library's host side ------------------------------------------------------------------------------------------------------------------------------------
def as_library_result(t, n_reads, first=0):
    """a restatement result in the shape of Mdbg.graph_transits()"""
    from rust_mdbg_amd import api
    out = {f: np.array([row[i] for row in t["rows"]], dtype=dt) for i, (f, dt, _) in enumerate(api.TRANSIT_FIELDS[:10])}
    out.update({f: np.array(t[f], dtype=dt) for f, dt, per in api.TRANSIT_FIELDS if per == "unitig"})
    out.update({f: t[f] for f in ("n_crossings", "n_explained", "n_passes", "n_transits", "n_unitigs", "n_repeats", "n_resolved")}, n_reads=n_reads, first_read=first)
    return out


def assert_same(a, b):
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]) and np.asarray(a[f]).dtype == np.asarray(b[f]).dtype, f


# A..R, R and R..B are unitigs 1, 2, 3 (the forward reads come first); the reads of the other strand meet D first and C last: unitigs 4 and 5, walked backwards
MIXED_TSV = ("T\tutg0000001l\t+\tutg0000002l\t+\tutg0000003l\t+\t3\n" "T\tutg0000001l\t+\tutg0000002l\t+\tutg0000004l\t-\t1\n"
             "T\tutg0000005l\t-\tutg0000002l\t+\tutg0000004l\t-\t3\n" "U\tutg0000002l\t2\t2\t7\tunresolved\n")


def test_tsv_text_character_for_character():
    from rust_mdbg_amd import api
    c = TG.BY_NAME["mixed"]
    nodes, u = list_of("mixed")
    t = restate(c.reads, c.k, nodes, u["walks"], u["edges"])
    assert T.tsv_text(t, u["circular"]) == MIXED_TSV
    assert api.transit_text(as_library_result(t, len(c.reads)), np.array(u["circular"], np.uint8)) == MIXED_TSV
    t2 = restate(c.reads, c.k, nodes, u["walks"], u["edges"], 2)
    assert T.tsv_text(t2, u["circular"]) == MIXED_TSV.replace("unresolved", "resolved") == api.transit_text(as_library_result(t2, len(c.reads)), u["circular"])
    nodes, u = list_of("ring")
    t = restate(TG.BY_NAME["ring"].reads, 3, nodes, u["walks"], u["edges"])
    assert T.tsv_text(t, u["circular"]) == "T\tutg0000001c\t+\tutg0000001c\t+\tutg0000001c\t+\t4\n" == api.transit_text(as_library_result(t, 2), u["circular"])


@pytest.mark.parametrize("seed,min_support", [(1, 1), (4, 2), (7, 4)])
def test_merge_of_ranges_and_the_verdicts_on_the_merge(seed, min_support):
    """api.merge_transits and api.transit_verdicts on the restatement's results of three ranges of reads: what run_file does with the chunks"""
    from rust_mdbg_amd import api
    k, A, presimp, reads, nodes = random_graph(seed)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    whole_t = restate(reads, k, nodes, u["walks"], u["edges"], min_support)
    whole = as_library_result(whole_t, len(reads))
    parts = [as_library_result(restate(reads[a:b], k, nodes, u["walks"], u["edges"], min_support), b - a, a) for a, b in ((0, 1), (1, 50), (50, len(reads)))]
    assert sum(p["n_transits"] for p in parts) > whole["n_transits"]                  # some key occurs in more than one range
    col = lambda i, dt, f=int: np.array([f(e[i]) for e in u["edges"]], dtype=dt)
    self_flags = api.transit_self_flags(dict(n1=col(0, np.uint32), n2=col(2, np.uint32)), len(u["walks"]))
    assert self_flags.tolist() == whole_t["self_flags"]
    merged = api.merge_transits(parts)
    assert "verdict" not in merged and "n_resolved" not in merged                    # verdicts belong to the range they were computed on
    for f in merged:
        assert np.array_equal(merged[f], whole[f]) and np.asarray(merged[f]).dtype == np.asarray(whole[f]).dtype, f
    verdict = api.transit_verdicts(merged["n_in"], merged["n_out"], self_flags, merged, min_support)
    assert verdict.dtype == np.uint8 and verdict.tolist() == whole_t["verdict"]
    assert_same(api.merge_transits(parts, self_flags, min_support), whole)
    if min_support > 1:
        assert any(p["verdict"].tolist() != whole_t["verdict"] for p in parts)


def test_merge_of_nothing():
    from rust_mdbg_amd import api
    m = api.merge_transits([], np.zeros(0, np.uint8))
    assert (m["n_transits"], m["n_unitigs"], m["n_passes"], m["n_repeats"], m["n_resolved"]) == (0, 0, 0, 0, 0) and all(len(m[f]) == 0 for f, _, _ in api.TRANSIT_FIELDS)
    assert api.transit_text(m, []) == ""


# ---- the columns and the verdict values of the result (its layout and prototypes: tests/test_abi_exports.py) -------------------------------------------------------
def test_the_column_table_and_the_verdict_values_follow_the_header(tmp_path):
    import subprocess
    from rust_mdbg_amd import api
    fields = [f for f, _ in api.TransitList._fields_]
    assert fields == ["first_read", "n_reads", "n_crossings", "n_explained", "n_passes", "n_transits", "n_unitigs", "n_repeats", "n_resolved", "unitig", "in_unitig",
                      "in_entry", "in_strand", "out_unitig", "out_entry", "out_strand", "in_record", "out_record", "count", "n_in", "n_out", "passes", "verdict"]
    assert [f for f, _, _ in api.TRANSIT_FIELDS] == fields[9:]
    src = tmp_path / "verdicts.c"
    src.write_text('#include <stdio.h>\n#include "mdbg_hip.h"\nint main(void) {\n'
                   'printf("%d %d %d %d\\n", MDBG_TRANSIT_PLAIN, MDBG_TRANSIT_RESOLVED, MDBG_TRANSIT_UNRESOLVED, MDBG_TRANSIT_SELF);\nreturn 0; }\n')
    exe = str(tmp_path / "verdicts")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [api.TRANSIT_PLAIN, api.TRANSIT_RESOLVED, api.TRANSIT_UNRESOLVED, api.TRANSIT_SELF]
    assert (T.PLAIN, T.RESOLVED, T.UNRESOLVED, T.SELF) == (0, 1, 2, 3) and tuple(T.VERDICT_NAMES) == api.TRANSIT_VERDICT_NAMES
    L = api.load_library()
    for f in ("mdbg_graph_transits", "mdbg_graph_transits_device", "mdbg_transits_ms"):
        assert hasattr(L, f) and f in api.EXPORTS
