"""The hand-built minimizer-space graphs of tests/sketch_graphs.py without a GPU: the plain node model is pinned to the oracle on real sketches, the two edge
references agree on every case, every recorded figure of the catalogue is what the references give, and each case reaches the corner it was built for.
The GPU side is tests/test_gpu_sketch_graphs.py."""
import functools
import random

import numpy as np
import pytest

import components_restatement as CR
import simplify_restatement as S
import sketch_graphs as G
import unitig_restatement as U
from oracle import oracle as O
from test_gpu_fuzz import fuzz_reads
from test_gpu_parity import NODE_FIELDS, rand_reads

F = ("n1", "o1", "n2", "o2", "overlap")
BY_NAME = {c.name: c for c in G.CASES}


def as_rows(e):
    return list(zip(*(np.asarray(e[f]).tolist() for f in F)))


@functools.lru_cache(maxsize=None)
def model_nodes(name):
    c = BY_NAME[name]
    return G.nodes_from_sketch(c.reads, c.k, G.L, c.A)


@functools.lru_cache(maxsize=None)
def case_strings(name):
    c = BY_NAME[name]
    return G.fake_bases(c.reads, G.L, 1) if c.strings else None


def host_edges(nodes, presimp):
    from rust_mdbg_amd import emit as E
    return E.Emitter().edges(nodes, presimp)


def reads_of_sketch(sk):
    off = sk["off"].tolist()
    return [(tuple(sk["hashes"][a:b].tolist()), tuple(sk["pos"][a:b].tolist())) for a, b in zip(off, off[1:])]


def assert_model_equals_oracle(bases, offs, k, l, d, A):
    sk = O.sketch(bases, offs, l, d, already_hpc=True)
    assert sk["err"] == 0
    g = O.Graph(k, l, d, A, already_hpc=True)
    assert g.ingest(bases, offs) == 0
    exp = g.finalize(with_edges=False)
    got = G.nodes_from_sketch(reads_of_sketch(sk), k, l, A)
    assert (got["n_nodes"], got["n_nodes_before"]) == (exp["n_nodes"], exp["n_nodes_before"])
    for f in NODE_FIELDS:
        assert got[f].dtype == exp[f].dtype and np.array_equal(got[f], exp[f]), f
    return exp


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_oracle_on_the_fuzz_sketches(seed):
    """the inputs of tests/test_gpu_edges.py (k of 3, 4, 7 and 12, A of 1, 2 and 3), sketched by the oracle"""
    rnd = random.Random(500 + seed)
    k, l, d, A = rnd.choice([(2, 8, 0.03, 1), (3, 8, 0.03, 1), (5, 10, 0.01, 2), (7, 12, 0.008, 2), (4, 6, 0.05, 3), (12, 12, 0.01, 1)])
    reads = fuzz_reads(rnd, n_reads=200, genome_len=rnd.choice([3000, 30000]), mean_len=4000, err=rnd.choice([0.0, 0.01]), p_lower=0.0, p_n=0.0,
                       p_hp=rnd.choice([0.0, 0.02]))
    exp = assert_model_equals_oracle(*O.concat_reads(reads), k, l, d, A)
    assert exp["n_nodes"] > 10


@pytest.mark.parametrize("A", [1, 2])
def test_model_equals_the_oracle_when_the_abundance_wraps_to_zero(A):
    """one read 65,536 times: every k-min-mer of it has the u16 abundance 0.  With A = 1 nothing is filtered, the nodes stay with abundance 0 (what the
    65535/1 presimp case relies on); with A = 2 they go"""
    read = rand_reads(3, 1, 420, 420)[0]
    other = rand_reads(4, 3, 900, 900)
    exp = assert_model_equals_oracle(*O.concat_reads(other + other + [read] * 65536), 3, 8, 0.05, A)
    zeros = int((exp["abundance"] == 0).sum())
    assert (zeros >= 3 and exp["n_nodes"] == exp["n_nodes_before"]) if A == 1 else (zeros == 0 and 6 <= exp["n_nodes"] < exp["n_nodes_before"])


def test_mread_and_fake_bases():
    assert G.mread([3, 4, 5]) == ((3, 4, 5), (0, 100, 200)) and G.mread([3, 4, 5], 7, rev=True) == ((5, 4, 3), (0, 7, 14))
    assert G.mread([3, 4, 5], [0, 10, 500], rev=True) == ((5, 4, 3), (0, 490, 500)) and G.mread([]) == ((), ())
    with pytest.raises(AssertionError):
        G.mread([1, 2], [5, 5])
    a, b = G.mread([1, 2, 3]), G.mread([])
    s = G.fake_bases([a, b, a], 10, 0)
    assert [len(x) for x in s] == [210, 0, 210] and s[0] == s[2] and set(s[0]) <= set(b"ACGT")
    h, p, o = G.sketch_arrays([a, b, a])
    assert (h.dtype, p.dtype, o.dtype) == (np.uint64, np.uint32, np.uint64) and o.tolist() == [0, 3, 3, 6] and p.tolist() == [0, 100, 200] * 2


# ---- the limits every sketch stays within ----------------------------------------------------------------------------------------------------------------
def all_sketches():
    for c in G.CASES:
        yield c.name, c.reads
    for seed in G.RANDOM_SEEDS:
        yield "random %d" % seed, G.random_case(seed)[3]


def test_every_sketch_is_one_a_real_sketch_could_be():
    assert G.HASH_LIMIT == O.hash_bound(G.D) and G.remap(G.REMAP_MAX) < G.HASH_LIMIT
    assert [G.remap(v) for v in range(1, G.REMAP_MAX + 1)] == sorted({G.remap(v) for v in range(1, G.REMAP_MAX + 1)})      # injective, order kept
    for name, reads in all_sketches():
        seen = set()
        for rd in reads:
            if id(rd) in seen:
                continue
            seen.add(id(rd))
            H, P = rd
            assert len(H) == len(P) and all(0 < h < G.HASH_LIMIT for h in H), name
            assert all(a < b for a, b in zip(P, P[1:])) and (not P or 0 <= P[0] and P[-1] < 1 << 32), name
            assert len(H) < 1 << 26, name
        h, p, o = G.sketch_arrays(reads[:1000])
        assert o[0] == 0 and np.all(o[1:] >= o[:-1]) and o[-1] == len(h) == len(p), name
    names = [c.name for c in G.CASES]
    assert len(names) == len(set(names))
    for c in G.CASES:
        assert c.split is None or 0 < c.split < len(c.reads)
    assert sum(c.split is not None for c in G.CASES if c.name.startswith(("fork", "bubble", "islands"))) >= 3


# ---- references agree, recorded figures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_references_agree_and_give_the_recorded_figures(name):
    c = BY_NAME[name]
    nodes, reads, x = model_nodes(name), case_strings(name), c.expect
    assert nodes["n_nodes"] == x["nodes"]
    assert sorted(x.get("edges", {})) == sorted(set(x.get("edges", {})) & set(c.presimps))       # no figure for a value that is not run
    for p in c.presimps:
        rows, removed = O.edges_from_nodes(nodes, p)
        host = host_edges(nodes, p)
        assert sorted(as_rows(host)) == rows and host["presimp_removed"] == removed
        if p in x.get("edges", {}):
            assert (len(rows), removed) == x["edges"][p]
    if "shifts" in x:
        assert nodes["shift"].tolist() == x["shifts"]
        assert [r[4] for r in as_rows(host_edges(nodes, 0.0))] == x["overlaps"]
    edges = host_edges(nodes, c.presimps[0])
    length_of = None if reads is not None else G.length_of_walk(nodes)
    cur, _ = S.current(nodes, edges, {int(i) for i in nodes["index"]}, reads, length_of)
    if "unitigs" in x:
        assert list(zip((len(w) for w in cur["walks"]), cur["length"])) == x["unitigs"]
    if "n_unitigs" in x:
        assert len(cur["walks"]) == x["n_unitigs"]
    if "components" in x:
        cc = CR.components(cur)
        assert (cc["nodes"], cc["bases"], cc["circular"]) == (x["components"]["nodes"], x["components"]["bases"], x["components"]["circular"])
        assert cc["n_components"] == len(x["components"]["nodes"])
    assert sorted(x.get("removed", {})) == sorted(tuple(s) for s in c.schedules if tuple(s) in x.get("removed", {}))
    for steps in c.schedules:
        log, final = CR.simplify(nodes, edges, steps, reads, length_of)
        if all(kind != CR.COMPONENTS for kind, _, _ in steps):                      # the same schedule through the tip / bubble restatement alone
            log2, final2 = S.simplify(nodes, edges, steps, reads, length_of)
            assert [st["nodes"] for st in log2] == [st["nodes"] for st in log] and final2["walks"] == final["walks"]
        else:
            with pytest.raises(AssertionError):
                S.simplify(nodes, edges, steps, reads, length_of)
        if tuple(steps) in x.get("removed", {}):
            assert [sorted(st["nodes"]) for st in log] == x["removed"][tuple(steps)], steps
        assert sorted(n for w in final["walks"] for n, _ in w) == sorted(set(nodes["index"].tolist()) - set().union(*(st["nodes"] for st in log)))


def test_length_of_walk_is_the_string_length():
    """what the 65,535-abundance rows use instead of strings gives the lengths the strings give"""
    for name in ("fork", "gaps", "hub", "islands", "odd k=2 1-2-1-3-1-4-1-1", "odd k=4 1-2-3-3-2-1-4-5"):
        nodes = model_nodes(name)
        u = U.unitigs(nodes, host_edges(nodes, 0.0), case_strings(name))
        assert [G.length_of_walk(nodes)(w) for w in u["walks"]] == u["length"], name


# ---- each case reaches what it was built for -------------------------------------------------------------------------------------------------------------
def removed_at(name, steps):
    return BY_NAME[name].expect["removed"][tuple(steps)]


def test_presimp_cases_sit_where_f32_and_f64_part():
    f32 = np.float32
    p = f32(0.01)
    # 100/1 at 0.01: the f32 product is exactly 1.0 and the edge stays.  The exact product of 0.01f and 100 is 0.99999998, below 1, so a double multiply keeps it
    # too: 0.01f lies below 0.01, and no u16 abundance makes the two disagree at 0.01 or 0.5 (searched exhaustively below)
    assert p * f32(100) == f32(1) and 0.9999999 < float(p) * 100.0 < 1.0 and not (f32(1) < p * f32(100))
    for pv in (0.01, 0.5):
        ar = np.arange(1, 65536)
        exact, rounded = float(f32(pv)) * ar.astype(np.float64), (f32(pv) * ar.astype(f32)).astype(np.float64)
        assert not np.any((rounded == np.floor(rounded)) & (exact > rounded))          # they part only where f32 rounds DOWN onto an integer a2: a2 < exact, not a2 < rounded
    # 10/1 at 0.1 and 10/3 at 0.3 are where they part: f32 keeps the edge, the exact (double) product removes it
    for pv, big, small in ((0.1, 10, 1), (0.3, 10, 3)):
        q = f32(pv)
        assert not (f32(small) < q * f32(big)) and float(small) < float(q) * float(big)
        assert BY_NAME["presimp %d/%d at %g" % (big, small, pv)].expect["edges"][pv] == (16, 0)
    assert BY_NAME["presimp 11/1 at 0.1"].expect["edges"][0.1] == (14, 1) and BY_NAME["presimp 10/2 at 0.3"].expect["edges"][0.3] == (14, 1)
    assert BY_NAME["presimp 100/1 at 0.01"].expect["edges"][0.01] == (16, 0)
    assert BY_NAME["presimp 200/1 at 0.01"].expect["edges"][0.01] == (14, 1) and BY_NAME["presimp 99/1 at 0.01"].expect["edges"][0.01] == (16, 0)
    assert not (f32(2) < f32(0.5) * f32(4)) and f32(2) < f32(0.5) * f32(5)          # 4/2 is an exact tie, 5/2 is past it
    assert BY_NAME["presimp 4/2 at 0.5"].expect["edges"][0.5] == (16, 0) and BY_NAME["presimp 5/2 at 0.5"].expect["edges"][0.5] == (14, 1)
    for name, ab in (("presimp 65535/656 at 0.01", [655, 656, 65535]), ("presimp 65535/655 at 0.01", [654, 655, 65535]), ("presimp 65535/1 at 0.01", [0, 1, 65535])):
        assert sorted(set(model_nodes(name)["abundance"].tolist())) == ab
    # 65535/656: aref = min(65535, 655) = 655 at the hub's last node, 0.01f * 655 = 6.55: nothing near; at x's first node aref = 655 too.  The row is there for the
    # abundances themselves: u16 values next to 65535 in the comparison and in kc_sum
    assert sum(model_nodes("presimp 65535/656 at 0.01")["abundance"].tolist()) == 3 * (655 + 656 + 65535)


def test_boundary_cases_differ_between_the_limit_and_one_below():
    T, B, K = G.TIPS, G.BUBBLES, G.COMPONENTS
    for name in ("fork", "fork, mirrored", "fork, arm ends in the trunk"):
        assert removed_at(name, [(T, 3, 0)]) == removed_at(name, [(T, 0, 410)]) == [[12, 13, 14]]
        assert removed_at(name, [(T, 2, 0)]) == removed_at(name, [(T, 0, 409)]) == [[]]
    assert removed_at("bubble at the limits", [(B, 4, 510)]) == [[12, 13, 14, 15]]
    assert removed_at("bubble at the limits", [(B, 3, 510)]) == removed_at("bubble at the limits", [(B, 4, 509)]) == [[]]
    weak = "bubble, weaker branch at the limits"
    assert removed_at(weak, [(B, 5, 610)]) == [[12, 13, 14, 15, 16]] and removed_at(weak, [(B, 4, 610)]) == removed_at(weak, [(B, 5, 609)]) == [[]]
    assert removed_at("islands", [(K, 2, 0)]) == removed_at("islands", [(K, 0, 310)]) == [[10, 11]]
    assert removed_at("islands", [(K, 1, 0)]) == removed_at("islands", [(K, 0, 309)]) == [[]] and removed_at("islands", [(K, 3, 0)]) == [[7, 8, 9, 10, 11]]


def test_tie_cases_are_ties():
    for name in ("fork, equal abundance", "bubble 5/5", "bubble, three branches, tie"):
        nodes = model_nodes(name)
        cur = U.unitigs(nodes, host_edges(nodes, 0.0), case_strings(name))
        mean = [s / len(w) for s, w in zip(cur["kc_sum"], cur["walks"])]
        if name.startswith("fork"):                                                 # the two arms: equal abundance, the longer one wins
            assert mean[1] == mean[2] and cur["length"][1] > cur["length"][2]
        else:                                                                       # the branches: equal abundance and length, the smaller unitig number wins
            br = [i for i in range(len(cur["walks"])) if cur["walks"][i][0][0] not in (0, 8)]
            assert len(br) >= 2 and len({(mean[i], cur["length"][i]) for i in br}) == 1


def test_odd_cases_hold_what_fuzz_graphs_lack():
    pal = lambda t: tuple(t) == tuple(t)[::-1]
    for k, written, _, _, _ in G.ODD:
        c = BY_NAME[G.odd_name(k, written)]
        nodes = model_nodes(c.name)
        keys = nodes["keys"].tolist()
        norm = lambda t: min(tuple(t), tuple(t)[::-1])
        # a palindromic (k-1)-mer (the span_reversed tie), or a node whose prefix and suffix are one (k-1)-mer: both its listings fall into one bucket
        assert any(pal(key[:-1]) or pal(key[1:]) or norm(key[:-1]) == norm(key[1:]) for key in keys), c.name
    nodes = model_nodes("odd k=3 5-5-5-5-5-5")
    rows = as_rows(host_edges(nodes, 0.0))
    assert len(rows) == 16 and {(r[0], r[2]) for r in rows} == {(0, 0)} and {(chr(r[1]), chr(r[3])) for r in rows} == {("+", "+"), ("+", "-"), ("-", "+"), ("-", "-")}
    nodes = model_nodes("odd k=2 1-2-1-3-1-4-1-1")
    rows = as_rows(host_edges(nodes, 0.0))
    pairs = [(r[0], r[2]) for r in rows]
    assert max(pairs.count(p) for p in set(pairs)) >= 4                                # a pair of nodes joined by several edges
    assert any(pal(key) for key in nodes["keys"].tolist())                             # a k-min-mer equal to its reverse: `reversed` is 1 on the tie
    assert all(int(r) == 1 for key, r in zip(nodes["keys"].tolist(), nodes["reversed"]) if pal(key))


def test_gap_and_hub_cases_reach_their_targets():
    nodes = model_nodes("gaps")
    assert int(nodes["shift_full"].max()) > 65535 and not np.array_equal(nodes["shift_full"], nodes["shift"].astype(np.uint64))
    rows = as_rows(host_edges(nodes, 0.0))
    full = {int(i): (int(sl), sf.tolist()) for i, sl, sf in zip(nodes["index"], nodes["seqlen"], nodes["shift_full"])}
    untruncated = [min(full[r[0]][0] - full[r[0]][1][0 if chr(r[1]) == "+" else 1], full[r[2]][0] - 1) for r in rows]
    assert untruncated != [r[4] for r in rows]                                         # an overlap from the full shift would be another number
    nodes = model_nodes("hub")
    listing = {}
    for key in nodes["keys"].tolist():
        for part in (tuple(key[:-1]), tuple(key[1:])):
            listing[min(part, part[::-1])] = listing.get(min(part, part[::-1]), 0) + 1
    assert max(listing.values()) == 80                                                 # one (k-1)-mer shared by dozens of nodes


def test_short_read_case():
    c = BY_NAME["short reads"]
    assert sorted({len(h) for h, _ in c.reads}) == [0, 1, c.k, c.k + 1, c.k + 2]
    nodes = model_nodes(c.name)
    assert 1 not in nodes["src_read"].tolist() and 6 not in nodes["src_read"].tolist() and nodes["src_read"].tolist()[:2] == [2, 2]


# ---- random minimizer-space graphs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_graph(seed):
    k, A, presimp, reads = G.random_case(seed)
    return k, A, presimp, reads, G.nodes_from_sketch(reads, k, G.L, A)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_seeds_are_admissible(seed):
    """the unitig restatement accepts the graph (its own assertion: no chain holds a vertex and its complement), and the two edge references agree on it"""
    k, A, presimp, reads, nodes = random_graph(seed)
    rows, removed = O.edges_from_nodes(nodes, presimp)
    host = host_edges(nodes, presimp)
    assert sorted(as_rows(host)) == rows and host["presimp_removed"] == removed
    u = U.unitigs(nodes, host, G.fake_bases(reads, G.L, seed))
    assert nodes["n_nodes"] > 50 and len(rows) > nodes["n_nodes"] and sum(len(w) for w in u["walks"]) == nodes["n_nodes"]


def test_random_seeds_cover_the_parameters():
    assert len(G.RANDOM_SEEDS) == 8
    got = [random_graph(s)[:3] for s in G.RANDOM_SEEDS]
    assert {g[0] for g in got} == {2, 3, 4} and {g[1] for g in got} == {1, 2} and {g[2] for g in got} == {0.0, 0.01, 0.5}
    assert any(int(random_graph(s)[4]["shift_full"].max()) > 65535 for s in G.RANDOM_SEEDS)
    assert any(any(tuple(key) == tuple(key)[::-1] for key in random_graph(s)[4]["keys"].tolist()) for s in G.RANDOM_SEEDS)
    total = sum(sum(p[-1] + G.L for _, p in random_graph(s)[3] if p) for s in G.RANDOM_SEEDS)
    assert total < 32 << 20                                                             # the fake strings of all eight stay small
