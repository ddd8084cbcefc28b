"""The nested-repeat restatement (tests/nested_restatement.py: the NESTED step of include/mdbg_hip.h, mdbg_graph_simplify, and the placement on a list that
holds copies) pinned without a GPU: the hand-built catalogue of tests/nested_graphs.py with the figures written down beside each case and the second run that
makes it sharp, the placements against a brute force over each read's walk, the schedules the library refuses, the step on graphs without copies against the
REPEATS restatement, base space, and the new constant in the header and in api.  The GPU side is tests/test_gpu_nested.py."""
import functools
import os

import pytest

import nested_graphs as NG
import nested_restatement as NR
import repeats_restatement as RR
import sketch_graphs as G
import transit_graphs as TG
import unitig_restatement as U
from conftest import ROOT
from test_read_paths_cpu import hashes
from test_repeats_cpu import BASE_PARAMS, HAND, MIXED, base_space_hashes, check_invariants, hand_graph, pieces_of, tiled_reads
from test_sketch_graphs_cpu import host_edges, random_graph

TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS, NESTED = NR.TIPS, NR.BUBBLES, NR.COMPONENTS, NR.EDGES, NR.REPEATS, NR.NESTED
COUNTS = ("ambiguous", "resolved", "conflicts", "unanchored")


@functools.lru_cache(maxsize=None)
def graph_of(reads, k, A):
    nodes = G.nodes_from_sketch(list(reads), k, G.L, A)
    return nodes, host_edges(nodes, 0.0)


def run(reads, k, A, steps):
    """-> (log, final, the four placement counts) of the checker"""
    nodes, edges = graph_of(tuple(reads), k, A)
    tally = {}
    log, final = NR.simplify(nodes, edges, steps, hashes(reads), k, None, G.length_of_walk(nodes), tally)
    return log, final, tuple(tally.get(f, 0) for f in COUNTS)


@functools.lru_cache(maxsize=None)
def expected(name):
    c = NG.BY_NAME[name]
    return run(c.reads, c.k, c.A, c.steps)


def nested_invariants(nodes, edges, log, final):
    """test_repeats_cpu.check_invariants, which knows REPEATS steps only, and the same for NESTED steps; every origin is a table row"""
    check_invariants(nodes, edges, log, final)
    rows = {int(i) for i in nodes["index"]}
    assert set(final["origin"].values()) <= rows and all(c > max(rows) for c in final["origin"])
    assert sorted(final["origin"]) == list(range(max(rows) + 1, max(rows) + 1 + final["copies"]))      # X stays the table's, the numbering goes on
    for st in log:
        if st["kind"] == NESTED:
            assert st["nodes"] == set() and st["unitigs"] == [] and st["edges"] == 0


@pytest.mark.parametrize("name", NG.CASE_IDS)
def test_catalogue_is_what_was_written_down_and_every_case_is_sharp(name):
    c = NG.BY_NAME[name]
    log, final, counts = expected(name)
    assert sorted(len(w) for w in final["walks"]) == c.expect
    assert c.counts is None or counts == c.counts
    nodes, edges = graph_of(tuple(c.reads), c.k, c.A)
    nested_invariants(nodes, edges, log, final)
    _, other, other_counts = run(c.other_reads or c.reads, c.k, c.A, c.other_steps or c.steps)
    if c.differs == "list":
        assert other["walks_original"] != final["walks_original"]
    else:
        assert other_counts != counts and counts[0] == sum(counts[1:])
    assert c.other_counts is None or other_counts == c.other_counts


@pytest.mark.parametrize("name", NG.CASE_IDS)
def test_placements_against_a_brute_force_over_each_read(name):
    """on the list every NESTED step of the case decides against: the windows placed by walking outwards from each ambiguous window == every entry of the
    window's row tried against both anchors"""
    c = NG.BY_NAME[name]
    nodes, edges = graph_of(tuple(c.reads), c.k, c.A)
    H = hashes(c.reads)
    seen = 0
    for n in range(1, len(c.steps)):
        if c.steps[n][0] != NESTED:
            continue
        _, cur, _ = run(c.reads, c.k, c.A, c.steps[:n])
        if not cur["origin"]:
            continue
        args = (H, c.k, nodes["keys"].tolist(), nodes["index"].tolist(), cur["walks"], cur["origin"])
        got, brute = NR.placements(*args), NR.brute_force_placements(*args)
        assert got == brute
        placed_twice = [v for p in got for v in p if v is not None]
        assert all(0 <= j < len(cur["walks"][u]) for u, j, _ in placed_twice)
        seen += 1
    assert seen >= 1


def _wrapping(anchor, distance, behind, row, rev, walks, origin):
    """a WRONG candidate rule: the same unitig, but round its end"""
    u, j, s = anchor
    j2 = (j + distance if behind == (s == 0) else j - distance) % len(walks[u])
    idx, o = walks[u][j2]
    return (u, j2, s) if origin.get(int(idx), int(idx)) == row and int(rev != (o == "-")) == s else None


def _any_row(anchor, distance, behind, row, rev, walks, origin):
    """a WRONG candidate rule: the entry's row is not compared with the window's"""
    u, j, s = anchor
    j2 = j + distance if behind == (s == 0) else j - distance
    return (u, j2, s) if 0 <= j2 < len(walks[u]) and int(rev != (walks[u][j2][1] == "-")) == s else None


@pytest.mark.parametrize("wrong, name, counts", [(_wrapping, "a circular unitig that holds copies", (50, 48, 0, 2)), (_any_row, "a candidate on another row", (106, 97, 9, 0))],
                         ids=["no wrap", "row(e) is w's row"])
def test_a_wrong_candidate_rule_misses_the_pinned_counts(monkeypatch, wrong, name, counts):
    """the case that is there for a clause of "a candidate is VALID iff" pins counts that a placement without that clause does not give.  counts: what the wrong
    rule gives (for the ring worked out beside the case in tests/nested_graphs.py; for the row the number of conflicts depends on the hashes); they are not the
    pinned ones, which the library has to meet in tests/test_gpu_nested.py"""
    c = NG.BY_NAME[name]
    monkeypatch.setattr(NR, "candidate", wrong)
    assert run(c.reads, c.k, c.A, c.steps)[2] == counts != c.counts


def test_many_nested_side_by_side():
    reads = NG.many_nested(300)
    log, final, counts = run(reads, 3, 1, [(REPEATS, 1, 0), (NESTED, 1, 0)])
    assert (log[0]["copies"], log[1]["copies"], sorted({len(w) for w in final["walks"]}), len(final["edges"])) == (900, 3300, [11, 19], 0)
    assert len(final["walks"]) == 900 and counts == (2700, 2700, 0, 0)
    nodes, edges = graph_of(tuple(reads), 3, 1)
    nested_invariants(nodes, edges, log, final)


def test_both_strands_and_a_copy_in_a_minus_entry():
    """the catalogue holds reads of both strands on one repeat, and a copy that lies in a '-' oriented entry of the unitig it has joined"""
    _, final, _ = expected("nested")
    assert "-" in {o for w in final["walks"] for i, o in w if i in final["origin"]}
    f, c = NG.nested_family(801), NG.BY_NAME["nested"]
    assert G.mread(f["p1"]) in c.reads and G.mread(f["p2"], rev=True) in c.reads      # the two occurrences of x u y are read from different strands


# ---- what the library refuses -----------------------------------------------------------------------------------------------------------------------------------
REFUSED = ([(NESTED, 0, 0)], [(NESTED, 1, 5)], [(NESTED, 1, 0), (EDGES, 1, 0)], [(NESTED, 1, 0), (REPEATS, 1, 0)], [(REPEATS, 1, 0), (NESTED, 1, 0), (EDGES, 1, 0)],
           [(REPEATS, 1, 0), (NESTED, 1, 0), (REPEATS, 1, 0)], [(REPEATS, 1, 0), (TIPS, 0, 0), (REPEATS, 1, 0)], [(REPEATS, 1, 0), (EDGES, 1, 0)], [(32, 1, 0)])
ACCEPTED = ([(EDGES, 1, 0), (NESTED, 1, 0)], [(NESTED, 1, 0), (NESTED, 2, 0), (TIPS, 0, 0), (NESTED, 1, 0)], [(EDGES, 1, 0), (REPEATS, 1, 0), (TIPS, 0, 0), (NESTED, 1, 0), (COMPONENTS, 2, 0)])


def test_the_checker_refuses_what_the_library_refuses():
    c = NG.BY_NAME["nested"]
    for bad in REFUSED:
        with pytest.raises(AssertionError):
            run(c.reads, c.k, c.A, bad)
    for good in ACCEPTED:
        run(c.reads, c.k, c.A, good)


# ---- on a graph without copies the step IS the REPEATS step ----------------------------------------------------------------------------------------------------
def same_as_repeats(nodes, edges, steps, reads, k, strings=None):
    length = None if strings is not None else G.length_of_walk(nodes)
    as_nested = [(NESTED if kind == REPEATS else kind, a, b) for kind, a, b in steps]
    log, final = NR.simplify(nodes, edges, as_nested, hashes(reads), k, strings, length)
    rlog, rfinal = RR.simplify(nodes, edges, steps, hashes(reads), k, strings, length)
    assert final == rfinal and [dict(st, kind=0) for st in log] == [dict(st, kind=0) for st in rlog]
    return log


@pytest.mark.parametrize("name", TG.CASE_IDS)
def test_transit_catalogue_as_the_repeats_step(name):
    c, nodes, edges = hand_graph(name)
    for ms in sorted(c.expect["resolved"]):
        log = same_as_repeats(nodes, edges, (c.steps or []) + [(REPEATS, ms, 0)], c.reads, c.k)
        if (name, ms) in HAND:
            assert log[-1]["copies"] == HAND[(name, ms)][0]


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_graphs_as_the_repeats_step(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    edges = host_edges(nodes, presimp)
    same_as_repeats(nodes, edges, [(REPEATS, 1, 0)], reads, k, G.fake_bases(reads, G.L, seed))
    if seed in (1, 4, 7):
        same_as_repeats(nodes, edges, MIXED, reads, k, G.fake_bases(reads, G.L, seed))


@pytest.mark.parametrize("seed", [1, 4, 7])
def test_a_second_round_on_the_random_graphs_keeps_the_invariants(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    edges = host_edges(nodes, presimp)
    log, final = NR.simplify(nodes, edges, [(EDGES, 1, 0), (REPEATS, 1, 0), (TIPS, 3, 0), (NESTED, 1, 0), (NESTED, 1, 0), (COMPONENTS, 2, 0)], hashes(reads), k,
                             G.fake_bases(reads, G.L, seed))
    nested_invariants(nodes, edges, log, final)


# ---- base space: an error-free genome with the nested repeat ---------------------------------------------------------------------------------------------------
def genome_with_nested_repeat(seed, flank=4000, part=1000):
    """A xuy M1 xuy M2 u B: u (1,000 bases) occurs three times, x u y (3,000 bases) twice"""
    import random
    rnd = random.Random(seed)
    seq = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    x, u, y = seq(part), seq(part), seq(part)
    return seq(flank) + x + u + y + seq(flank) + x + u + y + seq(flank) + u + seq(flank)


NESTED_READS = dict(length=5000, step=250)      # long enough to span x u y with 2,000 bases to spare


@functools.lru_cache(maxsize=None)
def base_space_case():
    from oracle import oracle as O
    k, l, d, A = BASE_PARAMS
    genome = genome_with_nested_repeat(2)
    reads = tiled_reads(genome, **NESTED_READS)
    b, o, H = base_space_hashes(reads)
    g = O.Graph(k, l, d, A, already_hpc=True)
    assert g.ingest(b, o) == 0
    nodes = g.finalize(with_edges=False)
    return genome, reads, b, o, H, nodes, host_edges(nodes, 0.0)


def test_one_contig_through_the_nested_repeat_in_base_space():
    k = BASE_PARAMS[0]
    genome, reads, b, o, H, nodes, edges = base_space_case()
    plain = U.unitigs(nodes, edges, reads)
    assert pieces_of(genome, plain["seqs"]) and len(plain["walks"]) > 4
    log1, once = NR.simplify(nodes, edges, [(REPEATS, 2, 0)], H, k, reads)
    assert log1[0]["copies"] > k - 1 and len(log1[0]["resolved"]) == 1 and len(once["seqs"]) > 1 and pieces_of(genome, once["seqs"])
    log2, twice = NR.simplify(nodes, edges, [(REPEATS, 2, 0), (NESTED, 2, 0)], H, k, reads)
    assert log2[0] == log1[0] and len(log2[1]["resolved"]) == 1 and log2[1]["copies"] > 2 * log2[0]["copies"]      # x u y is copied, the copy of u in it included
    assert len(twice["seqs"]) == 1 and pieces_of(genome, twice["seqs"]) and len(twice["seqs"][0]) > len(genome) - 2 * 1000
    nested_invariants(nodes, edges, log2, twice)


# ---- the constant ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_python_mirror_and_the_header():
    from rust_mdbg_amd import api
    header = open(os.path.join(ROOT, "include", "mdbg_hip.h")).read()
    assert "#define MDBG_SIMPLIFY_NESTED 128u" in header and "PLACEMENT ON A LIST THAT HOLDS COPIES" in header
    assert api.MDBG_SIMPLIFY_NESTED == NESTED == NG.NESTED == 128
    arr, n = api.simplify_steps([(api.MDBG_SIMPLIFY_REPEATS, 2, 0), (api.MDBG_SIMPLIFY_NESTED, 2, 0)])
    assert n == 2 and (arr[1].kind, arr[1].max_nodes, arr[1].max_bases) == (128, 2, 0)
    assert len(api.MAGIC_SIMPLIFY_STEPS) == 14 and all(kind in (1, 2) for kind, _, _ in api.MAGIC_SIMPLIFY_STEPS)
    assert all(kind in (1, 64) for kind, _, _ in api.MAGIC_SUPERBUBBLE_STEPS)
