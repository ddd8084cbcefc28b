"""Tip clipping and simple-bubble popping without a GPU: the checker (tests/simplify_restatement.py) is itself checked on hand-made graphs with the
answer written out, by properties that follow from the rules on the fuzz graphs, and against a ground truth that needs no reference (planted
read-end errors and a planted minor allele: what is left stitches to pieces of the genome).  The GPU side is tests/test_gpu_simplify.py."""
import random

import numpy as np
import pytest

import simplify_restatement as S
import unitig_restatement as U
from oracle import oracle as O
from rust_mdbg_amd.api import MAGIC_SIMPLIFY_STEPS, MDBG_SIMPLIFY_BUBBLES, MDBG_SIMPLIFY_TIPS
from test_unitigs_cpu import assert_genome_substrings, fuzz_case, oracle_graph, synth_case

T, B = MDBG_SIMPLIFY_TIPS, MDBG_SIMPLIFY_BUBBLES
P, M = "+", "-"


def test_constants_and_default_schedule():
    assert (T, B) == (S.TIPS, S.BUBBLES) == (1, 2)
    # utils/magic_simplify, first gfatools line: -t 10,50000 -t 10,50000 -b 100000 -b 100000 -t 10,50000 -b 100000 x3 -t 10,50000 -b 100000 -t 10,50000 -b 1000000 -t 10,150000 -b 1000000
    t, b, b6 = (T, 10, 50000), (B, 0, 100000), (B, 0, 1000000)
    assert [tuple(s) for s in MAGIC_SIMPLIFY_STEPS] == [t, t, b, b, t, b, b, b, t, b, t, b6, (T, 10, 150000), b6]


def hand(abund, edges, length=None):
    """abund: {node index: abundance}; length: {node index: bases} (default 100 each; a walk's length is the sum: no overlaps in these toy graphs)"""
    idx = sorted(abund)
    nodes = dict(index=idx, abundance=[abund[i] for i in idx])
    ln = {i: 100 for i in idx}
    ln.update(length or {})
    return nodes, edges, (lambda walk: sum(ln[i] for i, _ in walk))


def run_hand(abund, edges, steps, length=None):
    nodes, edges, length_of = hand(abund, edges, length)
    log, final = S.simplify(nodes, edges, steps, length_of=length_of)
    return [sorted(st["nodes"]) for st in log], final["walks"]


def path(*ns):
    return [(a, P, b, P, 5) for a, b in zip(ns, ns[1:])]


FORK = path(1, 2, 3, 4, 5, 6, 7) + [(3, P, 8, P, 5)]                          # trunk 1-2-3, arms 4-5-6-7 and 8
FORK_AB = {1: 5, 2: 5, 3: 5, 4: 9, 5: 9, 6: 9, 7: 9, 8: 2}


def test_fork_with_a_short_and_a_long_arm():
    removed, walks = run_hand(FORK_AB, FORK, [(T, 2, 0)])
    assert removed == [[8]] and walks == [[(n, P) for n in range(1, 8)]]


def test_fork_whose_two_arms_are_both_small_tips_loses_only_the_weaker():
    removed, walks = run_hand(FORK_AB, FORK, [(T, 0, 0)])                  # no limit: trunk and both arms are candidates; the trunk is the only way into 4 and 8
    assert removed == [[8]] and walks == [[(n, P) for n in range(1, 8)]]
    ab = {**FORK_AB, **{8: 9}}                                            # equal mean abundance: the longer arm wins
    assert run_hand(ab, FORK, [(T, 0, 0)])[0] == [[8]]
    ab = {**FORK_AB, **{8: 10}}
    assert run_hand(ab, FORK, [(T, 0, 0)])[0] == [[4, 5, 6, 7]]
    ab = {**FORK_AB, **{8: 9}}                                            # equal abundance and length: the smaller unitig number (first node 4 < 8) wins
    assert run_hand(ab, FORK, [(T, 0, 0)], length={8: 400})[0] == [[8]]
    assert run_hand(ab, FORK, [(T, 0, 0)], length={8: 401})[0] == [[4, 5, 6, 7]]


def test_fork_given_on_the_other_strand():
    mirrored = [(b, P if ob == M else M, a, P if oa == M else M, ov) for a, oa, b, ob, ov in FORK]
    assert run_hand(FORK_AB, mirrored, [(T, 2, 0)])[0] == [[8]]
    joining = path(4, 3, 2, 1) + [(8, P, 3, P, 5), (7, P, 6, P, 5), (6, P, 5, P, 5), (5, P, 4, P, 5)]      # arms that END in the trunk: the dead end is the first vertex
    assert run_hand(FORK_AB, joining, [(T, 2, 0)])[0] == [[8]]


def test_tip_whose_attached_end_is_the_only_way_into_its_targets_is_kept():
    edges = [(1, P, 2, P, 5), (1, P, 3, P, 5)] + path(2, 4, 5, 6) + path(3, 7, 8, 9)
    removed, walks = run_hand({n: 3 for n in range(1, 10)}, edges, [(T, 1, 0)])
    assert removed == [[]] and len(walks) == 3
    edges.append((10, P, 2, P, 5))                                          # node 2 has a second way in, node 3 has not: 1 stays; 1 and 10 tie and 1 has the smaller number
    assert run_hand({n: 3 for n in range(1, 11)}, edges, [(T, 1, 0)])[0] == [[10]]
    edges.append((11, P, 3, P, 5))                                          # 1, 10 and 11 are all small tips: 10 is the best way into 2, 1 the best into 3, so only 11 goes
    removed, _ = run_hand({**{n: 3 for n in range(1, 12)}, **{10: 9, 11: 1}}, edges, [(T, 1, 0)])
    assert removed == [[11]]


def test_isolated_short_unitig_is_kept():
    removed, walks = run_hand({**FORK_AB, **{20: 1, 21: 1}}, FORK + path(20, 21), [(T, 2, 0)])
    assert removed == [[8]] and [(20, P), (21, P)] in walks
    assert run_hand({20: 1}, [], [(T, 0, 0), (B, 0, 0)]) == ([[], []], [[(20, P)]])


BUBBLE = path(0, 1, 2, 4, 5) + [(1, P, 3, P, 5), (3, P, 4, P, 5)]
BUBBLE_AB = {0: 5, 1: 5, 2: 7, 3: 3, 4: 5, 5: 5}


def test_two_branch_bubble_loses_the_weaker_branch():
    removed, walks = run_hand(BUBBLE_AB, BUBBLE, [(B, 0, 0)])
    assert removed == [[3]] and walks == [[(n, P) for n in (0, 1, 2, 4, 5)]]
    assert run_hand({**BUBBLE_AB, **{3: 8}}, BUBBLE, [(B, 0, 0)])[0] == [[2]]
    assert run_hand(BUBBLE_AB, BUBBLE, [(T, 0, 0)])[0] == [[]]            # no dead end but the flanks', which are the only way in


def test_three_branch_bubble_keeps_one():
    edges = BUBBLE + [(1, P, 6, P, 5), (6, P, 7, P, 5), (7, P, 4, P, 5)]
    removed, walks = run_hand({**BUBBLE_AB, **{6: 6, 7: 6}}, edges, [(B, 0, 0)])
    assert removed == [[3, 6, 7]] and walks == [[(n, P) for n in (0, 1, 2, 4, 5)]]
    assert run_hand({**BUBBLE_AB, **{6: 9, 7: 9}}, edges, [(B, 0, 0)])[0] == [[2, 3]]


def test_branch_between_a_vertex_and_its_complement_is_kept():
    edges = [(0, P, 1, P, 5), (1, P, 2, P, 5), (2, P, 1, M, 5), (1, P, 3, P, 5), (3, P, 1, M, 5)]
    removed, walks = run_hand({0: 5, 1: 5, 2: 7, 3: 3}, edges, [(B, 0, 0)])
    assert removed == [[]] and len(walks) == 3


def test_bubble_given_once_per_strand():
    flip = lambda o: P if o == M else M
    for pick in (lambda i: True, lambda i: i % 2 == 0, lambda i: i % 3 == 0):
        edges = [(b, flip(ob), a, flip(oa), ov) if pick(i) else (a, oa, b, ob, ov) for i, (a, oa, b, ob, ov) in enumerate(BUBBLE)]
        assert run_hand(BUBBLE_AB, edges, [(B, 0, 0)])[0] == [[3]]
    both = BUBBLE + [(b, flip(ob), a, flip(oa), ov) for a, oa, b, ob, ov in BUBBLE]
    assert run_hand(BUBBLE_AB, both, [(B, 0, 0)])[0] == [[3]]


def test_limits_at_the_boundary():
    two = path(1, 2, 3, 4, 5, 6, 7) + [(3, P, 8, P, 5), (8, P, 9, P, 5)]    # the short arm has two nodes, 200 bases
    ab = {**FORK_AB, **{9: 2}}
    assert run_hand(ab, two, [(T, 2, 0)])[0] == [[8, 9]] and run_hand(ab, two, [(T, 1, 0)])[0] == [[]]
    assert run_hand(ab, two, [(T, 0, 200)])[0] == [[8, 9]] and run_hand(ab, two, [(T, 0, 199)])[0] == [[]]
    assert run_hand(ab, two, [(T, 2, 200)])[0] == [[8, 9]] and run_hand(ab, two, [(T, 2, 199)])[0] == [[]] and run_hand(ab, two, [(T, 1, 200)])[0] == [[]]
    assert run_hand(BUBBLE_AB, BUBBLE, [(B, 1, 100)])[0] == [[3]]
    assert run_hand(BUBBLE_AB, BUBBLE, [(B, 0, 99)])[0] == [[]]
    assert run_hand(BUBBLE_AB, BUBBLE, [(B, 0, 100)], length={2: 101})[0] == [[]]     # the stronger branch is not small: it is no branch, nothing to compare with
    with pytest.raises(AssertionError):
        S.simplify(*hand(BUBBLE_AB, BUBBLE)[:2], [(3, 0, 0)], length_of=len)


# ---- properties on the fuzz graphs ------------------------------------------------------------------------------------------------------
SCHEDULES = {"magic": MAGIC_SIMPLIFY_STEPS, "tips": [(T, 10, 50000)], "bubbles": [(B, 0, 100000)], "tips then bubbles, no limits": [(T, 0, 0), (B, 0, 0)]}


def arc_sets(edges, alive):
    arcs = set()
    for u, v, _ in U.as_records(edges):
        if u[0] in alive and v[0] in alive:
            arcs.add((u, v))
            arcs.add((U.comp(v), U.comp(u)))
    return arcs


def check_properties(nodes, edges, reads, steps, log):
    alive = {int(i) for i in nodes["index"]}
    for (kind, mn, mb), st in zip(S.as_steps(steps), log):
        sub, recs = S.induced(nodes, edges, alive)
        cur = U.unitigs(sub, recs, reads)
        for w in cur["walks"]:                                              # whole unitigs of the step's current graph
            hit = [n in st["nodes"] for n, _ in w]
            assert all(hit) or not any(hit)
        gone = [i for i, w in enumerate(cur["walks"]) if w[0][0] in st["nodes"]]
        assert all(S.small(i, cur, mn, mb) for i in gone)
        after = alive - st["nodes"]
        assert st["nodes"] <= alive
        if kind == T:                                                       # no surviving vertex lost its last in-arc
            had = {b for _, b in arc_sets(edges, alive)}
            has = {b for _, b in arc_sets(edges, after)}
            assert {v for v in had if v[0] in after} == has
        else:                                                               # among the survivors no two small branches share a bubble
            succ, pred = S.arcs_of(recs)
            keys = [k for i, k in S.branches(cur, succ, pred, mn, mb).items() if i not in gone]
            assert len(keys) == len(set(keys))
        alive = after
    return alive


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("seed", range(6))
def test_properties_on_fuzz_graphs(seed, sched):
    k, l, d, A, reads = fuzz_case(seed)
    nodes, edges = oracle_graph(reads, k, l, d, A, 0.0)
    steps = SCHEDULES[sched]
    log, final = S.simplify(nodes, edges, steps, reads)
    alive = check_properties(nodes, edges, reads, steps, log)
    assert sorted(n for w in final["walks"] for n, _ in w) == sorted(alive)
    # the strand an edge record is written on does not matter
    rnd = random.Random(seed)
    flip = lambda o: P if o == M else M
    renamed = [(b[0], flip(b[1]), a[0], flip(a[1]), ov) if rnd.random() < 0.5 else (a[0], a[1], b[0], b[1], ov) for a, b, ov in U.as_records(edges)]
    log2, final2 = S.simplify(nodes, renamed, steps, reads)
    assert [st["nodes"] for st in log2] == [st["nodes"] for st in log]
    assert (final2["walks"], final2["seqs"], final2["kc_sum"], final2["circular"]) == (final["walks"], final["seqs"], final["kc_sum"], final["circular"])


def test_fuzz_graphs_reach_both_kinds():
    """seeds 0, 1, 3, 5 hold dead-end unitigs of <= 10 nodes, seeds 0 and 5 simple bubbles: the default schedule removes some of each there"""
    tips, bubbles = {}, {}
    for seed in (0, 1, 3, 5):
        k, l, d, A, reads = fuzz_case(seed)
        nodes, edges = oracle_graph(reads, k, l, d, A, 0.0)
        log, _ = S.simplify(nodes, edges, MAGIC_SIMPLIFY_STEPS, reads)
        tips[seed] = sum(len(st["unitigs"]) for st in log if st["kind"] == T)
        bubbles[seed] = sum(len(st["unitigs"]) for st in log if st["kind"] == B)
    assert all(tips[s] > 0 for s in (0, 1, 3, 5)), tips
    assert all(bubbles[s] > 0 for s in (0, 5)), bubbles


@pytest.mark.parametrize("seed", range(6))
def test_empty_schedule_is_the_unitig_list(seed):
    k, l, d, A, reads = fuzz_case(seed)
    nodes, edges = oracle_graph(reads, k, l, d, A, 0.01)
    log, final = S.simplify(nodes, edges, [], reads)
    assert log == [] and final == U.unitigs(nodes, edges, reads)


# ---- planted ground truth ---------------------------------------------------------------------------------------------------------------
PLANTED_PARAMS = (21, 12, 0.003, 2)
PLANTED_STEPS = [(T, 30, 0), (B, 0, 100000), (T, 30, 0)]


def planted_case(seed, what):
    """error-free reads of a random genome plus (tips) reads whose last 300 bases are random, each given min_abundance times, and / or (bubbles) reads
    tiled over a copy of the genome in which one minimizer every 20 kb carries a substitution, at half the depth of the true allele"""
    k, l, d, A = PLANTED_PARAMS
    reads, genome = synth_case(seed, 500)
    rnd = random.Random(seed)
    extra = []
    if "tips" in what:
        for i in rnd.sample(range(len(reads)), 12):
            bad = reads[i][:-300] + bytes(rnd.choice(b"ACGT") for _ in range(300))
            extra += [bad] * A
    if "bubbles" in what:
        g = np.frombuffer(genome.encode(), np.uint8)
        pos = O.sketch(g.copy(), np.array([0, len(g)], np.uint64), l, d)["pos"].tolist()
        alt = bytearray(genome.encode())
        last = 0
        for p in pos:
            if p >= last + 20000 and p < len(alt) - 20000:
                at = int(p) + l // 2
                alt[at] = {65: 67, 67: 71, 71: 84, 84: 65}[alt[at]]
                last = p
        alt = bytes(alt)
        for st in range(0, len(alt) - 15000 + 1, 1000):
            s = alt[st:st + 15000]
            extra.append(s if rnd.random() < 0.5 else U.revcomp(s.decode()).encode())
    return reads + extra, genome


@pytest.mark.parametrize("what", ["tips", "bubbles", "tips+bubbles"])
@pytest.mark.parametrize("seed", [1, 2])
def test_planted_errors_are_removed_and_the_rest_is_the_genome(seed, what):
    reads, genome = planted_case(seed, what)
    k, l, d, A = PLANTED_PARAMS
    nodes, edges = oracle_graph(reads, k, l, d, A, 0.0, hpc=True)
    plain = U.unitigs(nodes, edges, reads)
    rc = U.revcomp(genome)
    assert any(s not in genome and s not in rc for s in plain["seqs"])      # the planted errors are in the graph
    log, final = S.simplify(nodes, edges, PLANTED_STEPS, reads)
    assert_genome_substrings(final["names"], final["seqs"], final["length"], genome)
    assert len(final["walks"]) < len(plain["walks"])
    if "tips" in what:
        assert len(log[0]["unitigs"]) > 0
    if "bubbles" in what:
        assert len(log[1]["unitigs"]) > 0
    check_properties(nodes, edges, reads, PLANTED_STEPS, log)
