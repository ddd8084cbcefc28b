"""The superbubble restatement (tests/superbubble_restatement.py: the SUPERBUBBLES step of include/mdbg_hip.h, mdbg_graph_simplify) pinned without a GPU: the
hand-built catalogue of tests/superbubble_graphs.py against the removed sets written beside it, the restatement against a brute force that enumerates every
(s, t) pair and every path on small random graphs, how often that family holds a bubble the BUBBLES rule cannot pop, the braid in base space, the Python and
C side of the new step kind.  The GPU side is tests/test_gpu_superbubbles.py."""
import functools
import os
import random
import subprocess
from fractions import Fraction

import pytest

import simplify_restatement as S
import sketch_graphs as G
import superbubble_graphs as SG
import superbubble_restatement as SR
import unitig_restatement as U
from conftest import ROOT
from test_repeats_cpu import BASE_PARAMS, pieces_of, tiled_reads
from test_sketch_graphs_cpu import host_edges

TIPS, BUBBLES, SUPERBUBBLES = 1, 2, 64
SB = (SUPERBUBBLES, 0, 0)


def graph_of(reads, k=SG.K, A=SG.A):
    nodes = G.nodes_from_sketch(reads, k, G.L, A)
    return nodes, host_edges(nodes, 0.0)


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SG.CASE_IDS)
def test_catalogue_against_the_hand_written_removed_sets(name):
    c = SG.BY_NAME[name]
    nodes, edges = graph_of(c.reads, c.k, c.A)
    for steps in c.schedules:
        log, final = SR.simplify(nodes, edges, steps, None, G.length_of_walk(nodes))
        want = c.expect.get("removed", {}).get(tuple(steps))
        if want is not None:
            assert [sorted(x["nodes"]) for x in log] == want, steps
        assert sum(len(w) for w in final["walks"]) == nodes["n_nodes"] - sum(len(x["nodes"]) for x in log)
    assert c.expect.get("removed") or name.startswith("odd ")


def test_what_the_catalogue_is_there_for():
    names = set(SG.CASE_IDS)
    assert {"braid", "ladder", "nested", "back to back", "interior dead end", "in-arc from outside", "out-arc to outside", "inversion", "interior cycle", "sink is the source",
            "braid, all equal", "braid, minus side", "fan of 64", "fan of 65", "hub", "simple bubble"} <= names
    braid = SG.BY_NAME["braid"]
    nodes, edges = graph_of(braid.reads)
    cur, _ = S.current(nodes, edges, set(nodes["index"].tolist()), None, G.length_of_walk(nodes))
    assert sorted(len(w) for w in cur["walks"]) == [1, 1, 2, 3, 3, 4, 4]                # source, sink and five unitigs between them
    succ, pred = S.arcs_of(S.induced(nodes, edges, set(nodes["index"].tolist()))[1])
    keys = list(S.branches(cur, succ, pred, 0, 0).values())
    assert len(set(keys)) == len(keys)                                                  # no two branches share a (p, q) key: the BUBBLES rule has nothing to compare
    report = []
    SR.simplify(nodes, edges, [SB], None, G.length_of_walk(nodes), report=report)
    (s, t, I, keep), = report[0]["applied"]
    assert len(I) == 5 and len(keep) == 5
    nodes, edges = graph_of(SG.BY_NAME["fan of 64"].reads)
    report = []
    SR.simplify(nodes, edges, [SB], None, G.length_of_walk(nodes), report=report)
    assert len(report[0]["applied"][0][2]) == 64 == SR.MAX_UNITIGS                       # (f) is met exactly


# ---- an independent brute force: every (s, t) pair, every path ------------------------------------------------------------------------------------------------
def brute_force(cur, max_nodes, max_bases):
    """-> the unitigs the step removes, from path enumeration alone"""
    succ, pred = {}, {}
    for a, oa, b, ob, _ in cur["edges"]:
        for x, y in (((a, oa), (b, ob)), ((b, "-" if ob == "+" else "+"), (a, "-" if oa == "+" else "+"))):
            succ.setdefault(x, set()).add(y)
            pred.setdefault(y, set()).add(x)
    vertices = [(u, o) for u in range(len(cur["walks"])) for o in "+-"]

    def all_paths(s, t):
        """every walk from s that stops at t; None if one of them ends elsewhere or comes back to a vertex it has seen"""
        out, stack = [], [[s]]
        while stack:
            p = stack.pop()
            if p[-1] == t:
                out.append(p)
                continue
            nxt = succ.get(p[-1], ())
            if not nxt or any(y in p for y in nxt):
                return None
            stack.extend(p + [y] for y in nxt)
            if len(stack) + len(out) > 20000:
                return None
        return out

    def bubble(s, t):
        if s == t or len(succ.get(s, ())) < 2:
            return None
        ps = all_paths(s, t)
        if not ps:
            return None
        I = {x for p in ps for x in p[1:-1]}
        members = I | {s, t}
        if not I or len(I) > 64 or len({x[0] for x in members}) != len(members) or s in succ.get(t, ()):
            return None
        if any(y not in I and y != s for x in I | {t} for y in pred.get(x, ())):
            return None
        return I, ps
    found = {(s, t): b for s in vertices for t in vertices for b in [bubble(s, t)] if b}
    minimal = {(s, t): b for (s, t), b in found.items() if not any((s, t2) in found for t2 in b[0])}
    mean = lambda x: Fraction(cur["kc_sum"][x[0]], len(cur["walks"][x[0]]))
    fitting = {}
    for (s, t), (I, ps) in minimal.items():
        if (max_nodes == 0 or sum(len(cur["walks"][u]) for u, _ in I) <= max_nodes) and (max_bases == 0 or sum(cur["length"][u] for u, _ in I) <= max_bases):
            fitting[(s, t)] = (I, ps)
    J = {v for I, _ in fitting.values() for x in I for v in (x, U.comp(x))}
    gone = set()
    for (s, t), (I, ps) in fitting.items():
        if s in J or t in J or (s[0], s[1] == "-") > (t[0], t[1] == "+"):           # not applied, or the other reading is the canonical one
            continue

        @functools.lru_cache(None)
        def val(x):
            if x == s:
                return None                                                          # +infinity
            through = val(best(x))
            return mean(x) if through is None else min(mean(x), through)

        def best(x):
            inf = [y for y in pred[x] if y == s]
            return inf[0] if inf else max(pred[x], key=lambda y: (val(y), mean(y), cur["length"][y[0]], -y[0]))
        keep, x = set(), t
        while x != s:
            x = best(x)
            keep.add(x)
        gone |= {x[0] for x in I - keep}
    return gone


RANDOM_SEEDS = list(range(40))
# the seeds whose graph holds an applied bubble of three or more unitigs inside that the BUBBLES rule leaves alone (measured with the restatement)
BRANCHING = {0, 5, 6, 8, 9, 10, 11, 15, 16, 18, 20, 21, 24, 26, 27, 31, 34, 35, 36, 37, 39}


def small_case(seed):
    reads = SG.random_braids(seed)
    return reads, graph_of(reads)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_restatement_equals_brute_force(seed):
    reads, (nodes, edges) = small_case(seed)
    alive = set(nodes["index"].tolist())
    cur, recs = S.current(nodes, edges, alive, None, G.length_of_walk(nodes))
    for mn, mb in ((0, 0), (6, 0), (0, 1200)):
        assert SR.superbubbles_to_remove(cur, mn, mb) == brute_force(cur, mn, mb), (seed, mn, mb)
    SR.simplify(nodes, edges, [(TIPS, 0, 0), SB, (BUBBLES, 0, 0), SB], None, G.length_of_walk(nodes))      # the driver's assertions on every step


def test_the_random_family_holds_bubbles_only_this_step_pops():
    got = set()
    sizes = []
    for seed in RANDOM_SEEDS:
        reads, (nodes, edges) = small_case(seed)
        cur, recs = S.current(nodes, edges, set(nodes["index"].tolist()), None, G.length_of_walk(nodes))
        sizes.append(len(cur["walks"]))
        succ, pred = S.arcs_of(recs)
        simple = S.bubbles_to_remove(cur, succ, pred, 0, 0)
        report = []
        SR.superbubbles_to_remove(cur, 0, 0, report)
        if any(len(I) >= 3 and not ({x[0] for x in I} & simple) for s, t, I, keep in report[0]["applied"]):
            got.add(seed)
    print("unitigs per graph:", sizes, "branching:", sorted(got))
    assert max(sizes) <= 12
    assert got == BRANCHING and 4 * len(got) >= len(RANDOM_SEEDS)


# ---- base space -------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def braid_genomes(seed=11, length=9000, apart=2):
    """a random genome and two variants of one base each, in the l-mers of two minimizers `apart` < k places from each other"""
    from oracle import oracle as O
    k, l, d, A = BASE_PARAMS
    rnd = random.Random(seed)
    genome = "".join(rnd.choice("ACGT") for _ in range(length))

    def sketch(s):
        b, o = O.concat_reads([s.encode()])
        sk = O.sketch(b, o, l, d, already_hpc=True)
        return sk["hashes"].tolist(), sk["pos"].tolist()
    H, P = sketch(genome)
    assert apart < k and len(H) > 4 * k

    def variant(i):
        at = P[i] + l // 2
        v = genome[:at] + {"A": "C", "C": "G", "G": "T", "T": "A"}[genome[at]] + genome[at + 1:]
        Hv, _ = sketch(v)
        assert Hv != H and Hv[:i - 1] == H[:i - 1] and Hv[-(len(H) - i - 2):] == H[-(len(H) - i - 2):]      # the sketch changes there and nowhere else
        return v
    return genome, variant(len(H) // 2), variant(len(H) // 2 + apart)


def test_the_braid_in_base_space():
    from oracle import oracle as O
    from rust_mdbg_amd import api
    k, l, d, A = BASE_PARAMS
    genome, h1, h2 = braid_genomes()
    reads = tiled_reads(genome) + tiled_reads(h1, step=1000) + tiled_reads(h2, step=1000)
    b, o = O.concat_reads(reads)
    g = O.Graph(k, l, d, A, already_hpc=True)
    assert g.ingest(b, o) == 0
    nodes = g.finalize(with_edges=False)
    edges = host_edges(nodes, 0.0)
    log, usual = SR.simplify(nodes, edges, api.MAGIC_SIMPLIFY_STEPS, reads)
    assert len(usual["walks"]) >= 5 and not any(x["nodes"] for x in log)               # tips and simple bubbles: nothing to do, the contig ends at the source
    log, final = SR.simplify(nodes, edges, api.MAGIC_SUPERBUBBLE_STEPS, reads)
    assert len(final["seqs"]) == 1 and pieces_of(genome, final["seqs"]) and len(final["seqs"][0]) > max(len(s) for s in usual["seqs"])


# ---- the public side --------------------------------------------------------------------------------------------------------------------------------------------
def test_python_mirror_and_the_header():
    from rust_mdbg_amd import api
    header = open(os.path.join(ROOT, "include", "mdbg_hip.h")).read()
    assert "#define MDBG_SIMPLIFY_SUPERBUBBLES 64u" in header and "#define MDBG_SUPERBUBBLE_MAX_UNITIGS 64u" in header
    assert api.MDBG_SIMPLIFY_SUPERBUBBLES == SUPERBUBBLES == SR.SUPERBUBBLES == 64 and api.MDBG_SUPERBUBBLE_MAX_UNITIGS == SR.MAX_UNITIGS == 64
    arr, n = api.simplify_steps([(api.MDBG_SIMPLIFY_TIPS, 10, 50000), (api.MDBG_SIMPLIFY_SUPERBUBBLES, 7, 100000)])
    assert n == 2 and (arr[1].kind, arr[1].max_nodes, arr[1].max_bases) == (64, 7, 100000)
    magic, sup = api.MAGIC_SIMPLIFY_STEPS, api.MAGIC_SUPERBUBBLE_STEPS
    assert len(sup) == len(magic) == 14 and all(kind in (1, 2) for kind, _, _ in magic)
    assert [(64 if kind == 2 else kind, mn, mb) for kind, mn, mb in magic] == [tuple(s) for s in sup] and sum(kind == 64 for kind, _, _ in sup) == 8


def test_the_c_program_parses_the_new_option(tmp_path):
    from test_gpu_unitigs import build_cli
    exe = build_cli(tmp_path)
    for args, said in ((["-B", "5"], "-B wants N,L"), (["-B", "5,x"], "bad or too many"), (["-B", "5,100000"], "[-B N,L]")):      # (no input file: the usage line)
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 2 and said in r.stderr, (args, r.stderr)
