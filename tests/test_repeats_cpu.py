"""The repeat restatement (tests/repeats_restatement.py: the REPEATS step of include/mdbg_hip.h, mdbg_graph_simplify) pinned without a GPU: the hand-built
repeats of tests/transit_graphs.py with the figures written down beside them, two repeats behind an EDGES step, the recorded figures of three random graphs,
the step's invariants on the catalogue of tests/sketch_graphs.py and on every random graph, the schedules the library refuses, and the C side of the new step
kind.  The GPU side is tests/test_gpu_repeats.py."""
import functools
import os
import subprocess
from collections import Counter

import pytest

import repeats_restatement as RR
import sketch_graphs as G
import transit_graphs as TG
import unitig_restatement as U
from conftest import ROOT
from test_read_paths_cpu import hashes
from test_sketch_graphs_cpu import BY_NAME, host_edges, model_nodes, random_graph

TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS = RR.TIPS, RR.BUBBLES, RR.COMPONENTS, RR.EDGES, RR.REPEATS


def run(nodes, edges, steps, reads, k, strings=None):
    return RR.simplify(nodes, edges, steps, hashes(reads), k, strings, None if strings is not None else G.length_of_walk(nodes))


def check_invariants(nodes, edges, log, final):
    """include/mdbg_hip.h, the consequences of the step, on a restatement's or a library's result (final: walks_original, kc_sum, and copies if known)"""
    walks = final["walks_original"]
    arcs = set()
    for u, v, _ in U.as_records(edges):
        arcs.add((u, v))
        arcs.add((U.comp(v), U.comp(u)))
    for w in walks:                                  # consecutive entries are joined by an arc of the ORIGINAL edge list
        assert all((a, b) in arcs for a, b in zip(w, w[1:]))
    removed = sum(len(st["nodes"]) for st in log)
    copies = sum(st.get("copies", 0) for st in log)
    n_entries = sum(len(w) for w in walks)
    assert n_entries == len(nodes["index"]) - removed + copies            # the n_entries identity
    ab = {int(i): int(a) for i, a in zip(nodes["index"], nodes["abundance"])}
    assert final["kc_sum"] == [sum(ab[i] for i, _ in w) for w in walks]   # abundances are not divided
    seen = Counter(i for w in walks for i, _ in w)
    if removed == 0:                                 # a node of a resolved unitig with m strong keys occurs m times, every other node once
        assert sum(seen.values()) - len(seen) == copies and set(seen) == {int(i) for i in nodes["index"]}
    for st in log:
        if st["kind"] == REPEATS:
            assert st["nodes"] == set() and st["unitigs"] == [] and st["edges"] == 0
    return seen


# ---- the hand-built repeats: (case, min_support) -> (copies, entries of the unitigs that are left, sorted; unitig edge records left) ----------------------------
HAND = {("cross r=3", 1): (1, [13, 13], 0), ("cross r=3", 2): (1, [13, 13], 0), ("cross r=3", 3): (1, [13, 13], 0), ("cross r=3", 4): (0, [1, 6, 6, 6, 6], 8),
        ("cross r=8", 1): (6, [18, 18], 0), ("cross r=8", 4): (0, [6, 6, 6, 6, 6], 8),
        ("mixed", 1): (0, [3, 6, 6, 6, 6], 8), ("mixed", 2): (3, [15, 15], 0),
        ("three-way", 1): (4, [14, 14, 14], 0), ("three-way", 2): (4, [14, 14, 14], 0), ("three-way", 3): (0, [2, 6, 6, 6, 6, 6, 6], 12),
        ("long", 1): (4998, [5010, 5010], 0), ("long", 2): (0, [6, 6, 6, 6, 4998], 8),
        ("unspanned", 1): (0, [2, 6, 6, 6, 6], 8), ("three-way, one exit fewer", 1): (0, [2, 6, 6, 6, 6, 6], 10), ("ring", 1): (0, [6], 2),
        ("cross r=2", 1): (0, [6, 6, 6, 6], 8),
        # two repeats S1 and S2 of one entry behind [(EDGES, 2, 0)]: P1 S1 (A rr B) = 6 + 1 + 14, P2 S1 E1 = 6 + 1 + 6, (C rr D) S2 Q1 = 14 + 1 + 6, E2 S2 Q2 = 6 + 1 + 6
        ("break by a missing crossing", 1): (2, [13, 13, 21, 21], 0), ("break by a missing crossing", 3): (2, [13, 13, 21, 21], 0),
        ("break by a missing crossing", 4): (0, [1, 1, 6, 6, 6, 6, 6, 6, 14, 14], 16)}


@functools.lru_cache(maxsize=None)
def hand_graph(name):
    c = TG.BY_NAME[name]
    nodes = G.nodes_from_sketch(c.reads, c.k, G.L, c.A)
    return c, nodes, host_edges(nodes, c.presimp)


@pytest.mark.parametrize("name,ms", sorted(HAND))
def test_hand_built_repeats(name, ms):
    c, nodes, edges = hand_graph(name)
    copies, left, records = HAND[(name, ms)]
    log, final = run(nodes, edges, (c.steps or []) + [(REPEATS, ms, 0)], c.reads, c.k)
    assert (log[-1]["copies"], sorted(len(w) for w in final["walks"]), len(final["edges"]), final["copies"]) == (copies, left, records, copies)
    seen = check_invariants(nodes, edges, log, final)
    if copies == 0 and not c.steps:
        plain = U.unitigs(nodes, edges)
        assert final["walks"] == plain["walks"] == final["walks_original"] and final["edges"] == plain["edges"]
    if name == "three-way" and copies:                   # the repeat's two nodes occur three times, once per strong key
        assert sorted(seen.values())[-2:] == [3, 3] and sorted(seen.values())[-3] == 1
    if name == "cross r=3" and copies:
        assert final["copies"] == 1 and max(final["origin"]) == int(nodes["index"].max()) + 1


def test_many_crosses_side_by_side():
    reads = TG.many_crosses(300)
    nodes = G.nodes_from_sketch(reads, 3, G.L, 1)
    edges = host_edges(nodes, 0.0)
    log, final = run(nodes, edges, [(REPEATS, 1, 0)], reads, 3)
    assert len(U.unitigs(nodes, edges)["walks"]) == 1500
    assert (log[0]["copies"], len(final["walks"]), {len(w) for w in final["walks"]}, len(final["edges"])) == (300, 600, {9}, 0)
    check_invariants(nodes, edges, log, final)
    assert run(nodes, edges, [(REPEATS, 2, 0)], reads, 3)[0][0]["copies"] == 0


def test_no_resident_read_means_nothing_resolves():
    c, nodes, edges = hand_graph("cross r=8")
    log, final = RR.simplify(nodes, edges, [(REPEATS, 1, 0)], [], c.k, None, G.length_of_walk(nodes))
    assert log[0]["copies"] == 0 and final["walks"] == U.unitigs(nodes, edges)["walks"]


# ---- the random graphs: seed -> (copies, unitigs before and after, entries before and after, unitig edge records before and after) at min_support 1 ------------
RANDOM = {1: (5, 96, 101, 295, 300, 518, 518), 4: (15, 101, 105, 291, 306, 558, 534), 7: (7, 101, 99, 295, 302, 508, 484)}


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_graphs(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    edges = host_edges(nodes, presimp)
    plain = U.unitigs(nodes, edges)
    log, final = run(nodes, edges, [(REPEATS, 1, 0)], reads, k, G.fake_bases(reads, G.L, seed))
    check_invariants(nodes, edges, log, final)
    got = (log[0]["copies"], len(plain["walks"]), len(final["walks"]), sum(map(len, plain["walks"])), sum(map(len, final["walks"])), len(plain["edges"]), len(final["edges"]))
    if seed in RANDOM:
        assert got == RANDOM[seed] and log[0]["copies"] > 0
    else:
        assert log[0]["copies"] == 0 and final["walks"] == plain["walks"] and final["edges"] == plain["edges"]


MIXED = [(EDGES, 1, 0), (REPEATS, 1, 0), (TIPS, 3, 0), (BUBBLES, 0, 0), (COMPONENTS, 2, 0)]


@pytest.mark.parametrize("seed", [1, 4, 7])
def test_a_schedule_of_all_five_kinds(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    edges = host_edges(nodes, presimp)
    log, final = run(nodes, edges, MIXED, reads, k, G.fake_bases(reads, G.L, seed))
    check_invariants(nodes, edges, log, final)
    assert log[0]["edges"] > 0 and [st["kind"] for st in log] == [s[0] for s in MIXED]


@pytest.mark.parametrize("name", G.CASE_IDS)
def test_invariants_on_the_catalogue(name):
    c, nodes = BY_NAME[name], model_nodes(name)
    edges = host_edges(nodes, c.presimps[0])
    for ms in (1, 2):
        log, final = run(nodes, edges, [(REPEATS, ms, 0)], c.reads, c.k)
        check_invariants(nodes, edges, log, final)


# ---- base space: an error-free genome with one two-copy repeat, longer than k - 1 minimizers and shorter than the reads ----------------------------------------
BASE_PARAMS = (5, 10, 0.02, 2)                 # k, l, density, min_abundance; reads_already_hpc: the random bases are taken as they are


def genome_with_repeat(seed, flank=4000, repeat=1000):
    import random
    rnd = random.Random(seed)
    seq = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    r = seq(repeat)
    return seq(flank) + r + seq(flank) + r + seq(flank)


def tiled_reads(genome, length=3000, step=250):
    """every read spans the repeat or lies beside it; every second one is sequenced from the other strand"""
    out = []
    for i, a in enumerate(range(0, len(genome) - length + 1, step)):
        s = genome[a:a + length]
        out.append((U.revcomp(s) if i % 2 else s).encode())
    return out


def pieces_of(genome, seqs):
    rc = U.revcomp(genome)
    return all(s in genome or s in rc for s in seqs)


def base_space_hashes(reads):
    from oracle import oracle as O
    k, l, d, A = BASE_PARAMS
    b, o = O.concat_reads(reads)
    sk = O.sketch(b, o, l, d, already_hpc=True)
    off = sk["off"].tolist()
    return b, o, [sk["hashes"][x:y].tolist() for x, y in zip(off, off[1:])]


def test_a_contig_crosses_the_repeat_in_base_space():
    from oracle import oracle as O
    k, l, d, A = BASE_PARAMS
    genome = genome_with_repeat(1)
    reads = tiled_reads(genome)
    b, o, H = base_space_hashes(reads)
    g = O.Graph(k, l, d, A, already_hpc=True)
    assert g.ingest(b, o) == 0
    nodes = g.finalize(with_edges=False)
    edges = host_edges(nodes, 0.0)
    plain = U.unitigs(nodes, edges, reads)
    log, final = RR.simplify(nodes, edges, [(REPEATS, 2, 0)], H, k, reads)
    assert len(plain["walks"]) == 4 and pieces_of(genome, plain["seqs"])           # the two flanks, the repeat, the stretch between its copies
    assert log[0]["copies"] == len(plain["walks"][log[0]["resolved"][0]]) > k - 1 and len(log[0]["resolved"]) == 1
    assert len(final["seqs"]) == 1 and pieces_of(genome, final["seqs"]) and len(final["seqs"][0]) > max(len(s) for s in plain["seqs"]) + 2 * 1000
    check_invariants(nodes, edges, log, final)


# ---- what the library refuses -----------------------------------------------------------------------------------------------------------------------------------
REFUSED = ([(REPEATS, 0, 0)], [(REPEATS, 1, 5)], [(REPEATS, 1, 0), (TIPS, 0, 0), (REPEATS, 1, 0)], [(REPEATS, 1, 0), (EDGES, 1, 0)])


def test_the_checker_refuses_what_the_library_refuses():
    c, nodes, edges = hand_graph("cross r=3")
    for bad in REFUSED + ([(32, 1, 0)],):
        with pytest.raises(AssertionError):
            run(nodes, edges, bad, c.reads, c.k)
    run(nodes, edges, [(EDGES, 1, 0), (REPEATS, 1, 0), (TIPS, 0, 0)], c.reads, c.k)      # an EDGES step IN FRONT of the REPEATS step is fine


def test_python_mirror_and_the_c99_header(tmp_path):
    """the constant in the header and in api; the four refused schedules written as C step arrays against the header (without a GPU no context exists, so the
    call answers MDBG_E_PARAM for the null context: the refusals themselves are tests/test_gpu_repeats.py's)"""
    from rust_mdbg_amd import api
    header = open(os.path.join(ROOT, "include", "mdbg_hip.h")).read()
    assert "#define MDBG_SIMPLIFY_REPEATS 16u" in header
    assert api.MDBG_SIMPLIFY_REPEATS == REPEATS == 16
    arr, n = api.simplify_steps([(api.MDBG_SIMPLIFY_EDGES, 2, 0), (api.MDBG_SIMPLIFY_REPEATS, 2, 0)])
    assert n == 2 and (arr[1].kind, arr[1].max_nodes, arr[1].max_bases) == (16, 2, 0)
    assert len(api.MAGIC_SIMPLIFY_STEPS) == 14 and all(kind in (1, 2) for kind, _, _ in api.MAGIC_SIMPLIFY_STEPS)
    src = tmp_path / "repeats_step.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mdbg_hip.h"\n'
                   "int main(void) {\n"
                   "    mdbg_simplify_step a[] = {{MDBG_SIMPLIFY_REPEATS, 0, 0}};\n"
                   "    mdbg_simplify_step b[] = {{MDBG_SIMPLIFY_REPEATS, 1, 5}};\n"
                   "    mdbg_simplify_step c[] = {{MDBG_SIMPLIFY_REPEATS, 1, 0}, {MDBG_SIMPLIFY_TIPS, 0, 0}, {MDBG_SIMPLIFY_REPEATS, 1, 0}};\n"
                   "    mdbg_simplify_step d[] = {{MDBG_SIMPLIFY_REPEATS, 1, 0}, {MDBG_SIMPLIFY_EDGES, 1, 0}};\n"
                   "    mdbg_unitig_list ul; mdbg_simplify_stats st;\n"
                   "    int ra = mdbg_graph_simplify(NULL, a, 1, &ul, &st), rb = mdbg_graph_simplify(NULL, b, 1, &ul, &st);\n"
                   "    int rc = mdbg_graph_simplify_device(NULL, c, 3, &ul, &st), rd = mdbg_graph_simplify_device(NULL, d, 2, &ul, &st);\n"
                   '    printf("%u %d %d %d %d %u\\n", a[0].kind, ra, rb, rc, rd, (unsigned)MDBG_ABI_VERSION);\n    return 0;\n}\n')
    exe = str(tmp_path / "repeats_step")
    lib = os.path.join(ROOT, "rust_mdbg_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib, "-lmdbg_hip", "-Wl,-rpath," + lib,
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["16", "-1", "-1", "-1", "-1", "3"]
