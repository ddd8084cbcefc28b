"""Unitigs and base-space contigs without a GPU: the checker (tests/unitig_restatement.py) is itself checked by brute force and against a
ground truth that needs no reference (error-free reads: every contig is a piece of the genome), and libmdbg_emit's stitching and
writers (mdbg_emit_contigs_*) are fed the checker's unitigs through a copy plan derived here.  The GPU side is tests/test_gpu_unitigs.py."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import unitig_restatement as U
from conftest import GOLDEN
from oracle import oracle as O
from test_gpu_fuzz import fuzz_reads

EDGE_CASES = [(2, 8, 0.03, 1), (3, 8, 0.03, 1), (5, 10, 0.01, 2), (7, 12, 0.008, 2), (4, 6, 0.05, 3), (12, 12, 0.01, 1)]      # the parameter list of tests/test_gpu_edges.py


def fuzz_case(seed):
    rnd = random.Random(500 + seed)
    k, l, d, A = rnd.choice(EDGE_CASES)
    reads = fuzz_reads(rnd, n_reads=200, genome_len=rnd.choice([3000, 30000]), mean_len=4000, err=rnd.choice([0.0, 0.01]), p_lower=0.0, p_n=0.0,
                       p_hp=rnd.choice([0.0, 0.02]))
    return k, l, d, A, reads


def oracle_graph(reads, k, l, d, A, presimp, hpc=False):
    g = O.Graph(k, l, d, A, already_hpc=hpc, presimp=presimp)
    b, o = O.concat_reads(reads)
    assert g.ingest(b, o) == 0
    nodes = g.finalize(with_edges=True)
    edges = dict(n1=nodes["edge_n1"], o1=nodes["edge_o1"], n2=nodes["edge_n2"], o2=nodes["edge_o2"], overlap=nodes["edge_overlap"])
    return nodes, edges


def plan_of(u, nodes):
    """the restatement's walks as the arrays of mdbg_unitig_list, with the copy plan by the rule of include/mdbg_hip.h (the test's own derivation)"""
    row = {int(x): i for i, x in enumerate(nodes["index"])}
    f = {n: [] for n in ("node", "ori", "src_read", "src_begin", "len", "revcomp", "dst_offset")}
    offsets, length = [0], []
    for w in u["walks"]:
        at = 0
        for j, (idx, o) in enumerate(w):
            i = row[idx]
            a, b, rev = int(nodes["src_start"][i]), int(nodes["src_end"][i]), bool(nodes["reversed"][i])
            s0, s1 = (int(x) for x in nodes["shift_full"][i])
            if j == 0:
                begin, n = a, b - a
            else:
                n = min(s1 if o == "+" else s0, b - a)
                begin = b - n if (o == "-") == rev else a
            for name, val in (("node", idx), ("ori", ord(o)), ("src_read", int(nodes["src_read"][i])), ("src_begin", begin), ("len", n),
                              ("revcomp", int(rev) + (o == "-")), ("dst_offset", at)):
                f[name].append(val)
            at += n
        offsets.append(len(f["node"]))
        length.append(at)
    e = u["edges"]
    return dict(f, offsets=offsets, length=length, kc_sum=u["kc_sum"], circular=[int(c) for c in u["circular"]], n_unitigs=len(u["walks"]), n_entries=len(f["node"]),
                edges=dict(n1=[x[0] for x in e], o1=[ord(x[1]) for x in e], n2=[x[2] for x in e], o2=[ord(x[3]) for x in e], overlap=[x[4] for x in e]))


def brute_check(index, edges, walks, circ, uedges):
    """the definition checked without the restatement's bookkeeping: degrees are counted over the distinct arc set by scanning it"""
    recs = U.as_records(edges)
    arcs = set()
    for u, v, _ in recs:
        arcs.add((u, v))
        arcs.add((U.comp(v), U.comp(u)))
    out_of, in_of = {}, {}
    for a, b in arcs:
        out_of.setdefault(a, []).append(b)
        in_of.setdefault(b, []).append(a)
    outs = lambda x: out_of.get(x, [])
    ins = lambda x: in_of.get(x, [])
    link = lambda a, b: outs(a) == [b] and ins(b) == [a] and a[0] != b[0]
    assert sorted(i for w in walks for i, _ in w) == sorted(int(i) for i in index)            # every node on exactly one unitig, once
    assert [w[0][0] for w in walks] == sorted(w[0][0] for w in walks)
    inner = set()
    for w, c in zip(walks, circ):
        assert all(link(a, b) for a, b in zip(w, w[1:]))
        for a, b in zip(w, w[1:]):
            inner.add((a, b))
            inner.add((U.comp(b), U.comp(a)))
        if c:
            assert link(w[-1], w[0]) and w[0][1] == "+" and w[0][0] == min(i for i, _ in w)
        else:
            assert not any(link(p, w[0]) for p in ins(w[0])) and not any(link(w[-1], q) for q in outs(w[-1]))      # cannot be extended at either end
            assert w[0][0] < w[-1][0] or (len(w) == 1 and w[0][1] == "+")
    ends = {}
    for i, w in enumerate(walks):
        ends[(i, "+")] = (w[0], w[-1])
        ends[(i, "-")] = (U.comp(w[-1]), U.comp(w[0]))
    kept = [(u, v, ov) for u, v, ov in recs if (u, v) not in inner]
    assert len(kept) == len(uedges)
    for (u, v, ov), (a, oa, b, ob, ov2) in zip(kept, uedges):                                   # each non-interior record once, in order
        assert ends[(a, oa)][1] == u and ends[(b, ob)][0] == v and ov == ov2


@pytest.mark.parametrize("presimp", [0.0, 0.01, 0.5])
@pytest.mark.parametrize("seed", range(6))
def test_restatement_structure_on_fuzz_graphs(seed, presimp):
    k, l, d, A, reads = fuzz_case(seed)
    nodes, edges = oracle_graph(reads, k, l, d, A, presimp)
    walks, circ, ue = U.compact(nodes["index"], edges)
    brute_check(nodes["index"], edges, walks, circ, ue)


P, M = "+", "-"
HAND = {
    "isolated node": ([7], [], [[(7, P)]], [False], []),
    "path, one direction of each edge only": ([1, 2, 3], [(1, P, 2, P, 5), (2, P, 3, M, 5)], [[(1, P), (2, P), (3, M)]], [False], []),
    "branch": ([1, 2, 3], [(1, P, 2, P, 5), (1, P, 3, P, 5)], [[(1, P)], [(2, P)], [(3, P)]], [False] * 3, [(0, P, 1, P, 5), (0, P, 2, P, 5)]),
    "duplicate records": ([1, 2], [(1, P, 2, P, 5), (1, P, 2, P, 5), (2, M, 1, M, 4)], [[(1, P), (2, P)]], [False], []),
    "self-loop a+ -> a+": ([4, 5], [(4, P, 4, P, 3), (5, P, 4, P, 2)], [[(4, P)], [(5, P)]], [False, False], [(0, P, 0, P, 3), (1, P, 0, P, 2)]),
    "hairpin a+ -> a-": ([4, 5], [(4, P, 4, M, 3), (5, P, 4, P, 2)], [[(4, M), (5, M)]], [False], [(0, M, 0, P, 3)]),
    "3-cycle": ([3, 1, 2], [(2, P, 3, P, 9), (3, P, 1, P, 9), (1, P, 2, P, 9)], [[(1, P), (2, P), (3, P)]], [True], [(0, P, 0, P, 9)]),
    "2-cycle": ([8, 6], [(8, M, 6, P, 2), (6, P, 8, M, 2)], [[(6, P), (8, M)]], [True], [(0, P, 0, P, 2)]),
    "2-cycle given on the mirror side": ([8, 6], [(8, P, 6, M, 2), (6, M, 8, P, 2)], [[(6, P), (8, M)]], [True], [(0, M, 0, M, 2)]),
    "path whose canonical orientation is the mirror": ([1, 2, 3], [(3, P, 2, M, 5), (2, M, 1, P, 5)], [[(1, M), (2, P), (3, M)]], [False], []),
}


@pytest.mark.parametrize("case", sorted(HAND))
def test_restatement_on_hand_made_edge_lists(case):
    index, edges, walks, circ, uedges = HAND[case]
    got = U.compact(index, edges)
    assert got == (walks, circ, uedges)
    brute_check(index, edges, *got)


def synth_case(seed, n):
    from rust_mdbg_amd import synth
    glen = 250000
    reads = synth.synth_reads(seed, glen, n, mean_len=15000, sd_len=1500, min_len=8000, max_len=25000, err_ppm=0)
    genome = "".join("ACGT"[synth.rnd3(seed, p, 0x47) >> 62] for p in range(glen))
    return reads, genome


def assert_genome_substrings(names, seqs, lengths, genome):
    rc = U.revcomp(genome)
    for nm, s, ln in zip(names, seqs, lengths):
        assert ln == len(s) > 0, nm
        assert s in genome or s in rc, "%s (%d bases) is not a piece of the genome" % (nm, len(s))          # no unitig is exempt


@pytest.mark.parametrize("n", [500, 70])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_error_free_reads_stitch_to_pieces_of_the_genome(seed, n):
    """ground truth that needs no reference: reads without errors and without homopolymer compression (reads_already_hpc: with HPC on the reference's
    own rule cuts pieces in raw coordinates that need not abut, include/mdbg_hip.h) -> every unitig is an exact substring of the genome or of its
    reverse complement"""
    reads, genome = synth_case(seed, n)
    nodes, edges = oracle_graph(reads, 21, 12, 0.003, 2, 0.01, hpc=True)
    u = U.unitigs(nodes, edges, reads)
    assert_genome_substrings(u["names"], u["seqs"], u["length"], genome)
    if n == 500:
        assert len(u["walks"]) == 1 and 1400 < len(u["walks"][0]) < 1700 and 249000 < u["length"][0] < 250000
    else:
        assert 6 <= len(u["walks"]) <= 7 and 440 < max(len(w) for w in u["walks"]) < 500
    assert not any(u["circular"])


def parse_gfa(text):
    S, L = [], []
    lines = text.split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    for ln in lines[1:-1]:
        f = ln.split("\t")
        if f[0] == "S":
            assert len(f) == 5 and f[3].startswith("LN:i:") and f[4].startswith("mc:f:")
            S.append((f[1], f[2], int(f[3][5:]), f[4][5:]))
        else:
            assert f[0] == "L" and len(f) == 6 and f[5].endswith("M")
            L.append((f[1], f[2], f[3], f[4], int(f[5][:-1])))
    return S, L


def emit_case():
    """a graph with several unitigs, both orientations, reversed nodes and unitig edges: fuzz seed 3 of the edge tests, without presimp"""
    k, l, d, A, reads = fuzz_case(3)
    nodes, edges = oracle_graph(reads, k, l, d, A, 0.0)
    return reads, nodes, U.unitigs(nodes, edges, reads)


def test_emit_contigs_stitching_and_writers(tmp_path):
    """libmdbg_emit (mdbg_emit_contigs_*) through ctypes == the restatement's strings; fails without the feature: the symbols are absent"""
    from rust_mdbg_amd import emit as E
    reads, nodes, u = emit_case()
    assert len(u["walks"]) > 3 and u["edges"] and any(o == "-" for w in u["walks"] for _, o in w[1:]) and any(len(w) > 2 for w in u["walks"])
    plan = plan_of(u, nodes)
    assert plan["length"] == u["length"]
    b, o = O.concat_reads(reads)
    gfa, fa, fa2 = (str(tmp_path / x) for x in ("u.gfa", "u.fa", "u2.fa"))
    with E.Emitter().contigs(plan, [(b, o, 0)], gfa, fa, n_nodes=len(nodes["index"])) as c:
        assert [s.decode() for s in c.sequences()] == u["seqs"]
        cut = sorted(u["length"])[len(u["length"]) // 2]
        c.write_fasta(fa2, cut)
    text = open(gfa).read()
    assert text == U.gfa_text(u)
    S, L = parse_gfa(text)
    assert [s[0] for s in S] == u["names"] and [s[1] for s in S] == u["seqs"] and [s[2] for s in S] == u["length"]
    assert [s[3] for s in S] == ["%.1f" % (kc / len(w)) for kc, w in zip(u["kc_sum"], u["walks"])]
    assert L == [(u["names"][a], oa, u["names"][b], ob, ov) for a, oa, b, ob, ov in u["edges"]]
    assert open(fa).read() == U.fasta_text(u)
    assert open(fa2).read() == U.fasta_text(u, cut) != U.fasta_text(u)
    # batches split at arbitrary record boundaries and fed in any order give the same files
    rnd = random.Random(9)
    cuts = sorted(set([0, len(reads)] + [rnd.randrange(len(reads)) for _ in range(7)]))
    parts = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
    rnd.shuffle(parts)
    batches = [O.concat_reads(reads[lo:hi]) + (lo,) for lo, hi in parts]
    g2, f2 = str(tmp_path / "v.gfa"), str(tmp_path / "v.fa")
    E.Emitter().contigs(plan, batches, g2, f2).close()
    assert open(g2).read() == text and open(f2).read() == open(fa).read()
    # a missing batch: the writers refuse
    used = sorted({int(r) for r in plan["src_read"]})
    miss = next(i for i, (lo, hi) in enumerate(parts) if any(lo <= r < hi for r in used))
    with E.Contigs(plan) as c:
        for i, bt in enumerate(batches):
            if i != miss:
                c.add_batch(*bt)
        for call in (lambda: c.write_gfa(g2), lambda: c.write_fasta(f2), c.sequences):
            with pytest.raises(E.MdbgError) as ei:
                call()
            assert ei.value.code == -6
        c.add_batch(*batches[miss])
        assert [s.decode() for s in c.sequences()] == u["seqs"]


def test_emit_contigs_reverse_complement_bytes():
    """a byte outside ACGTU / acgtu becomes N wherever a piece is reverse-complemented, once or twice (src/utils.rs:3-24)"""
    from rust_mdbg_amd import emit as E
    read = b"ACGTNacgtuUxRYACGT"
    nodes = dict(index=[0, 1], abundance=[2, 3], src_read=[0, 0], src_start=[0, 4], src_end=[12, 18], reversed=[1, 1], shift_full=[[3, 4], [5, 6]])
    for edges in ([(0, "+", 1, "+", 1)], [(0, "+", 1, "-", 1)], [(1, "-", 0, "-", 1)], []):
        u = U.unitigs(nodes, edges, [read])
        with E.Contigs(plan_of(u, nodes), n_nodes=2) as c:
            c.add_batch(*O.concat_reads([read]), 0)
            assert [s.decode() for s in c.sequences()] == u["seqs"], edges
    assert "N" in "".join(u["seqs"])


def example_unitigs(example_reads):
    nodes, edges = oracle_graph(example_reads, 7, 10, 0.0008, 2, 0.01)
    assert nodes["n_nodes"] == 104 and nodes["n_edges"] == 206
    return U.unitigs(nodes, edges, example_reads)


def test_example_fixture_unitigs_golden(example_reads):
    """tests/golden/example_cfg1_unitigs.json: recorded from the restatement (HPC on: compared with the restatement only, never with a genome)"""
    u = example_unitigs(example_reads)
    gold = json.load(open(os.path.join(GOLDEN, "example_cfg1_unitigs.json")))
    assert len(u["walks"]) == gold["n_unitigs"] and sum(len(w) for w in u["walks"]) == 104
    assert hashlib.sha256(U.fasta_text(u).encode()).hexdigest() == gold["fasta_sha256"]
    assert hashlib.sha256(U.gfa_text(u).encode()).hexdigest() == gold["gfa_sha256"]
