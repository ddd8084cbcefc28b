"""The alignment restatement (tests/alignments_restatement.py) pinned without a GPU: hand-computed alignments of the catalogue of tests/sketch_graphs.py (a chain
of three unitigs on both strands, a ring walked once and a window more, a read cut at a missing crossing), the invariants of include/mdbg_align.h against the
junction and read-path restatements on every case and random graph, the range-partition property, the independent GAF formatter against hand-written lines,
libmdbg_emit's writer against that formatter, and the binding of include/mdbg_align.h (exports, struct layout, prototypes).  The GPU side is
tests/test_gpu_alignments.py."""
import functools
import os
import re

import numpy as np
import pytest

import alignments_restatement as AL
import junctions_restatement as J
import sketch_graphs as G
import unitig_restatement as U
from conftest import ROOT
from test_read_paths_cpu import hashes
from test_sketch_graphs_cpu import BY_NAME, host_edges, model_nodes, random_graph

NONE = AL.NO_RECORD


def read_lengths(reads, l=G.L):
    return [p[-1] + l if p else 0 for _, p in reads]


def on_list(nodes, reads, k, u):
    """-> (alignments, layout) of one list of the unitig restatement; the invariants of the header are asserted on the way"""
    lay = AL.layout_of_model(nodes, u)
    a = AL.alignments(reads, k, G.L, nodes, lay)
    j = J.junctions(hashes(reads), k, nodes["keys"].tolist(), nodes["index"].tolist(), u["walks"], [e[:4] for e in u["edges"]])
    assert a["n_alignments"] == a["n_steps"] - a["n_chained"]
    assert j["n_explained"] == a["n_chained"] + a["n_wraps"]
    for steps, alns, W, placed in zip(a["steps"], a["alns"], a["windows"], a["placed"]):
        assert [s[5] == NONE for s in steps].count(True) == len(alns) and sum(r[1] for r in alns) == len(steps) and sum(r[2] for r in alns) == placed
        assert [r[0] for r in alns] == list(np.cumsum([0] + [r[1] for r in alns[:-1]])) if alns else True          # the alignments partition the steps in order
        for first, n, windows, qb, qe, occ, plen, pb, pe in alns:
            assert steps[first][5] == NONE and all(s[5] != NONE for s in steps[first + 1:first + n]) and 0 <= pb < pe <= plen and qb < qe
        if j["n_missing"] == 0 and placed == W and W:                                     # no missing key: only unplaced windows separate alignments
            assert len(alns) == 1
    return a, lay


@functools.lru_cache(maxsize=None)
def plain(name, presimp=0.0):
    c, nodes = BY_NAME[name], model_nodes(name)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    return (c, u) + on_list(nodes, c.reads, c.k, u)


# ---- hand-computed, from the definition (k = 3, l = 10, minimizers 100 bases apart: a node has 210 bases, a unitig of m nodes 210 + 100 (m - 1), two
# ---- neighbouring nodes share 110 bases: the record's overlap 102 and l - 2) ---------------------------------------------------------------------------------
def test_a_chain_of_three_unitigs_on_both_strands():
    """bubble 7/3: read `one` walks u0, its branch u1 and u2 forwards; read `two`, sequenced from the other strand, walks u2 backwards, its branch u3 forwards and u0
    backwards.  14 minimizers: 12 windows, 1310 bases; the path has 3 * 510 - 2 * 110 = 1310 bases and the alignment covers all of it"""
    c, u, a, lay = plain("bubble 7/3")
    assert lay["length"] == [510] * 4 and {e[4] for e in u["edges"]} == {102}
    assert a["steps"][0] == [(0, 4, 0, 0, 0, NONE), (4, 4, 1, 0, 0, 0), (8, 4, 2, 0, 0, 3)]
    assert a["alns"][0] == [(0, 3, 12, 0, 1310, [(0, 0), (1, 0), (2, 0)], 1310, 0, 1310)]
    assert a["steps"][7] == [(0, 4, 2, 3, 1, NONE), (4, 4, 3, 0, 0, 5), (8, 4, 0, 3, 1, 1)]
    assert a["alns"][7] == [(0, 3, 12, 0, 1310, [(2, 1), (3, 0), (0, 1)], 1310, 0, 1310)]
    assert (a["n_steps"], a["n_chained"], a["n_alignments"], a["n_wraps"]) == (30, 20, 10, 0)
    # the records the steps name carry the key of the pair the read crosses, and they are the smallest with that key
    assert u["edges"][0][:4] == (0, "+", 1, "+") and u["edges"][3][:4] == (1, "+", 2, "+")


def test_a_ring_walked_once_and_one_window_more():
    """islands: the ring has 6 nodes and 710 bases (its first node whole: the 110 bases the closing record overlaps are there twice); the ring reads have 9 minimizers,
    7 windows, 810 bases, and walk it against the walk from entry 0: entries 0, 5, 4, 3, 2, 1, 0.  One step, one wrap, the unitig listed twice: the path has
    2 * 710 - 110 = 1310 bases; on the reversed ring entry 0 covers [500, 710), the second turn starts at 600, and its entry 0 covers [1100, 1310)"""
    c, u, a, lay = plain("islands")
    assert u["circular"] == [False, False, False, True] and lay["length"] == [810, 410, 310, 710] and lay["ends"][3] == [210, 310, 410, 510, 610, 710]
    assert a["steps"][7] == [(0, 7, 3, 0, 1, NONE)] and a["alns"][7] == [(0, 1, 7, 0, 810, [(3, 1), (3, 1)], 1310, 500, 1310)]
    assert (a["n_chained"], a["n_wraps"], a["n_alignments"]) == (0, 2, 9)
    assert a["alns"][0] == [(0, 1, 7, 0, 810, [(0, 0)], 810, 0, 810)]                 # a read that is all of a linear unitig


def test_a_missing_crossing_cuts_the_alignment():
    """presimp 200/1 at 0.01, edges built at 0.01: the small branch's records are gone.  The one read that takes it (8 minimizers, 6 windows, 710 bases) is cut
    where it leaves the trunk at entry 2: windows 0..2 on the trunk, bases [0, 410) of its 710; windows 3..5 all of the branch, bases [300, 710) of the read"""
    c, u, a, lay = plain("presimp 200/1 at 0.01", 0.01)
    assert u["edges"] == [] and lay["length"] == [710, 410]
    assert a["steps"][200] == [(0, 3, 0, 0, 0, NONE), (3, 3, 1, 0, 0, NONE)]
    assert a["alns"][200] == [(0, 1, 3, 0, 410, [(0, 0)], 710, 0, 410), (1, 1, 3, 300, 710, [(1, 0)], 410, 0, 410)]
    assert (a["n_chained"], a["n_alignments"]) == (0, 202)
    c, u, a, lay = plain("presimp 200/1 at 0.01")                                      # with the records: one alignment of two steps
    assert a["alns"][200] == [(0, 2, 6, 0, 710, [(0, 0), (2, 0)], 710, 0, 710)] and a["steps"][200][1][5] != NONE


def test_fork_both_reads_chain_over_their_own_record():
    c, u, a, lay = plain("fork")
    assert a["alns"][0] == [(0, 2, 12, 0, 1310, [(0, 0), (1, 0)], 1310, 0, 1310)] and a["alns"][5] == [(0, 2, 7, 0, 810, [(0, 0), (2, 0)], 810, 0, 810)]
    assert [s[5] for s in a["steps"][0]] == [NONE, 0] and [s[5] for s in a["steps"][5]] == [NONE, 1]


# ---- the catalogue and the random graphs: invariants ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_invariants_on_the_catalogue(name):
    c = BY_NAME[name]
    for p in c.presimps:
        plain(name, p)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_invariants_and_ranges_on_the_random_graphs(seed):
    k, A, presimp, reads, nodes = random_graph(seed)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    whole, lay = on_list(nodes, reads, k, u)
    assert whole["n_alignments"] > 0
    cuts = [0, 1, len(reads) // 3, len(reads)]                                          # a partition of the reads: the columns concatenate, the counters add up
    parts = [AL.alignments(reads[a:b], k, G.L, nodes, lay) for a, b in zip(cuts, cuts[1:])]
    assert sum((p["steps"] for p in parts), []) == whole["steps"] and sum((p["alns"] for p in parts), []) == whole["alns"]
    for f in ("n_windows", "n_placed", "n_steps", "n_chained", "n_alignments", "n_wraps"):
        assert sum(p[f] for p in parts) == whole[f], f


# ---- GAF --------------------------------------------------------------------------------------------------------------------------------------------------------
HAND_LINES = {
    ("bubble 7/3", 0): "0\t1310\t0\t1310\t+\t>utg0000001l>utg0000002l>utg0000003l\t1310\t0\t1310\t1310\t1310\t255\tnw:i:12\tns:i:3\n",
    ("bubble 7/3", 9): "9\t1310\t0\t1310\t+\t<utg0000003l>utg0000004l<utg0000001l\t1310\t0\t1310\t1310\t1310\t255\tnw:i:12\tns:i:3\n",
    ("islands", 8): "8\t810\t0\t810\t+\t<utg0000004c<utg0000004c\t1310\t500\t1310\t810\t810\t255\tnw:i:7\tns:i:1\n",
    ("fork", 6): "6\t810\t0\t810\t+\t>utg0000001l>utg0000003l\t810\t0\t810\t810\t810\t255\tnw:i:7\tns:i:2\n"}


def test_the_formatter_against_hand_written_lines():
    for (name, q), line in HAND_LINES.items():
        c, u, a, _ = plain(name)
        lines = AL.gaf_lines(a, range(len(c.reads)), read_lengths(c.reads), u["circular"])
        assert len(lines) == a["n_alignments"] and [ln for ln in lines if ln.startswith("%d\t" % q)] == [line], name
    c, u, a, _ = plain("presimp 200/1 at 0.01", 0.01)                                  # two lines of one read, and columns 10 and 11 where the two blocks agree
    lines = AL.gaf_lines(a, range(len(c.reads)), read_lengths(c.reads), u["circular"])
    assert lines[-2:] == ["200\t710\t0\t410\t+\t>utg0000001l\t710\t0\t410\t410\t410\t255\tnw:i:3\tns:i:1\n",
                          "200\t710\t300\t710\t+\t>utg0000002l\t410\t0\t410\t410\t410\t255\tnw:i:3\tns:i:1\n"]


def as_result(a, reads, first=0):
    """a restatement result in the shape of Mdbg.graph_alignments(): the columns of rust_mdbg_amd.align.ALIGNMENT_FIELDS with their dtypes, the three offset
    columns, the counts"""
    from rust_mdbg_amd import align
    steps = [s for st in a["steps"] for s in st]
    alns = [r for rows in a["alns"] for r in rows]
    col = dict(ordinal=list(range(len(reads))), read_windows=a["windows"],
               first_window=[s[0] for s in steps], step_windows=[s[1] for s in steps], unitig=[s[2] for s in steps], first_entry=[s[3] for s in steps], strand=[s[4] for s in steps],
               step_record=[s[5] for s in steps], aln_windows=[r[2] for r in alns], query_begin=[r[3] for r in alns], query_end=[r[4] for r in alns],
               path_length=[r[6] for r in alns], path_begin=[r[7] for r in alns], path_end=[r[8] for r in alns])
    out = {f: np.array(col[f], dtype=t) for f, t, _ in align.ALIGNMENT_FIELDS}
    out["step_offsets"] = np.cumsum([0] + [len(st) for st in a["steps"]]).astype(np.uint64)
    out["aln_offsets"] = np.cumsum([0] + [len(rows) for rows in a["alns"]]).astype(np.uint64)
    out["aln_step_offsets"] = np.cumsum([0] + [r[1] for r in alns]).astype(np.uint64)
    out.update({f: a[f] for f in align.ALIGNMENT_COUNTS if f != "n_reads"}, n_reads=len(reads), first_read=first)
    return out


def as_unitig_dict(u, lay):
    """the columns of a unitig list mdbg_gaf_append reads (offsets, circular), the others zero, in the shape of Mdbg.graph_unitigs()"""
    from rust_mdbg_amd import api
    n = [len(w) for w in u["walks"]]
    out = {f: np.zeros(sum(n) if f not in ("offsets", "length", "kc_sum", "circular") else len(n), t) for f, t in api.UNITIG_FIELDS}
    out.update(offsets=np.cumsum([0] + n).astype(np.uint64), circular=np.array(u["circular"], np.uint8), length=np.array(lay["length"], np.uint64))
    out["edges"] = {f: np.zeros(0, t) for f, t in api.EDGE_FIELDS}
    return out


@pytest.mark.parametrize("name", ["bubble 7/3", "islands", "fork", "hub", "short reads"])
def test_the_library_writer_prints_the_formatter_s_lines(name, tmp_path):
    from rust_mdbg_amd import align
    c, u, a, lay = plain(name)
    path = str(tmp_path / "a.gaf")
    open(path, "w").write("stale\n")
    align.gaf_append(path, as_result(a, c.reads), as_unitig_dict(u, lay), read_lengths(c.reads), truncate=True)
    lines = AL.gaf_lines(a, range(len(c.reads)), read_lengths(c.reads), u["circular"])
    assert open(path).read() == "".join(lines) and len(lines) > 0
    align.gaf_append(path, as_result(a, c.reads), as_unitig_dict(u, lay), read_lengths(c.reads))      # appended behind what is there
    assert open(path).read() == "".join(lines) * 2
    with pytest.raises(Exception):
        align.gaf_append(str(tmp_path / "no" / "such" / "dir.gaf"), as_result(a, c.reads), as_unitig_dict(u, lay), read_lengths(c.reads))


# ---- the binding of include/mdbg_align.h -------------------------------------------------------------------------------------------------------------------------
def test_the_header_s_symbols_struct_and_prototypes_are_the_binding_s(tmp_path):
    """what tests/test_abi_exports.py checks of the other headers, with its own helpers: every symbol exported, the mirror's layout is gcc's, every prototype agrees"""
    import test_abi_exports as ABI
    from rust_mdbg_amd import align, api, emit
    text = open(os.path.join(ROOT, "include", "mdbg_align.h")).read()
    syms = sorted(set(re.findall(r"\b(mdbg_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert syms == sorted(align.HIP_EXPORTS + align.EMIT_EXPORTS) and len(syms) == 6
    hip, em = api.load_library(), emit.load_library()
    assert all(hasattr(hip, s) for s in align.HIP_EXPORTS) and all(hasattr(em, s) for s in align.EMIT_EXPORTS)
    by_name = dict(ABI.mirrors(), mdbg_alignment_list=align.AlignmentList)
    # the mirror's layout against gcc's, as test_abi_exports.layout_errors does it for the headers it includes
    import ctypes as C
    import subprocess
    cls, t = align.AlignmentList, "mdbg_alignment_list"
    lines = ['printf("%%zu\\n", sizeof(%s));' % t] + ['printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (t, f[0], t, f[0]) for f in cls._fields_]
    (tmp_path / "layout.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mdbg_align.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [tuple(int(w) for w in ln.split()) for ln in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert got == [(C.sizeof(cls),)] + [(getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_]
    rows = {n: (getattr(hip if n in align.HIP_EXPORTS else em, n).restype, getattr(hip if n in align.HIP_EXPORTS else em, n).argtypes) for n in syms}
    assert ABI.prototype_errors(text, rows, by_name) == []
    broken = dict(rows, mdbg_graph_alignments=(rows["mdbg_graph_alignments"][0], rows["mdbg_graph_alignments"][1][:-1]))
    assert [e.split(":")[0] for e in ABI.prototype_errors(text, broken, by_name)] == ["mdbg_graph_alignments"]
    assert api.ALIGNMENT_FIELDS is align.ALIGNMENT_FIELDS and {f for f, _, _ in align.ALIGNMENT_FIELDS} | {f for f, _ in align.ALIGNMENT_OFFSETS} | set(align.ALIGNMENT_COUNTS) | {
        "first_read", "n_unitigs"} == {f for f, _ in align.AlignmentList._fields_}


# ---- base space: the arbiter of the coordinate definition, on the oracle's node table ----------------------------------------------------------------------------
BASE_SEED = 1


def base_space_input(seed=BASE_SEED):
    """an error-free genome of about 61 kb with one two-copy repeat of 1,000 bases (genome_with_repeat of the repeat tests: several linear unitigs) and one circular
    sequence of 30 kb; reads of 5 kb at about 20x from both, every one from either strand, the ring's reads cut across its origin too -> (genome, ring, reads)"""
    import random
    from test_repeats_cpu import genome_with_repeat
    rnd = random.Random(seed + 1000)                                                  # (genome_with_repeat draws from Random(seed): another stream for the ring)
    genome = genome_with_repeat(seed, flank=19700, repeat=1000)
    ring = "".join(rnd.choice("ACGT") for _ in range(30000))
    reads = []
    for src, circular in ((genome, False), (ring, True)):
        for _ in range(len(src) * 20 // 5000):
            a = rnd.randrange(0, len(src) if circular else len(src) - 5000 + 1)
            s = (src + src)[a:a + 5000]
            reads.append((U.revcomp(s) if rnd.random() < 0.5 else s).encode())
    return genome, ring, reads


def path_sequence(steps, lay, seqs, l):
    """the sequence of an alignment's path from the unitig sequences and the records: an occurrence of strand 1 reverse-complemented, every occurrence behind the
    first without the bases it shares with the one in front (the record's overlap + l - 2) -> (sequence, occurrences)"""
    first_record = {}
    for r, e in enumerate(lay["edges"]):
        first_record.setdefault(J.record_key(e, lay["walks"]), r)
    seq, n_occ = "", 0
    for fw, n, u, j0, s, rec in steps:
        m = len(lay["walks"][u])
        wraps = ((j0 if s == 0 else m - 1 - j0) + n - 1) // m if lay["circular"][u] else 0
        for turn in range(wraps + 1):
            piece = seqs[u] if s == 0 else U.revcomp(seqs[u])
            if n_occ:
                r = rec if turn == 0 else first_record[J.key_of(((u, m - 1, 0), (u, 0, 0)))]
                piece = piece[lay["edges"][r][4] + l - 2:]
            seq += piece
            n_occ += 1
    return seq, n_occ


def check_base_space(a, reads, lay, seqs, l):
    """every alignment's bases on the path are its bases on the read; every read all of whose windows are placed is ONE alignment; some alignment has two steps or
    more and some wraps a ring (otherwise the check shows nothing) -> (alignments of two steps or more, alignments that wrap)"""
    multi = wrapped = 0
    for q, rows in enumerate(a["alns"]):
        read = reads[q].decode()
        if a["windows"][q] and a["windows"][q] == a["placed"][q]:
            assert len(rows) == 1, q
        for first, n, windows, qb, qe, occ, plen, pb, pe in rows:
            seq, n_occ = path_sequence(a["steps"][q][first:first + n], lay, seqs, l)
            assert len(seq) == plen and n_occ == len(occ) and seq[pb:pe] == read[qb:qe], (q, first)
            multi += n >= 2
            wrapped += n_occ > n
    assert multi >= 1 and wrapped >= 1
    return multi, wrapped


def sketched(reads, l, d):
    from oracle import oracle as O
    b, o = O.concat_reads(reads)
    sk = O.sketch(b, o, l, d, already_hpc=True)
    off = sk["off"].tolist()
    return b, o, [(tuple(sk["hashes"][x:y].tolist()), tuple(sk["pos"][x:y].tolist())) for x, y in zip(off, off[1:])]


def test_base_space_on_the_oracle_s_table():
    """the definition's coordinates against sequences, without a GPU: the oracle's node table, the host edges, the unitig restatement's sequences"""
    from oracle import oracle as O
    from test_repeats_cpu import BASE_PARAMS
    k, l, d, A = BASE_PARAMS
    genome, ring, reads = base_space_input()
    b, o, sreads = sketched(reads, l, d)
    g = O.Graph(k, l, d, A, already_hpc=True)
    assert g.ingest(b, o) == 0
    nodes = g.finalize(with_edges=False)
    u = U.unitigs(nodes, host_edges(nodes, 0.0), reads)
    lay = AL.layout_of_model(nodes, u)
    assert lay["length"] == u["length"] and u["circular"].count(True) == 1 and len(u["walks"]) >= 4
    ring_u = u["circular"].index(True)
    closing = [e[4] for e in u["edges"] if e[:4] == (ring_u, "+", ring_u, "+")]
    assert len(closing) == 1 and u["length"][ring_u] == len(ring) + closing[0] + l - 2          # length[] of a ring INCLUDES the bases its closing record overlaps
    a = AL.alignments(sreads, k, l, nodes, lay)
    multi, wrapped = check_base_space(a, reads, lay, u["seqs"], l)
    print("alignments %d, of two steps or more %d, wrapping %d" % (a["n_alignments"], multi, wrapped))
