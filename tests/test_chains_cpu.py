"""The chain restatement (tests/chains_restatement.py) pinned without a GPU: the hand-written expectations of tests/chain_graphs.py, the invariants of
include/mdbg_chain.h and the range-partition property on random graphs with mutated reads, monotonicity in both parameters, the independent GAF formatter against
hand-written lines and libmdbg_emit's writer against that formatter, the binding of include/mdbg_chain.h (exports, struct layout, prototypes), and base space on
the oracle's table: planted substitutions come back as ONE chain with the clean read's coordinates.  The GPU side is tests/test_gpu_chains.py."""
import functools
import os
import random
import re

import numpy as np
import pytest

import alignments_restatement as AL
import chain_graphs as CG
import chains_restatement as CH
import sketch_graphs as G
import unitig_restatement as U
from conftest import ROOT
from test_alignments_cpu import as_result, as_unitig_dict, base_space_input, path_sequence, read_lengths, sketched
from test_sketch_graphs_cpu import host_edges, random_graph

KIND = {CH.NOT_BRIDGED: "-", CH.INSIDE: "I"}
PARAMS = [(0, 0), (1, 0), (2, 0), (1, 2), (3, 4)]                   # (max_skew, max_gap) of the random graphs


def check_invariants(c):
    """what include/mdbg_chain.h states about one chains() result"""
    a = c["a"]
    assert c["n_chains"] == a["n_alignments"] - c["n_bridges"] and c["n_bridges"] == c["n_bridges_inside"] + c["n_bridges_record"]
    assert sum(row[2] for rows in c["chains"] for row in rows) == a["n_placed"] and c["n_gap_windows"] <= a["n_windows"] - a["n_placed"]
    assert c["n_gap_windows"] == sum(row[3] for rows in c["chains"] for row in rows)
    for rows, bridges, alns in zip(c["chains"], c["bridges"], a["alns"]):
        assert [r[0] for r in rows] == (list(np.cumsum([0] + [r[1] for r in rows[:-1]])) if rows else []) and sum(r[1] for r in rows) == len(alns) == len(bridges)
        assert [b[0] == CH.NOT_BRIDGED for b in bridges].count(True) == len(rows) and all(b[1] == 0 for b in bridges if b[0] == CH.NOT_BRIDGED)
        for first, n, windows, gap, qb, qe, occ, plen, pb, pe, n_steps in rows:
            assert bridges[first][0] == CH.NOT_BRIDGED and all(b[0] != CH.NOT_BRIDGED for b in bridges[first + 1:first + n])
            assert 0 <= pb < pe <= plen and qb < qe and (qb, pb) == (alns[first][3], alns[first][7]) and qe == alns[first + n - 1][4]
            if n == 1:
                assert (occ, plen, pe) == (alns[first][5], alns[first][6], alns[first][8])


@functools.lru_cache(maxsize=None)
def model(name):
    """a case of tests/chain_graphs.py -> (case, node table, unitig list, layout) of the plain models"""
    c = CG.BY_NAME[name]
    nodes = G.nodes_from_sketch(c.reads, c.k, G.L, c.A)
    u = U.unitigs(nodes, host_edges(nodes, c.presimp))
    return c, nodes, u, AL.layout_of_model(nodes, u)


def bridges_of(res, q):
    return [(KIND.get(kind, "R"), e) for kind, e in res["bridges"][q]]


# ---- the hand-built cases against expectations written out by hand -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CG.CASE_IDS)
def test_hand_built_cases(name):
    c, nodes, u, lay = model(name)
    for (skew, gap), want in c.expect.items():
        res = CH.chains(c.reads, c.k, G.L, nodes, lay, skew, gap)
        check_invariants(res)
        assert [bridges_of(res, q) for q in c.probe] == want, (skew, gap)
        for q in range(len(c.reads)):                              # every read that is not a probe is error-free: no unplaced window, so no bridge
            if q not in c.probe:
                assert len(res["chains"][q]) == len(res["a"]["alns"][q])


def test_hand_computed_coordinates():
    """k = 3, l = 10, minimizers 100 apart: a node has 210 bases, the unitig of 18 nodes 1910 (the read's own length), a record overlaps 102 + 8.
    substituted: alignments of windows 0 .. 5 ([0, 710) of the read) and 9 .. 17 ([900, 1910)), one chain over the whole read and the whole unitig.
    removed: the read is 100 bases shorter than the path between its ends: [0, 1810) on the read, [0, 1910) on the path.
    gap over a fork: u0 (3 nodes, 410 bases) and u2 (3 nodes, 410) overlap by 110: the path has 710 bases, the read's 710"""
    c, nodes, u, lay = model("substituted")
    res = CH.chains(c.reads, c.k, G.L, nodes, lay, 0, 0)
    assert lay["length"] == [1910] and [r[3:5] + r[6:9] for r in res["a"]["alns"][2]] == [(0, 710, 1910, 0, 710), (900, 1910, 1910, 900, 1910)]
    assert res["chains"][2] == [(0, 2, 15, 3, 0, 1910, [(0, 0)], 1910, 0, 1910, 2)] and (res["n_bridges_inside"], res["n_bridges_record"], res["n_chains"], res["n_gap_windows"]) == (1, 0, 3, 3)
    assert res["chains"][0] == [(0, 1, 18, 0, 0, 1910, [(0, 0)], 1910, 0, 1910, 1)]
    c, nodes, u, lay = model("removed")
    assert CH.chains(c.reads, c.k, G.L, nodes, lay, 1, 0)["chains"][2] == [(0, 2, 15, 2, 0, 1810, [(0, 0)], 1910, 0, 1910, 2)]
    assert len(CH.chains(c.reads, c.k, G.L, nodes, lay, 0, 0)["chains"][2]) == 2
    c, nodes, u, lay = model("gap over a fork")
    res = CH.chains(c.reads, c.k, G.L, nodes, lay, 0, 0)
    assert lay["length"] == [410, 410, 410] and res["chains"][12] == [(0, 2, 3, 3, 0, 710, [(0, 0), (2, 0)], 710, 0, 710, 2)]
    rec = res["bridges"][12][1][0]
    assert u["edges"][rec][:4] == (0, "+", 2, "+") and [e[:4] for e in u["edges"]].index((0, "+", 2, "+")) == rec
    c, nodes, u, lay = model("ring, over the closing record")           # the ring of 6 has 710 bases, two turns 2 * 710 - 110 = 1310; the read's 1110 end at entry 3 of the second turn: 600 + 510
    res = CH.chains(c.reads, c.k, G.L, nodes, lay, 0, 0)
    assert res["chains"][2] == [(0, 2, 7, 3, 0, 1110, [(0, 0), (0, 0)], 1310, 0, 1110, 2)]
    c, nodes, u, lay = model("ring, inside a turn")
    assert CH.chains(c.reads, c.k, G.L, nodes, lay, 0, 0)["chains"][2] == [(0, 2, 7, 3, 0, 1110, [(0, 0), (0, 0)], 1310, 0, 1110, 2)]


# ---- random graphs with mutated reads: invariants, ranges, monotonicity -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_model(seed):
    """a random graph of tests/sketch_graphs.py, and its reads mutated at 2 % per minimizer as QUERIES (they are not part of the graph)"""
    k, A, presimp, reads, nodes = random_graph(seed)
    u = U.unitigs(nodes, host_edges(nodes, presimp))
    return k, nodes, u, AL.layout_of_model(nodes, u), CG.mutated(reads, 0.02, seed)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_invariants_ranges_and_monotonicity_on_random_graphs(seed):
    k, nodes, u, lay, queries = random_model(seed)
    bridged = {}
    for skew, gap in PARAMS + [(0, 1), (0, 2), (3, 0)]:
        res = CH.chains(queries, k, G.L, nodes, lay, skew, gap)
        check_invariants(res)
        bridged[skew, gap] = {(q, i): b for q, bs in enumerate(res["bridges"]) for i, b in enumerate(bs) if b[0] != CH.NOT_BRIDGED}
    assert bridged[3, 0], "no bridge on this seed"
    for small, large in (((0, 0), (1, 0)), ((1, 0), (2, 0)), ((2, 0), (3, 0)), ((0, 1), (0, 2)), ((0, 2), (0, 0)), ((1, 2), (1, 0)), ((1, 2), (3, 4)), ((3, 4), (3, 0))):
        assert bridged[small].items() <= bridged[large].items(), (small, large)      # a superset, and the kind and the entries of a bridge do not change
    whole = CH.chains(queries, k, G.L, nodes, lay, 1, 0)
    cuts = [0, 1, len(queries) // 3, len(queries)]
    parts = [CH.chains(queries[a:b], k, G.L, nodes, lay, 1, 0) for a, b in zip(cuts, cuts[1:])]
    assert sum((p["chains"] for p in parts), []) == whole["chains"] and sum((p["bridges"] for p in parts), []) == whole["bridges"]
    for f in ("n_bridges", "n_bridges_inside", "n_bridges_record", "n_chains", "n_gap_windows"):
        assert sum(p[f] for p in parts) == whole[f], f


# ---- GAF --------------------------------------------------------------------------------------------------------------------------------------------------------
HAND_LINES = {
    ("substituted", 2, 0): "2\t1910\t0\t1910\t+\t>utg0000001l\t1910\t0\t1910\t1910\t1910\t255\tnw:i:15\tns:i:2\tng:i:1\tgw:i:3\n",
    ("removed", 2, 1): "2\t1810\t0\t1810\t+\t>utg0000001l\t1910\t0\t1910\t1810\t1910\t255\tnw:i:15\tns:i:2\tng:i:1\tgw:i:2\n",
    ("gap over a fork", 12, 0): "12\t710\t0\t710\t+\t>utg0000001l>utg0000003l\t710\t0\t710\t710\t710\t255\tnw:i:3\tns:i:2\tng:i:1\tgw:i:3\n",
    ("ring, over the closing record", 2, 0): "2\t1110\t0\t1110\t+\t>utg0000001c>utg0000001c\t1310\t0\t1110\t1110\t1110\t255\tnw:i:7\tns:i:2\tng:i:1\tgw:i:3\n"}


def test_the_formatter_against_hand_written_lines():
    for (name, q, skew), line in HAND_LINES.items():
        c, nodes, u, lay = model(name)
        res = CH.chains(c.reads, c.k, G.L, nodes, lay, skew, 0)
        lines = CH.gaf_lines(res, range(len(c.reads)), read_lengths(c.reads), u["circular"])
        assert len(lines) == res["n_chains"] and [ln for ln in lines if ln.startswith("%d\t" % q)] == [line], name
    c, nodes, u, lay = model("removed")                                 # not bridged at skew 0: the two lines are the alignments' lines with ng:i:0 and gw:i:0
    res = CH.chains(c.reads, c.k, G.L, nodes, lay, 0, 0)
    al = AL.gaf_lines(res["a"], range(3), read_lengths(c.reads), u["circular"])
    assert CH.gaf_lines(res, range(3), read_lengths(c.reads), u["circular"]) == [ln[:-1] + "\tng:i:0\tgw:i:0\n" for ln in al]


def as_chain_result(c, reads, first=0):
    """a restatement result in the shape of Mdbg.graph_chains(): the columns of rust_mdbg_amd.chains.CHAIN_FIELDS with their dtypes, the two offset columns, the
    counts, and the alignment list under "alignments\""""
    from rust_mdbg_amd import chains
    bridges = [b for bs in c["bridges"] for b in bs]
    rows = [r for rs in c["chains"] for r in rs]
    col = dict(bridge_record=[b[0] for b in bridges], bridge_entries=[b[1] for b in bridges], chain_windows=[r[2] for r in rows], chain_gap_windows=[r[3] for r in rows],
               query_begin=[r[4] for r in rows], query_end=[r[5] for r in rows], path_length=[r[7] for r in rows], path_begin=[r[8] for r in rows], path_end=[r[9] for r in rows])
    out = {f: np.array(col[f], dtype=t) for f, t, _ in chains.CHAIN_FIELDS}
    out["chain_offsets"] = np.cumsum([0] + [len(rs) for rs in c["chains"]]).astype(np.uint64)
    out["chain_aln_offsets"] = np.cumsum([0] + [r[1] for r in rows]).astype(np.uint64)
    out.update({f: c[f] for f in chains.CHAIN_COUNTS}, alignments=as_result(c["a"], reads, first))
    return out


@pytest.mark.parametrize("name,skew", [("substituted", 0), ("removed", 1), ("gap over a fork", 0), ("ring, over the closing record", 0), ("ring, a tie goes to INSIDE", 2),
                                       ("two errors far apart", 0), ("short and empty reads", 0)])
def test_the_library_writer_prints_the_formatter_s_lines(name, skew, tmp_path):
    from rust_mdbg_amd import chains
    c, nodes, u, lay = model(name)
    res = CH.chains(c.reads, c.k, G.L, nodes, lay, skew, 0)
    shaped = dict(as_chain_result(res, c.reads))
    shaped["alignments"] = dict(shaped["alignments"], n_unitigs=len(u["walks"]))
    path = str(tmp_path / "c.gaf")
    open(path, "w").write("stale\n")
    chains.gaf_append_chains(path, shaped, as_unitig_dict(u, lay), read_lengths(c.reads), truncate=True)
    lines = CH.gaf_lines(res, range(len(c.reads)), read_lengths(c.reads), u["circular"])
    assert open(path).read() == "".join(lines) and res["n_bridges"] > 0
    chains.gaf_append_chains(path, shaped, as_unitig_dict(u, lay), read_lengths(c.reads))      # appended behind what is there
    assert open(path).read() == "".join(lines) * 2
    with pytest.raises(Exception):
        chains.gaf_append_chains(str(tmp_path / "no" / "such" / "dir.gaf"), shaped, as_unitig_dict(u, lay), read_lengths(c.reads))
    # a list built by hand with a column missing, or with offsets that do not end where the lists do, answers MDBG_E_PARAM and writes nothing
    from rust_mdbg_amd import api, emit
    ul, keep_u = emit.unitig_list(as_unitig_dict(u, lay))
    lens = np.array(read_lengths(c.reads), np.uint64)
    call = lambda ch: emit.load_library().mdbg_gaf_append_chains(path.encode(), 1, api.C.byref(ch), api.C.byref(ul), lens.ctypes.data)
    for f in ("query_begin", "query_end", "path_length", "path_begin", "path_end", "chain_windows", "chain_gap_windows", "bridge_record", "chain_aln_offsets"):
        ch, keep = chains.chain_list(shaped)
        setattr(ch, f, None)
        assert call(ch) == api.MDBG_E_PARAM, f
    for f, n in (("n_chains", 1), ("n_chains", -1)):
        ch, keep = chains.chain_list(shaped)
        setattr(ch, f, getattr(ch, f) + n)
        assert call(ch) == api.MDBG_E_PARAM, f
    ch, keep = chains.chain_list(shaped)
    ch.alignments.n_steps -= 1
    assert call(ch) == api.MDBG_E_PARAM
    ch, keep = chains.chain_list(shaped)
    assert call(ch) == 0 and open(path).read() == "".join(lines)


# ---- the binding of include/mdbg_chain.h -------------------------------------------------------------------------------------------------------------------------
def test_the_header_s_symbols_struct_and_prototypes_are_the_binding_s(tmp_path):
    """what tests/test_abi_exports.py checks of the other headers, with its own helpers: every symbol exported, the mirror's layout is gcc's, every prototype agrees"""
    import ctypes as C
    import subprocess
    import test_abi_exports as ABI
    from rust_mdbg_amd import align, api, chains, emit
    text = open(os.path.join(ROOT, "include", "mdbg_chain.h")).read()
    syms = sorted(set(re.findall(r"\b(mdbg_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert syms == sorted(chains.HIP_EXPORTS + chains.EMIT_EXPORTS) and len(syms) == 6
    hip, em = api.load_library(), emit.load_library()
    assert all(hasattr(hip, s) for s in chains.HIP_EXPORTS) and all(hasattr(em, s) for s in chains.EMIT_EXPORTS)
    by_name = dict(ABI.mirrors(), mdbg_alignment_list=align.AlignmentList, mdbg_chain_list=chains.ChainList)
    cls, t = chains.ChainList, "mdbg_chain_list"
    lines = ['printf("%%zu\\n", sizeof(%s));' % t] + ['printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (t, f[0], t, f[0]) for f in cls._fields_]
    (tmp_path / "layout.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mdbg_chain.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [tuple(int(w) for w in ln.split()) for ln in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert got == [(C.sizeof(cls),)] + [(getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_]
    rows = {n: (getattr(hip if n in chains.HIP_EXPORTS else em, n).restype, getattr(hip if n in chains.HIP_EXPORTS else em, n).argtypes) for n in syms}
    assert ABI.prototype_errors(text, rows, by_name) == []
    broken = dict(rows, mdbg_graph_chains=(rows["mdbg_graph_chains"][0], rows["mdbg_graph_chains"][1][:-1]))
    assert [e.split(":")[0] for e in ABI.prototype_errors(text, broken, by_name)] == ["mdbg_graph_chains"]
    assert {f for f, _, _ in chains.CHAIN_FIELDS} | {f for f, _ in chains.CHAIN_OFFSETS} | set(chains.CHAIN_COUNTS) | {"alignments"} == {f for f, _ in chains.ChainList._fields_}
    assert (chains.NOT_BRIDGED, chains.INSIDE) == (CH.NOT_BRIDGED, CH.INSIDE) == tuple(int(v, 16) for v in re.findall(r"#define MDBG_BRIDGE_\w+\s+(0x[0-9A-F]+)u", text))


# ---- base space: planted substitutions on the oracle's table ------------------------------------------------------------------------------------------------------
def planted(clean, sk_clean, k, l, d, rnd, tries=200, max_change=1):
    """a copy of the read with one base substituted so that the sketch changes but its first and last k-min-mer window do not -> (query, position, its sketch).
    At this density (a minimizer every 24 bases, l = 10) one base lies under several overlapping l-mers, and substituting it can take two or three minimizers out at
    once: several minimizer errors in one gap, whose skews add up (include/mdbg_chain.h).  max_skew 1 is the bound for ONE minimizer error, so the base is chosen
    where the two sketches differ by at most one minimizer in number — decided on the oracle's sketches alone, before anything is aligned.  max_change=None lifts
    that: ANY base inside a minimizer.  A base lies under at most l l-mers, so it changes the number of minimizers by at most l: the bound those queries are held to."""
    hashes, pos = sk_clean
    for _ in range(tries):
        j = rnd.randrange(k, len(hashes) - k)                      # inside a minimizer that neither the first nor the last window holds
        p = pos[j] + rnd.randrange(l)
        new = rnd.choice([b for b in "ACGT" if b != clean[p]])
        query = clean[:p] + new + clean[p + 1:]
        sk = sketched([query.encode()], l, d)[2][0]
        if sk != sk_clean and (max_change is None or abs(len(sk[0]) - len(hashes)) <= max_change) and sk[0][:k] == hashes[:k] and sk[0][-k:] == hashes[-k:] and sk[1][:k] == pos[:k] and sk[1][-k:] == pos[-k:]:
            return query, p, sk
    raise AssertionError("no substitution found that spares the first and the last window")


def linear_genome_input(seed=5, n_reads=24):
    """error-free reads of 4 kb of a random genome of 30 kb, from either strand, tiled so that the graph is one linear unitig -> (genome, reads as str)"""
    rnd = random.Random(seed)
    genome = "".join(rnd.choice("ACGT") for _ in range(30000))
    starts = [0, len(genome) - 4000] + [rnd.randrange(0, len(genome) - 4000) for _ in range(n_reads - 2)] + list(range(0, len(genome) - 4000, 1500))
    reads = [genome[a:a + 4000] for a in starts]
    reads = [U.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    return genome, reads + reads                                   # every k-min-mer at least twice: A = 2


def base_space_queries(reads, k, l, d, seed, max_change=1):
    """-> (queries as bytes, planted positions, sketches of the queries, sketches of the clean reads); every read gets one: none is left out"""
    rnd = random.Random(seed)
    clean_sk = sketched([r.encode() for r in reads], l, d)[2]
    made = [planted(r, sk, k, l, d, rnd, max_change=max_change) for r, sk in zip(reads, clean_sk)]
    return [q.encode() for q, _, _ in made], [p for _, p, _ in made], [sk for _, _, sk in made], clean_sk


def chain_sequence(res, q, row, lay, seqs, l):
    """the sequence of a chain's path: its occurrences' sequences one behind the other, an occurrence of strand 1 reverse-complemented, every occurrence behind the
    first without the bases it shares with the one in front — taken from where the restatement's alignments' own path sequences overlap it"""
    first, n = row[0], row[1]
    a = res["a"]
    seq = ""
    for i in range(first, first + n):
        f, ns = a["alns"][q][i][0], a["alns"][q][i][1]
        piece, _ = path_sequence(a["steps"][q][f:f + ns], lay, seqs, l)
        kind = res["bridges"][q][i][0]
        if i == first:
            seq = piece
        elif kind == CH.INSIDE:
            u = a["steps"][q][f][2]
            seq += piece[lay["length"][u]:]
        else:
            seq += piece[lay["edges"][kind][4] + l - 2:]
    return seq


def check_planted(res, clean, queries, positions, reads, lay, seqs, l):
    """every query is exactly one chain with at most one bridge, with the coordinates and the path of the clean read's single alignment, and the two aligned blocks
    differ at exactly the planted position -> the number of queries with a bridge (the callers hold it to ALL of them: a sketch that changed between a read's first and
    last window leaves unplaced windows there)"""
    n_bridged = 0
    for q, (query, p) in enumerate(zip(queries, positions)):
        assert len(res["chains"][q]) == 1 and len(clean["alns"][q]) == 1, q
        row, want = res["chains"][q][0], clean["alns"][q][0]
        assert row[1] <= 2 and (row[4], row[5], row[6], row[7], row[8], row[9]) == (want[3], want[4], want[5], want[6], want[7], want[8]), q
        n_bridged += row[1] - 1
        block_p, block_q = chain_sequence(res, q, row, lay, seqs, l)[row[8]:row[9]], query.decode()[row[4]:row[5]]
        assert len(block_p) == len(block_q) and [i for i, (x, y) in enumerate(zip(block_p, block_q)) if x != y] == [p - row[4]], q
        assert block_p == reads[q][row[4]:row[5]]
    return n_bridged


def test_base_space_planted_substitutions_on_the_oracle_s_table():
    """one linear unitig from error-free reads; every read once more with one base substituted inside a minimizer (the first and the last window untouched, verified
    on the oracle's sketch of both versions): at max_skew 1 every query is ONE chain with the clean read's coordinates"""
    from oracle import oracle as O
    from test_repeats_cpu import BASE_PARAMS
    k, l, d, A = BASE_PARAMS
    genome, reads = linear_genome_input()
    b, o, sreads = sketched([r.encode() for r in reads], l, d)
    g = O.Graph(k, l, d, A, already_hpc=True)
    assert g.ingest(b, o) == 0
    nodes = g.finalize(with_edges=False)
    u = U.unitigs(nodes, host_edges(nodes, 0.0), [r.encode() for r in reads])
    lay = AL.layout_of_model(nodes, u)
    assert len(u["walks"]) == 1 and u["circular"] == [False]
    queries, positions, qsk, clean_sk = base_space_queries(reads, k, l, d, 11)
    clean = AL.alignments(clean_sk, k, l, nodes, lay)
    res = CH.chains(qsk, k, l, nodes, lay, 1, 0)
    check_invariants(res)
    n_bridged = check_planted(res, clean, queries, positions, reads, lay, u["seqs"], l)
    assert n_bridged == len(queries) == res["n_bridges_inside"]
    # ANY base inside a minimizer, also one that takes several overlapping minimizers out at once: the skews add up to at most l, and at max_skew l the same holds
    queries, positions, qsk, _ = base_space_queries(reads, k, l, d, 13, max_change=None)
    change = [abs(len(s[0]) - len(c[0])) for s, c in zip(qsk, clean_sk)]
    assert max(change) >= 2                                        # (otherwise the second half shows nothing the first did not)
    res = CH.chains(qsk, k, l, nodes, lay, l, 0)
    check_invariants(res)
    assert check_planted(res, clean, queries, positions, reads, lay, u["seqs"], l) == len(queries)
    assert CH.chains(qsk, k, l, nodes, lay, 1, 0)["n_chains"] > len(queries)      # and max_skew 1 does not join all of those


@functools.lru_cache(maxsize=None)
def ring_genome_queries():
    """the genome with a repeat and the ring of tests/test_alignments_cpu.py -> (its reads as bytes, every sixth read with one planted substitution as bytes, the
    sketches of those queries)"""
    from test_repeats_cpu import BASE_PARAMS
    k, l, d, A = BASE_PARAMS
    reads = base_space_input()[2]
    queries, _, qsk, _ = base_space_queries([r.decode() for r in reads[::6]], k, l, d, 12)
    return reads, queries, qsk


def test_base_space_on_the_repeat_and_ring_genome_restatement_only():
    """the genome with a repeat and the ring of tests/test_alignments_cpu.py: the same kind of queries, held against the restatement's own invariants, and every
    bridged chain's block lengths agree (a substitution moves no base).  One of the gaps lies over an edge record"""
    from oracle import oracle as O
    from test_repeats_cpu import BASE_PARAMS
    k, l, d, A = BASE_PARAMS
    reads, queries, qsk = ring_genome_queries()
    b, o, _ = sketched(reads, l, d)
    g = O.Graph(k, l, d, A, already_hpc=True)
    assert g.ingest(b, o) == 0
    nodes = g.finalize(with_edges=False)
    u = U.unitigs(nodes, host_edges(nodes, 0.0))
    lay = AL.layout_of_model(nodes, u)
    res = CH.chains(qsk, k, l, nodes, lay, 1, 0)
    check_invariants(res)
    assert res["n_bridges_inside"] > 0 and res["n_bridges_record"] > 0 and res["n_chains"] == len(queries)
    for rows in res["chains"]:
        for row in rows:
            if row[1] > 1:
                assert row[5] - row[4] == row[9] - row[8]
