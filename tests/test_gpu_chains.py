"""Chains on the GPU (Mdbg.graph_chains, Mdbg.chain_batch) against the plain restatement (tests/chains_restatement.py), exactly: every count, every column
element for element with its dtype, from the host and the device variant — on the hand-built cases of tests/chain_graphs.py, the random graphs with mutated reads,
a read of 2,101 alignments, ranges of reads, base space with planted substitutions through chain_batch, monotonicity, the state checks, what the call leaves
alone, the pipeline's files and the C program's.  CPU side: tests/test_chains_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import alignments_restatement as AL
import chain_graphs as CG
import chains_restatement as CH
import sketch_graphs as G
from conftest import GOLDEN
from oracle import oracle as O
from test_chains_cpu import as_chain_result, base_space_queries, check_planted, linear_genome_input
from test_gpu_alignments import assert_same, contig_strings, refused, sketch_reads
from test_gpu_parity import _mdbg
from test_gpu_read_paths import built
from test_gpu_simplify import same_list
from test_repeats_cpu import BASE_PARAMS

pytestmark = pytest.mark.gpu

REPEATS = 16


def expected(reads, k, nodes, ul, skew, gap, l=G.L):
    return CH.chains(reads, k, l, nodes, AL.layout_of_arrays(ul), skew, gap)


def shaped(exp, reads, ul, first=0):
    out = as_chain_result(exp, reads, first)
    out["alignments"] = dict(out["alignments"], n_unitigs=int(ul["n_unitigs"]))
    return out


def assert_same_chains(a, b):
    assert sorted(a) == sorted(b)
    assert_same(a["alignments"], b["alignments"])
    assert_same({f: v for f, v in a.items() if f != "alignments"}, {f: v for f, v in b.items() if f != "alignments"})


def assert_zeros(R, got, first=0):
    al = got["alignments"]
    assert al["first_read"] == first and all(al[f] == 0 for f in R.align.ALIGNMENT_COUNTS) and all(got[f] == 0 for f in R.chains.CHAIN_COUNTS)
    assert all(len(got[f]) == 0 for f, _, _ in R.chains.CHAIN_FIELDS) and all(got[f].tolist() == [0] for f, _ in R.chains.CHAIN_OFFSETS)


def device_copy(R, m, dev):
    """a ChainList with DEVICE pointers -> the dict graph_chains gives, every array copied back"""
    from test_gpu_alignments import device_copy as alignment_copy
    al = dev.alignments
    n = dict(read=int(al.n_reads), alignment=int(al.n_alignments), chain=int(dev.n_chains))
    addr = lambda p: R.api.C.cast(p, R.api.C.c_void_p).value
    out = {f: m.to_host(addr(getattr(dev, f)), n[per] * np.dtype(t).itemsize, t) if n[per] else np.zeros(0, t) for f, t, per in R.chains.CHAIN_FIELDS}
    out.update({f: m.to_host(addr(getattr(dev, f)), (n[per] + 1) * 8, np.uint64) for f, per in R.chains.CHAIN_OFFSETS})
    out.update({f: int(getattr(dev, f)) for f in R.chains.CHAIN_COUNTS}, alignments=alignment_copy(R, m, al))
    return out


def check(R, m, reads, k, nodes, ul, skew, gap, l=G.L):
    """the context's current list is `ul`: the whole store's chains equal the restatement's, twice from the host variant and once from the device variant, and the
    invariants of the header hold on the arrays; -> (got, exp)"""
    got = m.graph_chains(0, 0, skew, gap)
    exp = expected(reads, k, nodes, ul, skew, gap, l)
    print("skew %d gap %d: " % (skew, gap) + " ".join("%s %d" % (f, got[f]) for f in R.chains.CHAIN_COUNTS))
    assert_same_chains(got, shaped(exp, reads, ul))
    al = got["alignments"]
    assert got["n_chains"] == al["n_alignments"] - got["n_bridges"] and got["n_bridges"] == got["n_bridges_inside"] + got["n_bridges_record"]
    assert int(got["chain_windows"].sum()) == al["n_placed"] and got["n_gap_windows"] == int(got["chain_gap_windows"].sum()) <= al["n_windows"] - al["n_placed"]
    assert int(got["chain_aln_offsets"][-1]) == al["n_alignments"] and int(got["chain_offsets"][-1]) == got["n_chains"]
    assert_same_chains(m.graph_chains(0, 0, skew, gap), got)                          # nothing depends on scheduling
    assert_same_chains(device_copy(R, m, m.graph_chains_device(0, 0, skew, gap)), got)
    assert m.chains_ms() >= m.alignments_ms() >= 0.0
    return got, exp


# ---- the hand-built cases and the random graphs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CG.CASE_IDS)
def test_hand_built_cases(name):
    R = _mdbg()
    c = CG.BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        for skew, gap in c.expect:
            got, exp = check(R, m, c.reads, c.k, nodes, ul, skew, gap)
            kinds = [[("-" if r == 0xFFFFFFFF else "I" if r == 0xFFFFFFFE else "R", int(e)) for r, e in
                      zip(got["bridge_record"][a:b].tolist(), got["bridge_entries"][a:b].tolist())] for a, b in zip(got["alignments"]["aln_offsets"][:-1].tolist(), got["alignments"]["aln_offsets"][1:].tolist())]
            assert [kinds[q] for q in c.probe] == c.expect[skew, gap]                   # the hand-written expectation, on the GPU's own arrays
        same_list(m.graph_unitigs(), ul, R)


def mutated_resident(seed):
    """a random graph of tests/sketch_graphs.py with its reads once more, mutated at 2 % per minimizer, resident behind them; at abundance 2 whatever the seed's: a
    k-min-mer seen once, as a mutated one is, is then no node and its window is unplaced"""
    k, _, presimp, reads = G.random_case(seed)
    return k, 2, presimp, reads + CG.mutated(reads, 0.02, seed)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_graphs_with_mutated_reads(seed):
    R = _mdbg()
    k, A, presimp, reads = mutated_resident(seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        n = 0
        for skew, gap in ((0, 0), (1, 0), (2, 3)):
            got, _ = check(R, m, reads, k, nodes, ul, skew, gap)
            n += got["n_bridges"]
        assert n > 0 or k == 2                                                           # (k = 2 over 40 values: nearly every pair is a node, nearly nothing is unplaced)


def test_monotone_in_both_parameters():
    R = _mdbg()
    k, A, presimp, reads = mutated_resident(4)
    m, nodes, ul = built(R, reads, k, A, 40, presimp)
    with m:
        bridged = {}
        for key in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (1, 2), (3, 4)):
            got = m.graph_chains(0, 0, *key)
            rec = got["bridge_record"]
            bridged[key] = {(int(a), int(rec[a]), int(got["bridge_entries"][a])) for a in np.flatnonzero(rec != 0xFFFFFFFF)}
        assert bridged[3, 0] and bridged[0, 0] != bridged[3, 0]
        for small, large in (((0, 0), (1, 0)), ((1, 0), (2, 0)), ((2, 0), (3, 0)), ((0, 1), (0, 2)), ((0, 2), (0, 0)), ((1, 2), (1, 0)), ((1, 2), (3, 4)), ((3, 4), (3, 0))):
            assert bridged[small] <= bridged[large], (small, large)


# ---- a read of 2,101 alignments: the scan and the per-chain sums over many workgroups ----------------------------------------------------------------------------
def spoilt_trunk(n_seg=1050):
    """a trunk of 8 n_seg + 8 minimizers (twice) with a side read (twice) at every eighth node that shares three trunk minimizers and leaves: unitigs of 8 nodes.
    The probe is the trunk with, per segment, the minimizer behind the fork SUBSTITUTED (the gap lies over the fork's record: dw = 4 = de) and one in the middle
    of the segment REMOVED (dw = 3, de = 4 inside the unitig): 2 n_seg + 1 alignments"""
    h = G.fresh(808, 10 * n_seg + 8)
    trunk, extra = h[:8 * n_seg + 8], h[8 * n_seg + 8:]
    new = G.fresh(809, n_seg)
    reads = [G.mread(trunk)] * 2
    probe = list(trunk)
    for f in range(n_seg):
        i = 4 + 8 * f
        reads += [G.mread(trunk[i - 1:i + 2] + extra[2 * f:2 * f + 2])] * 2
        probe[i + 1] = new[f]
        probe[i + 5] = None
    return reads + [G.mread([v for v in probe if v is not None])]


def test_a_read_of_2101_alignments_all_bridged_or_none():
    R = _mdbg()
    reads = spoilt_trunk()
    m, nodes, ul = built(R, reads, 3, 2, split=2)
    q = len(reads) - 1
    with m:
        exp = {key: expected(reads[q:], 3, nodes, ul, *key) for key in ((0, 0), (1, 0), (1, 1), (1, 2))}
        for (skew, gap), (inside, record) in {(0, 0): (0, 1050), (1, 0): (1050, 1050), (1, 1): (0, 0), (1, 2): (1050, 0)}.items():
            one = m.graph_chains(q, 1, skew, gap)                                        # the probe alone
            assert one["alignments"]["n_alignments"] == 2101 > 2048
            assert (one["n_bridges_inside"], one["n_bridges_record"], one["n_chains"]) == (inside, record, 2101 - inside - record)
            assert_same_chains(one, dict(shaped(exp[skew, gap], reads[q:], ul, q), alignments=dict(shaped(exp[skew, gap], reads[q:], ul, q)["alignments"], ordinal=np.array([q], np.uint64))))
        assert one["n_gap_windows"] == 2100 and m.graph_chains(q, 1, 1, 0)["chain_gap_windows"].tolist() == [1050 * 3 + 1050 * 2]
        check(R, m, reads, 3, nodes, ul, 1, 0)                                           # and the whole store: 2,100 clean reads in front of it


# ---- ranges ------------------------------------------------------------------------------------------------------------------------------------------------------
def concatenated(R, parts):
    from test_gpu_alignments import concatenated as alignments_concatenated
    out = {f: np.concatenate([p[f] for p in parts]) for f, _, _ in R.chains.CHAIN_FIELDS}
    for f, per in R.chains.CHAIN_OFFSETS:
        base, cols = 0, [np.zeros(1, np.uint64)]
        for p in parts:
            cols.append(p[f][1:] + np.uint64(base))
            base += int(p[f][-1])
        out[f] = np.concatenate(cols)
    out.update({f: sum(p[f] for p in parts) for f in R.chains.CHAIN_COUNTS}, alignments=alignments_concatenated(R, [p["alignments"] for p in parts]))
    return out


def test_a_partition_into_three_ranges_concatenates_and_the_ends_of_a_range():
    R = _mdbg()
    k, A, presimp, reads = mutated_resident(5)
    n = len(reads)
    m, nodes, ul = built(R, reads, k, A, split=50, presimp=presimp)
    with m:
        whole, _ = check(R, m, reads, k, nodes, ul, 1, 0)
        assert whole["n_bridges_inside"] > 0 and whole["n_bridges_record"] > 0
        parts = []
        for a, b in ((0, 17), (17, 183), (183, n)):
            got = m.graph_chains(a, b - a, 1, 0)
            want = shaped(expected(reads[a:b], k, nodes, ul, 1, 0), reads[a:b], ul, a)
            want["alignments"]["ordinal"] = np.arange(a, b, dtype=np.uint64)
            assert_same_chains(got, want)
            parts.append(got)
        assert_same_chains(concatenated(R, parts), whole)
        assert_zeros(R, m.graph_chains(n, 0, 1, 0), n)
        assert_zeros(R, m.graph_chains(n + 3, 2, 1, 0), n + 3)
        assert_same_chains(m.graph_chains(0, 1000 + n, 1, 0), whole)
    c = CG.BY_NAME["short and empty reads"]                                              # empty and short reads in front of, between and behind reads that chain
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split)
    with m:
        got, _ = check(R, m, c.reads, c.k, nodes, ul, 0, 0)
        assert np.diff(got["chain_offsets"].astype(np.int64)).tolist() == [0, 1, 0, 1, 0, 1, 1, 0, 1] and got["n_bridges"] == 3
        for a, b in ((0, 1), (2, 4), (3, 4), (8, 9), (4, 9), (7, 8)):                    # (8, 9), (4, 9): the last chain ends at the range's last index
            part = m.graph_chains(a, b - a, 0, 0)
            want = shaped(expected(c.reads[a:b], c.k, nodes, ul, 0, 0), c.reads[a:b], ul, a)
            want["alignments"]["ordinal"] = np.arange(a, b, dtype=np.uint64)
            assert_same_chains(part, want)


# ---- state, and what the call leaves alone -------------------------------------------------------------------------------------------------------------------------
def test_state_errors_and_what_the_call_leaves_alone():
    R = _mdbg()
    c = CG.BY_NAME["gap over a fork"]
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        assert "no current unitig list" in refused(m.graph_chains)
        from test_gpu_sketch_graphs import feed
        feed(m, c.reads)
        nodes = m.finalize()
        m.graph_edges(0.0)
        assert "no current unitig list" in refused(m.graph_chains)
        ul = m.graph_unitigs()
        comps, stats = m.graph_components(), m.stats()
        jx = m.graph_junctions_device()
        tr = m.graph_transits_device(0, 0, 1)
        addr = lambda p: R.api.C.cast(p, R.api.C.c_void_p).value
        held = lambda: (m.to_host(addr(jx.support), int(jx.n_records) * 8, np.uint64), m.to_host(addr(tr.count), int(tr.n_transits) * 8, np.uint64))
        before = held()
        got, _ = check(R, m, c.reads, c.k, nodes, ul, 0, 0)
        assert got["n_bridges_record"] == 1
        after = held()
        assert all(np.array_equal(x, y) for x, y in zip(before, after)) and before[0].sum() > 0
        same_list(m.graph_unitigs(), ul, R)
        after = m.graph_components()
        assert sorted(comps) == sorted(after) and all(np.array_equal(comps[f], after[f]) for f in comps) and m.stats() == stats
        again = m.finalize()
        assert all(np.array_equal(nodes[f], again[f]) for f in ("keys", "index", "abundance", "src_start", "src_end"))
    m, nodes, ul = built(R, c.reads, c.k, c.A)
    with m:
        al0 = m.graph_alignments()
        ch = m.graph_chains(0, 0, 0, 0)
        assert_same(ch["alignments"], al0)                                               # the list inside IS the alignment call's
        assert_same(m.graph_alignments(), al0)                                           # which returns afterwards what it returned before
        rp = m.graph_read_paths_device()
        dev = m.graph_chains_device(0, 0, 0, 0)
        addr = lambda p: R.api.C.cast(p, R.api.C.c_void_p).value
        assert addr(dev.alignments.first_window) == addr(rp.first_window) and int(dev.alignments.n_steps) == int(rp.n_steps)      # the step columns are the read-path result's
        assert m.L.mdbg_graph_chains(m.h, 0, 0, 0, 0, None) == m.L.mdbg_graph_chains(None, 0, 0, 0, 0, None) == -1 and m.L.mdbg_chains_ms(m.h, None) == -1
        assert m.L.mdbg_graph_chain_batch(m.h, None, None, 0, 0, 0, None) == -1
    import transit_graphs as TG
    c = TG.BY_NAME["cross r=8"]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        check(R, m, c.reads, c.k, nodes, ul, 1, 0)
        assert m.graph_simplify([(REPEATS, 2, 0)])["stats"]["entries_copied"] > 0        # a list with copies refuses
        assert "copies" in refused(lambda: m.graph_chains(0, 0, 1, 0))
        b, o = O.concat_reads([b"ACGT" * 50])
        assert "copies" in refused(lambda: m.chain_batch(b, o, 1, 0))
        m.graph_unitigs()
        check(R, m, c.reads, c.k, nodes, ul, 1, 0)                                       # the context still works
    with R.Mdbg(3, G.L, G.D, 2) as m:
        m.set_partition(2, 0)
        assert "single-GPU" in refused(m.graph_chains)
    with R.Mdbg(3, G.L, G.D, 1) as m:                                                    # an empty context: MDBG_OK and zeros
        m.finalize()
        m.graph_edges(0.0)
        m.graph_unitigs()
        assert_zeros(R, m.graph_chains())
        assert_zeros(R, m.graph_chains(5, 2, 1, 1), 5)
        assert m.chains_ms() == 0.0


# ---- base space: planted substitutions, resident and through chain_batch -------------------------------------------------------------------------------------------
def test_base_space_planted_substitutions_and_a_batch_that_is_not_resident():
    """the linear genome of tests/test_chains_cpu.py: every read once more with one planted substitution, as a batch that is NOT resident: at max_skew 1 every query
    is one chain with the clean read's coordinates, and the two aligned blocks differ at exactly the planted base.  chain_batch leaves the store as it was"""
    R = _mdbg()
    k, l, d, A = BASE_PARAMS
    genome, reads = linear_genome_input()
    queries, positions, _, _ = base_space_queries(reads, k, l, d, 11)
    with R.Mdbg(k, l, d, A, reads_already_hpc=True, keep_reads=True) as m:
        b, o = O.concat_reads([r.encode() for r in reads])
        m.ingest(b, o, 0)
        nodes = m.finalize()
        qb, qo, qsk = sketch_reads(m, queries)                                           # (before the list is made: a sketch ends it)
        _, _, sreads = sketch_reads(m, [r.encode() for r in reads])
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        assert ul["n_unitigs"] == 1
        seqs, lay = contig_strings(m), AL.layout_of_arrays(ul)
        stats0, view0 = m.stats(), (int(m.sketch_view().n_minimizers), int(m.sketch_view().n_reads))
        al0 = m.graph_alignments()
        cs = m.graph_contigs(0, device=True)                                             # a held contig result: its device arrays are read again behind the chain calls
        addr = lambda p: R.api.C.cast(p, R.api.C.c_void_p).value
        held_contigs = lambda: (m.to_host(addr(cs.bases), int(cs.n_bases), np.uint8), m.to_host(addr(cs.offsets), (int(cs.n_contigs) + 1) * 8, np.uint64))
        ctg0 = held_contigs()
        assert bytes(ctg0[0]).decode("latin-1") == "".join(seqs) and ctg0[1].tolist() == [0, len(seqs[0])]
        res = m.chain_batch(qb, qo, 1, 0)
        assert all(np.array_equal(x, y) for x, y in zip(ctg0, held_contigs()))
        exp = expected(qsk, k, nodes, ul, 1, 0, l)
        want = shaped(exp, queries, ul)
        assert_same_chains(res, want)
        assert res["alignments"]["ordinal"].tolist() == list(range(len(queries)))
        clean = AL.alignments(sreads, k, l, nodes, lay)
        n_bridged = check_planted(exp, clean, queries, positions, reads, lay, seqs, l)
        assert res["n_chains"] == len(queries) == res["n_bridges"] == n_bridged
        assert m.stats() == stats0 and (int(m.sketch_view().n_minimizers), int(m.sketch_view().n_reads)) == view0      # the store is rolled back
        same_list(m.graph_unitigs(), ul, R)
        assert_same(m.graph_alignments(), al0)
        assert_same_chains(m.chain_batch(qb, qo, 1, 0), res)
        dev = R.chains.ChainList()
        m._chk(m.L.mdbg_graph_chain_batch_device(m.h, qb.ctypes.data, qo.ctypes.data, len(qo) - 1, 1, 0, R.api.C.byref(dev)))
        assert int(dev.n_chains) == res["n_chains"] and np.array_equal(m.to_host(addr(dev.path_end), int(dev.n_chains) * 8, np.uint64), res["path_end"])
        assert_zeros(R, m.chain_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 1, 0))                             # an empty batch
        resident, _ = check(R, m, sreads, k, nodes, ul, 1, 0, l)                         # the clean reads resident: one chain each, no bridge
        assert resident["n_bridges"] == 0 and resident["n_chains"] == len(reads)
        assert all(np.array_equal(x, y) for x, y in zip(ctg0, held_contigs()))           # the contig result is what it was behind graph_chains too
        again = m.graph_contigs(0)
        assert np.array_equal(again["bases"], ctg0[0]) and np.array_equal(again["offsets"], ctg0[1])


def test_chain_batch_on_a_genome_with_a_repeat_and_a_ring():
    """the batch path over RECORD bridges: the genome with a two-copy repeat and the ring of tests/test_alignments_cpu.py (several unitigs, one circular), every
    sixth read with one planted substitution as a batch that is not resident, against the restatement"""
    from test_chains_cpu import ring_genome_queries
    R = _mdbg()
    k, l, d, A = BASE_PARAMS
    reads, queries, _ = ring_genome_queries()
    with R.Mdbg(k, l, d, A, reads_already_hpc=True) as m:
        b, o = O.concat_reads(reads)
        m.ingest(b, o, 0)
        nodes = m.finalize()
        qb, qo, qsk = sketch_reads(m, queries)
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        assert ul["circular"].tolist().count(1) == 1 and ul["n_unitigs"] >= 4
        for skew in (0, 1):
            res = m.chain_batch(qb, qo, skew, 0)
            assert_same_chains(res, shaped(expected(qsk, k, nodes, ul, skew, 0, l), queries, ul))
        assert res["n_bridges_inside"] > 0 and res["n_bridges_record"] > 0 and res["n_chains"] == len(queries)
        same_list(m.graph_unitigs(), ul, R)


# ---- pipeline and the C program ------------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_files_and_the_c_program(example_reads, tmp_path):
    """tests/golden/reads-0.00.fa.gz with its first 20 reads as the query file: the .chains.gaf, .query.chains.gaf and .query.chains.tsv of run_file are the
    independent formatter's lines on the restatement's chains, the C program writes the same bytes, and the .gaf files of a run without `chains` are unchanged"""
    from rust_mdbg_amd import pipeline
    from test_gpu_unitigs import build_cli
    R = _mdbg()
    k, l, d, A = 7, 10, 0.0008, 2
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    qsrc = str(tmp_path / "query.fa")
    sk = O.sketch(*O.concat_reads(example_reads[:20]), l, d)                               # the reads are error-free: each query gets one base spoilt inside its middle minimizer
    queries = []
    for q, r in enumerate(example_reads[:20]):
        pos = sk["pos"][int(sk["off"][q]):int(sk["off"][q + 1])].tolist()
        p = pos[len(pos) // 2] + l // 2
        queries.append(r[:p] + b"ACGT"[(b"ACGT".index(r[p:p + 1]) + 1) % 4:][:1] + r[p + 1:])
    with open(qsrc, "w") as f:
        f.write("".join(">q%d\n%s\n" % (i, r.decode()) for i, r in enumerate(queries)))
    prefix, plain = str(tmp_path / "py"), str(tmp_path / "plain")
    steps = R.api.MAGIC_SIMPLIFY_STEPS
    common = dict(write_sequences=False, contigs=True, keep_reads=True, simplify=steps, gaf=True, query=qsrc, batch_bases=5_000_000)
    out = pipeline.run_file(src, prefix, k, l, d, A, chains=(1, 0), **common)
    without = pipeline.run_file(src, plain, k, l, d, A, **common)
    assert {f for f in out if f not in without} == {n + s for n in ("n_chains", "n_bridges", "n_query_chains", "n_query_bridges") for s in ("", "_simplified")}
    assert all(out[f] == without[f] for f in without if not f.startswith("seconds") and isinstance(without[f], (int, bool)))
    for name in ("unitigs.gaf", "msimpl.gaf", "unitigs.query.gaf", "unitigs.query.tsv", "msimpl.query.gaf", "msimpl.query.tsv", "unitigs.gfa", "msimpl.gfa"):
        assert open("%s.%s" % (prefix, name), "rb").read() == open("%s.%s" % (plain, name), "rb").read(), name
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("plain.") and "chains" in f]
    b, o = O.concat_reads(example_reads)
    want = {}
    with R.Mdbg(k, l, d, A) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        _, _, sreads = sketch_reads(m, example_reads)
        _, _, qreads = sketch_reads(m, queries)
        m.graph_edges(0.01)
        for kind in ("msimpl", "unitigs"):
            ul = m.graph_simplify(steps) if kind == "msimpl" else m.graph_unitigs()
            circ = ul["circular"].astype(bool).tolist()
            exp = expected(sreads, k, nodes, ul, 1, 0, l)
            qexp = expected(qreads, k, nodes, ul, 1, 0, l)
            want[kind + ".chains.gaf"] = "".join(CH.gaf_lines(exp, range(len(example_reads)), [len(r) for r in example_reads], circ))
            want[kind + ".query.chains.gaf"] = "".join(CH.gaf_lines(qexp, range(20), [len(r) for r in queries], circ))
            rows = [(q, W, sum(r[2] for r in rows), sum(r[3] for r in rows)) for q, (W, rows) in enumerate(zip(qexp["a"]["windows"], qexp["chains"]))]
            want[kind + ".query.chains.tsv"] = "".join("%d\t%d\t%d\t%d\t%.2f\n" % (q, W, p, g, 100.0 * (p + g) / W if W else 0.0) for q, W, p, g in rows)
            s = "_simplified" if kind == "msimpl" else ""
            assert (out["n_chains" + s], out["n_bridges" + s], out["n_query_chains" + s], out["n_query_bridges" + s]) == (exp["n_chains"], exp["n_bridges"], qexp["n_chains"], qexp["n_bridges"])
    print({f: out[f] for f in out if "chains" in f or "bridges" in f or "alignments" in f})
    assert out["n_query_bridges"] > 0 and out["n_query_chains"] < out["n_query_alignments"] and out["n_chains"] == out["n_alignments"]      # the resident reads are error-free
    for name, text in want.items():
        assert open("%s.%s" % (prefix, name)).read() == text, name
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "c")
    r = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--prefix", cpre, "--no-basespace", "--simplify", "--gaf", "--chains", "1",
                        "--query", qsrc], check=True, capture_output=True, text=True)
    for name in list(want) + ["unitigs.gaf", "msimpl.gaf", "unitigs.query.gaf", "unitigs.query.tsv"]:
        assert open("%s.%s" % (cpre, name), "rb").read() == open("%s.%s" % (prefix, name), "rb").read(), name
    lines = r.stdout.split("\n")
    assert any(ln.startswith("chains: ") for ln in lines) and any(ln.startswith("chains (simplified): ") for ln in lines) and any(ln.startswith("query chains: 20 sequences") for ln in lines)
