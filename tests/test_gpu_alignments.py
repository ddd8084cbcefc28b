"""Alignments on the GPU (Mdbg.graph_alignments, Mdbg.align_batch) against the plain restatement (tests/alignments_restatement.py), exactly: every count, every
column element for element with its dtype — on the catalogue of tests/sketch_graphs.py (plain and simplified lists), the random graphs, the shapes at which the
kernels can still go wrong, a ring, a cut, ranges of reads, the state checks, base space (the arbiter of the coordinate definition), queries that are not resident,
the pipeline's files and the C program's.  CPU side: tests/test_alignments_cpu.py."""
import os
import random
import subprocess

import numpy as np
import pytest

import alignments_restatement as AL
import sketch_graphs as G
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from test_alignments_cpu import as_result, base_space_input, check_base_space, read_lengths
from test_gpu_parity import _mdbg
from test_gpu_read_paths import built, distinct_hashes
from test_gpu_simplify import same_list
from test_gpu_sketch_graphs import BY_NAME, feed
from test_repeats_cpu import BASE_PARAMS

pytestmark = pytest.mark.gpu

E_PARAM, E_ALPHABET, E_STATE = -1, -2, -6
EDGES, REPEATS = 8, 16


def counts(R):
    return R.align.ALIGNMENT_COUNTS


def expected(reads, k, nodes, ul, l=G.L):
    return AL.alignments(reads, k, l, nodes, AL.layout_of_arrays(ul))


def assert_same(a, b):
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]) and np.asarray(a[f]).dtype == np.asarray(b[f]).dtype, f


def assert_zeros(R, got, first=0):
    assert got["first_read"] == first and got["n_unitigs"] == 0 and all(got[f] == 0 for f in counts(R)) and all(len(got[f]) == 0 for f, _, _ in R.align.ALIGNMENT_FIELDS)
    assert all(got[f].tolist() == [0] for f, _ in R.align.ALIGNMENT_OFFSETS)


def shaped(exp, reads, ul, first=0):
    return dict(as_result(exp, reads, first), n_unitigs=int(ul["n_unitigs"]))


def device_copy(R, m, dev):
    """an AlignmentList with DEVICE pointers -> the dict graph_alignments gives, every array copied back"""
    n = dict(read=int(dev.n_reads), step=int(dev.n_steps), alignment=int(dev.n_alignments))
    addr = lambda p: R.api.C.cast(p, R.api.C.c_void_p).value
    out = {f: m.to_host(addr(getattr(dev, f)), n[per] * np.dtype(t).itemsize, t) if n[per] else np.zeros(0, t) for f, t, per in R.align.ALIGNMENT_FIELDS}
    out.update({f: m.to_host(addr(getattr(dev, f)), (n[per] + 1) * 8, np.uint64) for f, per in R.align.ALIGNMENT_OFFSETS})
    out.update({f: int(getattr(dev, f)) for f in counts(R)}, first_read=int(dev.first_read), n_unitigs=int(dev.n_unitigs))
    return out


def check(R, m, reads, k, nodes, ul, l=G.L):
    """the context's current list is `ul` (host arrays): the whole store's alignments equal the restatement's, twice from the host variant and once from the device
    variant, and the invariants hold against the junction call; -> (got, exp)"""
    got = m.graph_alignments()
    if ul["n_unitigs"] == 0:                                                        # a schedule that removed everything: the empty list gives zeros
        assert_zeros(R, got)
        return got, None
    exp = expected(reads, k, nodes, ul, l)
    print(" ".join("%s %d" % (f, got[f]) for f in counts(R)))
    assert_same(got, shaped(exp, reads, ul))
    jx = m.graph_junctions()
    assert got["n_alignments"] == got["n_steps"] - got["n_chained"] and jx["n_explained"] == got["n_chained"] + got["n_wraps"]
    assert int(got["aln_step_offsets"][-1]) == got["n_steps"] and int(got["aln_offsets"][-1]) == got["n_alignments"]
    assert_same(m.graph_alignments(), got)                                          # nothing depends on scheduling
    assert_same(device_copy(R, m, m.graph_alignments_device()), got)
    assert m.alignments_ms() >= 0.0
    return got, exp


# ---- the catalogue and the random graphs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_catalogue_on_the_plain_and_on_every_simplified_list(name):
    R = _mdbg()
    c = BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimps[0])
    with m:
        got, _ = check(R, m, c.reads, c.k, nodes, ul)
        if c.presimps[0] == 0.0:                                                    # no missing key: the alignments of a read are separated by unplaced windows only
            assert m.graph_junctions()["n_missing"] == 0
            so, ao = got["step_offsets"].tolist(), got["aln_offsets"].tolist()
            for q, W in enumerate(got["read_windows"].tolist()):
                if W and int(got["step_windows"][so[q]:so[q + 1]].sum()) == W:
                    assert ao[q + 1] - ao[q] == 1, q
        same_list(m.graph_unitigs(), ul, R)                                         # the call left the list as it was
        for steps in c.schedules:
            simp = m.graph_simplify(steps)                                          # the simplified list is now the current one
            check(R, m, c.reads, c.k, nodes, simp)
            same_list(m.graph_simplify(steps), simp, R)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_minimizer_space_graphs(seed):
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        got, exp = check(R, m, reads, k, nodes, ul)
        assert got["n_alignments"] > 0 and got["n_chained"] > 0


# ---- shapes at which the kernels can still go wrong (k = 3) ----------------------------------------------------------------------------------------------------
def test_two_long_reads_cross_every_workgroup_span():
    """5,000 fresh minimizers and the same read from the other strand: one unitig, one step and one alignment per read, across every span of 256 and 1,024 indices"""
    R = _mdbg()
    h = distinct_hashes(1, 5000)
    reads = [G.mread(h), G.mread(h, rev=True)]
    m, nodes, ul = built(R, reads, 3, 1)
    with m:
        got, _ = check(R, m, reads, 3, nodes, ul)
        assert got["n_alignments"] == 2 and got["aln_windows"].tolist() == [4998, 4998] and got["path_length"].tolist() == [499910] * 2
        assert got["query_begin"].tolist() == [0, 0] and got["query_end"].tolist() == [499910] * 2 and got["path_begin"].tolist() == [0, 0] and got["path_end"].tolist() == [499910] * 2


def forked_trunk(n_forks=2100, side=3):
    """a trunk read of 2 n_forks + 8 minimizers once, and at every second trunk node a side read (three times) that shares three trunk minimizers and leaves: the
    trunk is cut into unitigs of two nodes.  On edges of presimp 0 every cut has its record; at presimp 0.5 the trunk's own record goes at every fork (the side
    node is three times as abundant), so the trunk read crosses n_forks missing keys"""
    h = random.Random(21).sample(range(1, G.HASH_LIMIT), 4 * n_forks + 8)
    trunk, extra = h[:2 * n_forks + 8], h[2 * n_forks + 8:]
    reads = [G.mread(trunk)]
    for f in range(n_forks):
        i = 2 + 2 * f
        reads += [G.mread(trunk[i - 1:i + 2] + extra[2 * f:2 * f + 2])] * side
    return reads


@pytest.mark.parametrize("presimp,chained", [(0.0, True), (0.5, False)])
def test_a_read_of_2101_steps_all_chained_or_none(presimp, chained):
    """both scans and the per-alignment accumulation cross workgroups: one alignment of 2,101 steps, or 2,101 alignments of one"""
    R = _mdbg()
    reads = forked_trunk()
    m, nodes, ul = built(R, reads, 3, 1, split=1, presimp=presimp)
    with m:
        got, _ = check(R, m, reads, 3, nodes, ul)
        one = m.graph_alignments(0, 1)                                              # the trunk read alone: the range ends inside the store
        assert one["n_steps"] == 2101 > 2048 and one["n_windows"] == one["n_placed"] == 4206
        assert (one["n_chained"], one["n_alignments"]) == ((2100, 1) if chained else (0, 2101))
        assert_same(one, shaped(expected(reads[:1], 3, nodes, ul), reads[:1], ul))
        if chained:
            assert one["aln_windows"].tolist() == [4206] and one["path_begin"].tolist() == [0] and one["path_end"].tolist() == one["path_length"].tolist() == one["query_end"].tolist()


def test_short_reads_empty_reads_and_the_ends_of_a_range():
    """reads with exactly k and k + 1 minimizers and with none, in front of, between and behind reads that align; the first and the last read of a range, and an
    alignment that ends at the range's last index"""
    R = _mdbg()
    h = distinct_hashes(31, 40)
    body = G.mread(h[:30])
    reads = [G.mread([]), G.mread(h[:3]), G.mread(h[:4]), body, G.mread([]), G.mread(h[10:13]), G.mread(h[5:9], rev=True), G.mread([]), body]
    m, nodes, ul = built(R, reads, 3, 1, split=4)
    with m:
        got, exp = check(R, m, reads, 3, nodes, ul)
        assert np.diff(got["aln_offsets"].astype(np.int64)).tolist() == [0, 0, 1, 1, 0, 0, 1, 0, 1] and got["read_windows"].tolist() == [0, 0, 2, 28, 0, 0, 2, 0, 28]
        n = len(reads)
        for a, b in ((0, 1), (1, 3), (2, 4), (8, 9), (3, 9), (6, 7), (4, 6)):       # (8, 9) and (3, 9): the last alignment ends at the range's last index
            part = m.graph_alignments(a, b - a)
            assert_same(part, dict(shaped(expected(reads[a:b], 3, nodes, ul), reads[a:b], ul, a), ordinal=np.arange(a, b, dtype=np.uint64)))
        assert_zeros(R, m.graph_alignments(n, 0), n)
        assert_zeros(R, m.graph_alignments(n + 3, 2), n + 3)


# ---- a ring ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_ring_of_four_entries_walked_two_and_a_half_times_on_either_strand():
    """12 minimizers round a ring of 4: 10 windows, one step, one alignment, two wraps, the unitig listed three times; nodes of 210 bases 100 apart: the ring has
    510 bases, its closing record overlaps 102 + 8, the path 3 * 510 - 2 * 110 = 1310 bases, and the alignment covers the read's 1110"""
    R = _mdbg()
    ring = sorted(distinct_hashes(41, 4))                                           # ascending: the first window is canonical as read, the ring starts there on strand 0
    reads = [G.mread(ring * 3), G.mread(ring * 3, rev=True)]
    m, nodes, ul = built(R, reads, 3, 1)
    with m:
        got, exp = check(R, m, reads, 3, nodes, ul)
        assert ul["n_unitigs"] == 1 and ul["circular"].tolist() == [1] and ul["n_entries"] == 4 and ul["length"].tolist() == [510]
        assert (got["n_steps"], got["n_alignments"], got["n_wraps"], got["n_chained"]) == (2, 2, 4, 0) and got["step_windows"].tolist() == [10, 10]
        assert sorted(got["strand"].tolist()) == [0, 1] and got["step_record"].tolist() == [0xFFFFFFFF] * 2
        assert got["path_length"].tolist() == [1310, 1310] and (got["path_end"] - got["path_begin"]).tolist() == [1110, 1110] == (got["query_end"] - got["query_begin"]).tolist()
        assert [len(r[0][5]) for r in exp["alns"]] == [3, 3]                        # three occurrences each
        assert ul["edges"]["n1"].tolist() == ul["edges"]["n2"].tolist() == [0, 0] and ul["edges"]["overlap"].tolist() == [102, 102]      # the closing record and its mirror


# ---- a cut -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_an_alignment_is_cut_exactly_at_a_missing_key():
    """edges built at a presimp that removes the small branch's records (presimp 200/1 at 0.01), and a list after an EDGES step: graph_junctions reports a missing
    key, and the read that crosses it has two alignments that meet there"""
    R = _mdbg()
    c = BY_NAME["presimp 200/1 at 0.01"]
    m, nodes, ul = built(R, c.reads, c.k, c.A, presimp=0.01)
    with m:
        got, exp = check(R, m, c.reads, c.k, nodes, ul)
        jx = m.graph_junctions()
        assert jx["n_missing"] == 1 and jx["n_missing_crossings"] == 1 and got["n_chained"] == 0
        a0, a1 = got["aln_offsets"][200:202].tolist()
        assert a1 - a0 == 2 and got["aln_windows"][a0:a1].tolist() == [3, 3]
        s0 = int(got["aln_step_offsets"][a0])                                       # the cut: the last window of the first and the first of the second are the missing key's pair
        assert (int(got["unitig"][s0]), int(got["first_entry"][s0]) + 2, int(got["unitig"][s0 + 1]), int(got["first_entry"][s0 + 1])) == (
            int(jx["missing_unitig1"][0]), int(jx["missing_entry1"][0]), int(jx["missing_unitig2"][0]), int(jx["missing_entry2"][0]))
        assert got["query_end"][a0] == 410 and got["query_begin"][a0 + 1] == 300
    k, A, presimp, reads = G.random_case(6)                                         # seed 6 has 64 missing keys on its plain list; an EDGES step removes records on top
    m, nodes, ul = built(R, reads, k, A, 40, presimp)
    with m:
        simp = m.graph_simplify([(EDGES, 2, 0)])
        got, exp = check(R, m, reads, k, nodes, simp)
        assert m.graph_junctions()["n_missing"] > 0 and got["n_alignments"] > 0


# ---- ranges ------------------------------------------------------------------------------------------------------------------------------------------------------
def concatenated(R, parts, first=0):
    out = {f: np.concatenate([p[f] for p in parts]) for f, _, _ in R.align.ALIGNMENT_FIELDS}
    for f, per in R.align.ALIGNMENT_OFFSETS:                                        # the offsets shifted by what came before
        base, cols = 0, [np.zeros(1, np.uint64)]
        for p in parts:
            cols.append(p[f][1:] + np.uint64(base))
            base += int(p[f][-1])
        out[f] = np.concatenate(cols)
    out.update({f: sum(p[f] for p in parts) for f in counts(R)}, first_read=first, n_unitigs=parts[0]["n_unitigs"])
    return out


@pytest.mark.parametrize("seed", [1, 6])
def test_a_partition_into_three_ranges_concatenates(seed):
    """the reads fed as two batches; three ranges, the second of which starts inside the first batch and ends inside the second"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    n, cut = len(reads), 50
    m, nodes, ul = built(R, reads, k, A, split=cut, presimp=presimp)
    with m:
        whole, _ = check(R, m, reads, k, nodes, ul)
        parts = []
        for a, b in ((0, 17), (17, 83), (83, n)):
            got = m.graph_alignments(a, b - a)
            assert_same(got, dict(shaped(expected(reads[a:b], k, nodes, ul), reads[a:b], ul, a), ordinal=np.arange(a, b, dtype=np.uint64)))
            parts.append(got)
        assert_same(concatenated(R, parts), whole)
        assert_zeros(R, m.graph_alignments(n, 0), n)
        assert_same(m.graph_alignments(0, 1000), whole)


# ---- state -------------------------------------------------------------------------------------------------------------------------------------------------------
def refused(call, code=E_STATE):
    with pytest.raises(_mdbg().MdbgError) as e:
        call()
    assert e.value.code == code
    return str(e.value)


def test_state_errors_and_what_the_call_leaves_alone():
    R = _mdbg()
    c = BY_NAME["fork"]
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        assert "no current unitig list" in refused(m.graph_alignments)              # nothing yet
        feed(m, c.reads)
        nodes = m.finalize()
        m.graph_edges(0.0)
        assert "no current unitig list" in refused(m.graph_alignments)
        ul = m.graph_unitigs()
        comps = m.graph_components()
        jx = m.graph_junctions_device()                                             # a held junction result
        addr = lambda p: R.api.C.cast(p, R.api.C.c_void_p).value
        held = lambda: m.to_host(addr(jx.support), int(jx.n_records) * 8, np.uint64)
        before = held()
        got, _ = check(R, m, c.reads, c.k, nodes, ul)
        same_list(m.graph_unitigs(), ul, R)
        after = m.graph_components()
        assert sorted(comps) == sorted(after) and all(np.array_equal(comps[f], after[f]) for f in comps)
        jx2 = m.graph_alignments_device()
        assert np.array_equal(before, held()) and before.sum() > 0
        # afterwards the read-path result is this call's result: the step columns of the list are the read-path buffers, and equal a read-path call's
        rp = m.graph_read_paths()
        for f in ("first_window", "step_windows", "unitig", "first_entry", "strand", "ordinal", "read_windows", "step_offsets"):
            assert np.array_equal(rp[f], got[f]), f
        part = m.graph_alignments(5, 2)
        rp = m.graph_read_paths_device(5, 2)
        dev = m.graph_alignments_device(5, 2)
        assert addr(dev.first_window) == addr(rp.first_window) and addr(dev.strand) == addr(rp.strand) and int(dev.n_steps) == int(rp.n_steps) == part["n_steps"]
        del jx2
        m.graph_simplify([(REPEATS, 1, 0)])                                         # nothing resolves on a fork: no copies, the call works
        m.graph_alignments()
        assert m.L.mdbg_graph_alignments(m.h, 0, 0, None) == m.L.mdbg_graph_alignments(None, 0, 0, None) == E_PARAM and m.L.mdbg_alignments_ms(m.h, None) == E_PARAM
    import transit_graphs as TG
    c = TG.BY_NAME["cross r=8"]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        check(R, m, c.reads, c.k, nodes, ul)
        assert m.graph_simplify([(REPEATS, 2, 0)])["stats"]["entries_copied"] > 0   # a list with copies
        assert "copies" in refused(m.graph_alignments)
        b, o = O.concat_reads([b"ACGT" * 50])
        assert "copies" in refused(lambda: m.align_batch(b, o))
        m.graph_unitigs()
        check(R, m, c.reads, c.k, nodes, ul)                                        # the context still works
    c = BY_NAME["fork"]
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        m.set_partition(2, 0)
        assert "single-GPU" in refused(m.graph_alignments)
        b, o = O.concat_reads([b"ACGT" * 50])
        assert "single-GPU" in refused(lambda: m.align_batch(b, o))
    with R.Mdbg(3, G.L, G.D, 1) as m:                                               # an empty context: MDBG_OK and zeros
        m.finalize()
        m.graph_edges(0.0)
        m.graph_unitigs()
        assert_zeros(R, m.graph_alignments())
        assert_zeros(R, m.graph_alignments(5, 2), 5)
        assert m.alignments_ms() == 0.0


# ---- base space, the arbiter of the coordinate definition, and queries that are not resident --------------------------------------------------------------------
def contig_strings(m):
    ctg = m.graph_contigs(0)
    offs = ctg["offsets"].tolist()
    return [bytes(ctg["bases"][x:y]).decode("latin-1") for x, y in zip(offs, offs[1:])]


def sketch_reads(m, reads):
    b, o = O.concat_reads(reads)
    sk = m.sketch(b, o)
    off = sk["off"].tolist()
    return b, o, [(tuple(sk["hashes"][x:y].tolist()), tuple(sk["pos"][x:y].tolist())) for x, y in zip(off, off[1:])]


def revcomp(s):
    import unitig_restatement as U
    return U.revcomp(s)


def test_base_space_and_a_batch_that_is_not_resident():
    """the genome and the ring of tests/test_alignments_cpu.py, reads of 5 kb at 20x: for every alignment the bases [path_begin, path_end) of the path's sequence —
    the unitig sequences of graph_contigs joined over the records — are the bases [query_begin, query_end) of the read.  Then align_batch on the same context"""
    R = _mdbg()
    k, l, d, A = BASE_PARAMS
    genome, ring, reads = base_space_input()
    rnd = random.Random(77)
    piece = lambda src, n: (lambda a: src[a:a + n])(rnd.randrange(0, len(src) - n))
    pieces = [piece(genome, 7001), piece(genome, 2500), (ring + ring)[1000:32000], genome[15000:24000]]       # the last two: once round the ring and 1,000 bases more; across the repeat's first copy
    chimera = genome[3000:6000] + genome[40000:43000]
    with R.Mdbg(k, l, d, A, reads_already_hpc=True, keep_reads=True) as m:
        b, o = O.concat_reads(reads)
        m.ingest(b, o, 0)
        nodes = m.finalize()
        # a query with exactly k minimizers: the shortest prefix of a piece that has k (found on the sketch of the prefixes)
        probe = [pieces[0][:n].encode() for n in range(30, 400, 2)]
        n_min = [len(h) for h, _ in sketch_reads(m, probe)[2]]
        assert k in n_min
        exactly_k = probe[n_min.index(k)]
        queries = [p.encode() for p in pieces] + [revcomp(p).encode() for p in pieces] + ["".join(rnd.choice("ACGT") for _ in range(4000)).encode(), chimera.encode(), exactly_k, b""]
        qb, qo, qsk = sketch_reads(m, queries)                                      # (before the list is made: a sketch ends it, as every ingest does)
        _, _, sreads = sketch_reads(m, reads)
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        seqs = contig_strings(m)
        lay = AL.layout_of_arrays(ul)
        got, exp = check(R, m, sreads, k, nodes, ul, l)
        assert ul["circular"].tolist().count(1) == 1 and ul["n_unitigs"] >= 4
        multi, wrapped = check_base_space(exp, reads, lay, seqs, l)
        print("alignments %d, of two steps or more %d, wrapping %d, wraps %d" % (got["n_alignments"], multi, wrapped, got["n_wraps"]))
        # ---- align_batch: nothing but the alignment and the read-path result changes
        stats0, view0 = m.stats(), (int(m.sketch_view().n_minimizers), int(m.sketch_view().n_reads))
        rp0 = m.graph_read_paths()
        jx = m.graph_junctions_device()
        addr = lambda p: R.api.C.cast(p, R.api.C.c_void_p).value
        sup0 = m.to_host(addr(jx.support), int(jx.n_records) * 8, np.uint64)
        res = m.align_batch(qb, qo)
        qexp = expected(qsk, k, nodes, ul, l)
        assert_same(res, dict(shaped(qexp, queries, ul), first_read=0))
        assert res["ordinal"].tolist() == list(range(len(queries)))
        assert_same(m.align_batch(qb, qo), res)
        n_p = len(pieces)
        per_query = np.diff(res["aln_offsets"].astype(np.int64)).tolist()
        assert per_query[:2 * n_p] == [1] * (2 * n_p) and per_query[2 * n_p:] == [0, 2, 0, 0], per_query
        for q in range(len(queries)):
            check_base_space_rows(qexp, q, queries, lay, seqs, l)
        for q in range(n_p):                                                        # the reverse complement walks the mirror path: the same bases
            f, r = qexp["alns"][q][0], qexp["alns"][q + n_p][0]
            assert [(u, 1 - s) for u, s in reversed(f[5])] == r[5] and f[6] == r[6] and (f[7], f[8]) == (r[6] - r[8], r[6] - r[7])
        assert res["read_windows"][-2:].tolist() == [0, 0] and res["n_wraps"] >= 2
        assert m.stats() == stats0 and (int(m.sketch_view().n_minimizers), int(m.sketch_view().n_reads)) == view0
        assert np.array_equal(sup0, m.to_host(addr(jx.support), int(jx.n_records) * 8, np.uint64))
        same_list(m.graph_unitigs(), ul, R)
        assert_same(m.graph_read_paths(), rp0)
        assert_zeros(R, m.align_batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64)))      # an empty batch
        # a byte outside the alphabet answers as query_batch does, and the context still works
        bad_b, bad_o = O.concat_reads([pieces[0][:3000].encode(), (pieces[1][:1000] + "X" + pieces[1][1000:2000]).encode()])
        refused(lambda: m.align_batch(bad_b, bad_o), E_ALPHABET)
        assert_same(m.align_batch(qb, qo), res)
        assert_same(m.graph_alignments(), got)
        assert m.stats() == stats0
        refused(lambda: m.query(bad_b, bad_o), E_ALPHABET)
        nd = R.api.Nodes()
        m._chk(m.L.mdbg_finalize_device(m.h, R.api.C.byref(nd)))
        digest = m.nodes_digest(nd)
    with R.Mdbg(k, l, d, A, reads_already_hpc=True) as m2:                          # the node table is the one a context gives that never saw a query
        m2.ingest(b, o, 0)
        nd = R.api.Nodes()
        m2._chk(m2.L.mdbg_finalize_device(m2.h, R.api.C.byref(nd)))
        assert m2.nodes_digest(nd) == digest


def check_base_space_rows(a, q, reads, lay, seqs, l):
    from test_alignments_cpu import path_sequence
    read = reads[q].decode()
    for first, n, windows, qb, qe, occ, plen, pb, pe in a["alns"][q]:
        seq, n_occ = path_sequence(a["steps"][q][first:first + n], lay, seqs, l)
        assert len(seq) == plen and n_occ == len(occ) and seq[pb:pe] == read[qb:qe], (q, first)


# ---- pipeline and the C program ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,l,d,A", [(7, 10, 0.0008, 2), (3, 10, 0.002, 1)])
def test_pipeline_files_and_the_c_program(example_reads, tmp_path, k, l, d, A):
    """tests/golden/reads-0.00.fa.gz with its first 20 reads as the query file: the .gaf, .query.gaf and .query.tsv of run_file, for the plain and the simplified
    list, are the independent formatter's lines on the restatement's alignments, and the C program writes the same bytes"""
    from rust_mdbg_amd import pipeline
    from test_gpu_unitigs import build_cli
    R = _mdbg()
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    qsrc = str(tmp_path / "query.fa")
    queries = example_reads[:20]
    with open(qsrc, "w") as f:
        f.write("".join(">q%d\n%s\n" % (i, r.decode()) for i, r in enumerate(queries)))
    prefix = str(tmp_path / "py")
    steps = R.api.MAGIC_SIMPLIFY_STEPS
    out = pipeline.run_file(src, prefix, k, l, d, A, write_sequences=False, contigs=True, keep_reads=True, simplify=steps, gaf=True, query=qsrc, batch_bases=5_000_000)
    b, o = O.concat_reads(example_reads)
    want = {}
    with R.Mdbg(k, l, d, A) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        _, _, sreads = sketch_reads(m, example_reads)
        m.graph_edges(0.01)
        for kind in ("msimpl", "unitigs"):
            ul = m.graph_simplify(steps) if kind == "msimpl" else m.graph_unitigs()
            circ = ul["circular"].astype(bool).tolist()
            exp = expected(sreads, k, nodes, ul, l)
            qexp = expected(sreads[:20], k, nodes, ul, l)
            want[kind + ".gaf"] = "".join(AL.gaf_lines(exp, range(len(example_reads)), [len(r) for r in example_reads], circ))
            want[kind + ".query.gaf"] = "".join(AL.gaf_lines(qexp, range(20), [len(r) for r in queries], circ))
            want[kind + ".query.tsv"] = "".join("%d\t%d\t%d\t%.2f\n" % (q, W, p, 100.0 * p / W if W else 0.0) for q, (W, p) in enumerate(zip(qexp["windows"], qexp["placed"])))
            assert out["n_alignments" + ("_simplified" if kind == "msimpl" else "")] == exp["n_alignments"]
            assert out["n_query_alignments" + ("_simplified" if kind == "msimpl" else "")] == qexp["n_alignments"]
    assert out["n_queries"] == 20 and want["unitigs.gaf"].count("\n") > 0 and want["unitigs.query.gaf"].count("\n") > 0
    for name, text in want.items():
        assert open("%s.%s" % (prefix, name)).read() == text, name
    assert all(float(ln.split("\t")[3]) == 100.0 for ln in want["unitigs.query.tsv"].splitlines() if A == 1 and int(ln.split("\t")[1]))      # A = 1: every k-min-mer of a read is a node
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "c")
    r = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--prefix", cpre, "--no-basespace", "--simplify", "--gaf", "--query", qsrc],
                       check=True, capture_output=True, text=True)
    for name in want:
        assert open("%s.%s" % (cpre, name), "rb").read() == open("%s.%s" % (prefix, name), "rb").read(), name
    assert any(ln.startswith("alignments: ") for ln in r.stdout.split("\n")) and any(ln.startswith("query (simplified): 20 sequences") for ln in r.stdout.split("\n"))
