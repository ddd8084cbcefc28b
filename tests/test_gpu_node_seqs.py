"""Node sequences gathered on the GPU from the kept reads (mdbg_graph_node_seqs) and the .sequences files written from them.  The checker everywhere is the host
rule applied to the original reads — reads[src_read][src_start:src_end], through utils::revcomp where `reversed` — computed here from the node table
m.finalize() returned (which tests/test_gpu_parity.py and tests/test_gpu_fuzz.py pin to the oracle), never by the code under test.  Equality is exact (bytes)."""
import functools
import random
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from test_emit_cpu import read_lz4_frame
from test_gpu_fuzz import fuzz_reads
from test_gpu_parity import _mdbg
from test_gpu_unitigs import build_cli, write_fasta
from test_unitigs_cpu import fuzz_case, synth_case

pytestmark = pytest.mark.gpu

REVCOMP = bytes(dict(zip(b"acgtuACGTU", b"tgcaaTGCAA")).get(c, ord("N")) for c in range(256))      # switch_base, src/utils.rs:10-24


def checker(reads, nodes):
    """-> the sequence of every row, by the host rule"""
    out = []
    for r, a, b, rev in zip(nodes["src_read"].tolist(), nodes["src_start"].tolist(), nodes["src_end"].tolist(), nodes["reversed"].tolist()):
        s = reads[r][a:b]
        out.append(s[::-1].translate(REVCOMP) if rev else s)
    return out


def rows_of(g):
    """a graph_node_seqs() dict -> list of bytes"""
    b, o = g["bases"].tobytes(), g["offsets"].astype(np.int64)
    assert len(o) == g["n_rows"] + 1 and o[0] == 0 and o[-1] == g["n_bases"] == len(b)
    return [b[o[i]:o[i + 1]] for i in range(g["n_rows"])]


def three_batches(reads):
    """the reads as three batches in the order 2, 0, 1: [(first ordinal, reads of the batch)]"""
    n = len(reads)
    cuts = [0, n // 3, 2 * n // 3, n]
    return [(cuts[p], reads[cuts[p]:cuts[p + 1]]) for p in (2, 0, 1)]


def ingest_batches(m, batches):
    for first, part in batches:
        m.ingest(*O.concat_reads(part), first)


def position_in_batch(batches):
    """read ordinal -> position of the read's first base in the kept batch that holds it"""
    at = {}
    for first, part in batches:
        p = 0
        for i, r in enumerate(part):
            at[first + i] = p
            p += len(r)
    return at


def exercise_counts(nodes, batches):
    """what the table makes the gather kernel do, in a whole-table chunk: rows of either orientation, rows whose length is no multiple of 16, and 16-byte groups
    whose 16 source positions start more than 16 bits into a 32-base word (the funnel then needs the next word too)"""
    at = position_in_batch(batches)
    ln = (nodes["src_end"] - nodes["src_start"]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(ln)])
    funnel = 0
    for i in range(len(ln)):
        first_group = -int(out_off[i]) % 16                  # offset inside the row of its first group that starts at a multiple of 16 of the output
        if ln[i] - first_group < 16:
            continue
        sb = at[int(nodes["src_read"][i])] + int(nodes["src_start"][i])
        qs = sb + int(ln[i]) - 16 - first_group if nodes["reversed"][i] else sb + first_group
        funnel += qs % 32 > 16
    return dict(reversed=int(np.count_nonzero(nodes["reversed"])), forward=int(np.count_nonzero(nodes["reversed"] == 0)), odd_length=int(np.count_nonzero(ln % 16)),
                funnel_start=int(np.count_nonzero((np.array([at[int(r)] for r in nodes["src_read"]], dtype=np.int64) + nodes["src_start"].astype(np.int64)) % 32 > 16)),
                funnel_groups=int(funnel))


@functools.lru_cache(maxsize=None)
def synth_reads_70(seed):
    """synth_case(seed, 70)'s reads, generated once for the tests that share them"""
    return synth_case(seed, 70)[0]


def case_reads(case):
    kind, seed, hpc = case
    if kind == "fuzz":
        return fuzz_case(seed)
    return 21, 12, 0.003, 2, synth_reads_70(seed)


CASES = [("fuzz", s, h) for s in range(6) for h in (False, True)] + [("synth", 2, True)]      # h = reads_already_hpc: homopolymer compression off


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s%d-%s" % (c[0], c[1], "raw" if c[2] else "hpc"))
def test_whole_table_equals_the_host_rule(case):
    R = _mdbg()
    k, l, d, A, reads = case_reads(case)
    batches = three_batches(reads)
    with R.Mdbg(k, l, d, A, reads_already_hpc=case[2], keep_reads=True) as m:
        ingest_batches(m, batches)
        nodes = m.finalize()
        want = checker(reads, nodes)
        g = m.graph_node_seqs(0, 0, 0)
        assert g["first_row"] == 0 and g["n_rows"] == nodes["n_nodes"] > 0
        assert np.array_equal(g["offsets"][1:], np.cumsum(nodes["src_end"] - nodes["src_start"], dtype=np.uint64))
        got = rows_of(g)
        for i in range(len(want)):
            assert got[i] == want[i], "row %d" % i
        dv = m.graph_node_seqs(0, 0, 0, device=True)
        assert (dv["first_row"], dv["n_rows"], dv["n_bases"]) == (0, g["n_rows"], g["n_bases"]) and dv["bases"] % 16 == 0
        assert np.array_equal(m.to_host(dv["bases"], dv["n_bases"]), g["bases"])
        assert np.array_equal(m.to_host(dv["offsets"], 8 * (dv["n_rows"] + 1), np.uint64), g["offsets"])
    c = exercise_counts(nodes, batches)
    print("%s: %d rows, %d bases; %s" % (case, len(want), g["n_bases"], c))
    # the equality is only worth what the input makes the kernel do
    assert c["reversed"] > 0 and c["forward"] > 0 and c["odd_length"] > 0 and c["funnel_start"] > 0 and c["funnel_groups"] > 0


def chunk_loop(m, **limits):
    out, row = [], 0
    while True:
        g = m.graph_node_seqs(row, **limits)
        assert g["first_row"] == row
        if not g["n_rows"]:
            return out
        out.append(g)
        row += g["n_rows"]


def test_chunks_concatenate_to_the_whole_and_respect_their_limits():
    R = _mdbg()
    k, l, d, A, reads = fuzz_case(0)
    with R.Mdbg(k, l, d, A, keep_reads=True) as m:
        ingest_batches(m, three_batches(reads))
        nodes = m.finalize()
        n = nodes["n_nodes"]
        whole = rows_of(m.graph_node_seqs())
        assert whole == checker(reads, nodes) and n > 20
        ln = [len(s) for s in whole]
        for limits in (dict(max_rows=1), dict(max_rows=5), dict(max_bases=max(ln) - 1), dict(max_bases=sum(ln[:3])), dict(max_rows=4, max_bases=sum(ln[:3]))):
            chunks = chunk_loop(m, **limits)
            assert [s for g in chunks for s in rows_of(g)] == whole, limits
            mr, mb = limits.get("max_rows", 0), limits.get("max_bases", 0)
            row = 0
            for g in chunks:
                r, b = g["n_rows"], g["n_bases"]
                assert (not mr or r <= mr) and (not mb or b <= mb or r == 1), (limits, row)
                # the LARGEST count within the limits: one more row would break one of them (or the table ends)
                assert row + r == n or (mr and r == mr) or (mb and b + ln[row + r] > mb), (limits, row)
                row += r
            if limits == dict(max_rows=1):
                assert len(chunks) == n
            if limits == dict(max_bases=max(ln) - 1):                    # the at-least-one rule: the longest row comes, alone and over the budget
                assert any(g["n_rows"] == 1 and g["n_bases"] == max(ln) for g in chunks)
            if limits == dict(max_bases=sum(ln[:3])):
                assert chunks[0]["n_rows"] >= 3 and chunks[0]["n_bases"] <= sum(ln[:3])
        longest = int(np.argmax(ln))
        g = m.graph_node_seqs(longest, 0, ln[longest] - 1)              # a row longer than the budget comes alone
        assert g["n_rows"] == 1 and rows_of(g) == [whole[longest]]
        for first in (n, n + 5):
            g = m.graph_node_seqs(first)
            assert g["n_rows"] == 0 and g["n_bases"] == 0 and g["first_row"] == first and g["offsets"].tolist() == [0]
            assert m.graph_node_seqs(first, device=True)["n_rows"] == 0


def exception_reads():
    """the input of test_gpu_contigs_device.test_exceptions_n_runs_inside_nodes_and_short_reads_of_arbitrary_bytes: N runs of 1 - 3 bases every ~400 bases, and
    reads shorter than l of arbitrary bytes (lower case among them) between the others"""
    rnd = random.Random(5)
    base = fuzz_reads(rnd, n_reads=150, genome_len=20000, mean_len=3000, err=0.0, p_lower=0.0, p_n=0.0, p_hp=0.0)
    reads = []
    for r in base:
        r = bytearray(r)
        for _ in range(len(r) // 400):
            p, n = rnd.randrange(len(r)), rnd.randint(1, 3)
            r[p:p + n] = b"N" * len(r[p:p + n])
        reads.append(bytes(r))
        if rnd.random() < 0.3:
            reads.append(bytes(rnd.randrange(256) for _ in range(rnd.randint(1, 7))))
    return reads


def exception_facts(want):
    """a fact about the expected output of a whole-table chunk: the number of 16-byte groups of the output (at multiples of 16, inside one row: the kernel's
    16-byte path) that hold two or more bytes outside ACGT"""
    two, at = 0, 0
    for s in want:
        for g in range(-at % 16, len(s) - 15, 16):
            two += sum(c not in b"ACGT" for c in s[g:g + 16]) >= 2
        at += len(s)
    return two


@pytest.mark.parametrize("hpc", [False, True], ids=["hpc", "raw"])
def test_bytes_outside_acgt_inside_node_spans(hpc):
    R = _mdbg()
    reads = exception_reads()
    batches = three_batches(reads)
    with R.Mdbg(4, 8, 0.03, 1, reads_already_hpc=hpc, keep_reads=True) as m:      # min_abundance 1: the spans with N runs survive
        ingest_batches(m, batches)
        nodes = m.finalize()
        want = checker(reads, nodes)
        got = rows_of(m.graph_node_seqs())
        for i in range(len(want)):
            assert got[i] == want[i], "row %d" % i
        chunks = chunk_loop(m, max_rows=3)                               # other group alignments of the same rows
        assert [s for g in chunks for s in rows_of(g)] == want
    rev_n = sum(1 for s, rev in zip(want, nodes["reversed"]) if rev and b"N" in s)
    fwd_n = sum(1 for s, rev in zip(want, nodes["reversed"]) if not rev and b"N" in s)
    two = exception_facts(want)
    print("%d rows; an N in %d reversed and %d forward rows; %d 16-byte groups with two or more exception bytes" % (len(want), rev_n, fwd_n, two))
    assert rev_n > 0 and fwd_n > 0 and two > 0
    # Lower case inside a node span cannot be tested: the sketch path answers MDBG_E_ALPHABET for a read of l bases or more that holds a lower-case byte
    # (include/mdbg_hip.h), so no node can span one.  Asserted here, so that this part is revisited if that ever changes; the lower-case bytes of the reads
    # shorter than l above are kept and never gathered.
    with R.Mdbg(4, 8, 0.03, 1, reads_already_hpc=hpc, keep_reads=True) as m:
        with pytest.raises(R.MdbgError) as ei:
            m.ingest_reads([reads[0][:40] + reads[0][40:60].lower() + reads[0][60:]], 0)
        assert ei.value.code == R.api.MDBG_E_ALPHABET


def test_state_rules_and_what_the_call_leaves_alone():
    R = _mdbg()
    k, l, d, A, reads = fuzz_case(2)
    b, o = O.concat_reads(reads)

    def state_error(call):
        with pytest.raises(R.MdbgError) as ei:
            call()
        assert ei.value.code == R.api.MDBG_E_STATE

    with R.Mdbg(k, l, d, A) as m:                                      # without the flag
        m.ingest(b, o, 0)
        m.finalize()
        state_error(m.graph_node_seqs)
        state_error(lambda: m.graph_node_seqs(device=True))
    with R.Mdbg(k, l, d, A, keep_reads=True) as m:
        m.ingest(b, o, 0)
        state_error(m.graph_node_seqs)                                 # before any finalize
        nodes = m.finalize()
        want = checker(reads, nodes)
        assert rows_of(m.graph_node_seqs()) == want
        # the call leaves the edge list, the unitig list and a contig result alone, and they leave its chunk alone
        m.graph_edges(0.01)
        u = m.graph_unitigs()
        ctg = m.graph_contigs(0)
        dev_ctg = m.graph_contigs(0, device=True)
        chunk = m.graph_node_seqs(1, 4, 0, device=True)
        assert np.array_equal(m.to_host(dev_ctg.bases, int(dev_ctg.n_bases)), ctg["bases"])
        again = m.graph_contigs(0)                                     # the unitig list is still current ...
        assert np.array_equal(again["bases"], ctg["bases"]) and np.array_equal(again["offsets"], ctg["offsets"])
        assert m.to_host(chunk["bases"], chunk["n_bases"]).tobytes() == b"".join(want[1:5])      # ... and the contig call did not touch the chunk
        u2 = m.graph_unitigs()                                         # the edge list is still current
        assert u2["n_unitigs"] == u["n_unitigs"] and np.array_equal(u2["node"], u["node"])
        assert rows_of(m.graph_node_seqs()) == want                    # edge and unitig calls do not end the node table
        m.ingest(b[:int(o[3])], o[:4], len(reads))                     # an ingest ends it
        state_error(m.graph_node_seqs)
        m.rewind(m.mark() - 1)
        state_error(m.graph_node_seqs)                                 # so does a rewind
        m.reset(k + 1)
        state_error(m.graph_node_seqs)                                 # and reset(k): no table until the next finalize
        nodes2 = m.finalize()
        want2 = checker(reads, nodes2)
        assert rows_of(m.graph_node_seqs()) == want2 and want2 != want      # the new k's table, a new prefix
        assert [s for g in chunk_loop(m, max_rows=6) for s in rows_of(g)] == want2
        m.reset(0)
        state_error(m.graph_node_seqs)                                 # and reset(0)
        m.ingest(b, o, 0)
        state_error(m.graph_node_seqs)
        m.reset(k)
        nodes3 = m.finalize(gfa_only=True)                             # a table of mdbg_finalize_gfa: the device rows are all there
        assert nodes3["n_nodes"] == len(want) and rows_of(m.graph_node_seqs()) == want
    with R.Mdbg(k, l, d, A, keep_reads=True) as m, R.Mdbg(k, l, d, A) as src:      # a context that imported a sketch: legal, but its reads are not kept
        src.ingest(b, o, 0)
        v = src.sketch_view()
        m.ingest_sketch(v.d_hashes, v.d_positions, v.d_read_offsets, int(v.n_reads), 0)
        m.insert_resident()
        assert m.finalize()["n_nodes"] == len(want)
        state_error(m.graph_node_seqs)


def sequence_lines(path):
    return read_lz4_frame(path).decode().split("\n")


def test_files_from_the_kept_reads_equal_the_second_pass(tmp_path):
    """pipeline.run_file and mdbg_cli with and without sequences_from_kept: the default batch_bases makes the small input ONE second-pass batch, so the files
    hold the same lines in the same order"""
    from rust_mdbg_amd import pipeline
    reads = synth_reads_70(2)
    fa = str(tmp_path / "reads.fa")
    write_fasta(fa, reads)
    for contigs in (False, True):
        for threads in (1, 3):
            res = {}
            for kept in (False, True):
                pre = str(tmp_path / ("c%d_t%d_k%d" % (contigs, threads, kept)))
                res[kept] = pipeline.run_file(fa, pre, 21, 12, 0.003, 2, reads_already_hpc=True, presimp=0.01, threads=threads, contigs=contigs, keep_reads=contigs,
                                              sequences_from_kept=kept)
            a, b = (str(tmp_path / ("c%d_t%d_k%d" % (contigs, threads, kept))) for kept in (False, True))
            for t in range(threads):
                la, lb = sequence_lines("%s.%d.sequences" % (a, t)), sequence_lines("%s.%d.sequences" % (b, t))
                assert la == lb and len(la) > 5, (contigs, threads, t)
                if threads == 1:
                    assert open(a + ".0.sequences", "rb").read() == open(b + ".0.sequences", "rb").read()
            assert sum(len([x for x in sequence_lines("%s.%d.sequences" % (b, t)) if x and not x.startswith("#")]) for t in range(threads)) == res[True]["n_nodes"] > 0
            for ext in [".gfa"] + ([".unitigs.gfa", ".unitigs.fa"] if contigs else []):
                x = open(a + ext, "rb").read()
                assert x == open(b + ext, "rb").read() and len(x) > 0, ext
            for f in ("n_reads", "n_bases", "n_nodes", "n_edges"):
                assert res[True][f] == res[False][f], f
            su = res[True]["seconds_until"]
            assert "sequences_kept" in su and "sequences" not in su and "kept_reads" in res[True], (contigs, su)      # no second pass at all: the contigs are stitched too
            assert "sequences" in res[False]["seconds_until"] and "sequences_kept" not in res[False]["seconds_until"]
    # contigs from the second pass, node sequences from the store: the pass still runs, for the contigs alone
    pre = str(tmp_path / "mixed")
    r = pipeline.run_file(fa, pre, 21, 12, 0.003, 2, reads_already_hpc=True, presimp=0.01, contigs=True, keep_reads=False, sequences_from_kept=True)
    assert "sequences" in r["seconds_until"] and "sequences_kept" in r["seconds_until"]
    for ext in (".0.sequences", ".unitigs.fa", ".unitigs.gfa"):
        assert open(pre + ext, "rb").read() == open(str(tmp_path / "c1_t1_k0") + ext, "rb").read(), ext
    exe = build_cli(tmp_path)
    for name, extra in (("cli_plain", []), ("cli_kept", ["--sequences-from-kept"]), ("cli_kept3", ["--sequences-from-kept", "--threads", "3"]), ("cli_plain3", ["--threads", "3"])):
        subprocess.run([exe, fa, "-k", "21", "-l", "12", "--density", "0.003", "--minabund", "2", "--presimp", "0.01", "--skiphpc", "--prefix", str(tmp_path / name)] + extra,
                       check=True, stdout=subprocess.DEVNULL)
    x = open(str(tmp_path / "cli_plain.0.sequences"), "rb").read()
    assert len(x) > 0 and x == open(str(tmp_path / "cli_kept.0.sequences"), "rb").read() and x == open(str(tmp_path / "c0_t1_k0.0.sequences"), "rb").read()
    for t in range(3):
        assert open(str(tmp_path / ("cli_plain3.%d.sequences" % t)), "rb").read() == open(str(tmp_path / ("cli_kept3.%d.sequences" % t)), "rb").read()


def test_full_size_measurement_printed():
    """BASELINE configs[1] (the input of test_gpu_contigs_device.test_full_size_contigs_equal_the_host_path): rows, bases, chunks of 256 MiB, device time of the
    gather kernel.  A printed measurement, no threshold; the totals are checked against the node table."""
    R = _mdbg()
    n_reads = 100000
    with R.Mdbg(21, 12, 0.003, 2, keep_reads=True) as m:
        db, do, nb = m.synth_reads_device(seed=2, genome_len=30_000_000, n_reads=n_reads)
        m.ingest_device(db, do, n_reads, nb, 0)
        nodes = m.finalize()
        ln = (nodes["src_end"] - nodes["src_start"]).astype(np.int64)
        row, bases, chunks, ms = 0, 0, 0, 0.0
        while True:
            g = m.graph_node_seqs(row, 0, 256 << 20, device=True)
            if not g["n_rows"]:
                break
            assert g["n_bases"] == int(ln[row:row + g["n_rows"]].sum()) <= 256 << 20
            row += g["n_rows"]
            bases += g["n_bases"]
            chunks += 1
            ms += m.node_seqs_ms()
        assert row == nodes["n_nodes"] > 100000 and bases == int(ln.sum())
        # a sample of rows of the last chunk against the host rule (the reads come back from the device for it)
        b, o = m.to_host(db, nb), m.to_host(do, 8 * (n_reads + 1), np.uint64).astype(np.int64)
        last = m.graph_node_seqs(nodes["n_nodes"] - 50, 0, 0)
        for j, s in enumerate(rows_of(last)):
            i = nodes["n_nodes"] - 50 + j
            r = int(nodes["src_read"][i])
            w = b[o[r] + int(nodes["src_start"][i]):o[r] + int(nodes["src_end"][i])].tobytes()
            assert s == (w[::-1].translate(REVCOMP) if nodes["reversed"][i] else w), i
        print("configs[1]: %d rows, %d bases of node sequences (%.1f x the %d input bases) in %d chunks of <= 256 MiB; gather kernel %.3f ms = %.1f GB/s written" %
              (row, bases, bases / nb, nb, chunks, ms, bases / ms / 1e6 if ms else 0.0))
