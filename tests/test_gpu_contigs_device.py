"""Contigs stitched on the GPU from reads kept packed in device memory (MDBG_FLAG_KEEP_READS, mdbg_graph_contigs) against the host path that
exists without them: Emitter.contigs / mdbg_emit_contigs_add_batch run over the same reads.  Equality is exact (bytes)."""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_fuzz import fuzz_reads
from test_gpu_parity import _mdbg
from test_gpu_unitigs import CYCLE_PARAMS, build_cli, cyclic_reads, write_fasta
from test_unitigs_cpu import fuzz_case, synth_case

pytestmark = pytest.mark.gpu


def split(g):
    """graph_contigs() dict -> list of bytes"""
    b, o = g["bases"].tobytes(), g["offsets"].astype(np.int64)
    assert len(o) == g["n_contigs"] + 1 and o[0] == 0 and o[-1] == g["n_bases"] == len(b)
    return [b[o[i]:o[i + 1]] for i in range(g["n_contigs"])]


def host_contigs(u, batches):
    """the checker: the plan of a unitig list (dict of graph_unitigs / graph_simplify) executed on the host over the reads"""
    from rust_mdbg_amd import emit as E
    with E.Emitter().contigs(u, batches) as c:
        return c.sequences()


def graph(m, presimp):
    m.finalize()
    m.graph_edges(presimp)


def check_both_lists(R, m, batches, presimp=0.01):
    """plain unitigs and the simplified list of the context's table: GPU-stitched == host-stitched; -> (plain list, its contigs)"""
    graph(m, presimp)
    s = m.graph_simplify(R.api.MAGIC_SIMPLIFY_STEPS)
    got_s = m.graph_contigs()
    assert np.array_equal(got_s["unitig"], np.arange(s["n_unitigs"], dtype=np.uint64)) and np.array_equal(got_s["offsets"][1:], np.cumsum(s["length"], dtype=np.uint64))
    assert split(got_s) == host_contigs(s, batches)
    u = m.graph_unitigs()
    got = m.graph_contigs()
    assert np.array_equal(got["unitig"], np.arange(u["n_unitigs"], dtype=np.uint64)) and np.array_equal(got["offsets"][1:], np.cumsum(u["length"], dtype=np.uint64))
    seqs = split(got)
    assert seqs == host_contigs(u, batches)
    return u, seqs


def case_reads(case):
    kind, seed, hpc, presimp = case
    if kind == "fuzz":
        k, l, d, A, reads = fuzz_case(seed)
    elif kind == "synth":
        reads, _ = synth_case(seed, 70)
        k, l, d, A = 21, 12, 0.003, 2
    else:
        rnd = random.Random(900 + seed)
        k, l, d, A = rnd.choice(CYCLE_PARAMS)
        reads = cyclic_reads(kind, rnd)
    return k, l, d, A, reads


# homopolymer compression on (hpc = reads_already_hpc False) and off, presimp 0 / 0.01 / 0.5, linear and circular unitigs
CASES = ([("fuzz", s, h, p) for s in range(6) for h, p in ((False, 0.01), (True, 0.0))] + [("fuzz", 1, False, 0.5), ("fuzz", 3, True, 0.5), ("synth", 2, True, 0.01), ("synth", 3, False, 0.01)] +
         [(kind, s, False, 0.0) for kind in ("circular", "tandem", "inverted") for s in range(2)] + [("circular", 2, True, 0.01), ("circular", 3, True, 0.0)])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s%d-%s-%g" % (c[0], c[1], "raw" if c[2] else "hpc", c[3]))
def test_gpu_contigs_equal_the_host_path(case, tmp_path):
    """per contig, and as whole files through pipeline.run_file with and without keep_reads"""
    from rust_mdbg_amd import pipeline
    R = _mdbg()
    k, l, d, A, reads = case_reads(case)
    b, o = O.concat_reads(reads)
    with R.Mdbg(k, l, d, A, reads_already_hpc=case[2], keep_reads=True) as m:
        m.ingest(b, o, 0)
        check_both_lists(R, m, [(b, o, 0)], case[3])
    fa = str(tmp_path / "reads.fa")
    write_fasta(fa, [r for r in reads if r])
    res = {}
    for keep in (False, True):
        pre = str(tmp_path / ("keep%d" % keep))
        res[keep] = pipeline.run_file(fa, pre, k, l, d, A, reads_already_hpc=case[2], presimp=case[3], contigs=True, simplify=R.api.MAGIC_SIMPLIFY_STEPS,
                                      write_sequences=False, keep_reads=keep)
    assert "kept_reads" in res[True] and "kept_reads" not in res[False] and "sequences" not in res[True]["seconds_until"] and "sequences" in res[False]["seconds_until"]
    for f in ("n_unitigs", "n_simplified", "n_nodes", "n_edges"):
        assert res[True][f] == res[False][f], f
    for ext in (".unitigs.gfa", ".unitigs.fa", ".msimpl.gfa", ".msimpl.fa", ".gfa"):
        x = open(str(tmp_path / "keep0") + ext, "rb").read()
        assert x == open(str(tmp_path / "keep1") + ext, "rb").read() and len(x) > 0, ext


def test_the_cases_cover_every_revcomp_value_and_multi_entry_unitigs():
    """the equality above is only worth what its inputs exercise: over CASES each revcomp value 0, 1, 2 occurs, some unitig has more than one entry, some is circular"""
    R = _mdbg()
    seen, multi, circ = set(), 0, 0
    for case in CASES:
        k, l, d, A, reads = case_reads(case)
        with R.Mdbg(k, l, d, A, reads_already_hpc=case[2]) as m:
            m.ingest_reads(reads, 0)
            graph(m, case[3])
            u = m.graph_unitigs()
        seen |= set(u["revcomp"].tolist())
        multi += int((np.diff(u["offsets"].astype(np.int64)) > 1).sum())
        circ += int(u["circular"].sum())
    print("revcomp values %s, %d unitigs with several entries, %d circular" % (sorted(seen), multi, circ))
    assert seen == {0, 1, 2} and multi > 0 and circ > 0


def way_in_reads():
    rnd = random.Random(77)
    reads = [r for r in fuzz_reads(rnd, n_reads=240, genome_len=30000, mean_len=3000, err=0.005, p_lower=0.0, p_n=0.0, p_hp=0.02)]
    return 5, 10, 0.01, 2, reads


def test_every_entry_point_keeps_the_same_reads():
    """the six ways in, each fed several batches in shuffled ordinal order; one device ASCII batch with offsets[0] > 0; batches that end inside a 32-base word"""
    import torch
    from rust_mdbg_amd import emit as E
    R = _mdbg()
    k, l, d, A, reads = way_in_reads()
    cuts = [0, 37, 90, 91, 170, len(reads)]
    parts = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]
    assert any(sum(len(r) for r in reads[lo:hi]) % 32 for lo, hi in parts)
    b_all, o_all = O.concat_reads(reads)
    want = None
    ways = ["ingest", "ingest_device", "ingest_packed", "ingest_packed_device", "sketch_device", "sketch_packed_device", "ingest_device_offset"]
    for wi, way in enumerate(ways):
        order = list(parts)
        random.Random(wi).shuffle(order)
        hold = []                                                      # device tensors stay alive until the context is done with them
        with R.Mdbg(k, l, d, A, keep_reads=True) as m:
            for lo, hi in order:
                b, o = O.concat_reads(reads[lo:hi])
                n, nb = hi - lo, len(b)
                if way == "ingest":
                    m.ingest(b, o, lo)
                elif way in ("ingest_device", "sketch_device", "ingest_device_offset"):
                    pad = 16 if way == "ingest_device_offset" else 0   # bytes in front of the first read (a multiple of 16: the pointer stays aligned)
                    tb = torch.from_numpy(np.concatenate([np.full(pad, ord("G"), np.uint8), b, np.zeros(64, np.uint8)])).cuda()
                    to = torch.from_numpy((o + np.uint64(pad)).astype(np.int64)).cuda()
                    torch.cuda.synchronize()
                    hold += [tb, to]
                    (m.sketch_device if way == "sketch_device" else m.ingest_device)(tb.data_ptr(), to.data_ptr(), n, nb + pad, lo)
                else:
                    pk = E.pack_reads(b, o)
                    if way == "ingest_packed":
                        m.ingest_packed(pk, lo)
                    else:
                        t = [torch.from_numpy(np.concatenate([pk[f].view(np.uint8), np.zeros(64, np.uint8)])).cuda() for f in ("words", "offsets", "exc_pos", "exc_val")]
                        torch.cuda.synchronize()
                        hold += t
                        m.ingest_packed_device(t[0].data_ptr(), t[1].data_ptr(), n, nb, lo, t[2].data_ptr(), t[3].data_ptr(), len(pk["exc_pos"]), sketch_only=way == "sketch_packed_device")
            if way.startswith("sketch"):
                m.insert_resident()
            kr = m.kept_reads()
            assert kr["n_reads"] == len(reads) and kr["n_bases"] == len(b_all) + (16 * len(parts) if way == "ingest_device_offset" else 0)
            u, seqs = check_both_lists(R, m, [(b_all, o_all, 0)])
        assert u["n_unitigs"] > 3
        if want is None:
            want = seqs
        assert seqs == want, way


def test_exceptions_n_runs_inside_nodes_and_short_reads_of_arbitrary_bytes():
    R = _mdbg()
    rnd = random.Random(5)
    base = fuzz_reads(rnd, n_reads=150, genome_len=20000, mean_len=3000, err=0.0, p_lower=0.0, p_n=0.0, p_hp=0.0)
    reads = []
    for r in base:
        r = bytearray(r)
        for _ in range(len(r) // 400):                                 # N runs of 1 - 3 bases, a few per read: between and inside the minimizers of a node
            p, n = rnd.randrange(len(r)), rnd.randint(1, 3)
            r[p:p + n] = b"N" * len(r[p:p + n])
        reads.append(bytes(r))
        if rnd.random() < 0.3:                                         # shorter than l: never looked at by the sketch, kept byte for byte all the same
            reads.append(bytes(rnd.randrange(256) for _ in range(rnd.randint(1, 7))))
    assert any(b"N" in r for r in reads) and any(len(r) < 8 and not set(r) <= set(b"ACGTN") for r in reads)
    b, o = O.concat_reads(reads)
    for hpc in (False, True):
        for packed in (False, True):
            with R.Mdbg(4, 8, 0.03, 1, reads_already_hpc=hpc, keep_reads=True) as m:
                if packed:
                    from rust_mdbg_amd import emit as E
                    half = len(reads) // 2
                    m.ingest_packed(E.pack_reads(*O.concat_reads(reads[half:])), half)
                    m.ingest_packed(E.pack_reads(*O.concat_reads(reads[:half])), 0)
                else:
                    m.ingest(b, o, 0)
                u, seqs = check_both_lists(R, m, [(b, o, 0)], 0.0)
                n_exc = sum(sum(c not in b"ACGT" for c in r) for r in reads)
                nw = (len(b) + 31) // 32 if not packed else sum((sum(len(r) for r in part) + 31) // 32 for part in (reads[:len(reads) // 2], reads[len(reads) // 2:]))
                assert m.kept_reads() == dict(n_reads=len(reads), n_bases=len(b), bytes=8 * nw + 8 * (len(reads) + (2 if packed else 1)) + 9 * n_exc)
            assert any(b"N" in s for s in seqs)                        # not vacuous: an N made it into a contig
            assert {1, 0} <= set(u["revcomp"].tolist())


def test_min_len_filters_like_the_host():
    R = _mdbg()
    k, l, d, A, reads = fuzz_case(3)
    b, o = O.concat_reads(reads)
    with R.Mdbg(k, l, d, A, keep_reads=True) as m:
        m.ingest(b, o, 0)
        graph(m, 0.0)
        u = m.graph_unitigs()
        allseq = split(m.graph_contigs(0))
        lens = sorted(set(u["length"].tolist()))
        assert len(lens) > 3
        for cut in (1, lens[len(lens) // 2], lens[-1], lens[-1] + 1, 1 << 40):
            g = m.graph_contigs(cut)
            keep = [i for i in range(u["n_unitigs"]) if u["length"][i] >= cut]
            assert g["unitig"].tolist() == keep and split(g) == [allseq[i] for i in keep]
            dev = m.graph_contigs(cut, device=True)
            assert int(dev.n_contigs) == len(keep) and int(dev.n_bases) == g["n_bases"]
            if g["n_bases"]:
                assert np.array_equal(m.to_host(dev.bases, g["n_bases"]), g["bases"])
            assert np.array_equal(m.to_host(dev.offsets, 8 * (len(keep) + 1), np.uint64), g["offsets"])
        g = m.graph_contigs(lens[-1] + 1)
        assert g["n_contigs"] == 0 and g["n_bases"] == 0 and g["offsets"].tolist() == [0]


def test_lifetime_and_state_rules():
    R = _mdbg()
    k, l, d, A, reads = fuzz_case(2)
    b, o = O.concat_reads(reads)
    half = len(reads) // 2
    b1, o1 = O.concat_reads(reads[:half])
    b2, o2 = O.concat_reads(reads[half:])

    def state_error(call):
        with pytest.raises(R.MdbgError) as ei:
            call()
        assert ei.value.code == R.api.MDBG_E_STATE

    with R.Mdbg(k, l, d, A) as m:                                      # without the flag
        m.ingest(b, o, 0)
        graph(m, 0.01)
        m.graph_unitigs()
        state_error(m.graph_contigs)
        assert m.kept_reads() == dict(n_reads=0, n_bases=0, bytes=0)
    with R.Mdbg(k, l, d, A, keep_reads=True) as m:
        state_error(m.graph_contigs)                                   # nothing yet
        m.ingest(b1, o1, 0)
        at_mark = m.kept_reads()
        # the footprint: n_bases / 4 + 8 per read + 9 per exception; exact up to the rounding of each batch to whole 32-base words and its one extra offset
        assert at_mark == dict(n_reads=half, n_bases=len(b1), bytes=8 * ((len(b1) + 31) // 32) + 8 * (half + 1))
        assert 0 <= at_mark["bytes"] - (len(b1) / 4 + 8 * half) < 16
        mark = m.mark()
        m.ingest(b2, o2, half)
        assert m.kept_reads()["n_reads"] == len(reads)
        state_error(m.graph_contigs)                                   # no list
        graph(m, 0.01)
        state_error(m.graph_contigs)                                   # finalize + edges, still no list
        u = m.graph_unitigs()
        seqs = split(m.graph_contigs())
        assert seqs == host_contigs(u, [(b, o, 0)])
        dev = m.graph_contigs(0, device=True)
        m.ingest(b1[:int(o1[3])], o1[:4], len(reads))                  # an ingest ends the list ...
        state_error(m.graph_contigs)
        assert m.to_host(dev.bases, int(dev.n_bases)).tobytes() == b"".join(seqs)      # ... and leaves the last result's buffers alone
        # reset(k): the store stays, a new graph's contigs equal the host path again
        m.rewind(m.mark() - 1)
        m.reset(k + 1)
        assert m.kept_reads()["n_reads"] == len(reads)
        state_error(m.graph_contigs)
        assert m.to_host(dev.bases, int(dev.n_bases)).tobytes() == b"".join(seqs)
        check_both_lists(R, m, [(b, o, 0)])
        m.finalize()
        state_error(m.graph_contigs)                                   # a finalize ends the list
        # rewind(mark): exactly the batches after the mark go
        m.rewind(mark)
        assert m.kept_reads() == at_mark
        m.reset(k)
        check_both_lists(R, m, [(b1, o1, 0)])
        m.reset(0)
        assert m.kept_reads() == dict(n_reads=0, n_bases=0, bytes=0)
        m.ingest(b2, o2, 0)
        check_both_lists(R, m, [(b2, o2, 0)])
    with R.Mdbg(k, l, d, A, keep_reads=True) as m, R.Mdbg(k, l, d, A) as src:      # a context that imported a sketch: legal, but its reads are not kept
        src.ingest(b, o, 0)
        v = src.sketch_view()
        m.ingest_sketch(v.d_hashes, v.d_positions, v.d_read_offsets, int(v.n_reads), 0)
        m.insert_resident()
        graph(m, 0.01)
        assert m.graph_unitigs()["n_unitigs"] > 0
        state_error(m.graph_contigs)


@pytest.mark.parametrize("producer", ["unitigs", "simplified"])
def test_multik_feeds_the_contigs_from_the_device(producer, tmp_path):
    from rust_mdbg_amd import pipeline
    reads, _ = synth_case(3, 70)
    fa = str(tmp_path / "reads.fa")
    write_fasta(fa, reads)
    ks, l, d = [15, 21, 25], 12, 0.003
    a = pipeline.run_multik(fa, str(tmp_path / "a"), ks, l, d, 2, reads_already_hpc=True, contigs_fn=producer, min_contig_len=20000)
    b = pipeline.run_multik(fa, str(tmp_path / "b"), ks, l, d, 2, reads_already_hpc=True, contigs_fn=producer, min_contig_len=20000, keep_reads=True)
    assert a == b and a[21]["n_contigs"] > 0 and a[25]["n_contigs"] > 0      # contigs pass min_contig_len in rounds before the last
    for k in ks:
        x = open(str(tmp_path / ("a-k%d.gfa" % k)), "rb").read()
        assert x == open(str(tmp_path / ("b-k%d.gfa" % k)), "rb").read() and len(x) > 0


def test_full_size_contigs_equal_the_host_path():
    """BASELINE configs[1] (196,846 nodes: the graph of the full-size unitig test): every contig, plain and simplified"""
    R = _mdbg()
    n_reads = 100000
    with R.Mdbg(21, 12, 0.003, 2, keep_reads=True) as m:
        db, do, nb = m.synth_reads_device(seed=2, genome_len=30_000_000, n_reads=n_reads)
        b, o = m.to_host(db, nb), m.to_host(do, 8 * (n_reads + 1), np.uint64)
        m.ingest_device(db, do, n_reads, nb, 0)
        kr = m.kept_reads()
        assert kr == dict(n_reads=n_reads, n_bases=nb, bytes=8 * ((nb + 31) // 32) + 8 * (n_reads + 1))
        u, seqs = check_both_lists(R, m, [(b, o, 0)])
        assert u["n_entries"] > 100000
        print("configs[1]: %d nodes -> %d contigs, %d bases; store %d bytes for %d bases; stitch kernel %.3f ms" %
              (u["n_entries"], len(seqs), sum(len(s) for s in seqs), kr["bytes"], nb, m.contigs_ms()))


def test_cli_keep_reads_writes_the_same_files(tmp_path):
    reads, _ = synth_case(2, 70)
    fa = str(tmp_path / "reads.fa")
    write_fasta(fa, reads)
    exe = build_cli(tmp_path)
    for pre, extra in (("plain", []), ("keep", ["--keep-reads"]), ("keep1", ["--keep-reads", "--no-basespace"])):
        subprocess.run([exe, fa, "-k", "21", "-l", "12", "--density", "0.003", "--minabund", "2", "--presimp", "0.01", "--skiphpc", "--contigs", "--simplify",
                        "--prefix", str(tmp_path / pre)] + extra, check=True, stdout=subprocess.DEVNULL)
    for ext in (".unitigs.gfa", ".unitigs.fa", ".msimpl.gfa", ".msimpl.fa"):
        x = open(str(tmp_path / "plain") + ext, "rb").read()
        assert len(x) > 0 and x == open(str(tmp_path / "keep") + ext, "rb").read() and x == open(str(tmp_path / "keep1") + ext, "rb").read(), ext
    assert os.path.exists(str(tmp_path / "keep.0.sequences")) and not os.path.exists(str(tmp_path / "keep1.0.sequences"))
