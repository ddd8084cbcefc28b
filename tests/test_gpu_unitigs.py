"""Unitigs compacted on the GPU (mdbg_graph_unitigs, csrc/unitigs.hip) == the plain restatement of the definition
(tests/unitig_restatement.py), field for field, and the copy plan executed by libmdbg_emit == the restatement's strings."""
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import unitig_restatement as U
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from test_gpu_parity import _mdbg
from test_unitigs_cpu import assert_genome_substrings, fuzz_case, synth_case

pytestmark = pytest.mark.gpu

ARRAYS = ("offsets", "node", "ori", "src_read", "src_begin", "len", "revcomp", "dst_offset", "length", "kc_sum", "circular")


def assert_equals_restatement(got, nodes, edges, reads):
    """got: Mdbg.graph_unitigs(); nodes / edges: what the same context returned; reads: list of bytes or None (no sequences)"""
    exp = U.unitigs(nodes, edges, reads)
    off = got["offsets"].tolist()
    walks = [list(zip(got["node"][a:b].tolist(), (chr(c) for c in got["ori"][a:b]))) for a, b in zip(off, off[1:])]
    assert walks == exp["walks"]                                                   # walks, orientations, order
    assert got["circular"].astype(bool).tolist() == exp["circular"] and got["kc_sum"].tolist() == exp["kc_sum"]
    assert got["n_unitigs"] == len(walks) and got["n_entries"] == len(nodes["index"]) == off[-1]
    e = got["edges"]
    rows = list(zip(e["n1"].tolist(), (chr(c) for c in e["o1"]), e["n2"].tolist(), (chr(c) for c in e["o2"]), e["overlap"].tolist()))
    if reads is None:
        assert [r[:4] for r in rows] == [r[:4] for r in exp["edges"]]
        return exp
    assert rows == exp["edges"]                                                    # unitig edges in source order, overlaps fixed
    assert got["length"].tolist() == exp["length"]
    for a, b in zip(off, off[1:]):                                                 # dst_offset: running sum of len inside the unitig
        assert got["dst_offset"][a:b].tolist() == np.concatenate([[0], np.cumsum(got["len"][a:b].astype(np.uint64))[:-1]]).astype(np.uint64).tolist()
    from rust_mdbg_amd import emit as E
    with E.Contigs(got, n_nodes=len(nodes["index"])) as c:                         # the plan executed
        c.add_batch(*O.concat_reads(reads), 0)
        assert [s.decode("latin-1") for s in c.sequences()] == exp["seqs"]
    return exp


def run_unitigs(R, reads, k, l, d, A, presimp, hpc=False):
    b, o = O.concat_reads(reads)
    with R.Mdbg(k, l, d, A, reads_already_hpc=hpc) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        edges = m.graph_edges(presimp)
        got = m.graph_unitigs()
        again = m.graph_unitigs()                                                  # buffers are reused: same answer
        dev = m.graph_unitigs_device()
        cnt = R.api.unitig_counts(dev)
        for f, t in R.api.UNITIG_FIELDS:                                           # host and device variants agree
            assert np.array_equal(m.to_host(getattr(dev, f), cnt[f] * np.dtype(t).itemsize, t) if cnt[f] else np.zeros(0, t), got[f][:cnt[f]]), f
        assert int(dev.edges.n) == len(got["edges"]["n1"])
        for f, t in R.api.EDGE_FIELDS:
            n = int(dev.edges.n)
            assert np.array_equal(m.to_host(getattr(dev.edges, f), n * np.dtype(t).itemsize, t) if n else np.zeros(0, t), got["edges"][f]), f
    for f in ARRAYS:
        assert np.array_equal(got[f], again[f]), f
    for f, _ in R.api.EDGE_FIELDS:
        assert np.array_equal(got["edges"][f], again["edges"][f]), f
    return nodes, edges, got


@pytest.mark.parametrize("presimp", [0.0, 0.01, 0.5])
@pytest.mark.parametrize("seed", range(6))
def test_gpu_unitigs_equal_restatement_on_fuzz_graphs(seed, presimp):
    R = _mdbg()
    k, l, d, A, reads = fuzz_case(seed)
    nodes, edges, got = run_unitigs(R, reads, k, l, d, A, presimp)
    assert_equals_restatement(got, nodes, edges, reads)


def cyclic_reads(kind, rnd):
    """reads of a short CIRCULAR genome (they wrap around its origin), of a tandem repeat, and of a genome with an inverted repeat (hairpins)"""
    g = bytes(rnd.choice(b"ACGT") for _ in range(rnd.choice([1500, 4000])))
    if kind == "tandem":
        unit = g[:700]
        g = g[700:1400] + unit * 6 + g[1400:]
    elif kind == "inverted":
        g = g + U.revcomp(g[-900:].decode()).encode() + bytes(rnd.choice(b"ACGT") for _ in range(300))
    reads = []
    for _ in range(150):
        ln = rnd.randint(len(g) // 2, 2 * len(g))
        st = rnd.randrange(len(g))
        s = (g * 4)[st:st + ln] if kind == "circular" else g[st:st + ln]
        reads.append(s if rnd.random() < 0.5 else U.revcomp(s.decode()).encode())
    return reads


CYCLE_PARAMS = [(3, 8, 0.03, 1), (5, 8, 0.05, 2), (4, 6, 0.05, 2)]


@pytest.mark.parametrize("kind", ["circular", "tandem", "inverted"])
@pytest.mark.parametrize("seed", range(4))
def test_gpu_unitigs_on_cycles_and_hairpins(seed, kind):
    R = _mdbg()
    rnd = random.Random(900 + seed)
    k, l, d, A = rnd.choice(CYCLE_PARAMS)
    reads = cyclic_reads(kind, rnd)
    nodes, edges, got = run_unitigs(R, reads, k, l, d, A, rnd.choice([0.0, 0.01]))
    exp = assert_equals_restatement(got, nodes, edges, reads)
    print("%s seed %d: %d nodes, %d unitigs, %d circular, %d rounds" % (kind, seed, len(nodes["index"]), len(exp["walks"]), sum(exp["circular"]), got["n_rounds"]))


def test_gpu_unitigs_circular_unitigs_occur():
    """the cycle branch of the ranking runs: across the circular-genome cases at least one unitig is circular"""
    R = _mdbg()
    seen = 0
    for seed in range(4):
        rnd = random.Random(900 + seed)
        k, l, d, A = rnd.choice(CYCLE_PARAMS)
        reads = cyclic_reads("circular", rnd)
        _, _, got = run_unitigs(R, reads, k, l, d, A, 0.0)
        seen += int(got["circular"].sum())
    assert seen > 0


def test_gpu_unitigs_state_rules(example_reads):
    R = _mdbg()
    with R.Mdbg(7, 10, 0.0008, 2) as m:
        m.ingest_reads(example_reads, 0)
        for step in (lambda: None, m.finalize):                                    # no finalize; finalized but no edge list
            step()
            with pytest.raises(R.MdbgError) as ei:
                m.graph_unitigs()
            assert ei.value.code == -6
        m.graph_edges(0.01)
        assert m.graph_unitigs()["n_entries"] == 104
        m.ingest_reads(example_reads[:10], len(example_reads))                    # the table changed: finalize + edges must be redone
        with pytest.raises(R.MdbgError) as ei:
            m.graph_unitigs()
        assert ei.value.code == -6
        m.finalize()
        with pytest.raises(R.MdbgError) as ei:
            m.graph_unitigs()
        assert ei.value.code == -6
        m.graph_edges(0.01)
        assert m.graph_unitigs()["n_entries"] == 104
    with R.Mdbg(7, 10, 0.0008, 2) as m:                                            # empty context: empty list, no error
        u = m.graph_unitigs()
        assert u["n_unitigs"] == 0 and u["n_entries"] == 0 and len(u["edges"]["n1"]) == 0


def write_fasta(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n%s\n" % (i, r))


def build_cli(tmp_path):
    lib = os.path.join(ROOT, "rust_mdbg_amd")
    exe = str(tmp_path / "mdbg_cli")
    subprocess.run(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mdbg_cli.c"), "-L" + lib, "-lmdbg_hip", "-lmdbg_emit",
                    "-lpthread", "-Wl,-rpath," + lib, "-o", exe], check=True)
    return exe


def read_fasta(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return [x[1:] for x in lines[0:-1:2]], lines[1:-1:2]


@pytest.mark.parametrize("n", [500, 70])
def test_contigs_of_error_free_reads_through_run_file_and_cli(n, tmp_path):
    """item 3's input end to end: pipeline.run_file(contigs=True) and mdbg_cli --contigs write identical files, and every contig is a piece of the genome"""
    from rust_mdbg_amd import pipeline
    reads, genome = synth_case(2, n)
    fa = str(tmp_path / "reads.fa")
    write_fasta(fa, reads)
    pre = str(tmp_path / "py")
    res = pipeline.run_file(fa, pre, 21, 12, 0.003, 2, reads_already_hpc=True, presimp=0.01, contigs=True)
    names, seqs = read_fasta(pre + ".unitigs.fa")
    assert res["n_unitigs"] == len(seqs) and (len(seqs) == 1 if n == 500 else 6 <= len(seqs) <= 7)
    assert_genome_substrings(names, seqs, [len(s) for s in seqs], genome)
    S = [ln.split("\t") for ln in open(pre + ".unitigs.gfa").read().split("\n") if ln.startswith("S\t")]
    assert [s[1] for s in S] == names and [s[2] for s in S] == seqs and [s[3] for s in S] == ["LN:i:%d" % len(s) for s in seqs]
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "c")
    subprocess.run([exe, fa, "-k", "21", "-l", "12", "--density", "0.003", "--minabund", "2", "--presimp", "0.01", "--skiphpc", "--contigs", "--prefix", cpre],
                   check=True, stdout=subprocess.DEVNULL)
    for ext in (".unitigs.fa", ".unitigs.gfa", ".gfa"):
        assert open(pre + ext, "rb").read() == open(cpre + ext, "rb").read(), ext


def test_example_fixture_reproduces_the_golden(tmp_path):
    from rust_mdbg_amd import pipeline
    gold = json.load(open(os.path.join(GOLDEN, "example_cfg1_unitigs.json")))
    pre = str(tmp_path / "ex")
    res = pipeline.run_file(os.path.join(GOLDEN, "reads-0.00.fa.gz"), pre, 7, 10, 0.0008, 2, contigs=True)
    assert res["n_unitigs"] == gold["n_unitigs"] and res["n_nodes"] == 104 and res["n_edges"] == 206
    assert hashlib.sha256(open(pre + ".unitigs.fa", "rb").read()).hexdigest() == gold["fasta_sha256"]
    assert hashlib.sha256(open(pre + ".unitigs.gfa", "rb").read()).hexdigest() == gold["gfa_sha256"]
    off = str(tmp_path / "off")
    res = pipeline.run_file(os.path.join(GOLDEN, "reads-0.00.fa.gz"), off, 7, 10, 0.0008, 2)      # default: nothing new
    assert "n_unitigs" not in res and not os.path.exists(off + ".unitigs.fa") and not os.path.exists(off + ".unitigs.gfa")


def test_full_size_unitigs_equal_restatement():
    """BASELINE configs[1] (the graph tests/test_gpu_fullsize.py builds): the unitig list equals the restatement; node-partition and edge-count invariants"""
    R = _mdbg()
    k, l, d, a = 21, 12, 0.003, 2
    n_reads = 100000
    with R.Mdbg(k, l, d, a) as m:
        db, do, nb = m.synth_reads_device(seed=2, genome_len=30_000_000, n_reads=n_reads)
        m.ingest_device(db, do, n_reads, nb, 0)
        nodes = m.finalize()
        edges = m.graph_edges(0.01)
        got = m.graph_unitigs()
    assert nodes["n_nodes"] > 100000 and len(edges["n1"]) > 100000
    assert sorted(got["node"].tolist()) == nodes["index"].tolist()                # every node on exactly one unitig
    exp = assert_equals_restatement(got, nodes, edges, None)
    # records minus the records that lie on interior links (as themselves or as mirrors) = unitig edges; links = nodes - unitigs (no cycles closed inside a walk)
    inner = set()
    for w in exp["walks"]:
        for x, y in zip(w, w[1:]):
            inner.add((x, y))
            inner.add((U.comp(y), U.comp(x)))
    assert len(got["edges"]["n1"]) == sum((u, v) not in inner for u, v, _ in U.as_records(edges))
    assert sum(len(w) - 1 for w in exp["walks"]) == len(nodes["index"]) - len(exp["walks"])
    # LN = sum of the pieces, and the overlaps lie within both unitigs
    assert np.array_equal(got["length"], np.add.reduceat(got["len"].astype(np.uint64), got["offsets"][:-1].astype(np.int64)))
    e = got["edges"]
    assert np.all(e["overlap"] <= got["length"][e["n1"]]) and np.all(e["overlap"] <= got["length"][e["n2"]])
    print("configs[1]: %d nodes, %d edges -> %d unitigs (%d circular), %d unitig edges, %d jumping rounds" %
          (len(nodes["index"]), len(edges["n1"]), got["n_unitigs"], int(got["circular"].sum()), len(e["n1"]), got["n_rounds"]))


def test_multik_with_unitigs_as_the_feedback_producer(tmp_path):
    """run_multik(contigs_fn="unitigs") == run_multik with a caller's function that returns the same unitigs (built here from the round's files by the restatement)"""
    from rust_mdbg_amd import pipeline
    reads, _ = synth_case(3, 70)
    fa = str(tmp_path / "reads.fa")
    write_fasta(fa, reads)
    ks, l, d = [15, 21], 12, 0.003
    fed = {}

    def by_restatement(k, gfa_path, nodes):
        L = [ln.split("\t") for ln in open(gfa_path).read().split("\n") if ln.startswith("L\t")]
        edges = [(int(f[1]), f[2], int(f[3]), f[4], int(f[5][:-1])) for f in L]
        prev = fed.get("contigs", [])
        src = {i: c for i, c in enumerate(prev + prev)}
        src.update({pipeline.READ_ORDINAL_BASE + i: r for i, r in enumerate(reads)})
        u = U.unitigs(nodes, edges, src)
        fed["contigs"] = [s.encode() for s in u["seqs"] if len(s) >= 20000]
        return [s.encode() for s in u["seqs"]]
    a = pipeline.run_multik(fa, str(tmp_path / "a"), ks, l, d, 2, reads_already_hpc=True, contigs_fn="unitigs", min_contig_len=20000)
    b = pipeline.run_multik(fa, str(tmp_path / "b"), ks, l, d, 2, reads_already_hpc=True, contigs_fn=by_restatement, min_contig_len=20000)
    assert a == b and a[21]["n_contigs"] > 0
    for k in ks:
        assert open(str(tmp_path / ("a-k%d.gfa" % k)), "rb").read() == open(str(tmp_path / ("b-k%d.gfa" % k)), "rb").read()
