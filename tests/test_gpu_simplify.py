"""Tips and simple bubbles removed on the GPU (mdbg_graph_simplify, csrc/simplify.hip) == the plain restatement of the rules
(tests/simplify_restatement.py): the unitig list that is left field for field, the per-step removal counts, and the copy plan executed by libmdbg_emit."""
import os
import random
import subprocess

import numpy as np
import pytest

import simplify_restatement as S
import unitig_restatement as U
from conftest import GOLDEN
from oracle import oracle as O
from test_gpu_parity import _mdbg
from test_gpu_unitigs import ARRAYS, CYCLE_PARAMS, build_cli, cyclic_reads, write_fasta
from test_simplify_cpu import PLANTED_PARAMS, PLANTED_STEPS, check_properties, planted_case
from test_unitigs_cpu import assert_genome_substrings, fuzz_case

pytestmark = pytest.mark.gpu


def magic():
    from rust_mdbg_amd.api import MAGIC_SIMPLIFY_STEPS
    return MAGIC_SIMPLIFY_STEPS


SCHEDULES = {"empty": lambda: [], "one tip step": lambda: [(1, 10, 50000)], "one bubble step": lambda: [(2, 0, 100000)], "magic": magic}


def assert_equals_restatement(got, nodes, edges, reads, steps):
    """the shape of test_gpu_unitigs.assert_equals_restatement, against the simplified graph; -> (log, expected unitigs)"""
    log, exp = S.simplify(nodes, edges, steps, reads)
    st = got["stats"]
    print("removed per step (unitigs, nodes):", list(zip(st["unitigs_removed"], st["nodes_removed"])), "compactions", st["n_compactions"], "syncs", st["n_syncs"])
    assert st["unitigs_removed"] == [len(x["unitigs"]) for x in log] and st["nodes_removed"] == [len(x["nodes"]) for x in log]
    assert st["total_unitigs_removed"] == sum(st["unitigs_removed"]) and st["total_nodes_removed"] == sum(st["nodes_removed"])
    off = got["offsets"].tolist()
    walks = [list(zip(got["node"][a:b].tolist(), (chr(c) for c in got["ori"][a:b]))) for a, b in zip(off, off[1:])]
    assert walks == exp["walks"]
    assert got["circular"].astype(bool).tolist() == exp["circular"] and got["kc_sum"].tolist() == exp["kc_sum"]
    assert got["n_unitigs"] == len(walks) and got["n_entries"] == len(nodes["index"]) - st["total_nodes_removed"] == off[-1]
    e = got["edges"]
    rows = list(zip(e["n1"].tolist(), (chr(c) for c in e["o1"]), e["n2"].tolist(), (chr(c) for c in e["o2"]), e["overlap"].tolist()))
    assert rows == exp["edges"]                                                    # unitig edges in source order, overlaps fixed
    assert got["length"].tolist() == exp["length"]
    for a, b in zip(off, off[1:]):
        assert got["dst_offset"][a:b].tolist() == np.concatenate([[0], np.cumsum(got["len"][a:b].astype(np.uint64))[:-1]]).astype(np.uint64).tolist()
    from rust_mdbg_amd import emit as E
    with E.Contigs(got) as c:                                                      # the plan executed (no node-count check: the list covers the survivors only)
        c.add_batch(*O.concat_reads(reads), 0)
        assert [s.decode("latin-1") for s in c.sequences()] == exp["seqs"]
    return log, exp


def same_list(a, b, R):
    for f in ARRAYS:
        assert np.array_equal(a[f], b[f]), f
    for f, _ in R.api.EDGE_FIELDS:
        assert np.array_equal(a["edges"][f], b["edges"][f]), f


def run_simplify(R, reads, k, l, d, A, presimp, steps, hpc=False):
    b, o = O.concat_reads(reads)
    with R.Mdbg(k, l, d, A, reads_already_hpc=hpc) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        edges = m.graph_edges(presimp)
        plain = m.graph_unitigs()
        got = m.graph_simplify(steps)
        again = m.graph_simplify(steps)                                            # buffers are reused: same answer
        dev, dstats = m.graph_simplify_device(steps)
        cnt = R.api.unitig_counts(dev)
        for f, t in R.api.UNITIG_FIELDS:                                           # host and device variants agree
            assert np.array_equal(m.to_host(getattr(dev, f), cnt[f] * np.dtype(t).itemsize, t) if cnt[f] else np.zeros(0, t), got[f][:cnt[f]]), f
        n = int(dev.edges.n)
        for f, t in R.api.EDGE_FIELDS:
            assert np.array_equal(m.to_host(getattr(dev.edges, f), n * np.dtype(t).itemsize, t) if n else np.zeros(0, t), got["edges"][f]), f
        assert dstats == got["stats"] == again["stats"]
        same_list(m.graph_unitigs(), plain, R)                                     # the unsimplified list again
        same_list(m.graph_simplify([]), plain, R)                                  # the empty schedule is the unitig call
    same_list(got, again, R)
    return nodes, edges, got, plain


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("presimp", [0.0, 0.01])
@pytest.mark.parametrize("seed", range(6))
def test_gpu_simplify_equals_restatement_on_fuzz_graphs(seed, presimp, sched):
    R = _mdbg()
    k, l, d, A, reads = fuzz_case(seed)
    steps = SCHEDULES[sched]()
    nodes, edges, got, plain = run_simplify(R, reads, k, l, d, A, presimp, steps)
    assert_equals_restatement(got, nodes, edges, reads, steps)
    if not steps:
        same_list(got, plain, R)
        assert got["stats"]["n_compactions"] == 1


def test_gpu_simplify_removes_both_kinds_on_the_fuzz_graphs():
    R = _mdbg()
    tips = bubbles = 0
    for seed in (0, 5):
        k, l, d, A, reads = fuzz_case(seed)
        _, _, got, _ = run_simplify(R, reads, k, l, d, A, 0.0, magic())
        for (kind, _, _), nu in zip(magic(), got["stats"]["unitigs_removed"]):
            tips += nu if kind == 1 else 0
            bubbles += nu if kind == 2 else 0
    assert tips > 0 and bubbles > 0


@pytest.mark.parametrize("kind", ["circular", "tandem", "inverted"])
@pytest.mark.parametrize("seed", range(4))
def test_gpu_simplify_on_cycles_and_hairpins(seed, kind):
    R = _mdbg()
    rnd = random.Random(900 + seed)
    k, l, d, A = rnd.choice(CYCLE_PARAMS)
    reads = cyclic_reads(kind, rnd)
    steps = [(1, 0, 0), (2, 0, 0)] + magic()                                       # without limits first: circular unitigs are never small, hairpins follow the rules
    nodes, edges, got, _ = run_simplify(R, reads, k, l, d, A, rnd.choice([0.0, 0.01]), steps)
    assert_equals_restatement(got, nodes, edges, reads, steps)


@pytest.mark.parametrize("what", ["tips", "bubbles", "tips+bubbles"])
def test_gpu_simplify_planted_errors(what):
    R = _mdbg()
    reads, genome = planted_case(1, what)
    k, l, d, A = PLANTED_PARAMS
    nodes, edges, got, plain = run_simplify(R, reads, k, l, d, A, 0.0, PLANTED_STEPS, hpc=True)
    log, exp = assert_equals_restatement(got, nodes, edges, reads, PLANTED_STEPS)
    assert_genome_substrings(exp["names"], exp["seqs"], exp["length"], genome)
    assert got["n_unitigs"] < plain["n_unitigs"]
    if "tips" in what:
        assert got["stats"]["unitigs_removed"][0] > 0
    if "bubbles" in what:
        assert got["stats"]["unitigs_removed"][1] > 0


def test_gpu_simplify_state_rules_and_errors(example_reads):
    R = _mdbg()
    with R.Mdbg(7, 10, 0.0008, 2) as m:
        m.ingest_reads(example_reads, 0)
        for step in (lambda: None, m.finalize):                                    # no finalize; finalized but no edge list
            step()
            with pytest.raises(R.MdbgError) as ei:
                m.graph_simplify(magic())
            assert ei.value.code == -6
        m.graph_edges(0.01)
        for bad in ([(0, 1, 1)], [(1, 10, 50000), (3, 0, 0)]):                     # unknown kind
            with pytest.raises(R.MdbgError) as ei:
                m.graph_simplify(bad)
            assert ei.value.code == -1
        u, st = R.api.UnitigList(), R.api.SimplifyStats()
        import ctypes as C
        assert m.L.mdbg_graph_simplify(m.h, None, 2, C.byref(u), C.byref(st)) == -1      # null steps with n_steps > 0
        got = m.graph_simplify(magic())
        assert got["n_entries"] == 104 - got["stats"]["total_nodes_removed"]
    with R.Mdbg(7, 10, 0.0008, 2) as m:                                            # partitioned context
        m.set_partition(2, 0)
        with pytest.raises(R.MdbgError) as ei:
            m.graph_simplify(magic())
        assert ei.value.code == -6
    with R.Mdbg(7, 10, 0.0008, 2) as m:                                            # empty context: empty list, no error
        u = m.graph_simplify(magic())
        assert u["n_unitigs"] == 0 and u["n_entries"] == 0 and u["stats"]["total_nodes_removed"] == 0


def parse_gfa_names(text):
    return [ln.split("\t")[1] for ln in text.split("\n") if ln.startswith("S\t")]


def test_run_file_and_cli_write_the_simplified_contigs(tmp_path):
    """pipeline.run_file(contigs=True, simplify=...) on the example fixture: .msimpl.gfa == the restatement's text, .unitigs.gfa untouched, and mdbg_cli --simplify
    writes the same files"""
    from rust_mdbg_amd import pipeline
    from test_unitigs_cpu import parse_gfa
    R = _mdbg()
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    pre, ref = str(tmp_path / "s"), str(tmp_path / "plain")
    res = pipeline.run_file(src, pre, 7, 10, 0.0008, 2, contigs=True, simplify=magic())
    pipeline.run_file(src, ref, 7, 10, 0.0008, 2, contigs=True)
    for ext in (".unitigs.gfa", ".unitigs.fa", ".gfa"):
        assert open(pre + ext, "rb").read() == open(ref + ext, "rb").read(), ext
    assert not os.path.exists(ref + ".msimpl.gfa")
    reads = Rreads(src)
    with R.Mdbg(7, 10, 0.0008, 2) as m:
        m.ingest_reads(reads, 0)
        nodes = m.finalize()
        edges = m.graph_edges(0.01)
    log, exp = S.simplify(nodes, edges, magic(), reads)
    text = open(pre + ".msimpl.gfa").read()
    parse_gfa(text)
    assert text == U.gfa_text(exp) and open(pre + ".msimpl.fa").read() == U.fasta_text(exp)
    assert res["n_simplified"] == len(exp["walks"]) and res["simplify"]["nodes_removed"] == [len(x["nodes"]) for x in log]
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "c")
    out = subprocess.run([exe, src, "-k", "7", "-l", "10", "--density", "0.0008", "--minabund", "2", "--simplify", "--prefix", cpre], check=True, capture_output=True, text=True).stdout
    assert "simplify" in out
    for ext in (".msimpl.gfa", ".msimpl.fa", ".unitigs.gfa", ".unitigs.fa"):
        assert open(pre + ext, "rb").read() == open(cpre + ext, "rb").read(), ext
    c2 = str(tmp_path / "c2")                                                      # -t / -b in command-line order == the same steps through Python
    subprocess.run([exe, src, "-k", "7", "-l", "10", "--density", "0.0008", "--minabund", "2", "-t", "10,50000", "-b", "100000", "-t", "3,0", "--prefix", c2], check=True,
                   stdout=subprocess.DEVNULL)
    p2 = str(tmp_path / "p2")
    pipeline.run_file(src, p2, 7, 10, 0.0008, 2, contigs=True, simplify=[(1, 10, 50000), (2, 0, 100000), (1, 3, 0)])
    for ext in (".msimpl.gfa", ".msimpl.fa"):
        assert open(p2 + ext, "rb").read() == open(c2 + ext, "rb").read(), ext


def Rreads(path):
    from rust_mdbg_amd.emit import Reader
    out = []
    with Reader(path) as r:
        for bases, offs in r.batches(1 << 30):
            out += [bytes(bases[int(a):int(b)]) for a, b in zip(offs, offs[1:])]
    return out


def test_multik_with_simplified_contigs_as_the_feedback_producer(tmp_path):
    """run_multik(contigs_fn="simplified") == run_multik with a caller's function that returns the restatement's simplified contigs"""
    from rust_mdbg_amd import pipeline
    reads, _ = planted_case(1, "tips")
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
        _, u = S.simplify(nodes, edges, magic(), src)
        fed["contigs"] = [s.encode() for s in u["seqs"] if len(s) >= 20000]
        return [s.encode() for s in u["seqs"]]
    a = pipeline.run_multik(fa, str(tmp_path / "a"), ks, l, d, 2, reads_already_hpc=True, contigs_fn="simplified", min_contig_len=20000)
    b = pipeline.run_multik(fa, str(tmp_path / "b"), ks, l, d, 2, reads_already_hpc=True, contigs_fn=by_restatement, min_contig_len=20000)
    assert a == b and a[21]["n_contigs"] > 0
    for k in ks:
        assert open(str(tmp_path / ("a-k%d.gfa" % k)), "rb").read() == open(str(tmp_path / ("b-k%d.gfa" % k)), "rb").read()


def test_full_size_simplify_properties():
    """BASELINE configs[1] with reads at synth.py's default err_ppm.  The restatement re-compacts the whole graph in Python once per step, which is minutes per step at
    this size, so this case checks the PROPERTIES (whole unitigs removed, no new dead ends, counts, node partition) and not equality with the restatement."""
    R = _mdbg()
    k, l, d, a = 21, 12, 0.003, 2
    n_reads = 100000
    steps = magic()
    with R.Mdbg(k, l, d, a) as m:
        db, do, nb = m.synth_reads_device(seed=2, genome_len=30_000_000, n_reads=n_reads)
        m.ingest_device(db, do, n_reads, nb, 0)
        nodes = m.finalize()
        edges = m.graph_edges(0.01)
        plain = m.graph_unitigs()
        one = m.graph_simplify(steps[:1])
        got = m.graph_simplify(steps)
    st = got["stats"]
    print("configs[1]: %d nodes, %d edges, %d unitigs -> %d unitigs, %d nodes; removed per step %s; %d compactions, %d rounds, %d syncs" %
          (len(nodes["index"]), len(edges["n1"]), plain["n_unitigs"], got["n_unitigs"], got["n_entries"], list(zip(st["unitigs_removed"], st["nodes_removed"])),
           st["n_compactions"], st["n_rounds_total"], st["n_syncs"]))
    assert st["total_nodes_removed"] > 0 and got["n_entries"] == len(nodes["index"]) - st["total_nodes_removed"]
    left = set(got["node"].tolist())
    assert len(left) == got["n_entries"] and left <= set(nodes["index"].tolist())
    # first step: the removed nodes are whole small unitigs of the plain list, and no surviving vertex lost its last in-arc
    off = plain["offsets"].tolist()
    left1 = set(one["node"].tolist())
    gone_u = 0
    for i, (x, y) in enumerate(zip(off, off[1:])):
        hit = [n in left1 for n in plain["node"][x:y].tolist()]
        assert all(hit) or not any(hit)
        if not hit[0]:
            gone_u += 1
            assert y - x <= steps[0][1] and plain["length"][i] <= steps[0][2] and not plain["circular"][i]
    assert gone_u == one["stats"]["unitigs_removed"][0] > 0 and len(nodes["index"]) - len(left1) == one["stats"]["nodes_removed"][0]
    recs = U.as_records(edges)
    had, has = set(), set()
    for u, v, _ in recs:
        for x, y in ((u, v), (U.comp(v), U.comp(u))):
            had.add(y)
            if x[0] in left1 and y[0] in left1:
                has.add(y)
    assert {v for v in had if v[0] in left1} == has
    # the final list is the compaction of the induced graph: every walk step is an arc between survivors, and kc_sum adds up
    ab = dict(zip(nodes["index"].tolist(), nodes["abundance"].tolist()))
    arcs = {(u, v) for u, v, _ in recs} | {(U.comp(v), U.comp(u)) for u, v, _ in recs}
    foff = got["offsets"].tolist()
    for i, (x, y) in enumerate(zip(foff, foff[1:])):
        w = list(zip(got["node"][x:y].tolist(), (chr(c) for c in got["ori"][x:y])))
        assert all((p, q) in arcs for p, q in zip(w, w[1:]))
        assert got["kc_sum"][i] == sum(ab[n] for n, _ in w)
