"""Connected components of the unitig graph found on the GPU (mdbg_graph_components, csrc/components.hip) and the small-component step of
mdbg_graph_simplify == the plain restatement (tests/components_restatement.py), field for field; state rules, errors, the pipeline's .tsv files and the CLI."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import components_restatement as CR
import simplify_restatement as S
import unitig_restatement as U
from oracle import oracle as O
from test_gpu_parity import _mdbg
from test_gpu_simplify import same_list
from test_gpu_unitigs import CYCLE_PARAMS, build_cli, cyclic_reads, write_fasta
from test_unitigs_cpu import fuzz_case

pytestmark = pytest.mark.gpu

K = CR.COMPONENTS
FIELDS = ("component", "first_unitig", "unitigs", "nodes", "bases", "kc_sum", "circular")


def magic():
    from rust_mdbg_amd.api import MAGIC_SIMPLIFY_STEPS
    return MAGIC_SIMPLIFY_STEPS


def check_components(R, m, cur):
    """the context's current unitig list is `cur` (a restatement's unitigs): its components equal the restatement's, from both variants, twice"""
    exp = CR.components(cur)
    got = m.graph_components()
    assert got["n_unitigs"] == len(cur["walks"]) and got["n_components"] == exp["n_components"]
    for f in FIELDS:
        assert got[f].tolist() == [int(x) for x in exp[f]], f
    again = m.graph_components()                                                   # no dependence on scheduling: identical arrays
    dev = m.graph_components_device()
    assert (int(dev.n_unitigs), int(dev.n_components)) == (got["n_unitigs"], got["n_components"]) == (again["n_unitigs"], again["n_components"])
    for f, t, per_unitig in R.api.COMPONENT_FIELDS:
        n = got["n_unitigs"] if per_unitig else got["n_components"]
        assert len(got[f]) == n and got[f].dtype == t and np.array_equal(got[f], again[f]), f
        assert np.array_equal(m.to_host(getattr(dev, f), n * np.dtype(t).itemsize, t) if n else np.zeros(0, t), got[f]), f
    return got


def assert_simplify_equals_restatement(got, nodes, edges, reads, steps):
    """the assertions of test_gpu_simplify.assert_equals_restatement with the component kind in the checker's step loop"""
    log, exp = CR.simplify(nodes, edges, steps, reads)
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
    assert rows == exp["edges"]
    assert got["length"].tolist() == exp["length"]
    for a, b in zip(off, off[1:]):
        assert got["dst_offset"][a:b].tolist() == np.concatenate([[0], np.cumsum(got["len"][a:b].astype(np.uint64))[:-1]]).astype(np.uint64).tolist()
    if got["n_unitigs"]:
        from rust_mdbg_amd import emit as E
        with E.Contigs(got) as c:                                                  # the plan executed
            c.add_batch(*O.concat_reads(reads), 0)
            assert [s.decode("latin-1") for s in c.sequences()] == exp["seqs"]
    return log, exp


def open_graph(R, reads, k, l, d, A, presimp, keep_reads=False):
    m = R.Mdbg(k, l, d, A, keep_reads=keep_reads)
    m.ingest(*O.concat_reads(reads), 0)
    nodes = m.finalize()
    edges = m.graph_edges(presimp)
    return m, nodes, edges


def contig_strings(g):
    off = g["offsets"].tolist()
    return [bytes(g["bases"][a:b]).decode("latin-1") for a, b in zip(off, off[1:])]


@pytest.mark.parametrize("presimp", [0.0, 0.01])
@pytest.mark.parametrize("seed", [0, 1, 3, 5])
def test_gpu_components_equal_restatement_on_fuzz_graphs(seed, presimp):
    """seed 5 is one component of thousands of unitigs (every edge contends for one root), seeds 0 and 1 fall into many tiny ones"""
    R = _mdbg()
    k, l, d, A, reads = fuzz_case(seed)
    m, nodes, edges = open_graph(R, reads, k, l, d, A, presimp, keep_reads=True)
    with m:
        plain = m.graph_unitigs()
        before = m.graph_contigs()
        cur = U.unitigs(nodes, edges, reads)
        got = check_components(R, m, cur)
        print("seed %d presimp %g: %d unitigs, %d components" % (seed, presimp, got["n_unitigs"], got["n_components"]))
        after = m.graph_contigs()                                                  # the list is left as it was: the same bytes
        assert np.array_equal(before["bases"], after["bases"]) and np.array_equal(before["offsets"], after["offsets"]) and contig_strings(after) == cur["seqs"]
        from rust_mdbg_amd import emit as E
        with E.Contigs(plain, n_nodes=len(nodes["index"])) as c:
            c.add_batch(*O.concat_reads(reads), 0)
            assert [s.decode("latin-1") for s in c.sequences()] == cur["seqs"]
        m.graph_simplify(magic())
        _, exp = S.simplify(nodes, edges, magic(), reads)
        check_components(R, m, exp)                                                # the simplified list is the current one now
        assert contig_strings(m.graph_contigs()) == exp["seqs"]
        same_list(m.graph_unitigs(), plain, R)


# ---- many components across workgroup borders ---------------------------------------------------------------------------------------------
MANY_PARAMS = (5, 10, 0.01, 2)


def many_genomes_case(seed, n_genomes):
    """random genomes of 1.5 to 6 kb, each given twice; every fourth also as an allele whose last third is drawn again (a fork: a component of several unitigs)"""
    rnd = random.Random(7000 + seed)
    reads = []
    for g in range(n_genomes):
        ln = rnd.randrange(1500, 6000)
        s = bytes(rnd.choice(b"ACGT") for _ in range(ln))
        reads += [s, s]
        if g % 4 == 0:
            alt = s[:2 * ln // 3] + bytes(rnd.choice(b"ACGT") for _ in range(ln // 3))
            reads += [alt, alt]
    rnd.shuffle(reads)
    return reads


@pytest.fixture(scope="module")
def many400():
    """(reads, nodes, edges, the restatement's unitigs and components) of the 400-genome case, computed once"""
    R = _mdbg()
    reads = many_genomes_case(0, 400)
    m, nodes, edges = open_graph(R, reads, *MANY_PARAMS, 0.0)
    m.close()
    cur = U.unitigs(nodes, edges, reads)
    return reads, nodes, edges, cur, CR.components(cur)


def test_many_components_across_workgroup_borders(many400):
    R = _mdbg()
    reads, nodes, edges, cur, cc = many400
    assert len(nodes["index"]) == 22644 and len(cur["walks"]) == 601 and cc["n_components"] == 400      # more components than a block has threads
    assert sum(x > 1 for x in cc["unitigs"]) == 100 and cc["unitigs"].count(3) == 99                      # every fourth genome forks: 99 components of three unitigs, one of four
    assert sum(b <= 3000 for b in cc["bases"]) == 123 and sum(n <= 20 for n in cc["nodes"]) == 25
    m, _, _ = open_graph(R, reads, *MANY_PARAMS, 0.0)
    with m:
        m.graph_unitigs()
        check_components(R, m, cur)


@pytest.mark.parametrize("steps", [[(K, 0, 3000)], [(K, 20, 0)], [(1, 10, 50000), (K, 20, 3000), (2, 0, 100000)]], ids=["bases", "nodes", "between tips and bubbles"])
def test_component_steps_equal_restatement(many400, steps):
    R = _mdbg()
    reads, nodes, edges, cur, cc = many400
    m, _, _ = open_graph(R, reads, *MANY_PARAMS, 0.0)
    with m:
        plain = m.graph_unitigs()
        got = m.graph_simplify(steps)
        again = m.graph_simplify(steps)
        dev, dstats = m.graph_simplify_device(steps)
        assert dstats == got["stats"] == again["stats"] and int(dev.n_unitigs) == got["n_unitigs"]
        same_list(got, again, R)
        log, exp = assert_simplify_equals_restatement(got, nodes, edges, reads, steps)
        check_components(R, m, exp)
        same_list(m.graph_unitigs(), plain, R)
    k = [s[0] for s in steps].index(K)
    assert got["stats"]["unitigs_removed"][k] > 0
    if len(steps) == 1:                                                            # what the step removes, counted from the components of the plain list
        small = [c for c in range(cc["n_components"]) if CR.small_component(c, cc, *steps[0][1:])]
        assert got["stats"]["unitigs_removed"] == [sum(cc["unitigs"][c] for c in small)] and got["stats"]["nodes_removed"] == [sum(cc["nodes"][c] for c in small)]
        assert len(small) == (123 if steps[0][2] else 25)


def test_a_step_may_remove_everything(many400):
    R = _mdbg()
    reads, nodes, edges, cur, _ = many400
    m, _, _ = open_graph(R, reads, *MANY_PARAMS, 0.0, keep_reads=True)
    with m:
        for steps in ([(K, 0, 10 ** 9)], [(K, 0, 10 ** 9), (1, 10, 50000), (K, 5, 0)]):
            got = m.graph_simplify(steps)
            assert got["n_unitigs"] == 0 and got["n_entries"] == 0 and len(got["edges"]["n1"]) == 0 and got["offsets"].tolist() == [0]
            assert got["stats"]["nodes_removed"] == [len(nodes["index"])] + [0] * (len(steps) - 1) and got["stats"]["unitigs_removed"][0] == len(cur["walks"])
            dev, dstats = m.graph_simplify_device(steps)
            assert int(dev.n_unitigs) == 0 and int(dev.n_entries) == 0 and int(dev.edges.n) == 0 and dstats == got["stats"]
            cc = m.graph_components()                                              # of the empty list
            assert cc["n_unitigs"] == 0 and cc["n_components"] == 0 and all(len(cc[f]) == 0 for f in FIELDS)
            assert m.graph_contigs()["n_contigs"] == 0
        assert m.graph_unitigs()["n_unitigs"] == len(cur["walks"])               # the context goes on


# ---- cycles, the example file -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["circular", "tandem", "inverted"])
@pytest.mark.parametrize("seed", range(4))
def test_gpu_components_on_cycles_and_hairpins(seed, kind):
    R = _mdbg()
    rnd = random.Random(900 + seed)
    k, l, d, A = rnd.choice(CYCLE_PARAMS)
    reads = cyclic_reads(kind, rnd)
    steps = [(K, 0, 10 ** 9)]
    m, nodes, edges = open_graph(R, reads, k, l, d, A, rnd.choice([0.0, 0.01]))
    with m:
        m.graph_unitigs()
        cur = U.unitigs(nodes, edges, reads)
        cc = check_components(R, m, cur)
        got = m.graph_simplify(steps)
        _, exp = assert_simplify_equals_restatement(got, nodes, edges, reads, steps)
        check_components(R, m, exp)
    keep = [u for u in range(len(cur["walks"])) if cc["circular"][cc["component"][u]]]      # exactly the components with a circular unitig stay
    assert exp["walks"] == [cur["walks"][u] for u in keep]
    print("%s seed %d: %d unitigs in %d components, %d circular; %d unitigs stay" % (kind, seed, len(cur["walks"]), cc["n_components"], int(cc["circular"].sum()), len(keep)))


def test_gpu_components_of_the_example_file(example_reads):
    R = _mdbg()
    m, nodes, edges = open_graph(R, example_reads, 7, 10, 0.0008, 2, 0.01)
    with m:
        m.graph_unitigs()
        cc = check_components(R, m, U.unitigs(nodes, edges, example_reads))
        assert int(cc["nodes"].sum()) == 104


# ---- state and errors ---------------------------------------------------------------------------------------------------------------------------
def code_of(fn, *a):
    R = _mdbg()
    with pytest.raises(R.MdbgError) as ei:
        fn(*a)
    return ei.value.code


def test_gpu_components_state_rules_and_errors(example_reads):
    import ctypes as C
    R = _mdbg()
    with R.Mdbg(7, 10, 0.0008, 2) as m:
        m.ingest_reads(example_reads, 0)
        assert code_of(m.graph_components) == -6                                   # before any unitig call
        m.finalize()
        assert code_of(m.graph_components) == -6
        m.graph_edges(0.01)
        assert code_of(m.graph_components) == -6 and code_of(m.graph_components_device) == -6
        plain = m.graph_unitigs()
        assert m.graph_components()["n_unitigs"] == plain["n_unitigs"]
        for end in (lambda: m.ingest_reads(example_reads[:10], len(example_reads)), m.finalize, lambda: m.graph_edges(0.01)):      # an ingest ends the unitig list; it takes a new one to have one again
            end()
            assert code_of(m.graph_components) == -6
        assert m.graph_unitigs()["n_unitigs"] == m.graph_components()["n_unitigs"] > 0
    with R.Mdbg(7, 10, 0.0008, 2) as m:
        m.ingest_reads(example_reads, 0)
        m.finalize()
        m.graph_edges(0.01)
        plain = m.graph_unitigs()
        for bad in ([(K, 0, 0)], [(1, 10, 50000), (K, 0, 0)], [(3, 0, 0)], [(5, 1, 1)]):      # a component step without a limit; unknown kinds
            assert code_of(m.graph_simplify, bad) == -1
        assert m.L.mdbg_graph_components(m.h, None) == -1 and m.L.mdbg_graph_components(None, C.byref(R.api.ComponentList())) == -1
        assert m.L.mdbg_graph_components_device(m.h, None) == -1
        same_list(m.graph_simplify([]), plain, R)                                  # the empty schedule is still the unitig call
        assert m.graph_components()["n_unitigs"] == plain["n_unitigs"]
    with R.Mdbg(7, 10, 0.0008, 2) as m:                                            # partitioned context
        m.set_partition(2, 0)
        assert code_of(m.graph_components) == -6
    with R.Mdbg(7, 10, 0.0008, 2) as m:                                            # empty context: zero counts, no error
        m.graph_unitigs()
        cc = m.graph_components()
        assert cc["n_unitigs"] == 0 and cc["n_components"] == 0 and len(cc["component"]) == 0
        dev = m.graph_components_device()
        assert int(dev.n_unitigs) == 0 and int(dev.n_components) == 0


# ---- pipeline and CLI ---------------------------------------------------------------------------------------------------------------------------
def read_tsv(path):
    rows = [ln.split("\t") for ln in open(path).read().split("\n")[:-1]]
    return [r[0] for r in rows], [int(r[1]) for r in rows]


def test_run_file_and_cli_report_the_components(tmp_path):
    from rust_mdbg_amd import pipeline
    R = _mdbg()
    k, l, d, A = MANY_PARAMS
    reads = many_genomes_case(0, 40)
    fa = str(tmp_path / "reads.fa")
    write_fasta(fa, reads)
    step = [(K, 20, 3000)]
    pre, ref = str(tmp_path / "c"), str(tmp_path / "plain")
    res = pipeline.run_file(fa, pre, k, l, d, A, contigs=True, simplify=step, components=True)
    off = pipeline.run_file(fa, ref, k, l, d, A, contigs=True, simplify=step)
    for ext in (".unitigs.gfa", ".unitigs.fa", ".gfa", ".msimpl.gfa", ".msimpl.fa"):
        assert open(pre + ext, "rb").read() == open(ref + ext, "rb").read(), ext
    assert not os.path.exists(ref + ".unitigs.components.tsv") and not os.path.exists(ref + ".msimpl.components.tsv") and "n_components" not in off
    with R.Mdbg(k, l, d, A) as m:
        m.ingest_reads(reads, 0)
        m.finalize()
        m.graph_edges(0.01)
        ul = m.graph_unitigs()
        cc = m.graph_components()
        sl = m.graph_simplify(step)
        sc = m.graph_components()
    names = lambda u: [R.api.unitig_name(i, c) for i, c in enumerate(u["circular"])]
    assert read_tsv(pre + ".unitigs.components.tsv") == (names(ul), cc["component"].tolist())
    assert read_tsv(pre + ".msimpl.components.tsv") == (names(sl), sc["component"].tolist())
    small = int(((cc["nodes"] <= 20) & (cc["bases"] <= 3000)).sum())
    assert res["n_components"] == cc["n_components"] == 40 and int((cc["bases"] <= 3000).sum()) == 14 and int((cc["nodes"] <= 20).sum()) == 6
    assert res["n_components_simplified"] == sc["n_components"] == 40 - small and small > 0
    assert res["simplify"]["unitigs_removed"] == sl["stats"]["unitigs_removed"] and res["simplify"]["nodes_removed"] == sl["stats"]["nodes_removed"]
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "cli")
    out = subprocess.run([exe, fa, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--contigs", "-c", "20,3000", "--components", "--prefix", cpre],
                         check=True, capture_output=True, text=True).stdout
    big = int(np.argmax(cc["nodes"]))
    assert "components: 40 (largest: %d nodes, %d bases)\n" % (cc["nodes"][big], cc["bases"][big]) in out
    assert "simplify step 1 (components 20,3000): %d unitigs, %d nodes removed\n" % (sl["stats"]["unitigs_removed"][0], sl["stats"]["nodes_removed"][0]) in out
    assert re.search(r"simplify: \d+ unitigs, \d+ nodes removed; %d contigs left" % sl["n_unitigs"], out)
    for ext in (".msimpl.gfa", ".msimpl.fa", ".unitigs.gfa", ".unitigs.fa"):
        assert open(pre + ext, "rb").read() == open(cpre + ext, "rb").read(), ext
