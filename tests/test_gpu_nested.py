"""The NESTED step on the GPU (MDBG_SIMPLIFY_NESTED of Mdbg.graph_simplify: csrc/placement.hip on a list that holds copies, csrc/repeats.hip on a graph that
holds copies) against the plain restatement (tests/nested_restatement.py), list for list from the host and the device variant, on the hand-built catalogue of
tests/nested_graphs.py; the four placement counts of the library (MDBG_NESTED_STATS) against the checker's on the same catalogue; the step on graphs without
copies against the REPEATS step, array for array; the refusals and the state round a list that holds copies; contexts that hold no reads; base space through the library, run_file and the C
program's -R; and the catalogue once more under MDBG_GUARD.  CPU side: tests/test_nested_cpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nested_graphs as NG
import nested_restatement as NR
import sketch_graphs as G
import transit_graphs as TG
import unitig_restatement as U
from conftest import ROOT
from test_gpu_components import check_components
from test_gpu_parity import _mdbg
from test_gpu_read_paths import built
from test_gpu_repeats import assert_equals_checker, device_list, refused, walks_of
from test_gpu_simplify import same_list
from test_gpu_unitigs import build_cli, read_fasta
from test_nested_cpu import ACCEPTED, COUNTS, REFUSED, base_space_case, expected, nested_invariants
from test_read_paths_cpu import hashes
from test_repeats_cpu import BASE_PARAMS, MIXED, pieces_of

pytestmark = pytest.mark.gpu

TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS, NESTED = NR.TIPS, NR.BUBBLES, NR.COMPONENTS, NR.EDGES, NR.REPEATS, NR.NESTED
E_PARAM, E_STATE = -1, -6


def check(R, m, nodes, edges, steps, log, exp, strings=None):
    """the schedule on the context: host variant twice and device variant, all against the checker's (log, exp) -> got"""
    got, again, dev = m.graph_simplify(steps), m.graph_simplify(steps), device_list(R, m, steps)
    assert got["stats"] == again["stats"] == dev["stats"]
    same_list(got, again, R)                                                        # two calls give identical arrays
    same_list(got, dev, R)
    assert_equals_checker(got, log, exp, nodes, strings)                            # with the stats identity n_entries == rows - removed + all copies
    nested_invariants(nodes, edges, log, dict(exp, walks_original=walks_of(got), kc_sum=got["kc_sum"].tolist()))
    return got


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------------------------------------
def run_case(R, name):
    c = NG.BY_NAME[name]
    log, exp, _ = expected(name)
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        got = check(R, m, nodes, m.graph_edges(c.presimp), c.steps, log, exp)
        assert sorted(np.diff(got["offsets"].astype(np.int64)).tolist()) == c.expect
        assert got["stats"]["n_compactions"] == 1 + sum(1 for st in log if st.get("copies") or st["nodes"] or st["edges"])
        same_list(m.graph_unitigs(), ul, R)                                         # the plain list is what it was
    return got


@pytest.mark.parametrize("name", NG.CASE_IDS)
def test_catalogue_against_the_checker(name):
    run_case(_mdbg(), name)


def test_many_nested_side_by_side():
    """300 families in two batches: more resolved unitigs in the second round, and more ambiguous runs, than one workgroup holds"""
    R = _mdbg()
    reads = NG.many_nested(300)
    steps = [(REPEATS, 1, 0), (NESTED, 1, 0)]
    m, nodes, ul = built(R, reads, 3, 1, split=500)
    with m:
        edges = m.graph_edges(0.0)
        log, exp = NR.simplify(nodes, edges, steps, hashes(reads), 3, None, G.length_of_walk(nodes))
        got = check(R, m, nodes, edges, steps, log, exp)
        assert (got["stats"]["entries_copied"], got["n_unitigs"], set(np.diff(got["offsets"].astype(np.int64)).tolist()), len(got["edges"]["n1"])) == (4200, 900, {11, 19}, 0)


# ---- the placement counts: what a wrong placement changes even where no list can change ----------------------------------------------------------------------------
STATS_LINE = re.compile(r"^mdbg nested: ambiguous (\d+) resolved (\d+) conflicts (\d+) unanchored (\d+)$", re.M)


def counts_child():
    import rust_mdbg_amd as R
    for name in NG.CASE_IDS:
        c = NG.BY_NAME[name]
        m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
        with m:
            print("CASE %s" % name, file=sys.stderr, flush=True)
            m.graph_simplify(c.steps)
    print("COUNTS_DONE")


def test_placement_counts_against_the_checker():
    """one child process with MDBG_NESTED_STATS set runs every case once; the library's line per simplify call carries the four counts summed over the NESTED
    steps that ran on a graph with copies"""
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_nested as T; T.counts_child()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, MDBG_NESTED_STATS="1"), timeout=600)
    assert r.returncode == 0 and "COUNTS_DONE" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    parts = r.stderr.split("CASE ")[1:]
    assert len(parts) == len(NG.CASE_IDS)
    for part in parts:
        name = part.split("\n", 1)[0]
        got = STATS_LINE.findall(part)
        assert len(got) == 1, (name, part)
        counts = tuple(int(x) for x in got[0])
        print(name, counts)
        assert counts == expected(name)[2], name
        assert NG.BY_NAME[name].counts in (None, counts)


# ---- on a graph without copies the step IS the REPEATS step ----------------------------------------------------------------------------------------------------------
def as_nested(steps):
    return [(NESTED if kind == REPEATS else kind, a, b) for kind, a, b in steps]


def same_as_repeats(R, m, steps):
    rep, nes = m.graph_simplify(steps), m.graph_simplify(as_nested(steps))
    same_list(rep, nes, R)
    assert rep["stats"] == nes["stats"]                                            # n_syncs and n_compactions among them
    assert (rep["n_unitigs"], rep["n_entries"]) == (nes["n_unitigs"], nes["n_entries"])
    return rep


@pytest.mark.parametrize("name", [c.name for c in TG.CASES if c.name != "long"] + ["long"])
def test_hand_built_repeats_as_the_repeats_step(name):
    R = _mdbg()
    c = TG.BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        m.graph_edges(c.presimp)
        copied = [same_as_repeats(R, m, (c.steps or []) + [(REPEATS, ms, 0)])["stats"]["entries_copied"] for ms in sorted(c.expect["resolved"])]
        assert [x > 0 for x in copied] == [c.expect["resolved"][ms] > 0 for ms in sorted(c.expect["resolved"])]


@pytest.mark.parametrize("seed", [1, 4, 7, 2])
def test_random_graphs_as_the_repeats_step(seed):
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        m.graph_edges(presimp)
        same_as_repeats(R, m, [(REPEATS, 1, 0)])
        same_as_repeats(R, m, MIXED)


def test_a_second_round_on_a_random_graph():
    """a schedule of every kind but SUPERBUBBLES with two NESTED steps behind the REPEATS step, against the checker"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(4)
    steps = [(EDGES, 1, 0), (REPEATS, 1, 0), (TIPS, 3, 0), (NESTED, 1, 0), (NESTED, 1, 0), (COMPONENTS, 2, 0)]
    strings = G.fake_bases(reads, G.L, 4)
    m, nodes, ul = built(R, reads, k, A, 40, presimp)
    with m:
        edges = m.graph_edges(presimp)
        log, exp = NR.simplify(nodes, edges, steps, hashes(reads), k, strings)
        got = check(R, m, nodes, edges, steps, log, exp, strings)
        assert got["stats"]["entries_copied"] > 0
        check_components(R, m, exp)


# ---- state ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_schedules_and_a_list_that_holds_copies():
    R = _mdbg()
    c = NG.BY_NAME["nested"]
    log, exp, _ = expected("nested")
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        n_resolved = m.graph_transits()["n_resolved"]
        for bad in REFUSED:                                                         # refused while the schedule is validated; the plain list stays current
            refused(lambda: m.graph_simplify(bad), E_PARAM)
            assert m.graph_transits()["n_resolved"] == n_resolved == 1
        for good in ACCEPTED:
            m.graph_simplify(good)
        m.graph_unitigs()
        none = m.graph_simplify([(NESTED, 3, 0)])                                   # a NESTED step that copied nothing: the list is placed as always
        assert none["stats"]["entries_copied"] == 0 and m.graph_transits()["n_resolved"] == 1 and m.graph_read_paths()["n_reads"] == len(c.reads)
        got = m.graph_simplify(c.steps)
        assert got["stats"]["entries_copied"] == exp["copies"] == 14 and m.transits_ms() > 0.0      # the device time of the two steps' transit stages
        for call in (m.graph_read_paths, m.graph_junctions, m.graph_transits, m.graph_read_paths_device, m.graph_junctions_device, m.graph_transits_device):
            assert "copies" in refused(call, E_STATE)
        got = m.graph_simplify([(NESTED, 1, 0)])                                    # a NESTED step alone that copied
        assert got["stats"]["entries_copied"] == 3
        assert "copies" in refused(m.graph_transits, E_STATE)
        m.graph_simplify(c.steps)
        check_components(R, m, exp)                                                 # components read the list, not the table
        ctg = m.graph_unitigs()
        same_list(ctg, ul, R)                                                       # the context is usable: the plain list again, and the reads are placed on it
        assert m.graph_transits()["n_resolved"] == 1 and m.graph_read_paths()["n_reads"] == len(c.reads)
    with R.Mdbg(3, G.L, G.D, 1) as m:                                               # an empty context: the empty list, no error
        got = m.graph_simplify([(REPEATS, 1, 0), (NESTED, 1, 0)])
        assert got["n_unitigs"] == 0 and got["stats"]["entries_copied"] == 0


WITHOUT_READS = ([(NESTED, 1, 0)], [(REPEATS, 1, 0), (NESTED, 1, 0)], [(NESTED, 1, 0), (NESTED, 1, 0)])


def test_contexts_without_resident_reads():
    """MDBG_OK and nothing copied wherever a context holds no reads a NESTED step could use.

    A context with a finalized table that HAS rows, an edge list and NO read in the store cannot be made through the public interface, so the `!has_reads` exit
    that the REPEATS and NESTED steps share in simplify_unitigs is defensive and no test reaches it, for either kind: rows come only from the windows of the
    store's batches (mdbg_ingest_*, mdbg_ingest_sketch, mdbg_sketch_commit*: each registers its reads with the batch; a routed table, mdbg_insert_records, is
    refused by every graph call), so a table with a row has a read behind it; and the two calls that take reads out of the store, mdbg_rewind and mdbg_reset,
    clear the table first (clear_table before store_truncate).  What CAN be made is below: a context whose batches were all taken back answers before the
    schedule's first step, with the empty list."""
    R = _mdbg()
    c = NG.BY_NAME["nested"]

    def nothing(m):
        for steps in WITHOUT_READS:
            for got in (m.graph_simplify(steps), device_list(R, m, steps)):
                assert (got["n_unitigs"], got["n_entries"], got["stats"]["entries_copied"], got["stats"]["total_nodes_removed"]) == (0, 0, 0, 0)
        for bad in REFUSED:                                                         # the schedule is validated first all the same
            refused(lambda: m.graph_simplify(bad), E_PARAM)

    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        assert m.graph_simplify(c.steps)["stats"]["entries_copied"] == 14
        mark = m.mark()
        assert mark >= 1
        m.rewind(0)                                                                 # every batch forgotten, and the table with them: an empty context again
        nothing(m)
        m.reset(0)
        nothing(m)


# ---- base space -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_contig_through_the_nested_repeat_in_base_space(tmp_path):
    """an error-free genome A xuy M1 xuy M2 u B with u of 1,000 and x u y of 3,000 bases, tiled reads of 5,000: [(REPEATS, 2, 0)] leaves several contigs,
    [(REPEATS, 2, 0), (NESTED, 2, 0)] one that is an exact piece of the genome — from graph_contigs on the kept reads, through run_file, and through the C
    program's -r 2 -R 2"""
    from rust_mdbg_amd import pipeline
    R = _mdbg()
    k, l, d, A = BASE_PARAMS
    genome, reads, b, o, H, _, _ = base_space_case()
    steps = [(REPEATS, 2, 0), (NESTED, 2, 0)]
    with R.Mdbg(k, l, d, A, reads_already_hpc=True, keep_reads=True) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        edges = m.graph_edges(0.0)
        ul = m.graph_unitigs()
        once = m.graph_simplify(steps[:1])
        assert once["n_unitigs"] > 1 and once["stats"]["entries_copied"] > 0
        log, exp = NR.simplify(nodes, edges, steps, H, k, reads)
        got = check(R, m, nodes, edges, steps, log, exp, reads)
        assert got["stats"]["entries_copied"] > 3 * once["stats"]["entries_copied"]
        ctg = m.graph_contigs(0)
        offs = ctg["offsets"].tolist()
        seqs = [bytes(ctg["bases"][x:y]).decode("latin-1") for x, y in zip(offs, offs[1:])]
        assert seqs == exp["seqs"] and pieces_of(genome, seqs) and len(seqs) == 1 < once["n_unitigs"] < ul["n_unitigs"]
        assert len(seqs[0]) > len(genome) - 2000
        check_components(R, m, exp)
    src = str(tmp_path / "reads.fa")
    with open(src, "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, r.decode()) for i, r in enumerate(reads)))
    pre = str(tmp_path / "p")
    res = pipeline.run_file(src, pre, k, l, d, A, reads_already_hpc=True, contigs=True, simplify=steps, transits=2)
    assert open(pre + ".msimpl.fa").read() == U.fasta_text(exp) and open(pre + ".msimpl.gfa").read() == U.gfa_text(exp)
    assert res["simplify"]["entries_copied"] == exp["copies"] > 0 and res["n_simplified"] == 1 and res["simplified_read_evidence_written"] is False
    assert os.path.exists(pre + ".unitigs.transits.tsv") and not os.path.exists(pre + ".msimpl.transits.tsv")
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "c")
    out = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--skiphpc", "-r", "2", "-R", "2", "--contigs", "--transits", "2",
                          "--prefix", cpre], check=True, capture_output=True, text=True).stdout
    assert "simplify step 1 (repeats 2)\n" in out and "simplify step 2 (nested repeats 2)\n" in out and "simplify: %d entries copied\n" % exp["copies"] in out
    for ext in (".msimpl.gfa", ".msimpl.fa", ".unitigs.gfa", ".unitigs.transits.tsv"):
        assert open(pre + ext, "rb").read() == open(cpre + ext, "rb").read(), ext
    names, cseqs = read_fasta(cpre + ".msimpl.fa")
    assert len(cseqs) == 1 and pieces_of(genome, cseqs)


# ---- under MDBG_GUARD: no kernel of the step writes outside its blocks -------------------------------------------------------------------------------------------------
GUARD_LINE = re.compile(r"^GUARD_OK calls=(\d+) blocks=(\d+) bytes=(\d+)$", re.M)


def guard_child():
    import rust_mdbg_amd as R
    from rust_mdbg_amd import api
    assert api.GUARD and api.load_library().mdbg_guard_selftest() == 0
    print("SELFTEST_OK", flush=True)
    for name in NG.CASE_IDS:
        run_case(R, name)
    api.guard_check()
    print("GUARD_OK calls=%d blocks=%d bytes=%d" % (api.GUARD_SEEN["calls"], api.GUARD_SEEN["blocks"], api.GUARD_SEEN["bytes"]))


def test_catalogue_under_guard():
    base = {k: v for k, v in os.environ.items() if k not in ("MDBG_GUARD", "MDBG_POISON")}
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_nested as T; T.guard_child()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(base, MDBG_GUARD="1"), timeout=600)
    print(r.stdout[-2500:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = GUARD_LINE.search(r.stdout)
    assert got is not None and r.stdout.startswith("SELFTEST_OK\n"), (r.stdout[-1500:], r.stderr[-3000:])
    assert all(int(x) > 0 for x in got.groups()), got.group(0)
