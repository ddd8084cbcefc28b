"""Transits on the GPU (Mdbg.graph_transits) against the plain restatement (tests/transits_restatement.py), exactly: every scalar, every column with its dtype, at
min_support 1, 2 and 4, twice from the host variant and once from the device variant — on the hand-built repeats of tests/transit_graphs.py, the catalogue of
tests/sketch_graphs.py (plain and simplified lists), the random graphs, ranges of reads, the invariants against the read paths and the junction support of the
same context, the other results a caller may hold, the state checks, the pipeline's files and the C program's.  CPU side: tests/test_transits_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import read_paths_restatement as RP
import sketch_graphs as G
import transit_graphs as TG
import transits_restatement as T
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from test_gpu_junctions import records_of
from test_gpu_parity import _mdbg
from test_gpu_read_paths import built, feed_batches
from test_gpu_simplify import same_list
from test_gpu_sketch_graphs import BY_NAME, feed
from test_read_paths_cpu import hashes
from test_transits_cpu import RANDOM, as_library_result, assert_same

pytestmark = pytest.mark.gpu

SCALARS = ("n_reads", "n_crossings", "n_explained", "n_passes", "n_transits", "n_unitigs", "n_repeats", "n_resolved")
MIN_SUPPORTS = (1, 2, 4)
E_PARAM, E_STATE = -1, -6
EDGES = 8


def expected(H, k, nodes, ul, min_support=1):
    """H: the reads as lists of minimizer hashes"""
    walks, _ = RP.walks_of(ul)
    return T.transits(H, k, nodes["keys"].tolist(), nodes["index"].tolist(), walks, records_of(ul), min_support)


def assert_zeros(R, got, first=0):
    assert got["first_read"] == first and all(got[f] == 0 for f in SCALARS) and all(len(got[f]) == 0 for f, _, _ in R.api.TRANSIT_FIELDS)


def check(R, m, H, k, nodes, ul, invariants=True):
    """the context's current list is `ul` (host arrays): the whole store's transits equal the restatement's at every min_support, twice from the host variant and
    once from the device variant; the invariants hold against the read paths and the junction support of the same context; -> (got at min_support 1, exp)"""
    if ul["n_unitigs"] == 0:                                                        # a schedule that removed everything: the empty list gives zeros
        got = m.graph_transits()
        assert_zeros(R, got)
        return got, None
    exp = expected(H, k, nodes, ul)
    first = None
    for ms in MIN_SUPPORTS:
        got = m.graph_transits(0, 0, ms)
        if first is None:
            first = got
            print(" ".join("%s %d" % (f, got[f]) for f in SCALARS))
        assert_same(got, as_library_result(T.at_min_support(exp, ms), len(H)))
        assert_same(m.graph_transits(min_support=ms), got)                          # nothing depends on scheduling
        dev = m.graph_transits_device(0, 0, ms)
        assert all(int(getattr(dev, f)) == got[f] for f in SCALARS) and int(dev.first_read) == 0
        for f, t, per in R.api.TRANSIT_FIELDS:
            back = np.empty(got["n_transits" if per == "transit" else "n_unitigs"], t)
            m._chk(m.L.mdbg_copy_to_host(m.h, back.ctypes.data, getattr(dev, f), back.nbytes))
            assert np.array_equal(back, got[f]), (f, ms)
    assert m.transits_ms() >= 0.0
    if invariants:
        check_invariants(m, first, ul)
    return first, exp


def check_invariants(m, t, ul, first_read=0, max_reads=0):
    """include/mdbg_hip.h: against graph_read_paths and graph_junctions of the same range on the same context"""
    rp, jx = m.graph_read_paths(first_read, max_reads), m.graph_junctions(first_read, max_reads)
    assert int(t["passes"].sum()) == t["n_passes"] == int(t["count"].sum()) and (t["n_crossings"], t["n_explained"]) == (jx["n_crossings"], jx["n_explained"])
    linear = ul["circular"] == 0
    assert np.all(t["passes"][linear] <= rp["support_steps"][linear])
    off = ul["offsets"].astype(np.int64)
    m_of = off[1:] - off[:-1]
    u = t["unitig"]
    # a pair that is its own mirror — (u, 0, 1) -> (u, 0, 0) coming in, (u, m - 1, 0) -> (u, m - 1, 1) going out — may serve a key twice
    twice_in = 1 + ((t["in_unitig"] == u) & (t["in_entry"] == 0) & (t["in_strand"] == 1))
    twice_out = 1 + ((t["out_unitig"] == u) & (t["out_entry"] == m_of[u] - 1) & (t["out_strand"] == 1))
    assert np.all(t["count"] <= np.minimum(jx["support"][t["in_record"]] * twice_in, jx["support"][t["out_record"]] * twice_out))


# ---- the hand-built repeats -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TG.CASE_IDS)
def test_hand_built_repeats(name):
    R = _mdbg()
    c = TG.BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        if c.steps is not None:
            ul = m.graph_simplify(c.steps)
        got, exp = check(R, m, hashes(c.reads), c.k, nodes, ul)
        e = c.expect
        assert (got["n_transits"], got["n_passes"], sorted(got["count"].tolist()), got["n_repeats"]) == (e["transits"], e["passes"], e["counts"], e["repeats"])
        for ms, n_resolved in e["resolved"].items():
            assert m.graph_transits(0, 0, ms)["n_resolved"] == n_resolved, ms
        assert (m.graph_junctions()["n_missing"] > 0) == bool(e.get("missing"))
        if "walks" in e:
            assert sorted((ul["offsets"][1:] - ul["offsets"][:-1]).tolist()) == e["walks"]
        if name == "long":                                                          # the two crossings of each transit lie in different workgroups and scan blocks
            assert int((ul["offsets"][1:] - ul["offsets"][:-1]).max()) > 4096


def test_more_keys_than_a_block_of_the_sort_holds():
    R = _mdbg()
    reads = TG.many_crosses(1100)
    m, nodes, ul = built(R, reads, 3, 1, split=700)
    with m:
        got, exp = check(R, m, hashes(reads), 3, nodes, ul)
        assert got["n_transits"] == 2200 > 2048 and got["count"].tolist() == [1] * 2200 and (got["n_repeats"], got["n_resolved"]) == (1100, 1100)
        assert m.graph_transits(0, 0, 2)["n_resolved"] == 0


# ---- the catalogue of sketch_graphs and the random graphs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_catalogue_on_the_plain_and_on_every_simplified_list(name):
    R = _mdbg()
    c = BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimps[0])
    H = hashes(c.reads)
    with m:
        got, _ = check(R, m, H, c.k, nodes, ul)
        if name == TG.SELF_CASE:
            assert got["verdict"].tolist() == [R.api.TRANSIT_SELF]
        same_list(m.graph_unitigs(), ul, R)                                         # the call left the list as it was
        for steps in c.schedules:
            simp = m.graph_simplify(steps)                                          # the simplified list is now the current one
            check(R, m, H, c.k, nodes, simp)
            same_list(m.graph_simplify(steps), simp, R)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_minimizer_space_graphs(seed):
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        got, exp = check(R, m, hashes(reads), k, nodes, ul)
        if seed in RANDOM:
            tally = np.bincount(got["verdict"], minlength=4).tolist()
            assert (got["n_transits"], got["n_passes"], tuple(tally)) == RANDOM[seed]
        if seed == 0:
            assert set(got["verdict"].tolist()) == {R.api.TRANSIT_SELF} and got["n_repeats"] == ul["n_unitigs"]
        if presimp > 0 and m.graph_junctions()["n_missing"]:                        # chains through a missing crossing: the restatement breaks them, so does the device
            assert got["n_explained"] < got["n_crossings"]


def test_a_list_after_an_edge_step_on_a_random_graph():
    """seed 6 built at presimp 0.5 has missing crossings already; an EDGES step on it leaves a list on which reads cross removed records"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(6)
    m, nodes, ul = built(R, reads, k, A, 40, presimp)
    with m:
        assert m.graph_junctions()["n_missing"] > 0
        simp = m.graph_simplify([(EDGES, 1, 0)])
        check(R, m, hashes(reads), k, nodes, simp)
        assert m.graph_junctions()["n_missing"] > 0


# ---- ranges -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,min_support", [(1, 1), (4, 2)])
def test_ranges_merge_into_the_whole_call(seed, min_support):
    """the reads fed as two batches cut in front of read 50: partitions into single reads, into chunks of 7, and at a cut off the batch bounds"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    n, cut = len(reads), 50
    H = hashes(reads)
    m, nodes, ul = built(R, reads, k, A, split=cut, presimp=presimp)
    with m:
        whole = m.graph_transits(0, 0, min_support)
        assert_same(whole, as_library_result(expected(H, k, nodes, ul, min_support), n))
        self_flags = R.api.transit_self_flags(ul["edges"], ul["n_unitigs"])
        for bounds in ([(a, a + 1) for a in range(n)], [(a, min(a + 7, n)) for a in range(0, n, 7)], [(0, 33), (33, cut), (cut, 77), (77, n)]):
            parts = [m.graph_transits(a, b - a, min_support) for a, b in bounds]
            for (a, b), got in list(zip(bounds, parts))[:12]:
                assert_same(got, as_library_result(expected(H[a:b], k, nodes, ul, min_support), b - a, a))
            merged = R.api.merge_transits(parts)
            for f in merged:
                assert np.array_equal(merged[f], whole[f]) and np.asarray(merged[f]).dtype == np.asarray(whole[f]).dtype, f
            verdict = R.api.transit_verdicts(merged["n_in"], merged["n_out"], self_flags, merged, min_support)
            assert np.array_equal(verdict, whole["verdict"]) and verdict.dtype == np.uint8
            assert_same(R.api.merge_transits(parts, self_flags, min_support), whole)
        check_invariants(m, m.graph_transits(33, 44, min_support), ul, 33, 44)
        assert_zeros(R, m.graph_transits(n, 0, min_support), n)
        assert_zeros(R, m.graph_transits(n + 1, 3, min_support), n + 1)
        assert_same(m.graph_transits(0, 1000, min_support), whole)


# ---- other results a caller may hold ----------------------------------------------------------------------------------------------------------------------------
GOLDEN_PARAMS = (3, 10, 0.002, 1)              # tests/golden/reads-0.00.fa.gz at k = 3: a list with records (k = 7 gives one unitig and no record)


def golden_hashes(example_reads):
    b, o = O.concat_reads(example_reads)
    sk = O.sketch(b, o, GOLDEN_PARAMS[1], GOLDEN_PARAMS[2])
    off = sk["off"].tolist()
    return b, o, [sk["hashes"][x:y].tolist() for x, y in zip(off, off[1:])]


def test_held_results_are_untouched_and_a_held_transit_result_survives(example_reads):
    """base-space reads kept on the device, so that a contig result can be held too"""
    R = _mdbg()
    k, l, d, A = GOLDEN_PARAMS
    b, o, H = golden_hashes(example_reads)
    C = R.api.C
    with R.Mdbg(k, l, d, A, keep_reads=True) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        m.graph_edges(0.01)
        ul = m.graph_unitigs()
        rp, jx, cl, cs = m.graph_read_paths_device(), m.graph_junctions_device(), m.graph_components_device(), m.graph_contigs(0, device=True)
        n = dict(read=int(rp.n_reads), step=int(rp.n_steps), unitig=int(rp.n_unitigs), record=int(jx.n_records), missing=int(jx.n_missing))
        held = [(getattr(rp, f), n[per], t) for f, t, per in R.api.READ_PATH_FIELDS] + [(rp.step_offsets, n["read"] + 1, np.uint64)]
        held += [(getattr(jx, f), n[per], t) for f, t, per in R.api.JUNCTION_FIELDS]
        held += [(getattr(cl, f), int(cl.n_unitigs if per_unitig else cl.n_components), t) for f, t, per_unitig in R.api.COMPONENT_FIELDS]
        held += [(cs.bases, int(cs.n_bases), np.uint8), (cs.offsets, int(cs.n_contigs) + 1, np.uint64), (cs.unitig, int(cs.n_contigs), np.uint64)]
        copy_back = lambda what: [m.to_host(C.cast(p, C.c_void_p).value, cnt * np.dtype(t).itemsize, t) for p, cnt, t in what if cnt]
        before = copy_back(held)
        assert n["step"] > 0 and n["record"] > 0 and int(cl.n_components) > 0 and int(cs.n_bases) > 0
        got, exp = check(R, m, H, k, nodes, ul, invariants=False)                   # nine transit calls and no other
        assert got["n_transits"] > 0 and got["n_repeats"] > 0
        assert all(np.array_equal(x, y) for x, y in zip(before, copy_back(held)))
        same_list(m.graph_unitigs(), ul, R)
        # a held transit result: a junction call and a simplify call with an EDGES step (which uses the junction buffers) leave it alone
        dev = m.graph_transits_device(0, 0, 2)
        mine = [(getattr(dev, f), int(dev.n_transits if per == "transit" else dev.n_unitigs), t) for f, t, per in R.api.TRANSIT_FIELDS]
        before = copy_back(mine)
        m.graph_junctions()
        m.graph_read_paths()
        assert m.graph_simplify([(EDGES, 1, 0)])["stats"]["edges_removed"][0] > 0
        m.graph_junctions()
        after = copy_back(mine)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        want = as_library_result(T.at_min_support(exp, 2), len(H))
        assert int(dev.n_transits) > 0 and all(np.array_equal(x, want[f]) for x, (f, _, _) in zip(after, R.api.TRANSIT_FIELDS))


# ---- state and parameters -----------------------------------------------------------------------------------------------------------------------------------------
def refused(m, code, *a):
    with pytest.raises(_mdbg().MdbgError) as e:
        m.graph_transits(*a)
    assert e.value.code == code
    return str(e.value)


def test_state_and_parameter_errors_leave_the_context_usable():
    R = _mdbg()
    c = TG.BY_NAME["mixed"]
    H = hashes(c.reads)
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        assert "no current unitig list" in refused(m, E_STATE)                      # nothing yet
        feed(m, c.reads[:5])
        nodes = m.finalize()
        assert "no current unitig list" in refused(m, E_STATE)                      # a node table, no list
        m.graph_edges(0.0)
        assert "no current unitig list" in refused(m, E_STATE)                      # after graph_edges
        ul = m.graph_unitigs()
        check(R, m, H[:5], c.k, nodes, ul)
        assert "min_support" in refused(m, E_PARAM, 0, 0, 0)                        # min_support 0; the list stays current
        check(R, m, H[:5], c.k, nodes, ul, invariants=False)
        keep = feed_batches(m, [(c.reads[5:], 5)])                                  # an ingest (and the insertion) ends the list
        refused(m, E_STATE)
        nodes = m.finalize()
        refused(m, E_STATE)                                                         # a finalize without a new unitig call
        m.graph_edges(0.0)
        refused(m, E_STATE)                                                         # an edge call
        ul = m.graph_unitigs()
        got, _ = check(R, m, H, c.k, nodes, ul)
        assert (got["n_transits"], got["n_passes"]) == (3, 7)
        m.graph_edges(0.0)                                                          # an edge call ends the list again
        refused(m, E_STATE)
        del keep
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        m.set_partition(2, 0)
        assert "single-GPU" in refused(m, E_STATE)
        m.set_partition(1, 0)                                                       # the same context, unpartitioned again: it works
        feed(m, c.reads)
        nodes = m.finalize()
        m.graph_edges(0.0)
        check(R, m, H, c.k, nodes, m.graph_unitigs())
        assert m.L.mdbg_graph_transits(m.h, 0, 0, 1, None) == m.L.mdbg_graph_transits(None, 0, 0, 1, None) == E_PARAM      # a null pointer
        assert m.L.mdbg_graph_transits_device(m.h, 0, 0, 1, None) == E_PARAM and m.L.mdbg_transits_ms(m.h, None) == E_PARAM
        tl = R.api.TransitList()
        assert m.L.mdbg_graph_transits(m.h, 0, 0, 0, R.api.C.byref(tl)) == m.L.mdbg_graph_transits_device(m.h, 0, 0, 0, R.api.C.byref(tl)) == E_PARAM
    with R.Mdbg(3, G.L, G.D, 1) as m:                                               # an empty context: MDBG_OK and zeros
        m.finalize()
        m.graph_edges(0.0)
        m.graph_unitigs()
        assert_zeros(R, m.graph_transits())
        assert_zeros(R, m.graph_transits(5, 2, 3), 5)
        assert m.transits_ms() == 0.0
        refused(m, E_PARAM, 0, 0, 0)


# ---- pipeline and the C program ------------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_files_and_the_c_program(example_reads, tmp_path):
    """tests/golden/reads-0.00.fa.gz at k = 3: both files of run_file hold the restatement's text, and the C program writes the same bytes"""
    from rust_mdbg_amd import pipeline
    R = _mdbg()
    k, l, d, A = GOLDEN_PARAMS
    steps = [(EDGES, 1, 0)]
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    prefix = str(tmp_path / "tx")
    out = pipeline.run_file(src, prefix, k, l, d, A, write_sequences=False, contigs=True, keep_reads=True, simplify=steps, transits=1, batch_bases=5_000_000)
    b, o, H = golden_hashes(example_reads)
    with R.Mdbg(k, l, d, A) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        m.graph_edges(0.01)
        ul = m.graph_unitigs()
        plain = expected(H, k, nodes, ul)
        sl = m.graph_simplify(steps)
        simplified = expected(H, k, nodes, sl)
    text, stext = open(prefix + ".unitigs.transits.tsv").read(), open(prefix + ".msimpl.transits.tsv").read()
    assert text == T.tsv_text(plain, ul["circular"]) and stext == T.tsv_text(simplified, sl["circular"])
    assert plain["n_transits"] > 0 and plain["n_repeats"] > 0 and text != stext
    for suffix, t in (("", plain), ("_simplified", simplified)):
        assert tuple(out[f + suffix] for f in ("n_transits", "n_passes", "n_repeats", "n_resolved")) == (t["n_transits"], t["n_passes"], t["n_repeats"], t["n_resolved"])
    assert text == R.api.transit_text(as_library_result(plain, len(H)), ul["circular"])
    exe = str(tmp_path / "mdbg_cli")
    libdir = os.path.join(ROOT, "rust_mdbg_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mdbg_cli.c"),
                    "-L" + libdir, "-lmdbg_hip", "-lmdbg_emit", "-lpthread", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    cpre = str(tmp_path / "c")
    r = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--prefix", cpre, "--no-basespace", "-e", "1", "--transits", "1"],
                       check=True, capture_output=True, text=True)
    for ext in (".unitigs.transits.tsv", ".msimpl.transits.tsv"):
        assert open(cpre + ext, "rb").read() == open(prefix + ext, "rb").read(), ext
    lines = r.stdout.split("\n")
    for label, t in (("", plain), (" (simplified)", simplified)):
        assert "transits%s: %d keys, %d passes, %d repeats, %d of them resolved at min_support 1" % (label, t["n_transits"], t["n_passes"], t["n_repeats"], t["n_resolved"]) in lines
