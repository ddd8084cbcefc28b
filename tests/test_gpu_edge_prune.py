"""Edge pruning on the GPU (the MDBG_SIMPLIFY_EDGES step of Mdbg.graph_simplify, csrc/simplify.hip) against the plain restatement
(tests/edge_prune_restatement.py), array for array: walks, offsets, length, kc_sum, circular, the edge columns and the per-step counts — on the hand cases,
the catalogue of tests/sketch_graphs.py, the random graphs alone and mixed with tip and bubble steps, and the contracts round the step: schedules without it,
the junction support of the pruned list, the other stages on the result, the refusals, a held result, the pipeline's files and the C program's.
CPU side: tests/test_edge_prune_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import edge_prune_restatement as EP
import read_paths_restatement as RP
import sketch_graphs as G
import unitig_restatement as U
from conftest import GOLDEN
from oracle import oracle as O
from test_edge_prune_cpu import CATALOGUE_REMOVED, HAND, HAND_A, HAND_K, MIXED, RANDOM, hand_reads
from test_gpu_components import check_components
from test_gpu_parity import _mdbg
from test_gpu_read_paths import built, feed_batches
from test_gpu_simplify import same_list
from test_gpu_sketch_graphs import BY_NAME, feed
from test_gpu_unitigs import build_cli
from test_read_paths_cpu import hashes

pytestmark = pytest.mark.gpu

EDGES, TIPS, BUBBLES = EP.EDGES, EP.TIPS, EP.BUBBLES
E_PARAM, E_STATE = -1, -6


def assert_equals_checker(got, log, exp, nodes, strings):
    """got: Mdbg.graph_simplify(steps); (log, exp): edge_prune_restatement.simplify of the same steps"""
    st = got["stats"]
    print("removed per step (unitigs, nodes, edge records):", list(zip(st["unitigs_removed"], st["nodes_removed"], st["edges_removed"])), "compactions", st["n_compactions"],
          "syncs", st["n_syncs"])
    assert st["unitigs_removed"] == [len(x["unitigs"]) for x in log] and st["nodes_removed"] == [len(x["nodes"]) for x in log]
    assert st["edges_removed"] == [x["edges"] for x in log]
    assert (st["total_unitigs_removed"], st["total_nodes_removed"], st["total_edges_removed"]) == (sum(st["unitigs_removed"]), sum(st["nodes_removed"]), sum(st["edges_removed"]))
    off = got["offsets"].tolist()
    walks = [list(zip(got["node"][a:b].tolist(), (chr(c) for c in got["ori"][a:b]))) for a, b in zip(off, off[1:])]
    assert walks == exp["walks"]
    assert off == np.cumsum([0] + [len(w) for w in exp["walks"]]).tolist()
    assert got["circular"].astype(bool).tolist() == exp["circular"] and got["kc_sum"].tolist() == exp["kc_sum"] and got["length"].tolist() == exp["length"]
    assert got["n_unitigs"] == len(walks) and got["n_entries"] == len(nodes["index"]) - st["total_nodes_removed"] == off[-1]
    e = got["edges"]
    rows = list(zip(e["n1"].tolist(), (chr(c) for c in e["o1"]), e["n2"].tolist(), (chr(c) for c in e["o2"]), e["overlap"].tolist()))
    assert rows == exp["edges"]                                                     # unitig edges in source order, overlaps fixed
    if strings is not None:
        from rust_mdbg_amd import emit as E
        with E.Contigs(got) as c:                                                   # the copy plan executed
            c.add_batch(*O.concat_reads(strings), 0)
            assert [s.decode("latin-1") for s in c.sequences()] == exp["seqs"]


def check(R, m, nodes, edges, reads, k, steps, strings, length_of=None):
    """the schedule on the context, twice, against the checker -> (got, log, exp)"""
    got = m.graph_simplify(steps)
    again = m.graph_simplify(steps)
    assert got["stats"] == again["stats"]
    same_list(got, again, R)                                                        # two identical calls give identical arrays
    log, exp = EP.simplify(nodes, edges, steps, hashes(reads), k, strings, length_of)
    assert_equals_checker(got, log, exp, nodes, strings)
    return got, log, exp


# ---- the hand cases, the catalogue, the random graphs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", sorted(HAND))
def test_hand_cases(name, T):
    R = _mdbg()
    reads = hand_reads()[name]
    weak, removed, left = HAND[(name, T)]
    m, nodes, ul = built(R, reads, HAND_K, HAND_A)
    with m:
        edges = m.graph_edges(0.0)
        got, log, _ = check(R, m, nodes, edges, reads, HAND_K, [(EDGES, T, 0)], G.fake_bases(reads, G.L, 1))
        assert (got["stats"]["edges_removed"], np.diff(got["offsets"].astype(np.int64)).tolist()) == ([removed], left) and log[0]["weak"] == weak
        assert got["stats"]["n_compactions"] == (2 if removed else 1)                # a compaction follows iff the step removed a record
        same_list(m.graph_unitigs(), ul, R)                                         # the plain list is what it was


@pytest.mark.parametrize("name", G.CASE_IDS)
def test_catalogue_at_min_support_one(name):
    R = _mdbg()
    c = BY_NAME[name]
    strings = G.fake_bases(c.reads, G.L, 1) if c.strings else None
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimps[0])
    with m:
        edges = m.graph_edges(c.presimps[0])
        got, log, exp = check(R, m, nodes, edges, c.reads, c.k, [(EDGES, 1, 0)], strings, None if strings is not None else G.length_of_walk(nodes))
        assert got["stats"]["edges_removed"] == [CATALOGUE_REMOVED.get(name, 0)]
        if strings is not None:
            check_components(R, m, exp)                                             # the pruned list is the current one


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_graphs_at_three_thresholds(seed):
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    strings = G.fake_bases(reads, G.L, seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        edges = m.graph_edges(presimp)
        for T, (weak, removed, left) in zip((1, 2, 3), RANDOM[seed][1]):
            got, log, _ = check(R, m, nodes, edges, reads, k, [(EDGES, T, 0)], strings)
            assert (log[0]["weak"], got["stats"]["edges_removed"], got["n_unitigs"]) == (weak, [removed], left)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_tips_and_bubbles_decide_on_a_graph_with_dead_arcs(seed):
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        check(R, m, nodes, m.graph_edges(presimp), reads, k, MIXED, G.fake_bases(reads, G.L, seed))


# ---- a schedule without the step is untouched by it ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 4])
def test_a_schedule_without_an_edge_step_is_what_it_was(seed):
    """the same context before and after calls with EDGES steps: the masks of one call do not reach the next"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    m, nodes, ul = built(R, reads, k, A, 40, presimp)
    with m:
        schedules = ([], [(TIPS, 3, 0), (BUBBLES, 0, 0), (TIPS, 0, 0)], R.api.MAGIC_SIMPLIFY_STEPS)
        before = [m.graph_simplify(s) for s in schedules]
        assert all(b["stats"]["edges_removed"] == [0] * len(s) and b["stats"]["total_edges_removed"] == 0 for b, s in zip(before, schedules))
        same_list(before[0], ul, R)
        pruned = m.graph_simplify(MIXED)
        assert pruned["stats"]["total_edges_removed"] > 0
        for s, b in zip(schedules, before):
            after = m.graph_simplify(s)
            same_list(after, b, R)
            assert after["stats"] == b["stats"]
            m.graph_simplify([(EDGES, 1, 0)])
        same_list(m.graph_unitigs(), ul, R)


# ---- the junction support of the pruned list -----------------------------------------------------------------------------------------------------------------------
def vertex(walks, u, j, s):
    v = walks[u][j]
    return U.comp(v) if s else v


def arc_key(x, y):
    return frozenset([(x, y), (U.comp(y), U.comp(x))])


@pytest.mark.parametrize("which", ["repeat + span", 0, 7])
def test_junctions_of_the_pruned_list(which):
    """presimp 0: every crossing of the plain list lies on a record.  After the step at min_support 3 no pruned record remains, and every crossing a pruned record
    had — at node level, the lists number their unitigs differently — is now a missing crossing with its old count, and nothing else is missing.  In the hand
    case the two spanning reads cross records that go at min_support 3: two crossings on one key"""
    R = _mdbg()
    k, A, presimp, reads = (HAND_K, HAND_A, 0.0, hand_reads()[which]) if isinstance(which, str) else G.random_case(which)
    assert presimp == 0.0
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        walks0, _ = RP.walks_of(ul)
        e = ul["edges"]
        recs0 = list(zip(e["n1"].tolist(), [chr(o) for o in e["o1"]], e["n2"].tolist(), [chr(o) for o in e["o2"]]))
        jx0 = m.graph_junctions()
        assert jx0["n_missing"] == 0
        sup0 = {}
        for r, s in zip(recs0, jx0["support"].tolist()):
            assert sup0.setdefault(arc_key(*EP.arc_of(r, walks0)), s) == s
        got = m.graph_simplify([(EDGES, 3, 0)])
        walks1, _ = RP.walks_of(got)
        e = got["edges"]
        left = {arc_key(*EP.arc_of(r, walks1)) for r in zip(e["n1"].tolist(), [chr(o) for o in e["o1"]], e["n2"].tolist(), [chr(o) for o in e["o2"]])}
        interior = {arc_key(a, b) for w, c in zip(walks1, got["circular"].tolist()) for a, b in zip(w, w[1:])}
        pruned = {key: s for key, s in sup0.items() if key not in left and key not in interior}
        assert sum(arc_key(*EP.arc_of(r, walks0)) in pruned for r in recs0) == got["stats"]["edges_removed"][0] and all(s < 3 for s in pruned.values())
        if isinstance(which, str):
            assert sorted(pruned.values()) == [0, 2]
        jx1 = m.graph_junctions()
        missing = {}
        for u1, j1, s1, u2, j2, s2, n in zip(*(jx1[f].tolist() for f in R.api.MISSING_COLUMNS)):
            key = arc_key(vertex(walks1, u1, j1, s1), vertex(walks1, u2, j2, s2))
            assert key not in missing
            missing[key] = n
        assert missing == {key: s for key, s in pruned.items() if s > 0}
        assert jx1["n_explained"] + jx1["n_missing_crossings"] == jx1["n_crossings"] and jx1["n_missing_crossings"] == sum(missing.values())
        assert jx1["n_records"] == len(e["n1"]) and jx1["n_adjacent"] == jx0["n_adjacent"]


# ---- contigs and components on the result (base-space reads, kept on the device) ------------------------------------------------------------------------------------
GOLDEN_PARAMS = (3, 10, 0.002, 1)              # tests/golden/reads-0.00.fa.gz at k = 3: a list with records (k = 7 gives one unitig and no record)


def golden_expected(R, example_reads, steps, presimp=0.01):
    k, l, d, A = GOLDEN_PARAMS
    b, o = O.concat_reads(example_reads)
    sk = O.sketch(b, o, l, d)
    off = sk["off"].tolist()
    H = [sk["hashes"][x:y].tolist() for x, y in zip(off, off[1:])]
    with R.Mdbg(k, l, d, A) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        edges = m.graph_edges(presimp)
    return EP.simplify(nodes, edges, steps, H, k, example_reads)


def test_contigs_and_components_run_on_the_result(example_reads):
    R = _mdbg()
    k, l, d, A = GOLDEN_PARAMS
    steps = [(EDGES, 1, 0)]
    log, exp = golden_expected(R, example_reads, steps)
    b, o = O.concat_reads(example_reads)
    with R.Mdbg(k, l, d, A, keep_reads=True) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        m.graph_edges(0.01)
        got = m.graph_simplify(steps)
        assert_equals_checker(got, log, exp, nodes, example_reads)
        assert got["stats"]["edges_removed"][0] > 0
        ctg = m.graph_contigs(0)
        offs = ctg["offsets"].tolist()
        assert [bytes(ctg["bases"][x:y]).decode("latin-1") for x, y in zip(offs, offs[1:])] == exp["seqs"]
        check_components(R, m, exp)


# ---- refusals; a held result ---------------------------------------------------------------------------------------------------------------------------------------
def refused(m, steps, code):
    with pytest.raises(_mdbg().MdbgError) as e:
        m.graph_simplify(steps)
    assert e.value.code == code
    return str(e.value)


def test_parameter_and_state_errors_leave_the_context_usable():
    R = _mdbg()
    reads = hand_reads()["repeat"]
    good = [(EDGES, 1, 0)]
    m, nodes, ul = built(R, reads, HAND_K, HAND_A)
    with m:
        refused(m, [(EDGES, 0, 0)], E_PARAM)                                        # min_support 0
        refused(m, [(TIPS, 0, 0), (EDGES, 1, 5)], E_PARAM)                          # max_bases is reserved
        assert m.graph_simplify(good)["stats"]["edges_removed"] == [4]
        keep = feed_batches(m, [(reads[:2], len(reads))])                           # an ingest: the node table, the edge list and the unitig list are gone
        assert "no current edge list" in refused(m, good, E_STATE)
        nodes = m.finalize()
        refused(m, good, E_STATE)                                                   # a finalize without a new edge call
        m.graph_edges(0.0)
        assert m.graph_simplify(good)["stats"]["edges_removed"] == [4]              # (eight reads now: the supports are 5, 0, 3, ...)
        del keep
    with R.Mdbg(HAND_K, G.L, G.D, HAND_A) as m:
        m.set_partition(2, 0)
        assert "single-GPU" in refused(m, good, E_STATE)
        m.set_partition(1, 0)                                                       # the same context, unpartitioned again: it works
        feed(m, reads)
        m.finalize()
        m.graph_edges(0.0)
        assert m.graph_simplify(good)["stats"]["edges_removed"] == [4]
    with R.Mdbg(HAND_K, G.L, G.D, HAND_A) as m:                                      # an empty context: the empty list, no error
        got = m.graph_simplify(good)
        assert got["n_unitigs"] == 0 and got["stats"]["edges_removed"] == [0]
        assert m.L.mdbg_simplify_edges_removed(None, None, None) == E_PARAM and m.L.mdbg_simplify_edges_removed(m.h, None, None) == 0


def test_a_held_read_path_result_is_unchanged_and_a_junction_result_ends():
    R = _mdbg()
    k, A, presimp, reads = G.random_case(6)
    m, nodes, ul = built(R, reads, k, A, 40, presimp)
    with m:
        rp = m.graph_read_paths_device()
        n = dict(read=int(rp.n_reads), step=int(rp.n_steps), unitig=int(rp.n_unitigs))
        held = [(getattr(rp, f), n[per], t) for f, t, per in R.api.READ_PATH_FIELDS] + [(rp.step_offsets, n["read"] + 1, np.uint64)]
        copy_back = lambda: [m.to_host(R.api.C.cast(p, R.api.C.c_void_p).value, cnt * np.dtype(t).itemsize, t) for p, cnt, t in held]
        before = copy_back()
        assert n["step"] > 0
        jx = m.graph_junctions()
        got = m.graph_simplify(MIXED)
        assert got["stats"]["total_edges_removed"] > 0
        assert all(np.array_equal(a, b) for a, b in zip(before, copy_back()))
        m.graph_unitigs()
        again = m.graph_junctions()                                                 # the step used the junction buffers: a new call gives the plain list's result again
        assert all(np.array_equal(jx[f], again[f]) for f in jx)


# ---- the pipeline and the C program ---------------------------------------------------------------------------------------------------------------------------------
def test_run_file_and_cli_write_the_pruned_contigs(example_reads, tmp_path):
    from rust_mdbg_amd import pipeline
    R = _mdbg()
    k, l, d, A = GOLDEN_PARAMS
    steps = [(EDGES, 1, 0)]
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    pre = str(tmp_path / "p")
    res = pipeline.run_file(src, pre, k, l, d, A, contigs=True, simplify=steps)
    log, exp = golden_expected(R, example_reads, steps)
    assert open(pre + ".msimpl.gfa").read() == U.gfa_text(exp) and open(pre + ".msimpl.fa").read() == U.fasta_text(exp)
    assert res["simplify"]["edges_removed"] == [log[0]["edges"]] and res["simplify"]["total_edges_removed"] == log[0]["edges"] > 0 and res["n_simplified"] == len(exp["walks"])
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "c")
    out = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "-e", "1", "--prefix", cpre], check=True, capture_output=True,
                         text=True).stdout
    assert "simplify step 1 (edges 1): %d edge records removed\n" % log[0]["edges"] in out and "simplify: %d edge records removed\n" % log[0]["edges"] in out
    for ext in (".msimpl.gfa", ".msimpl.fa", ".unitigs.gfa"):
        assert open(pre + ext, "rb").read() == open(cpre + ext, "rb").read(), ext
    one = str(tmp_path / "k7")                                                      # k = 7: one unitig, no record, nothing to prune
    r7 = pipeline.run_file(src, one, 7, 10, 0.0008, 2, contigs=True, simplify=steps)
    assert r7["simplify"]["edges_removed"] == [0] and r7["n_simplified"] == r7["n_unitigs"] == 1
    assert open(one + ".msimpl.gfa", "rb").read() == open(one + ".unitigs.gfa", "rb").read()
