"""MDBG_GUARD (include/mdbg_hip.h, csrc/blocks.inc): every device block exactly as large as the stage asked for, between two bands of 4096 bytes that nobody may
write.  Each test starts one fresh process with the hook set; the child runs the guard's self-test first, then calls test functions of the other modules as they
are — every comparison they make against the oracle, the host emitter and the restatements stays in force — while rust_mdbg_amd.api compares all bands after
every library call.  A child ends with `GUARD_OK calls=<n> blocks=<m> bytes=<b>`: a run that checked nothing does not pass.  One child per subject, each with
the smallest shapes that still reach every kernel of its subject (times: profiles/guard_notes.md).  Writes only: a read outside a block leaves no trace."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, read_fasta_gz

pytestmark = pytest.mark.gpu

GUARD_LINE = re.compile(r"^GUARD_OK calls=(\d+) blocks=(\d+) bytes=(\d+)$", re.M)


# ---- the parent's side ------------------------------------------------------------------------------------------------------------------------------------------
def run_child(name, env, timeout=600):
    """python -c '... child_main(name)' in a fresh process with `env` on top of the environment, neither hook inherited"""
    base = {k: v for k, v in os.environ.items() if k not in ("MDBG_GUARD", "MDBG_POISON")}
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_guard as T; T.child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), name)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(base, **env), timeout=timeout)
    print(r.stdout[-2500:])
    return r


def guarded(name):
    """the child `name` under MDBG_GUARD=1: it ended well, ran the self-test first and checked something after its calls -> its output"""
    r = run_child(name, {"MDBG_GUARD": "1"})
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = GUARD_LINE.search(r.stdout)
    assert got is not None and r.stdout.startswith("SELFTEST_OK\n"), (r.stdout[-1500:], r.stderr[-3000:])
    calls, blocks, nbytes = (int(x) for x in got.groups())
    assert calls > 0 and blocks > 0 and nbytes > 0, got.group(0)
    return r.stdout


def small_ingest_stats(R):
    """what the guarded and the unguarded child both report: the counters of one small context (no times)"""
    from oracle import oracle as O
    import test_gpu_parity as P
    reads = P.rand_reads(3, 20, 200, 3000) * 2                                     # every read twice: its k-min-mers reach min_abundance 2
    with R.Mdbg(5, 10, 0.02, 2) as m:
        m.ingest(*O.concat_reads(reads), 0)
        n = m.finalize()["n_nodes"]
        st = m.stats()
    return dict({f: int(v) for f, v in st.items() if not f.startswith("ms_")}, n_nodes=int(n))


def test_selftest_and_the_hook_unset():
    out = guarded("selftest")
    on = json.loads(re.search(r"^STATS (.*)$", out, re.M).group(1))
    r = run_child("unset", {})
    assert r.returncode == 0 and "UNSET_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    off = json.loads(re.search(r"^STATS (.*)$", r.stdout, re.M).group(1))
    assert on == off and on["n_nodes"] > 0 and on["n_minimizers"] > 0


@pytest.mark.parametrize("name", ["sketch_table", "input_formats", "nodes_to_simplify", "components_everything_removed", "read_paths_catalogue", "junctions_catalogue",
                                  "transits_catalogue_first_half", "transits_catalogue_second_half", "transits_hand_built_repeats", "edge_prune_catalogue", "read_evidence_shapes", "kept_contigs_fuzz",
                                  "kept_contigs_other", "kept_node_seqs_whole", "kept_node_seqs_chunks"])
def test_guarded_subject(name):
    guarded(name)


def test_one_context_large_small_large_under_guard():
    out = guarded("one_context")
    assert "ONE_CONTEXT_OK" in out


def test_one_context_large_small_large_under_poison():
    """the product allocator with the cache on — the path users run — handing out 0xA5 instead of whatever the block held"""
    r = run_child("one_context", {"MDBG_POISON": "1"})
    assert r.returncode == 0 and "ONE_CONTEXT_OK" in r.stdout and "GUARD_OK" not in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- the children -----------------------------------------------------------------------------------------------------------------------------------------------
def child_main(name):
    import time
    import rust_mdbg_amd as R
    from rust_mdbg_amd import api
    L = api.load_library()
    t0 = time.time()
    if name == "unset":
        return child_unset(R, api, L)
    if api.GUARD:
        assert L.mdbg_guard_selftest() == 0
        print("SELFTEST_OK", flush=True)
    CHILDREN[name](R)
    if api.GUARD:
        api.guard_check()
        print("GUARD_OK calls=%d blocks=%d bytes=%d" % (api.GUARD_SEEN["calls"], api.GUARD_SEEN["blocks"], api.GUARD_SEEN["bytes"]))
    print("CHILD_SECONDS %s %.1f" % (name, time.time() - t0))


def child_selftest(R):
    from rust_mdbg_amd import api
    L = api.load_library()
    assert L.mdbg_guard_selftest() == 0                                            # twice: the first run left nothing behind
    assert L.mdbg_guard_check(None, None) == 0 and L.mdbg_guard_report() == b""
    print("STATS " + json.dumps(small_ingest_stats(R), sort_keys=True))


def child_unset(R, api, L):
    C = api.C
    assert not api.GUARD and api.GUARD_SEEN["calls"] == 0
    nb, by = C.c_uint64(7), C.c_uint64(7)
    st = small_ingest_stats(R)
    with R.Mdbg(5, 10, 0.02, 2) as m:                                              # live blocks, and the check still looks at none
        m.ingest_reads([b"ACGTTGCA" * 40], 0)
        assert L.mdbg_guard_check(C.byref(nb), C.byref(by)) == 0 and (nb.value, by.value) == (0, 0)
    assert L.mdbg_guard_report() == b"" and L.mdbg_guard_selftest() == -1          # refused
    assert api.GUARD_SEEN["calls"] == 0
    print("STATS " + json.dumps(st, sort_keys=True))
    print("UNSET_OK")


def child_sketch_table(R):
    import numpy as np
    import test_gpu_fuzz as F
    from oracle import oracle as O
    for s in (70346, 70670, 3, 11):
        F.test_fuzz_sketch_and_nodes(s)
    for s in (0, 1):
        F.test_fuzz_long_reads_across_tiles(s)
    F.test_fuzz_multik_on_resident_sketches(0)
    with R.Mdbg(5, 10, 0.05, 1) as m:                                              # the empty-reads sequence of test_gpu_round4's poison test
        b, o = O.concat_reads([b"", b"", b""])
        sk = m.sketch(b, o)
        assert list(sk["off"]) == [0, 0, 0, 0], sk["off"]
        m.ingest_reads([b"ACGTTGCA" * 40], 0)
        m.ingest_reads([b"", b""], 1)
        m.ingest_reads([b"ACGTTGCA" * 40], 3)
        g = O.Graph(5, 10, 0.05, 1)
        bb, oo = O.concat_reads([b"ACGTTGCA" * 40, b"", b"", b"ACGTTGCA" * 40])
        assert g.ingest(bb, oo) == 0
        got, exp = m.finalize(), g.finalize(with_edges=False)
        assert got["n_nodes"] == exp["n_nodes"] and np.array_equal(got["keys"], exp["keys"]) and np.array_equal(got["abundance"], exp["abundance"])


def child_input_formats(R):
    import test_gpu_lmer
    import test_gpu_packed
    import test_gpu_syncmers
    test_gpu_packed.test_packed_with_n_exceptions_and_homopolymers_across_words()
    test_gpu_packed.test_pack_device_equals_host_packer_and_feeds_the_kernel()
    for l, s, d in ((5, 5, 1.0), (31, 13, 1.0), (12, 0, 0.3)):
        for hpc in (False, True):
            test_gpu_syncmers.test_gpu_syncmer_scan_edges(l, s, d, hpc)
    test_gpu_lmer.test_gpu_lmer_filter_corner_cases()


def child_nodes_to_simplify(R):
    import sketch_graphs as G
    import test_gpu_sketch_graphs as SG
    import test_gpu_unitigs as UT
    for name in G.CASE_IDS:
        SG.test_gpu_stages_on_hand_built_graphs(name)
    for seed in G.RANDOM_SEEDS:
        SG.test_gpu_stages_on_random_minimizer_space_graphs(seed)
    for kind in ("circular", "tandem", "inverted"):
        UT.test_gpu_unitigs_on_cycles_and_hairpins(0, kind)


def child_components_everything_removed(R):
    """test_gpu_components.test_a_step_may_remove_everything; its module fixture (many400) built as the fixture builds it"""
    import components_restatement as CR
    import test_gpu_components as TC
    import unitig_restatement as U
    reads = TC.many_genomes_case(0, 400)
    m, nodes, edges = TC.open_graph(R, reads, *TC.MANY_PARAMS, 0.0)
    m.close()
    cur = U.unitigs(nodes, edges, reads)
    TC.test_a_step_may_remove_everything((reads, nodes, edges, cur, CR.components(cur)))


def child_read_paths_catalogue(R):
    import sketch_graphs as G
    import test_gpu_read_paths as RP
    for name in G.CASE_IDS:
        RP.test_catalogue_on_the_plain_and_on_every_simplified_list(name)


def child_junctions_catalogue(R):
    import sketch_graphs as G
    import test_gpu_junctions as JX
    for name in G.CASE_IDS:
        JX.test_catalogue_on_the_plain_and_on_every_simplified_list(name)


def transits_catalogue(names):
    import test_gpu_transits as TX
    for name in names:
        TX.test_catalogue_on_the_plain_and_on_every_simplified_list(name)


def child_transits_catalogue_first_half(R):                                        # (three min_support values and the invariants per list: twice the calls of the other stages)
    import sketch_graphs as G
    transits_catalogue(G.CASE_IDS[:len(G.CASE_IDS) // 2])


def child_transits_catalogue_second_half(R):
    import sketch_graphs as G
    transits_catalogue(G.CASE_IDS[len(G.CASE_IDS) // 2:])


def child_transits_hand_built_repeats(R):
    import test_gpu_transits as TX
    import transit_graphs as TG
    for name in TG.CASE_IDS:
        TX.test_hand_built_repeats(name)


def child_edge_prune_catalogue(R):
    import sketch_graphs as G
    import test_edge_prune_cpu as EPC
    import test_gpu_edge_prune as EP
    for name in G.CASE_IDS:
        EP.test_catalogue_at_min_support_one(name)
    for name, T in sorted(EPC.HAND):
        EP.test_hand_cases(name, T)


def child_read_evidence_shapes(R):
    import test_gpu_junctions as JX
    import test_gpu_placement as PL
    import test_gpu_read_paths as RP
    import test_gpu_transits as TX
    PL.test_interleaved_stages_over_ranges_of_different_sizes()
    PL.test_a_list_without_records_after_a_list_with_records()
    JX.test_crossings_on_every_residue_of_the_index_modulo_256()
    RP.test_two_long_reads_cross_every_workgroup_span()
    TX.test_more_keys_than_a_block_of_the_sort_holds()


def contigs_cases(cases):
    import pathlib
    import tempfile
    import test_gpu_contigs_device as CD
    with tempfile.TemporaryDirectory() as tmp:                                     # the argument pytest would make of tmp_path
        for case in cases:
            d = pathlib.Path(tmp) / ("%s%d-%d-%g" % case)
            d.mkdir()
            CD.test_gpu_contigs_equal_the_host_path(case, d)


def child_kept_contigs_fuzz(R):
    import test_gpu_contigs_device as CD
    contigs_cases([c for c in CD.CASES if c[0] == "fuzz"])


def child_kept_contigs_other(R):
    import test_gpu_contigs_device as CD
    contigs_cases([c for c in CD.CASES if c[0] != "fuzz"])
    CD.test_exceptions_n_runs_inside_nodes_and_short_reads_of_arbitrary_bytes()


def child_kept_node_seqs_whole(R):
    import test_gpu_node_seqs as NS
    for case in NS.CASES:
        NS.test_whole_table_equals_the_host_rule(case)


def child_kept_node_seqs_chunks(R):
    import test_gpu_node_seqs as NS
    NS.test_chunks_concatenate_to_the_whole_and_respect_their_limits()
    for hpc in (False, True):
        NS.test_bytes_outside_acgt_inside_node_spans(hpc)


# ---- one context: a large graph, a small one behind it, the large one again ---------------------------------------------------------------------------------------
ONE_CONTEXT = (7, 10, 0.0008, 2)               # tests/golden/example_cfg1.json
TIPS_BUBBLES = [(1, 10, 50000), (2, 0, 100000)]


def every_stage(R, m, reads):
    """the reads ingested into m (kept), every stage run and checked by the helper its own test module uses -> every returned column, by name"""
    import numpy as np
    import test_gpu_components as TC
    import test_gpu_contigs_device as CD
    import test_gpu_edge_prune as EP
    import test_gpu_junctions as JX
    import test_gpu_node_seqs as NS
    import test_gpu_read_paths as RP
    import test_gpu_simplify as SX
    import test_gpu_transits as TX
    import test_gpu_unitigs as UT
    from oracle import oracle as O
    k, l, d, A = ONE_CONTEXT
    b, o = O.concat_reads(reads)
    sk = O.sketch(b, o, l, d)
    off = sk["off"].tolist()
    H = [sk["hashes"][x:y].tolist() for x, y in zip(off, off[1:])]
    mreads = [(tuple(h), ()) for h in H]                                           # the reads as the read-evidence restatements take them
    out = {}

    def evidence(tag, ul):
        out["components " + tag] = TC.check_components(R, m, ul_expected[tag])
        out["read_paths " + tag] = RP.check_paths(R, m, mreads, k, nodes, ul)[0]
        out["junctions " + tag] = JX.check(R, m, mreads, k, nodes, ul)[0]
        out["transits " + tag] = TX.check(R, m, H, k, nodes, ul)[0]
        g = m.graph_contigs(0)
        assert CD.split(g) == CD.host_contigs(ul, [(b, o, 0)])
        dv = m.graph_contigs(0, device=True)
        assert (int(dv.n_contigs), int(dv.n_bases)) == (g["n_contigs"], g["n_bases"])
        if g["n_bases"]:
            assert np.array_equal(m.to_host(R.api.C.cast(dv.bases, R.api.C.c_void_p).value, g["n_bases"]), g["bases"])
        assert np.array_equal(m.to_host(R.api.C.cast(dv.offsets, R.api.C.c_void_p).value, 8 * (g["n_contigs"] + 1), np.uint64), g["offsets"])
        out["contigs " + tag] = g

    ul_expected = {}
    nodes = out["nodes"] = m.finalize()
    edges = out["edges"] = m.graph_edges(0.01)
    plain = out["unitigs"] = m.graph_unitigs()
    ul_expected["plain"] = UT.assert_equals_restatement(plain, nodes, edges, reads)
    evidence("plain", plain)
    simp = out["tips and bubbles"] = m.graph_simplify(TIPS_BUBBLES)
    ul_expected["tips and bubbles"] = SX.assert_equals_restatement(simp, nodes, edges, reads, TIPS_BUBBLES)[1]
    evidence("tips and bubbles", simp)
    steps = [(R.api.MDBG_SIMPLIFY_EDGES, 1, 0), (1, 10, 50000)]
    pruned, _, ul_expected["edges and tips"] = EP.check(R, m, nodes, edges, mreads, k, steps, reads)
    out["edges and tips"] = pruned
    evidence("edges and tips", pruned)
    SX.same_list(m.graph_unitigs(), plain, R)                                      # the plain list is what it was
    g = out["node_seqs"] = m.graph_node_seqs(0, 0, 0)
    assert g["n_rows"] == nodes["n_nodes"] and NS.rows_of(g) == NS.checker(reads, nodes)
    dv = m.graph_node_seqs(0, 0, 0, device=True)
    assert (dv["n_rows"], dv["n_bases"]) == (g["n_rows"], g["n_bases"])
    if g["n_bases"]:
        assert np.array_equal(m.to_host(dv["bases"], dv["n_bases"]), g["bases"])
    assert np.array_equal(m.to_host(dv["offsets"], 8 * (dv["n_rows"] + 1), np.uint64), g["offsets"])
    return out


def columns(x, path=""):
    """every array and every scalar of a nested result, by its path"""
    import numpy as np
    if isinstance(x, dict):
        for f in sorted(x):
            yield from columns(x[f], path + "/" + str(f))
    elif isinstance(x, (list, tuple)):
        yield path, np.asarray(x)
    elif x is not None:
        yield path, np.asarray(x)


def assert_same_columns(a, b, what):
    import numpy as np
    ca, cb = dict(columns(a)), dict(columns(b))
    assert sorted(ca) == sorted(cb) and len(ca) > 50, what
    for f in ca:
        assert ca[f].dtype == cb[f].dtype and np.array_equal(ca[f], cb[f]), (what, f)
    return len(ca)


def child_one_context(R):
    from oracle import oracle as O
    reads = read_fasta_gz(os.path.join(GOLDEN, "reads-0.00.fa.gz"))
    k, l, d, A = ONE_CONTEXT
    with R.Mdbg(k, l, d, A, keep_reads=True) as m:
        m.ingest(*O.concat_reads(reads), 0)
        first = every_stage(R, m, reads)
        assert len(first["edges"]["n1"]) == 206                                    # tests/golden/example_cfg1.json
        m.reset(0)                                                                 # every grow-only buffer now holds the large graph's arrays behind the small graph's extent
        m.ingest(*O.concat_reads(reads[:10]), 0)
        small = every_stage(R, m, reads[:10])
        with R.Mdbg(k, l, d, A, keep_reads=True) as fresh:
            fresh.ingest(*O.concat_reads(reads[:10]), 0)
            n = assert_same_columns(small, every_stage(R, fresh, reads[:10]), "10 reads behind all reads == 10 reads in a fresh context")
        assert small["nodes"]["n_nodes"] < first["nodes"]["n_nodes"]
        m.reset(0)
        m.ingest(*O.concat_reads(reads), 0)
        assert_same_columns(first, every_stage(R, m, reads), "all reads again == the first pass")
    print("ONE_CONTEXT_OK columns=%d nodes=%d/%d" % (n, small["nodes"]["n_nodes"], first["nodes"]["n_nodes"]))


CHILDREN = {"selftest": child_selftest, "sketch_table": child_sketch_table, "input_formats": child_input_formats, "nodes_to_simplify": child_nodes_to_simplify,
            "components_everything_removed": child_components_everything_removed, "read_paths_catalogue": child_read_paths_catalogue,
            "junctions_catalogue": child_junctions_catalogue, "transits_catalogue_first_half": child_transits_catalogue_first_half,
            "transits_catalogue_second_half": child_transits_catalogue_second_half, "edge_prune_catalogue": child_edge_prune_catalogue,
            "transits_hand_built_repeats": child_transits_hand_built_repeats,
            "read_evidence_shapes": child_read_evidence_shapes, "kept_contigs_fuzz": child_kept_contigs_fuzz, "kept_contigs_other": child_kept_contigs_other,
            "kept_node_seqs_whole": child_kept_node_seqs_whole, "kept_node_seqs_chunks": child_kept_node_seqs_chunks, "one_context": child_one_context}
