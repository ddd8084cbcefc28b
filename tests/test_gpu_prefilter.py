"""The counting pre-filter (MDBG_FLAG_PREFILTER: csrc/prefilter.hip, the gated insert_windows_kernel, csrc/prefilter_api.inc) through the C ABI.

What the table must hold is restated from the header's definition (tests/prefilter_restatement.py) over the CPU oracle's table of all keys; every row field is the
oracle's at the same min_abundance.  Small set: 60 reads, one workgroup's span of window starts; large set: 240 reads, several spans and their borders.  The
conditions these inputs meet are checked without a GPU in tests/test_prefilter_cpu.py."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import prefilter_restatement as PR
from conftest import GOLDEN, ROOT, TESTS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

K, L, D = 5, 8, 0.008
NODE_FIELDS = ("keys", "index", "abundance", "seqlen", "shift", "shift_full", "src_read", "src_start", "src_end", "reversed")
CELLS = (1, 1024, 16384, 0)             # everything admitted; two medium sizes; the default 2^32


@functools.lru_cache(maxsize=None)
def reads_of(which):
    from rust_mdbg_amd import synth
    return tuple(synth.synth_reads(7, 20000, {"small": 60, "large": 240}[which], mean_len=3000, sd_len=300, min_len=1500, max_len=4500, err_ppm=10000))


@functools.lru_cache(maxsize=None)
def oracle_nodes(which, A, k=K, n_reads=None):
    """the oracle's node table of the set's first n_reads reads (ordinals from 0) — computed once, shared, never written to"""
    g = O.Graph(k, L, D, A)
    b, o = O.concat_reads(list(reads_of(which)[:n_reads]))
    assert g.ingest(b, o, 0) == 0
    return g.finalize(with_edges=False)


def expected(which, A, n_cells, k=K, n_reads=None):
    return PR.expected_nodes(oracle_nodes(which, A, k, n_reads), oracle_nodes(which, 1, k, n_reads), n_cells)


def assert_nodes_equal(got, exp, what):
    assert got["n_nodes_before"] == exp["n_nodes_before"], what
    assert got["n_nodes"] == exp["n_nodes"], what
    assert got["n_wrapped"] == 0, what
    for f in NODE_FIELDS:
        assert np.array_equal(np.asarray(got[f]), np.asarray(exp[f])), (what, f)


def ctx(A=2, n_cells=16384, k=K, **kw):
    import rust_mdbg_amd as R
    return R.Mdbg(k, L, D, A, prefilter=True, prefilter_cells=n_cells, **kw)


def exact_ctx(A=2, k=K, **kw):
    import rust_mdbg_amd as R
    return R.Mdbg(k, L, D, A, **kw)


# ---- 1. every A at every filter size -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells", CELLS)
@pytest.mark.parametrize("A", [2, 3, 9])
@pytest.mark.parametrize("which", ["small", "large"])
def test_table_equals_oracle_rows_and_restated_index(which, A, n_cells):
    reads = list(reads_of(which))
    exp, r = expected(which, A, n_cells)
    assert exp["n_nodes"] > 0
    with ctx(A, n_cells) as m:
        m.ingest_reads(reads, 0)
        got = m.finalize()
        st = m.stats()
    assert_nodes_equal(got, exp, (which, A, n_cells))
    assert st["n_windows_admitted"] == r["n_windows_admitted"] and st["n_distinct"] == r["n_distinct"]
    assert st["n_windows"] == oracle_nodes(which, 1)["n_windows"] and st["prefilter_cells"] == (n_cells or 1 << 32)
    if n_cells == 1:
        with exact_ctx(A) as e:
            e.ingest_reads(reads, 0)
            ex = e.finalize()
            est = e.stats()
        assert_nodes_equal(got, ex, (which, A, "exact context"))
        assert (est["n_windows"], est["n_distinct"], est["n_windows_admitted"], est["prefilter_cells"]) == (st["n_windows"], st["n_distinct"], 0, 0)


# ---- 2. the same reads in four arrangements ------------------------------------------------------------------------------------------------------------------------------
def three_batches(reads):
    n = len(reads)
    cuts = [0, n // 3, 2 * n // 3 + 1, n]
    return [(reads[cuts[i]:cuts[i + 1]], cuts[i]) for i in (2, 0, 1)]          # the last third first: neither ascending nor descending ordinals


@pytest.mark.parametrize("which", ["small", "large"])
def test_four_arrangements_give_one_table(which):
    import torch
    reads = list(reads_of(which))
    exp, r = expected(which, 2, 16384)
    tables = {}
    with ctx() as m:
        m.ingest_reads(reads, 0)
        tables["one batch"] = m.finalize()
    with ctx() as m:
        for part, first in three_batches(reads):
            m.ingest_reads(part, first)
        tables["three shuffled batches"] = m.finalize()
        assert m.stats()["n_windows_admitted"] == r["n_windows_admitted"]
    with ctx() as m:
        for part, first in three_batches(reads):
            m.ingest_reads(part, first)
            mid = m.finalize()
            assert mid["n_nodes"] <= exp["n_nodes"]
        tables["a finalize after every batch"] = mid
        assert m.stats()["n_windows_admitted"] == r["n_windows_admitted"]
    with ctx() as m:
        keep = []
        for part, first in three_batches(reads):
            b, o = O.concat_reads(part)
            tb, to = torch.from_numpy(b).cuda(), torch.from_numpy(o.view(np.int64)).cuda()
            torch.cuda.synchronize()
            keep.append((tb, to))
            m.sketch_device(tb.data_ptr(), to.data_ptr(), len(part), len(b), first)
        m.insert_resident()
        assert m.stats()["n_windows_admitted"] == r["n_windows_admitted"]
        tables["sketch_device + insert_resident"] = m.finalize()
    for name, got in tables.items():
        assert_nodes_equal(got, exp, (which, name))


def test_a_round_in_slices(monkeypatch):
    """insert_sliced with the gate: MDBG_INSERT_SLICE (read at every round) cuts the large set's batches into slices of one workgroup's span"""
    monkeypatch.setenv("MDBG_INSERT_SLICE", "2048")
    reads = list(reads_of("large"))
    exp, r = expected("large", 2, 16384)
    with ctx() as m:
        for part, first in three_batches(reads):
            m.ingest_reads(part, first)
        assert_nodes_equal(m.finalize(), exp, "sliced")
        assert m.stats()["n_windows_admitted"] == r["n_windows_admitted"]


# ---- 3. reset to another k, mark / rewind --------------------------------------------------------------------------------------------------------------------------------
def test_reset_to_another_k_equals_a_fresh_context():
    reads = list(reads_of("small"))
    with ctx() as m:
        m.ingest_reads(reads, 0)
        assert_nodes_equal(m.finalize(), expected("small", 2, 16384)[0], "k = 5")
        m.reset(7)
        again = m.finalize()
        st = m.stats()
    exp, r = expected("small", 2, 16384, k=7)
    assert exp["n_nodes"] > 0 and r["rejected"] > 0
    assert_nodes_equal(again, exp, "reset to k = 7")
    assert st["n_windows_admitted"] == r["n_windows_admitted"]
    with ctx(k=7) as f:
        f.ingest_reads(reads, 0)
        assert_nodes_equal(again, f.finalize(), "fresh context at k = 7")


def test_mark_ingest_rewind_equals_a_fresh_context():
    reads = list(reads_of("small"))
    with ctx() as m:
        m.ingest_reads(reads[:40], 0)
        mk = m.mark()
        m.ingest_reads(reads[40:], 40)
        assert_nodes_equal(m.finalize(), expected("small", 2, 16384)[0], "all reads")
        m.rewind(mk)
        back = m.finalize()
    exp, r = expected("small", 2, 16384, n_reads=40)
    assert 0 < exp["n_nodes"] < expected("small", 2, 16384)[0]["n_nodes"]
    assert_nodes_equal(back, exp, "after the rewind")
    with ctx() as f:
        f.ingest_reads(reads[:40], 0)
        assert_nodes_equal(back, f.finalize(), "fresh context with the first 40 reads")


# ---- 4. - 6. the calls that look windows up ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 3])
def test_query_batch_equals_the_exact_context(A):
    reads = list(reads_of("small"))
    qb, qo = O.concat_reads(reads[:7] + [reads[3][::-1]])          # the last one shares next to no k-min-mer with the table: absent keys
    with ctx(A) as m, exact_ctx(A) as e:
        m.ingest_reads(reads, 0)
        e.ingest_reads(reads, 0)
        (gc, go), (ec, eo) = m.query(qb, qo), e.query(qb, qo)      # (the first call that reads the table: it runs the insertion round)
        assert m.stats()["n_distinct"] == expected("small", A, 16384)[1]["n_distinct"]
    assert np.array_equal(go, eo) and np.array_equal(gc, ec) and len(gc) > 100 and (gc > 0).any() and (gc == 0).any()


def by_row(nodes, idx):
    row = {int(v): i for i, v in enumerate(nodes["index"])}
    return np.array([row[int(v)] for v in idx], dtype=np.int64)


def graph_of(m, reads, read_paths=False):
    m.ingest_reads(reads, 0)
    nodes = m.finalize()
    e = m.graph_edges(0.01)
    u = m.graph_unitigs()
    out = dict(nodes=nodes, edges=dict(e, n1=by_row(nodes, e["n1"]), n2=by_row(nodes, e["n2"])), unitigs=dict(u, node=by_row(nodes, u["node"])))
    if read_paths:
        out["read_paths"] = m.graph_read_paths()
    return out


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for f in a:
        if isinstance(a[f], dict):
            assert_same(a[f], b[f], (what, f))
        elif isinstance(a[f], np.ndarray):
            assert np.array_equal(a[f], b[f]), (what, f)
        else:
            assert a[f] == b[f], (what, f)


@pytest.mark.parametrize("which", ["small", "large"])
def test_edges_and_unitigs_equal_the_exact_contexts_by_row(which):
    reads = list(reads_of(which))
    with ctx() as m, exact_ctx() as e:
        g, x = graph_of(m, reads), graph_of(e, reads)
    assert g["nodes"]["n_nodes_before"] < x["nodes"]["n_nodes_before"] and len(g["edges"]["n1"]) > 50 and g["unitigs"]["n_unitigs"] > 5
    assert not np.array_equal(g["nodes"]["index"], x["nodes"]["index"])          # the names differ, the graph does not
    assert_same(g["edges"], x["edges"], "edges")
    assert_same(g["unitigs"], x["unitigs"], "unitigs")


def test_read_paths_on_a_keeping_context_equal_the_exact_contexts():
    reads = list(reads_of("small"))
    with ctx(keep_reads=True) as m, exact_ctx(keep_reads=True) as e:
        g, x = graph_of(m, reads, read_paths=True), graph_of(e, reads, read_paths=True)
    assert g["read_paths"]["n_reads"] == 60 and g["read_paths"]["n_placed"] > 0 and g["read_paths"]["n_windows"] == 1679
    assert_same(g["read_paths"], x["read_paths"], "read paths")


# ---- 7. the table is sized from the admitted windows ---------------------------------------------------------------------------------------------------------------------
def test_table_capacity_is_below_the_exact_contexts():
    reads = list(reads_of("small"))
    with ctx() as m, exact_ctx() as e:
        m.ingest_reads(reads, 0)
        e.ingest_reads(reads, 0)
        m.finalize()
        e.finalize()
        a, b = m.stats(), e.stats()
    assert 0 < a["table_capacity"] < b["table_capacity"]          # slots_for over 1,066 admitted windows against 1,679
    assert (a["n_windows"], a["n_windows_admitted"], b["n_windows"]) == (1679, 1066, 1679)


# ---- 8. error answers ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_error_answers():
    import rust_mdbg_amd as R
    from rust_mdbg_amd import api
    with pytest.raises(R.MdbgError) as e:
        R.Mdbg(K, L, D, 1, prefilter=True)
    assert e.value.code == api.MDBG_E_PARAM
    with pytest.raises(R.MdbgError) as e:
        R.Mdbg(K, L, D, 2, prefilter=True, prefilter_cells=(1 << 36) + 1)
    assert e.value.code == api.MDBG_E_PARAM
    with ctx() as m:
        m.set_partition(1, 0)
        with pytest.raises(R.MdbgError) as e:
            m.set_partition(2, 0)
        assert e.value.code == api.MDBG_E_STATE and "pre-filter" in str(e.value)
        m.ingest_reads(list(reads_of("small"))[:10], 0)
        with pytest.raises(R.MdbgError) as e:
            m.route_pack(2)
        assert e.value.code == api.MDBG_E_STATE
        with pytest.raises(R.MdbgError) as e:
            m.insert_records(0, 0)
        assert e.value.code == api.MDBG_E_STATE
        assert m.finalize()["n_nodes"] == oracle_nodes("small", 2, K, 10)["n_nodes"]          # the context is none the worse for the refusals


# ---- 9. under MDBG_GUARD: no kernel of the mode writes outside its blocks ------------------------------------------------------------------------------------------------
GUARD_LINE = re.compile(r"^GUARD_OK calls=(\d+) blocks=(\d+) bytes=(\d+)$", re.M)


def child_main():
    from rust_mdbg_amd import api
    assert api.GUARD and api.load_library().mdbg_guard_selftest() == 0
    print("SELFTEST_OK", flush=True)
    for which in ("small", "large"):
        for n_cells in (1, 1024, 16384):
            reads = list(reads_of(which))
            with ctx(2, n_cells) as m:
                for part, first in three_batches(reads):
                    m.ingest_reads(part, first)
                    m.finalize()
                assert_nodes_equal(m.finalize(), expected(which, 2, n_cells)[0], (which, n_cells))
                m.reset(7)
                m.finalize()
    api.guard_check()
    print("GUARD_OK calls=%d blocks=%d bytes=%d" % (api.GUARD_SEEN["calls"], api.GUARD_SEEN["blocks"], api.GUARD_SEEN["bytes"]))


def test_the_mode_under_guard():
    base = {k: v for k, v in os.environ.items() if k not in ("MDBG_GUARD", "MDBG_POISON")}
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_prefilter as T; T.child_main()" % (ROOT, TESTS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(base, MDBG_GUARD="1"), timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = GUARD_LINE.search(r.stdout)
    assert got is not None and r.stdout.startswith("SELFTEST_OK\n"), (r.stdout[-1500:], r.stderr[-3000:])
    assert all(int(x) > 0 for x in got.groups()), got.group(0)


def test_guard_is_clean_after_the_module():
    from rust_mdbg_amd import api
    api.guard_check()


# ---- 10., 11. the drivers ------------------------------------------------------------------------------------------------------------------------------------------------
def renamed_gfa(path):
    """S and L lines with the nodes renamed by order of appearance among the S lines"""
    lines = open(path).read().split("\n")
    s = [x.split("\t") for x in lines if x.startswith("S")]
    name = {f[1]: str(i) for i, f in enumerate(s)}
    l_ = [x.split("\t") for x in lines if x.startswith("L")]
    return ["\t".join([f[0], name[f[1]]] + f[2:]) for f in s], sorted("\t".join([f[0], name[f[1]], f[2], name[f[3]]] + f[4:]) for f in l_)


def test_run_file_with_the_prefilter(tmp_path):
    from rust_mdbg_amd import pipeline
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    a = pipeline.run_file(src, str(tmp_path / "bf"), 7, 10, 0.0008, 2, batch_bases=3_000_000, prefilter=True)
    b = pipeline.run_file(src, str(tmp_path / "exact"), 7, 10, 0.0008, 2, batch_bases=3_000_000)
    assert renamed_gfa(str(tmp_path / "bf.gfa")) == renamed_gfa(str(tmp_path / "exact.gfa"))
    assert (a["n_nodes"], a["n_edges"], a["n_windows"]) == (b["n_nodes"], b["n_edges"], b["n_windows"]) == (104, 206, 12127)
    assert a["n_nodes_before"] <= b["n_nodes_before"] and 0 < a["n_windows_admitted"] <= a["n_windows"]


def test_run_multik_with_the_prefilter(tmp_path):
    """the reference's multik is a --bf run: every k of the sweep re-windows the resident sketches and counts the filter anew"""
    from rust_mdbg_amd import pipeline
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    ks = [7, 5]
    a = pipeline.run_multik(src, str(tmp_path / "bf"), ks, 10, 0.0008, 2, batch_bases=5_000_000, prefilter=True, prefilter_cells=1 << 20)
    b = pipeline.run_multik(src, str(tmp_path / "exact"), ks, 10, 0.0008, 2, batch_bases=5_000_000)
    for k in ks:
        assert renamed_gfa("%s-k%d.gfa" % (tmp_path / "bf", k)) == renamed_gfa("%s-k%d.gfa" % (tmp_path / "exact", k))
        assert (a[k]["n_nodes"], a[k]["n_edges"], a[k]["n_windows"]) == (b[k]["n_nodes"], b[k]["n_edges"], b[k]["n_windows"])
        assert a[k]["n_nodes_before"] <= b[k]["n_nodes_before"]
    assert a[7]["n_nodes"] == 104 and a[5]["n_nodes"] > 104


def test_plain_c_program_with_bf(tmp_path):
    from rust_mdbg_amd import pipeline
    exe = str(tmp_path / "mdbg_cli")
    lib = os.path.join(ROOT, "rust_mdbg_amd")
    subprocess.run(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mdbg_cli.c"), "-L" + lib, "-lmdbg_hip", "-lmdbg_emit",
                    "-lpthread", "-Wl,-rpath," + lib, "-o", exe], check=True)
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    r = subprocess.run([exe, src, "-k", "7", "-l", "10", "--density", "0.0008", "--minabund", "2", "--bf", "--bf-cells", "65536", "--no-basespace", "--prefix", str(tmp_path / "c")],
                       check=True, capture_output=True, text=True)
    assert "Number of nodes after abundance filter: 104" in r.stdout and "Number of mdBG edges: 206" in r.stdout
    pipeline.run_file(src, str(tmp_path / "py"), 7, 10, 0.0008, 2, write_sequences=False)
    assert renamed_gfa(str(tmp_path / "c.gfa")) == renamed_gfa(str(tmp_path / "py.gfa"))
    bad = subprocess.run([exe, src, "-k", "7", "-l", "10", "--density", "0.0008", "--minabund", "1", "--bf"], capture_output=True, text=True)
    assert bad.returncode == 1 and "invalid parameter" in bad.stderr
