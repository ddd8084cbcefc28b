"""The resident reads threaded through the unitig graph on the GPU (Mdbg.graph_read_paths) against the plain restatement (tests/read_paths_restatement.py),
exactly, array for array: the catalogue of tests/sketch_graphs.py on the plain and on every simplified list, the shapes at which the kernels can still go
wrong, ordinals and ranges, base-space reads, the state checks, the pipeline's files and the C program's summary.  CPU side: tests/test_read_paths_cpu.py."""
import os
import random

import numpy as np
import pytest

import read_paths_restatement as RP
import sketch_graphs as G
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from test_gpu_parity import _mdbg
from test_gpu_simplify import same_list
from test_gpu_sketch_graphs import BY_NAME, feed
from test_read_paths_cpu import WRAPPED, hashes

pytestmark = pytest.mark.gpu

STEP_COLUMNS = ("first_window", "step_windows", "unitig", "first_entry", "strand")
E_STATE = -6


def expected(reads, k, nodes, ul):
    walks, circular = RP.walks_of(ul) if ul["n_unitigs"] else ([], [])
    return RP.read_paths(hashes(reads), k, nodes["keys"].tolist(), nodes["index"].tolist(), walks, circular)


def assert_same_arrays(a, b):
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]) and np.asarray(a[f]).dtype == np.asarray(b[f]).dtype, f


def assert_equals_restatement(got, exp, ordinals, first=0, last=None):
    """got: a graph_read_paths() result for the reads [first, last) of the restatement's"""
    steps = exp["steps"][first:last]
    flat = [s for st in steps for s in st]
    assert got["first_read"] == first and got["n_reads"] == len(steps) and got["n_steps"] == len(flat)
    assert got["n_windows"] == sum(exp["windows"][first:last]) and got["n_placed"] == sum(exp["placed"][first:last])
    assert got["step_offsets"].tolist() == np.cumsum([0] + [len(st) for st in steps]).tolist()
    for i, f in enumerate(STEP_COLUMNS):
        assert got[f].tolist() == [s[i] for s in flat], f
    assert got["read_windows"].tolist() == exp["windows"][first:last] and got["ordinal"].tolist() == list(ordinals)[first:last]


def assert_zeros(got, first=0):
    assert (got["first_read"], got["n_reads"], got["n_windows"], got["n_placed"], got["n_steps"], got["n_unitigs"]) == (first, 0, 0, 0, 0, 0)
    assert got["step_offsets"].tolist() == [0] and all(len(got[f]) == 0 for f in STEP_COLUMNS + ("ordinal", "read_windows", "support_windows", "support_steps"))


def check_paths(R, m, reads, k, nodes, ul, ordinals=None, invariant=True):
    """the context's current list is `ul` (host arrays): the whole store's paths equal the restatement's, twice, from both variants; -> (got, exp)"""
    got = m.graph_read_paths()
    if ul["n_unitigs"] == 0:                                                        # a schedule that removed everything: the empty list gives zeros
        assert_zeros(got)
        return got, None
    exp = expected(reads, k, nodes, ul)
    print("reads %d windows %d placed %d steps %d unitigs %d" % (got["n_reads"], got["n_windows"], got["n_placed"], got["n_steps"], got["n_unitigs"]))
    assert_equals_restatement(got, exp, range(len(reads)) if ordinals is None else ordinals)
    assert got["n_unitigs"] == ul["n_unitigs"] and got["support_windows"].tolist() == exp["support_windows"] and got["support_steps"].tolist() == exp["support_steps"]
    if invariant is not None:
        assert (got["support_windows"].tolist() == ul["kc_sum"].tolist()) == invariant  # an abundance is a count of windows, until its u16 wraps or saturates
    assert_same_arrays(got, m.graph_read_paths())                                   # nothing depends on scheduling
    dev = m.graph_read_paths_device()
    assert (int(dev.n_reads), int(dev.n_windows), int(dev.n_placed), int(dev.n_steps), int(dev.n_unitigs)) == tuple(got[f] for f in ("n_reads", "n_windows", "n_placed", "n_steps", "n_unitigs"))
    for f, t, per in R.api.READ_PATH_FIELDS:
        n = got["n_" + per + "s"]
        back = np.empty(n, t)
        m._chk(m.L.mdbg_copy_to_host(m.h, back.ctypes.data, getattr(dev, f), back.nbytes))
        assert np.array_equal(back, got[f]), f
    assert m.read_paths_ms() >= 0.0
    return got, exp


def built(R, reads, k, A, split=None, presimp=0.0):
    """context with the reads fed as sketches, finalized, edges and the plain unitig list made -> (m, nodes, ul); the caller closes m"""
    m = R.Mdbg(k, G.L, G.D, A)
    feed(m, reads, split)
    nodes = m.finalize()
    m.graph_edges(presimp)
    return m, nodes, m.graph_unitigs()


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_catalogue_on_the_plain_and_on_every_simplified_list(name):
    R = _mdbg()
    c = BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimps[0])
    with m:
        before = m.graph_components()
        check_paths(R, m, c.reads, c.k, nodes, ul, invariant=name not in WRAPPED)
        same_list(m.graph_unitigs(), ul, R)                                         # the call left the list, and what is built on it, as it was
        after = m.graph_components()
        assert sorted(before) == sorted(after) and all(np.array_equal(before[f], after[f]) for f in before)
        for steps in c.schedules:
            simp = m.graph_simplify(steps)                                          # the simplified list is now the current one
            check_paths(R, m, c.reads, c.k, nodes, simp, invariant=None if name in WRAPPED else True)
            same_list(m.graph_simplify(steps), simp, R)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_minimizer_space_graphs(seed):
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        got, exp = check_paths(R, m, reads, k, nodes, ul)
        from test_read_paths_cpu import RANDOM
        assert (got["n_windows"], got["n_placed"], got["n_steps"]) == RANDOM[seed]


# ---- shapes at which the kernels can still go wrong (k = 3) -----------------------------------------------------------------------------------------------
def distinct_hashes(seed, n):
    return random.Random(seed).sample(range(1, G.HASH_LIMIT), n)


def test_two_long_reads_cross_every_workgroup_span():
    """5,000 fresh minimizers and the same read from the other strand: one unitig of 4,998 nodes, one step per read, runs across every span of 256, 1,024 and
    2,048 indices and across the scan's blocks, both strands"""
    R = _mdbg()
    h = distinct_hashes(1, 5000)
    reads = [G.mread(h), G.mread(h, rev=True)]
    m, nodes, ul = built(R, reads, 3, 1)
    with m:
        got, exp = check_paths(R, m, reads, 3, nodes, ul)
        assert got["n_steps"] == 2 and got["step_windows"].tolist() == [4998, 4998] and sorted(got["strand"].tolist()) == [0, 1]


def test_many_short_reads_on_a_ring():
    """3,000 reads of k + 1 minimizers from a ring of 60 hashes, half of them from the other strand: read boundaries and step heads in every block, steps that wrap"""
    R = _mdbg()
    ring = distinct_hashes(2, 60)
    rnd = random.Random(3)
    reads = []
    for _ in range(3000):
        p = rnd.randrange(60)
        reads.append(G.mread([ring[(p + j) % 60] for j in range(4)], rev=rnd.random() < 0.5))
    m, nodes, ul = built(R, reads, 3, 1, split=1000)
    with m:
        got, exp = check_paths(R, m, reads, 3, nodes, ul)
        assert ul["n_unitigs"] == 1 and ul["circular"].tolist() == [1] and got["n_steps"] == 3000 and set(got["step_windows"].tolist()) == {2}
        wrapped = [s for st in exp["steps"] for s in st if s[3] in (0, 59) and s[1] == 2]
        assert any(s[3] == 59 and s[4] == 0 for s in wrapped) and any(s[3] == 0 and s[4] == 1 for s in wrapped)      # 59 -> 0 and 0 -> 59


def test_a_read_that_visits_one_node_twice():
    """p q a b c x y a b c r s: the issue's read `a b c x y a b c` with a flank on either side.  Alone it is a ring of five nodes walked once (one step); with the
    flanks the node a-b-c has two ways in and two ways out, so it is a unitig of its own, and the read steps on it twice"""
    R = _mdbg()
    p, q, a, b, c, x, y, r, s = distinct_hashes(4, 9)
    reads = [G.mread([p, q, a, b, c, x, y, a, b, c, r, s])]
    m, nodes, ul = built(R, reads, 3, 1)
    with m:
        got, exp = check_paths(R, m, reads, 3, nodes, ul)
        assert max(got["support_steps"].tolist()) == 2 and got["unitig"].tolist().count(int(np.argmax(got["support_steps"]))) == 2


def test_short_and_empty_reads_at_the_ends_and_in_between():
    R = _mdbg()
    h = distinct_hashes(5, 40)
    reads = [G.mread(h[:3]), G.mread([]), G.mread(h[3:20]), G.mread([]), G.mread([]), G.mread(h[10:30], rev=True), G.mread(h[30:32]), G.mread([]), G.mread(h[37:40])]
    m, nodes, ul = built(R, reads, 3, 1, split=4)
    with m:
        got, exp = check_paths(R, m, reads, 3, nodes, ul)
        assert got["read_windows"].tolist() == [0, 0, 15, 0, 0, 18, 0, 0, 0] and got["step_offsets"].tolist()[-1] == got["n_steps"] > 0


def test_a_store_of_zero_reads_and_a_store_without_minimizers():
    R = _mdbg()
    with R.Mdbg(3, G.L, G.D, 1) as m:
        m.finalize()
        m.graph_edges(0.0)
        m.graph_unitigs()
        assert_zeros(m.graph_read_paths())
        assert_zeros(m.graph_read_paths(5, 2), 5)
    with R.Mdbg(3, G.L, G.D, 1) as m:
        feed(m, [G.mread([])] * 3)
        m.finalize()
        m.graph_edges(0.0)
        m.graph_unitigs()
        assert_zeros(m.graph_read_paths())


def test_unplaced_windows_split_one_visit_into_two_steps():
    """A = 2: a stretch seen twice is one unitig; a third read carries a foreign minimizer in its middle, the three windows over it occur once and are no rows"""
    R = _mdbg()
    h = distinct_hashes(6, 13)
    x, foreign = h[:12], h[12]
    reads = [G.mread(x), G.mread(x), G.mread(x[:5] + [foreign] + x[5:])]
    m, nodes, ul = built(R, reads, 3, 2)
    with m:
        got, exp = check_paths(R, m, reads, 3, nodes, ul)                           # (the filter drops a row AND its windows: the invariant holds)
        assert ul["n_unitigs"] == 1 and exp["steps"][2] == [(0, 3, 0, 0, 0), (6, 5, 0, 5, 0)] and (got["n_windows"], got["n_placed"]) == (31, 28)


# ---- ordinals and ranges -----------------------------------------------------------------------------------------------------------------------------------
def feed_batches(m, batches):
    """[(reads, first ordinal)] as ingest_sketch batches in this order, then the insertion"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []
    for reads, first in batches:
        h, p, o = G.sketch_arrays(reads)
        t = [torch.from_numpy(h.view(np.int64)).to(dev), torch.from_numpy(p.view(np.int32)).to(dev), torch.from_numpy(o.view(np.int64)).to(dev)]
        torch.cuda.synchronize()
        m.ingest_sketch(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(reads), first)
        keep.append(t)
    m.insert_resident()
    return keep


def test_ordinals_of_batches_out_of_order():
    """two batches with first ordinals (1000, 0) against the same reads as ONE batch in ordinal order: the same node table, and per ordinal rank the same steps"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(1)
    reads = reads[:30]
    late, early = reads[:12], reads[12:]
    with R.Mdbg(k, G.L, G.D, A) as m:
        feed_batches(m, [(late, 1000), (early, 0)])
        nodes = m.finalize()
        m.graph_edges(presimp)
        ul = m.graph_unitigs()
        ordinals = list(range(1000, 1012)) + list(range(18))
        two, _ = check_paths(R, m, reads, k, nodes, ul, ordinals=ordinals)
    with R.Mdbg(k, G.L, G.D, A) as m:
        feed_batches(m, [(early + late, 0)])
        nodes1 = m.finalize()
        assert np.array_equal(nodes1["keys"], nodes["keys"]) and np.array_equal(nodes1["index"], nodes["index"])
        m.graph_edges(presimp)
        ul1 = m.graph_unitigs()
        one, _ = check_paths(R, m, early + late, k, nodes1, ul1)
    per_read = lambda g: [tuple(tuple(g[f][a:b].tolist()) for f in STEP_COLUMNS) for a, b in zip(g["step_offsets"][:-1].tolist(), g["step_offsets"][1:].tolist())]
    by_rank = [s for _, s in sorted(zip(two["ordinal"].tolist(), per_read(two)))]
    assert by_rank == per_read(one) and np.array_equal(two["support_windows"], one["support_windows"]) and np.array_equal(two["support_steps"], one["support_steps"])


def test_ranges_concatenate_and_their_supports_add_up():
    R = _mdbg()
    k, A, presimp, reads = G.random_case(4)
    reads = reads[:20]
    m, nodes, ul = built(R, reads, k, A, split=6, presimp=presimp)
    with m:
        whole, exp = check_paths(R, m, reads, k, nodes, ul)
        parts = []
        for first, count, last in ((0, 1, 1), (1, 7, 8), (8, 0, 20)):
            got = m.graph_read_paths(first, count)
            assert_equals_restatement(got, exp, range(20), first, last)
            parts.append(got)
        for f in STEP_COLUMNS + ("ordinal", "read_windows"):
            assert np.array_equal(np.concatenate([p[f] for p in parts]), whole[f]), f
        for f in ("support_windows", "support_steps"):
            assert np.array_equal(sum(p[f] for p in parts), whole[f]), f
        assert sum(p["n_steps"] for p in parts) == whole["n_steps"] and sum(p["n_placed"] for p in parts) == whole["n_placed"]
        assert_zeros(m.graph_read_paths(20, 0), 20)
        assert_zeros(m.graph_read_paths(21, 3), 21)
        assert_same_arrays(m.graph_read_paths(0, 1000), whole)


# ---- base space --------------------------------------------------------------------------------------------------------------------------------------------
def test_base_space_reads_plain_and_simplified(example_reads):
    """tests/golden/reads-0.00.fa.gz at the example_cfg1 parameters through ingest; the restatement works on the oracle's sketch"""
    R = _mdbg()
    k, l, d, A = 7, 10, 0.0008, 2
    b, o = O.concat_reads(example_reads)
    sk = O.sketch(b, o, l, d)
    off = sk["off"].tolist()
    reads = [(tuple(sk["hashes"][x:y].tolist()), ()) for x, y in zip(off, off[1:])]
    with R.Mdbg(k, l, d, A, keep_reads=True) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        m.graph_edges(0.01)
        ul = m.graph_unitigs()
        contigs = m.graph_contigs(0)
        got, exp = check_paths(R, m, reads, k, nodes, ul, invariant=True)
        assert got["n_windows"] == 12127 and got["n_placed"] > 0
        same_list(m.graph_unitigs(), ul, R)
        assert_same_arrays(m.graph_contigs(0), contigs)
        simp = m.graph_simplify(R.api.MAGIC_SIMPLIFY_STEPS)
        check_paths(R, m, reads, k, nodes, simp)                                     # (a removed node takes its windows AND its abundance out: the invariant holds)


# ---- state -------------------------------------------------------------------------------------------------------------------------------------------------
def state_error(m, *a):
    with pytest.raises(_mdbg().MdbgError) as e:
        m.graph_read_paths(*a)
    assert e.value.code == E_STATE
    return str(e.value)


def test_state_errors_leave_the_context_usable():
    R = _mdbg()
    c = BY_NAME["fork"]
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        assert "no current unitig list" in state_error(m)                           # nothing yet
        feed(m, c.reads[:5])
        nodes = m.finalize()
        assert "no current unitig list" in state_error(m)                           # a node table, no list
        m.graph_edges(0.0)
        assert "no current unitig list" in state_error(m)
        ul = m.graph_unitigs()
        check_paths(R, m, c.reads[:5], c.k, nodes, ul)
        keep = feed_batches(m, [(c.reads[5:], 5)])                                  # an ingest (and the insertion) ends the list
        state_error(m)
        nodes = m.finalize()
        state_error(m)                                                              # a finalize without a new unitig call
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        check_paths(R, m, c.reads, c.k, nodes, ul)
        m.reset(c.k)                                                                # the store stays, the table and everything built on it go
        state_error(m)
        m.insert_resident()
        nodes = m.finalize()
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        check_paths(R, m, c.reads, c.k, nodes, ul)
        del keep
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        m.set_partition(2, 0)
        assert "single-GPU" in state_error(m)
        m.set_partition(1, 0)                                                       # the same context, unpartitioned again: it works
        feed(m, c.reads)
        nodes = m.finalize()
        m.graph_edges(0.0)
        check_paths(R, m, c.reads, c.k, nodes, m.graph_unitigs())
        assert m.L.mdbg_graph_read_paths(m.h, 0, 0, None) == m.L.mdbg_graph_read_paths(None, 0, 0, None) == -1      # MDBG_E_PARAM: a null pointer


# ---- pipeline and the C program -------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_files_and_the_c_program(example_reads, tmp_path):
    import subprocess
    from rust_mdbg_amd import pipeline
    R = _mdbg()
    k, l, d, A = 7, 10, 0.0008, 2
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    prefix = str(tmp_path / "rp")
    out = pipeline.run_file(src, prefix, k, l, d, A, write_sequences=False, contigs=True, keep_reads=True, simplify=R.api.MAGIC_SIMPLIFY_STEPS, read_paths=True,
                            batch_bases=5_000_000)
    b, o = O.concat_reads(example_reads)
    sk = O.sketch(b, o, l, d)
    off = sk["off"].tolist()
    reads = [(tuple(sk["hashes"][x:y].tolist()), ()) for x, y in zip(off, off[1:])]
    with R.Mdbg(k, l, d, A) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        m.graph_edges(0.01)
        ul = m.graph_unitigs()
        plain = expected(reads, k, nodes, ul)
        lib = m.graph_read_paths()
        sl = m.graph_simplify(R.api.MAGIC_SIMPLIFY_STEPS)
        simplified = expected(reads, k, nodes, sl)
    assert open(prefix + ".unitigs.read_paths.tsv").read() == RP.tsv_text(plain, range(len(reads)), ul["circular"].astype(bool).tolist())
    assert open(prefix + ".msimpl.read_paths.tsv").read() == RP.tsv_text(simplified, range(len(reads)), sl["circular"].astype(bool).tolist())
    assert (out["n_read_steps"], out["n_read_steps_simplified"]) == (plain["n_steps"], simplified["n_steps"])
    exe = str(tmp_path / "mdbg_cli")
    libdir = os.path.join(ROOT, "rust_mdbg_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mdbg_cli.c"),
                    "-L" + libdir, "-lmdbg_hip", "-lmdbg_emit", "-lpthread", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--prefix", str(tmp_path / "c"), "--no-basespace", "--read-paths"],
                       check=True, capture_output=True, text=True)
    n_per_read = np.diff(lib["step_offsets"].astype(np.int64))
    line = "read paths: %d reads with a step, %d / %d windows placed, %d reads with more than one step" % (
        int((n_per_read >= 1).sum()), lib["n_placed"], lib["n_windows"], int((n_per_read > 1).sum()))
    assert line in r.stdout.split("\n") and os.path.exists(str(tmp_path / "c.unitigs.fa"))
