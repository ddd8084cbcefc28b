"""Read support per junction on the GPU (Mdbg.graph_junctions) against the plain restatement (tests/junctions_restatement.py), exactly: every scalar, the supports
element for element, the seven missing columns with their dtypes — on the catalogue of tests/sketch_graphs.py (plain and simplified lists), the random graphs, the
shapes at which the kernels can still go wrong, ranges of reads, the state checks, the other results a caller may hold, the pipeline's files and the C program's
summary.  CPU side: tests/test_junctions_cpu.py."""
import os
import random

import numpy as np
import pytest

import junctions_restatement as J
import read_paths_restatement as RP
import sketch_graphs as G
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from test_gpu_parity import _mdbg
from test_gpu_read_paths import built, distinct_hashes, feed_batches
from test_gpu_simplify import same_list
from test_gpu_sketch_graphs import BY_NAME, feed
from test_junctions_cpu import RANDOM, figures
from test_read_paths_cpu import hashes

pytestmark = pytest.mark.gpu

SCALARS = ("n_reads", "n_adjacent", "n_links", "n_crossings", "n_explained", "n_missing_crossings", "n_records", "n_missing")
E_STATE = -6


def records_of(ul):
    e = ul["edges"]
    return list(zip(e["n1"].tolist(), [chr(o) for o in e["o1"].tolist()], e["n2"].tolist(), [chr(o) for o in e["o2"].tolist()]))


def expected(reads, k, nodes, ul):
    walks, _ = RP.walks_of(ul)
    return J.junctions(hashes(reads), k, nodes["keys"].tolist(), nodes["index"].tolist(), walks, records_of(ul))


def shaped(R, exp, n_reads, first=0):
    """a restatement result in the shape of Mdbg.graph_junctions()"""
    out = {f: np.array([row[i] for row in exp["missing_rows"]], dtype=t) for i, (f, t, _) in enumerate(R.api.JUNCTION_FIELDS[1:])}
    out.update({f: exp[f] for f in SCALARS if f != "n_reads"}, support=np.array(exp["support"], np.uint64), n_reads=n_reads, first_read=first)
    return out


def assert_same(a, b):
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]) and np.asarray(a[f]).dtype == np.asarray(b[f]).dtype, f


def assert_zeros(R, got, first=0):
    assert got["first_read"] == first and all(got[f] == 0 for f in SCALARS) and all(len(got[f]) == 0 for f, _, _ in R.api.JUNCTION_FIELDS)


def check(R, m, reads, k, nodes, ul):
    """the context's current list is `ul` (host arrays): the whole store's junction support equals the restatement's, twice from the host variant and once from the
    device variant; -> (got, exp)"""
    got = m.graph_junctions()
    if ul["n_unitigs"] == 0:                                                        # a schedule that removed everything: the empty list gives zeros
        assert_zeros(R, got)
        return got, None
    exp = expected(reads, k, nodes, ul)
    print(" ".join("%s %d" % (f, got[f]) for f in SCALARS))
    assert_same(got, shaped(R, exp, len(reads)))
    assert got["n_explained"] + got["n_missing_crossings"] == got["n_crossings"] and got["n_links"] + got["n_crossings"] == got["n_adjacent"]
    assert_same(m.graph_junctions(), got)                                           # nothing depends on scheduling
    dev = m.graph_junctions_device()
    assert all(int(getattr(dev, f)) == got[f] for f in SCALARS) and int(dev.first_read) == 0
    for f, t, per in R.api.JUNCTION_FIELDS:
        back = np.empty(got["n_records" if per == "record" else "n_missing"], t)
        m._chk(m.L.mdbg_copy_to_host(m.h, back.ctypes.data, getattr(dev, f), back.nbytes))
        assert np.array_equal(back, got[f]), f
    assert m.junctions_ms() >= 0.0
    return got, exp


# ---- the catalogue and the random graphs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_IDS)
def test_catalogue_on_the_plain_and_on_every_simplified_list(name):
    R = _mdbg()
    c = BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimps[0])
    with m:
        got, _ = check(R, m, c.reads, c.k, nodes, ul)
        if c.presimps[0] == 0.0:
            assert got["n_missing"] == 0
        same_list(m.graph_unitigs(), ul, R)                                         # the call left the list as it was
        for steps in c.schedules:
            simp = m.graph_simplify(steps)                                          # the simplified list is now the current one
            check(R, m, c.reads, c.k, nodes, simp)
            same_list(m.graph_simplify(steps), simp, R)


@pytest.mark.parametrize("seed", G.RANDOM_SEEDS)
def test_random_minimizer_space_graphs(seed):
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        got, exp = check(R, m, reads, k, nodes, ul)
        if seed in RANDOM:
            fig = figures(exp) + (exp["n_missing_crossings"],)
            assert all(w is None or g == w for g, w in zip(fig, RANDOM[seed])), fig
        if seed == 0:
            assert len(set(exp["keys"])) > 2048                                     # the sorted record keys and their binary search cross the sort's blocks


# ---- other results a caller may hold -----------------------------------------------------------------------------------------------------------------------------
def test_a_held_read_path_result_and_a_held_component_result_are_untouched():
    R = _mdbg()
    k, A, presimp, reads = G.random_case(6)
    m, nodes, ul = built(R, reads, k, A, 40, presimp)
    with m:
        rp, cl = m.graph_read_paths_device(), m.graph_components_device()
        n = dict(read=int(rp.n_reads), step=int(rp.n_steps), unitig=int(rp.n_unitigs))
        held = [(getattr(rp, f), n[per], t) for f, t, per in R.api.READ_PATH_FIELDS] + [(rp.step_offsets, n["read"] + 1, np.uint64)]
        held += [(getattr(cl, f), int(cl.n_unitigs if per_unitig else cl.n_components), t) for f, t, per_unitig in R.api.COMPONENT_FIELDS]
        copy_back = lambda: [m.to_host(R.api.C.cast(p, R.api.C.c_void_p).value, cnt * np.dtype(t).itemsize, t) for p, cnt, t in held]
        before = copy_back()
        assert n["step"] > 0 and int(cl.n_components) > 0
        got, _ = check(R, m, reads, k, nodes, ul)                                   # three junction calls
        assert got["n_missing"] == 64
        assert all(np.array_equal(a, b) for a, b in zip(before, copy_back()))
        same_list(m.graph_unitigs(), ul, R)


# ---- shapes at which the kernels can still go wrong (k = 3) ----------------------------------------------------------------------------------------------------
def test_crossings_on_every_residue_of_the_index_modulo_256():
    """a trunk of 300 minimizers with an arm that leaves it behind minimizer 150; 600 reads of 6 minimizers (4 windows) cut round the fork so that the one crossing of
    read q — path windows 148 -> 149 — sits at read-local window 1, 2 or 3: the thread that finds it has index 6 q + that, every residue modulo 256 among them;
    every second read comes from the other strand, every other pair of reads takes the arm.  Two keys take 301 crossings each"""
    R = _mdbg()
    h = distinct_hashes(11, 310)
    trunk, arm = h[:300], h[:151] + h[300:310]
    reads, at = [], []
    for q in range(600):
        path, s, rev = (arm if (q // 2) % 2 else trunk), 146 + q % 3, q % 2 == 1
        reads.append(G.mread(path[s:s + 6], rev=rev))
        at.append(6 * q + (s - 145 if rev else 149 - s))                            # the index of the second window of the crossing pair
    assert {t % 256 for t in at} == set(range(256)) and len(at) // 256 >= 2
    reads += [G.mread(trunk), G.mread(arm)]                                         # behind the short reads: their indices stay 6 q + ...
    m, nodes, ul = built(R, reads, 3, 1)
    with m:
        got, exp = check(R, m, reads, 3, nodes, ul)
        assert got["n_crossings"] == 602 and sorted(set(got["support"].tolist())) == [301] and got["n_records"] == 4 and got["n_missing"] == 0


def test_a_read_boundary_on_a_multiple_of_256_indices_is_no_adjacent_pair():
    """read 0 has exactly 256 minimizers and read 1 starts with the last two of them: the last window of read 0 and the first of read 1 are neighbours on the unitig
    (read 2 covers everything), a link if they were counted"""
    R = _mdbg()
    h = distinct_hashes(12, 400)
    reads = [G.mread(h[:256]), G.mread(h[254:330]), G.mread(h)]
    m, nodes, ul = built(R, reads, 3, 1)
    with m:
        got, exp = check(R, m, reads, 3, nodes, ul)
        assert ul["n_unitigs"] == 1 and got["n_adjacent"] == exp["n_adjacent"] == 253 + 73 + 397 and got["n_links"] == got["n_adjacent"]
        both = m.graph_junctions(0, 2)
        assert both["n_adjacent"] == 253 + 73 == both["n_links"]


def test_many_missing_keys():
    """a trunk read of 3,000 minimizers ten times and 2,500 branch reads that share three trunk minimizers, each at its own position, and then leave; the edges are
    built at presimp 0.5, which removes every branch's edge: each branch read leaves the trunk at an interior entry of its own"""
    R = _mdbg()
    h = distinct_hashes(13, 3000 + 3 * 2500)
    trunk = h[:3000]
    reads = [G.mread(trunk)] * 10 + [G.mread(trunk[i:i + 3] + h[3000 + 3 * i:3003 + 3 * i], rev=i % 2 == 1) for i in range(2500)]
    m, nodes, ul = built(R, reads, 3, 1, presimp=0.5)
    with m:
        got, exp = check(R, m, reads, 3, nodes, ul)
        assert exp["n_missing"] > 2048 and got["n_missing"] == 2500 == got["n_missing_crossings"] and got["n_records"] == 0
        # (a branch read from the other strand enters the trunk backwards; its key is the mirror, which leaves the trunk forwards: every key starts on the trunk)
        assert got["missing_count"].tolist() == [1] * 2500 and len(set(zip(got["missing_unitig1"].tolist(), got["missing_entry1"].tolist()))) == 2500


def test_the_closing_record_of_a_ring_counts_the_wraps():
    """many_short_reads_on_a_ring of the read-path tests: 3,000 reads of two windows from a ring of 60, half of them from the other strand.  The wraps are counted here
    from the reads: a read wraps iff its two windows lie on entries 0 and 59"""
    R = _mdbg()
    ring = distinct_hashes(2, 60)
    rnd = random.Random(3)
    reads = []
    for _ in range(3000):
        p = rnd.randrange(60)
        reads.append(G.mread([ring[(p + j) % 60] for j in range(4)], rev=rnd.random() < 0.5))
    m, nodes, ul = built(R, reads, 3, 1, split=1000)
    with m:
        got, exp = check(R, m, reads, 3, nodes, ul)
        assert ul["n_unitigs"] == 1 and ul["circular"].tolist() == [1] and ul["n_entries"] == 60
        entry_of_index = {int(idx): j for j, idx in enumerate(ul["node"].tolist())}
        entry = {tuple(key): entry_of_index[int(i)] for key, i in zip(nodes["keys"].tolist(), nodes["index"].tolist())}
        wraps = sum({entry[RP.canonical(tuple(H[w:w + 3]))[0]] for w in (0, 1)} == {0, 59} for H in hashes(reads))
        assert 0 < wraps < 3000 and sorted(records_of(ul)) == [(0, "+", 0, "+"), (0, "-", 0, "-")]      # the closing record and its mirror
        assert got["support"].tolist() == [wraps, wraps] and got["n_crossings"] == wraps and got["n_links"] == 3000 - wraps


def test_a_list_without_records_and_a_range_without_windows():
    R = _mdbg()
    c = BY_NAME["presimp 200/1 at 0.01"]                                            # at presimp 0.01 the small branch's edges go: two unitigs, no record
    m, nodes, ul = built(R, c.reads, c.k, c.A, presimp=0.01)
    with m:
        got, _ = check(R, m, c.reads, c.k, nodes, ul)
        assert got["n_records"] == 0 and len(got["support"]) == 0 and got["n_crossings"] == got["n_missing_crossings"] == 1 and got["n_missing"] == 1
    c = BY_NAME["fork"]
    h = distinct_hashes(14, 3)
    reads = c.reads + [G.mread(h), G.mread([]), G.mread([])]                        # k minimizers give no window; two reads without a minimizer
    m, nodes, ul = built(R, reads, c.k, c.A)
    with m:
        whole, _ = check(R, m, reads, c.k, nodes, ul)
        for first, n_reads in ((7, 1), (7, 3), (8, 2)):                               # three indices and no window; no index at all
            got = m.graph_junctions(first, n_reads)
            assert got["n_records"] == 4 and got["support"].tolist() == [0] * 4 and got["n_reads"] == n_reads and got["first_read"] == first
            assert all(got[f] == 0 for f in SCALARS if f not in ("n_reads", "n_records"))
        assert_same(m.graph_junctions(0, 7), dict(whole, n_reads=7))


# ---- ranges --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 6])
def test_ranges_add_up_and_their_missing_lists_merge(seed):
    """the reads fed as two batches, split at 0, 1, the batch boundary, n - 1 and n (seed 6 has missing keys to merge)"""
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    n, cut = len(reads), 50
    m, nodes, ul = built(R, reads, k, A, split=cut, presimp=presimp)
    with m:
        whole, exp = check(R, m, reads, k, nodes, ul)
        parts = []
        for a, b in ((0, 1), (1, cut), (cut, n - 1), (n - 1, n)):
            got = m.graph_junctions(a, b - a)
            assert_same(got, shaped(R, expected(reads[a:b], k, nodes, ul), b - a, a))
            parts.append(got)
        assert np.array_equal(sum(p["support"] for p in parts), whole["support"])
        assert_same(R.api.merge_junctions(parts), whole)
        assert_zeros(R, m.graph_junctions(n, 0), n)
        assert_zeros(R, m.graph_junctions(n + 1, 3), n + 1)
        assert_same(m.graph_junctions(0, 1000), whole)
        if seed == 6:
            assert whole["n_missing"] == 64 and sum(p["n_missing"] for p in parts) > 64   # some key is missing in more than one range


# ---- state ---------------------------------------------------------------------------------------------------------------------------------------------------------
def state_error(m, *a):
    with pytest.raises(_mdbg().MdbgError) as e:
        m.graph_junctions(*a)
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
        assert "no current unitig list" in state_error(m)                           # after graph_edges
        ul = m.graph_unitigs()
        check(R, m, c.reads[:5], c.k, nodes, ul)
        keep = feed_batches(m, [(c.reads[5:], 5)])                                  # an ingest (and the insertion) ends the list
        state_error(m)
        nodes = m.finalize()
        state_error(m)                                                              # a finalize without a new unitig call
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        check(R, m, c.reads, c.k, nodes, ul)
        m.reset(c.k)                                                                # the store stays, the table and everything built on it go
        state_error(m)
        m.insert_resident()
        nodes = m.finalize()
        m.graph_edges(0.0)
        ul = m.graph_unitigs()
        check(R, m, c.reads, c.k, nodes, ul)
        del keep
    with R.Mdbg(c.k, G.L, G.D, c.A) as m:
        m.set_partition(2, 0)
        assert "single-GPU" in state_error(m)
        m.set_partition(1, 0)                                                       # the same context, unpartitioned again: it works
        feed(m, c.reads)
        nodes = m.finalize()
        m.graph_edges(0.0)
        check(R, m, c.reads, c.k, nodes, m.graph_unitigs())
        assert m.L.mdbg_graph_junctions(m.h, 0, 0, None) == m.L.mdbg_graph_junctions(None, 0, 0, None) == -1      # MDBG_E_PARAM: a null pointer
        assert m.L.mdbg_junctions_ms(m.h, None) == -1
    with R.Mdbg(3, G.L, G.D, 1) as m:                                               # an empty context: MDBG_OK and zeros
        m.finalize()
        m.graph_edges(0.0)
        m.graph_unitigs()
        assert_zeros(R, m.graph_junctions())
        assert_zeros(R, m.graph_junctions(5, 2), 5)
        assert m.junctions_ms() == 0.0


# ---- pipeline and the C program ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,l,d,A,with_records", [(7, 10, 0.0008, 2, False), (3, 10, 0.002, 1, True)])
def test_pipeline_files_and_the_c_program(example_reads, tmp_path, k, l, d, A, with_records):
    """tests/golden/reads-0.00.fa.gz at the example_cfg1 parameters, where the graph is ONE unitig without an edge record (the files hold no line), and at k = 3,
    where the unitig list has 178 records, 68 of them crossed by no read"""
    import subprocess
    from rust_mdbg_amd import pipeline
    R = _mdbg()
    src = os.path.join(GOLDEN, "reads-0.00.fa.gz")
    prefix = str(tmp_path / "jx")
    out = pipeline.run_file(src, prefix, k, l, d, A, write_sequences=False, contigs=True, keep_reads=True, simplify=R.api.MAGIC_SIMPLIFY_STEPS, junctions=True,
                            batch_bases=5_000_000)
    b, o = O.concat_reads(example_reads)
    with R.Mdbg(k, l, d, A) as m:
        m.ingest(b, o, 0)
        m.finalize()
        m.graph_edges(0.01)
        ul = m.graph_unitigs()
        plain = m.graph_junctions()                                                 # one call over the whole store
        sl = m.graph_simplify(R.api.MAGIC_SIMPLIFY_STEPS)
        simplified = m.graph_junctions()
    out0 = pipeline.run_file(src, prefix + "0", k, l, d, A, presimp=0.0, write_sequences=False, contigs=True, keep_reads=True, junctions=True, batch_bases=5_000_000)
    text0 = open(prefix + "0.unitigs.junctions.tsv").read()
    text = open(prefix + ".unitigs.junctions.tsv").read()
    assert text == R.api.junction_text(ul["edges"], plain["support"], plain, ul["circular"])
    assert open(prefix + ".msimpl.junctions.tsv").read() == R.api.junction_text(sl["edges"], simplified["support"], simplified, sl["circular"])
    gfa_links = [ln.split("\t") for ln in open(prefix + ".unitigs.gfa").read().split("\n") if ln.startswith("L\t")]
    tsv_links = [ln.split("\t") for ln in text.split("\n") if ln.startswith("L\t")]
    assert len(gfa_links) == len(tsv_links) == plain["n_records"] and all(a[:6] == b[:6] and len(b) == 7 for a, b in zip(gfa_links, tsv_links))
    assert (plain["n_records"] > 0) == with_records and (not with_records or 0 < out["n_junction_records_unsupported"] < plain["n_records"])
    assert [int(b[6]) for b in tsv_links] == plain["support"].tolist()
    assert len(text.split("\n")) - 1 == plain["n_records"] + plain["n_missing"]
    lines0 = text0.split("\n")[:-1]                                                  # presimp 0: every crossing has its record, the file has no X line
    assert len(lines0) == out0["n_junction_records"] and (len(lines0) > 0) == with_records and all(ln.startswith("L\t") for ln in lines0) and out0["n_missing_crossings"] == 0
    assert (out["n_junction_records"], out["n_junction_records_unsupported"], out["n_crossings"], out["n_missing_crossings"]) == (
        plain["n_records"], int((plain["support"] == 0).sum()), plain["n_crossings"], plain["n_missing_crossings"])
    assert (out["n_junction_records_simplified"], out["n_junction_records_unsupported_simplified"], out["n_crossings_simplified"], out["n_missing_crossings_simplified"]) == (
        simplified["n_records"], int((simplified["support"] == 0).sum()), simplified["n_crossings"], simplified["n_missing_crossings"])
    exe = str(tmp_path / "mdbg_cli")
    libdir = os.path.join(ROOT, "rust_mdbg_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mdbg_cli.c"),
                    "-L" + libdir, "-lmdbg_hip", "-lmdbg_emit", "-lpthread", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    r = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--prefix", str(tmp_path / "c"), "--no-basespace", "--junctions"],
                       check=True, capture_output=True, text=True)
    line = "junctions: %d records, %d crossed by no read, %d crossings, %d of them on no record" % (
        plain["n_records"], int((plain["support"] == 0).sum()), plain["n_crossings"], plain["n_missing_crossings"])
    assert line in r.stdout.split("\n") and os.path.exists(str(tmp_path / "c.unitigs.fa"))
