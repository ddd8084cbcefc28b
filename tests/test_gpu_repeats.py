"""The REPEATS step on the GPU (MDBG_SIMPLIFY_REPEATS of Mdbg.graph_simplify, csrc/repeats.hip) against the plain restatement (tests/repeats_restatement.py),
array for array from the host and the device variant: walks (node[] names the originals), offsets, length, kc_sum, circular, the edge columns and the counts —
on the hand-built repeats of tests/transit_graphs.py at every min_support they were written for, many crosses side by side, the random graphs, a schedule of
all five kinds; the step's invariants on every result; the state round the step (the refusals, a list with copies, a held transit result, components and
contigs on the copied list); base space through the library, run_file and the C program; and the hand-built cases once more under MDBG_GUARD.
CPU side: tests/test_repeats_cpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import repeats_restatement as RR
import sketch_graphs as G
import transit_graphs as TG
import unitig_restatement as U
from conftest import ROOT
from test_gpu_components import check_components
from test_gpu_parity import _mdbg
from test_gpu_read_paths import built
from test_gpu_simplify import same_list
from test_gpu_unitigs import build_cli, read_fasta
from test_read_paths_cpu import hashes
from test_repeats_cpu import BASE_PARAMS, HAND, MIXED, RANDOM, REFUSED, base_space_hashes, check_invariants, genome_with_repeat, pieces_of, tiled_reads

pytestmark = pytest.mark.gpu

TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS = RR.TIPS, RR.BUBBLES, RR.COMPONENTS, RR.EDGES, RR.REPEATS
E_PARAM, E_STATE = -1, -6


def walks_of(got):
    off = got["offsets"].tolist()
    return [list(zip(got["node"][a:b].tolist(), (chr(c) for c in got["ori"][a:b]))) for a, b in zip(off, off[1:])]


def device_list(R, m, steps):
    """graph_simplify_device -> the dict graph_simplify gives, every array copied back"""
    u, stats = m.graph_simplify_device(steps)
    cnt = R.api.unitig_counts(u)
    addr = lambda p: R.api.C.cast(p, R.api.C.c_void_p).value
    out = {f: m.to_host(addr(getattr(u, f)), cnt[f] * np.dtype(t).itemsize, t) if cnt[f] else np.zeros(0, t) for f, t in R.api.UNITIG_FIELDS}
    n = int(u.edges.n)
    out["edges"] = {f: m.to_host(addr(getattr(u.edges, f)), n * np.dtype(t).itemsize, t) if n else np.zeros(0, t) for f, t in R.api.EDGE_FIELDS}
    out.update(n_unitigs=int(u.n_unitigs), n_entries=int(u.n_entries), stats=stats)
    return out


def assert_equals_checker(got, log, exp, nodes, strings=None):
    st = got["stats"]
    print("copied", st["entries_copied"], "removed per step (unitigs, nodes, edge records):", list(zip(st["unitigs_removed"], st["nodes_removed"], st["edges_removed"])),
          "compactions", st["n_compactions"], "syncs", st["n_syncs"])
    assert st["unitigs_removed"] == [len(x["unitigs"]) for x in log] and st["nodes_removed"] == [len(x["nodes"]) for x in log] and st["edges_removed"] == [x["edges"] for x in log]
    assert st["entries_copied"] == exp["copies"] == sum(x.get("copies", 0) for x in log)
    walks = walks_of(got)
    assert walks == exp["walks_original"]                                           # node[] reports the ORIGINAL's index
    assert got["offsets"].tolist() == np.cumsum([0] + [len(w) for w in walks]).tolist()
    assert got["circular"].astype(bool).tolist() == exp["circular"] and got["kc_sum"].tolist() == exp["kc_sum"] and got["length"].tolist() == exp["length"]
    assert got["n_unitigs"] == len(walks) and got["n_entries"] == len(nodes["index"]) - st["total_nodes_removed"] + st["entries_copied"]      # the n_entries identity
    e = got["edges"]
    assert list(zip(e["n1"].tolist(), (chr(c) for c in e["o1"]), e["n2"].tolist(), (chr(c) for c in e["o2"]), e["overlap"].tolist())) == exp["edges"]
    if strings is not None:                                                          # the copy plan executed == the restatement's stitch of the walks
        from oracle import oracle as O
        from rust_mdbg_amd import emit as E
        with E.Contigs(got) as c:
            c.add_batch(*O.concat_reads(strings), 0)
            assert [s.decode("latin-1") for s in c.sequences()] == exp["seqs"]


def check(R, m, nodes, edges, reads, k, steps, strings=None):
    """the schedule on the context: host variant twice and device variant, all against the checker, and the invariants -> (got, log, exp)"""
    got, again, dev = m.graph_simplify(steps), m.graph_simplify(steps), device_list(R, m, steps)
    assert got["stats"] == again["stats"] == dev["stats"]
    same_list(got, again, R)                                                        # two calls give identical arrays
    same_list(got, dev, R)
    log, exp = RR.simplify(nodes, edges, steps, hashes(reads), k, strings, None if strings is not None else G.length_of_walk(nodes))
    assert_equals_checker(got, log, exp, nodes, strings)
    check_invariants(nodes, edges, log, dict(walks_original=walks_of(got), kc_sum=got["kc_sum"].tolist()))
    assert got["stats"]["n_compactions"] >= (2 if exp["copies"] else 1)
    return got, log, exp


# ---- the hand-built repeats --------------------------------------------------------------------------------------------------------------------------------------
HAND_PARAMS = [(c.name, ms) for c in TG.CASES for ms in sorted(c.expect["resolved"])]


def run_hand_case(R, name, ms):
    c = TG.BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        edges = m.graph_edges(c.presimp)
        steps = (c.steps or []) + [(REPEATS, ms, 0)]
        got, log, exp = check(R, m, nodes, edges, c.reads, c.k, steps, G.fake_bases(c.reads, G.L, 1))
        resolved = c.expect["resolved"][ms]
        assert len(log[-1]["resolved"]) == resolved and (got["stats"]["entries_copied"] > 0) == (resolved > 0)
        assert got["stats"]["n_compactions"] == 1 + (1 if resolved else 0) + (1 if c.steps and log[0]["edges"] else 0)      # a compaction follows iff the step copied something
        if (name, ms) in HAND:
            copies, left, records = HAND[(name, ms)]
            assert (got["stats"]["entries_copied"], sorted(np.diff(got["offsets"].astype(np.int64)).tolist()), len(got["edges"]["n1"])) == (copies, left, records)
        if name == "long" and resolved:                                             # more than 4096 entries in one copied unitig
            assert got["stats"]["entries_copied"] == 4998 > 4096
        same_list(m.graph_unitigs(), ul, R)                                         # the plain list is what it was
        return got


@pytest.mark.parametrize("name,ms", HAND_PARAMS)
def test_hand_built_repeats(name, ms):
    run_hand_case(_mdbg(), name, ms)


@pytest.mark.parametrize("n,split", [(300, None), (1100, 700)])
def test_many_crosses_side_by_side(n, split):
    """300: more than one workgroup of resolved unitigs; 1100 in two batches: more strong rows than one block of the sort holds"""
    R = _mdbg()
    reads = TG.many_crosses(n)
    m, nodes, ul = built(R, reads, 3, 1, split=split)
    with m:
        got, log, exp = check(R, m, nodes, m.graph_edges(0.0), reads, 3, [(REPEATS, 1, 0)])
        assert (ul["n_unitigs"], got["stats"]["entries_copied"], got["n_unitigs"], set(np.diff(got["offsets"].astype(np.int64)).tolist())) == (5 * n, n, 2 * n, {9})
        assert len(got["edges"]["n1"]) == 0 and 2 * n > (256 if split is None else 2048)
        assert m.graph_simplify([(REPEATS, 2, 0)])["stats"]["entries_copied"] == 0


# ---- the random graphs ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 4, 7, 2])
def test_random_graphs(seed):
    R = _mdbg()
    k, A, presimp, reads = G.random_case(seed)
    m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
    with m:
        edges = m.graph_edges(presimp)
        got, log, exp = check(R, m, nodes, edges, reads, k, [(REPEATS, 1, 0)], G.fake_bases(reads, G.L, seed))
        if seed in RANDOM:
            assert (got["stats"]["entries_copied"], ul["n_unitigs"], got["n_unitigs"], ul["n_entries"], got["n_entries"], len(ul["edges"]["n1"]), len(got["edges"]["n1"])) == RANDOM[seed]
        else:                                                                       # nothing resolves: the schedule without the step, array for array, and as many compactions
            plain = m.graph_simplify([])
            same_list(got, plain, R)
            same_list(got, ul, R)
            assert got["stats"]["entries_copied"] == 0 and got["stats"]["n_compactions"] == plain["stats"]["n_compactions"] == 1
            both, alone = m.graph_simplify([(REPEATS, 1, 0), (TIPS, 3, 0), (BUBBLES, 0, 0)]), m.graph_simplify([(TIPS, 3, 0), (BUBBLES, 0, 0)])
            same_list(both, alone, R)
            assert both["stats"]["n_compactions"] == alone["stats"]["n_compactions"] and both["stats"]["nodes_removed"][1:] == alone["stats"]["nodes_removed"]


def test_a_schedule_of_all_five_kinds():
    R = _mdbg()
    k, A, presimp, reads = G.random_case(4)
    m, nodes, ul = built(R, reads, k, A, 40, presimp)
    with m:
        got, log, exp = check(R, m, nodes, m.graph_edges(presimp), reads, k, MIXED, G.fake_bases(reads, G.L, 4))
        assert log[0]["edges"] > 0 and got["stats"]["entries_copied"] > 0 and got["stats"]["total_nodes_removed"] > 0
        check_components(R, m, exp)


# ---- state ----------------------------------------------------------------------------------------------------------------------------------------------------------
def refused(call, code):
    with pytest.raises(_mdbg().MdbgError) as e:
        call()
    assert e.value.code == code
    return str(e.value)


def test_refused_schedules_and_a_list_that_holds_copies():
    R = _mdbg()
    c = TG.BY_NAME["cross r=8"]
    H = hashes(c.reads)
    m, nodes, ul = built(R, c.reads, c.k, c.A, c.split, c.presimp)
    with m:
        for bad in REFUSED + ([(32, 1, 0)],):                                       # refused while the schedule is validated; the plain list stays current
            refused(lambda: m.graph_simplify(bad), E_PARAM)
            assert m.graph_transits()["n_resolved"] == 1
        m.graph_simplify([(EDGES, 1, 0), (REPEATS, 1, 0), (TIPS, 0, 0)])            # an EDGES step IN FRONT of the REPEATS step is fine
        m.graph_unitigs()
        held = m.graph_transits_device(0, 0, 4)                                     # a transit result the caller holds: nothing resolves at 4
        addr = R.api.C.cast(held.verdict, R.api.C.c_void_p).value
        before = m.to_host(addr, int(held.n_unitigs))
        assert int(held.n_resolved) == 0 and R.api.TRANSIT_RESOLVED not in before.tolist()
        none = m.graph_simplify([(REPEATS, 4, 0)])                                  # a REPEATS step that copied nothing: the list is placed as always
        assert none["stats"]["entries_copied"] == 0 and m.graph_transits()["n_resolved"] == 1 and m.graph_read_paths()["n_reads"] == len(H) and m.graph_junctions()["n_records"] == 8
        got = m.graph_simplify([(REPEATS, 1, 0)])
        assert got["stats"]["entries_copied"] == 6 and m.transits_ms() > 0.0        # the device time of the step's transit stage
        assert R.api.TRANSIT_RESOLVED in m.to_host(addr, int(held.n_unitigs)).tolist()      # the held result has ended: the step's own verdicts stand in its place
        for call in (m.graph_read_paths, m.graph_junctions, m.graph_transits, m.graph_read_paths_device, m.graph_junctions_device, m.graph_transits_device):
            assert "copies" in refused(call, E_STATE)
        log, exp = RR.simplify(nodes, m.graph_edges(c.presimp), [(REPEATS, 1, 0)], H, c.k, None, G.length_of_walk(nodes))
        refused(m.graph_transits, E_STATE)                                          # (the edge call ended the list)
        got = m.graph_simplify([(REPEATS, 1, 0)])
        check_components(R, m, exp)                                                 # components read the list, not the table
        same_list(m.graph_unitigs(), ul, R)                                         # the context is usable: the plain list again, and the reads are placed on it
        assert m.graph_transits()["n_resolved"] == 1 and m.graph_read_paths()["n_reads"] == len(H)
    with R.Mdbg(3, G.L, G.D, 1) as m:                                               # an empty context: the empty list, no error
        got = m.graph_simplify([(REPEATS, 1, 0)])
        assert got["n_unitigs"] == 0 and got["stats"]["entries_copied"] == 0


# ---- base space -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_contigs_cross_the_repeat_in_base_space(tmp_path):
    """an error-free genome with one two-copy repeat of 1,000 bases, reads of 3,000: the plain list has four unitigs, after [(REPEATS, 2, 0)] one contig that is an
    exact piece of the genome — from graph_contigs on the kept reads, through run_file, and through the C program's -r 2"""
    from oracle import oracle as O
    from rust_mdbg_amd import pipeline
    R = _mdbg()
    k, l, d, A = BASE_PARAMS
    genome = genome_with_repeat(1)
    reads = tiled_reads(genome)
    b, o, H = base_space_hashes(reads)
    steps = [(REPEATS, 2, 0)]
    with R.Mdbg(k, l, d, A, reads_already_hpc=True, keep_reads=True) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        edges = m.graph_edges(0.0)
        ul = m.graph_unitigs()
        got, log, exp = check(R, m, nodes, edges, [(tuple(h), ()) for h in H], k, steps, reads)
        ctg = m.graph_contigs(0)
        offs = ctg["offsets"].tolist()
        seqs = [bytes(ctg["bases"][x:y]).decode("latin-1") for x, y in zip(offs, offs[1:])]
        assert seqs == exp["seqs"] and pieces_of(genome, seqs) and len(seqs) == 1 < ul["n_unitigs"] == 4
        assert len(seqs[0]) > int(ul["length"].max()) + 2000
        check_components(R, m, exp)
    src = str(tmp_path / "reads.fa")
    with open(src, "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, r.decode()) for i, r in enumerate(reads)))
    pre = str(tmp_path / "p")
    res = pipeline.run_file(src, pre, k, l, d, A, reads_already_hpc=True, contigs=True, simplify=steps, read_paths=True, junctions=True, transits=2)
    assert open(pre + ".msimpl.fa").read() == U.fasta_text(exp) and open(pre + ".msimpl.gfa").read() == U.gfa_text(exp)
    assert res["simplify"]["entries_copied"] == exp["copies"] > 0 and res["n_simplified"] == 1 < res["n_unitigs"] == 4 and res["simplified_read_evidence_written"] is False
    for kind in ("read_paths", "junctions", "transits"):                            # written for the plain list as always, not for the list with copies
        assert os.path.exists("%s.unitigs.%s.tsv" % (pre, kind)) and not os.path.exists("%s.msimpl.%s.tsv" % (pre, kind))
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "c")
    out = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--skiphpc", "-r", "2", "--contigs", "--transits", "2", "--prefix", cpre],
                         check=True, capture_output=True, text=True).stdout
    assert "simplify step 1 (repeats 2)\n" in out and "simplify: %d entries copied\n" % exp["copies"] in out
    for ext in (".msimpl.gfa", ".msimpl.fa", ".unitigs.gfa", ".unitigs.transits.tsv"):
        assert open(pre + ext, "rb").read() == open(cpre + ext, "rb").read(), ext
    assert not os.path.exists(cpre + ".msimpl.transits.tsv")
    names, cseqs = read_fasta(cpre + ".msimpl.fa")
    assert len(cseqs) == 1 and pieces_of(genome, cseqs)


# ---- under MDBG_GUARD: no kernel of the step writes outside its blocks -------------------------------------------------------------------------------------------------
GUARD_LINE = re.compile(r"^GUARD_OK calls=(\d+) blocks=(\d+) bytes=(\d+)$", re.M)


def child_main():
    import rust_mdbg_amd as R
    from rust_mdbg_amd import api
    assert api.GUARD and api.load_library().mdbg_guard_selftest() == 0
    print("SELFTEST_OK", flush=True)
    for name, ms in HAND_PARAMS:
        if name != "long" or ms == 1:
            run_hand_case(R, name, ms)
    api.guard_check()
    print("GUARD_OK calls=%d blocks=%d bytes=%d" % (api.GUARD_SEEN["calls"], api.GUARD_SEEN["blocks"], api.GUARD_SEEN["bytes"]))


def test_hand_built_repeats_under_guard():
    base = {k: v for k, v in os.environ.items() if k not in ("MDBG_GUARD", "MDBG_POISON")}
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_repeats as T; T.child_main()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(base, MDBG_GUARD="1"), timeout=600)
    print(r.stdout[-2500:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = GUARD_LINE.search(r.stdout)
    assert got is not None and r.stdout.startswith("SELFTEST_OK\n"), (r.stdout[-1500:], r.stderr[-3000:])
    assert all(int(x) > 0 for x in got.groups()), got.group(0)
