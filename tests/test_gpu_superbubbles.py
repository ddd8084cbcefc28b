"""The SUPERBUBBLES step on the GPU (MDBG_SIMPLIFY_SUPERBUBBLES of Mdbg.graph_simplify, csrc/superbubbles.hip) against the plain restatement
(tests/superbubble_restatement.py), list for list from the host and the device variant: the removed nodes and the counts per step, the walks, offsets, length,
kc_sum, circular, the edge columns and the executed copy plan — on the hand-built catalogue of tests/superbubble_graphs.py with its hand-written removed sets, on
the random family, in a schedule with EDGES and REPEATS steps (by invariants), in base space, and once more under MDBG_GUARD.  CPU side: tests/test_superbubbles_cpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sketch_graphs as G
import superbubble_graphs as SG
import superbubble_restatement as SR
import transit_graphs as TG
import unitig_restatement as U
from conftest import ROOT
from test_gpu_components import check_components
from test_gpu_parity import _mdbg
from test_gpu_read_paths import built
from test_gpu_repeats import device_list, walks_of
from test_gpu_simplify import same_list
from test_repeats_cpu import BASE_PARAMS, pieces_of, tiled_reads
from test_superbubbles_cpu import RANDOM_SEEDS, braid_genomes

pytestmark = pytest.mark.gpu

TIPS, BUBBLES, SUPERBUBBLES, EDGES, REPEATS = 1, 2, 64, 8, 16
SB = (SUPERBUBBLES, 0, 0)
E_PARAM = -1


def edge_rows(got):
    e = got["edges"]
    return list(zip(e["n1"].tolist(), (chr(c) for c in e["o1"]), e["n2"].tolist(), (chr(c) for c in e["o2"]), e["overlap"].tolist()))


def assert_equals_restatement(got, nodes, edges, steps, strings):
    """-> (log, expected unitigs)"""
    log, exp = SR.simplify(nodes, edges, steps, strings, None if strings is not None else G.length_of_walk(nodes))
    st = got["stats"]
    print("removed per step (unitigs, nodes):", list(zip(st["unitigs_removed"], st["nodes_removed"])), "compactions", st["n_compactions"], "syncs", st["n_syncs"])
    assert st["unitigs_removed"] == [len(x["unitigs"]) for x in log] and st["nodes_removed"] == [len(x["nodes"]) for x in log]
    assert st["total_unitigs_removed"] == sum(st["unitigs_removed"]) and st["total_nodes_removed"] == sum(st["nodes_removed"]) and st["edges_removed"] == [0] * len(steps)
    assert st["n_compactions"] == 1 + sum(1 for x in log if x["nodes"])             # a compaction follows iff something was removed
    walks = walks_of(got)
    assert walks == exp["walks"]
    assert sorted(got["node"].tolist()) == sorted(set(nodes["index"].tolist()) - {n for x in log for n in x["nodes"]})      # the removed sets
    assert got["offsets"].tolist() == np.cumsum([0] + [len(w) for w in walks]).tolist()
    assert got["circular"].astype(bool).tolist() == exp["circular"] and got["kc_sum"].tolist() == exp["kc_sum"] and got["length"].tolist() == exp["length"]
    assert got["n_unitigs"] == len(walks) and got["n_entries"] == len(nodes["index"]) - st["total_nodes_removed"]
    assert edge_rows(got) == exp["edges"]
    if strings is not None:
        from oracle import oracle as O
        from rust_mdbg_amd import emit as E
        with E.Contigs(got) as c:
            c.add_batch(*O.concat_reads(strings), 0)
            assert [s.decode("latin-1") for s in c.sequences()] == exp["seqs"]
    return log, exp


def check(R, m, nodes, edges, steps, strings=None):
    """the schedule on the context: host variant twice and device variant, all against the restatement -> (got, log, exp)"""
    got, again, dev = m.graph_simplify(steps), m.graph_simplify(steps), device_list(R, m, steps)
    assert got["stats"] == again["stats"] == dev["stats"]
    same_list(got, again, R)                                                        # two calls give identical arrays
    same_list(got, dev, R)
    log, exp = assert_equals_restatement(got, nodes, edges, steps, strings)
    return got, log, exp


def run_catalogue_case(R, name):
    c = SG.BY_NAME[name]
    m, nodes, ul = built(R, c.reads, c.k, c.A)
    strings = G.fake_bases(c.reads, G.L, 1)
    with m:
        edges = m.graph_edges(0.0)
        for steps in c.schedules:
            got, log, exp = check(R, m, nodes, edges, steps, strings)
            want = c.expect.get("removed", {}).get(tuple(steps))
            if want is not None:
                assert [sorted(x["nodes"]) for x in log] == want
                assert sorted(got["node"].tolist()) == sorted(set(nodes["index"].tolist()) - {n for x in want for n in x})
            check_components(R, m, exp)                                             # the simplified list is the current one
        same_list(m.graph_unitigs(), ul, R)                                         # and the plain list is what it was


@pytest.mark.parametrize("name", SG.CASE_IDS)
def test_catalogue(name):
    run_catalogue_case(_mdbg(), name)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)                                  # all 40; 21 of them hold a bubble only this step pops (BRANCHING)
def test_random_family(seed):
    R = _mdbg()
    reads = SG.random_braids(seed)
    m, nodes, ul = built(R, reads, SG.K, SG.A, len(reads) // 2)
    with m:
        edges = m.graph_edges(0.0)
        for steps in ([SB], [(TIPS, 0, 0), SB, (BUBBLES, 0, 0), SB], [(SUPERBUBBLES, 12, 0), SB]):
            check(R, m, nodes, edges, steps, G.fake_bases(reads, G.L, seed))


def test_dense_random_graphs():
    """the dense graphs of tests/sketch_graphs.py (hubs, palindromes, repeats): candidates everywhere, hardly a bubble — no defect, and the restatement's lists"""
    R = _mdbg()
    for seed in (1, 4):
        k, A, presimp, reads = G.random_case(seed)
        m, nodes, ul = built(R, reads, k, A, len(reads) // 3, presimp)
        with m:
            check(R, m, nodes, m.graph_edges(presimp), [SB, (TIPS, 3, 0), SB], G.fake_bases(reads, G.L, seed))


def test_a_schedule_with_edges_and_repeats_steps():
    """a braid beside a repeat the reads resolve: by invariants (the restatements of the REPEATS step and of this one do not know each other)"""
    R = _mdbg()
    braid = SG.BY_NAME["braid"].reads                                               # fed first: its nodes are 0 .. 17, the step removes 12 .. 17
    cross = TG.cross_reads(703, 8)[0]
    reads = braid + cross
    steps = [(EDGES, 1, 0), (REPEATS, 1, 0), SB, (TIPS, 0, 0)]
    m, nodes, ul = built(R, reads, 3, 1, len(braid))
    with m:
        m.graph_edges(0.0)
        got, again = m.graph_simplify(steps), m.graph_simplify(steps)
        same_list(got, again, R)
        st = got["stats"]
        assert st == again["stats"] and st["entries_copied"] > 0 and st["unitigs_removed"][2] == 2 and st["nodes_removed"][2] == 6
        assert got["n_entries"] == len(nodes["index"]) - st["total_nodes_removed"] + st["entries_copied"]      # the n_entries identity
        walks = walks_of(got)
        rows = [[n for n, _ in w] for w in walks]
        assert list(range(12)) in rows or list(range(11, -1, -1)) in rows           # no dead end at s or t: source, kept path and sink are one unitig again
        assert not ({n for w in walks for n, _ in w} & set(range(12, 18)))
        alone = m.graph_simplify(steps[:2] + steps[3:])                             # without the step the braid stays: seven unitigs where one is left
        assert alone["n_unitigs"] == got["n_unitigs"] + 6 and alone["stats"]["entries_copied"] == st["entries_copied"]
        cur = dict(walks=walks, edges=edge_rows(got), length=got["length"].tolist(), kc_sum=got["kc_sum"].tolist(), circular=got["circular"].astype(bool).tolist())
        m.graph_simplify(steps)
        check_components(R, m, cur)
        from oracle import oracle as O
        from rust_mdbg_amd import emit as E
        with E.Contigs(got) as c:
            c.add_batch(*O.concat_reads(G.fake_bases(reads, G.L, 1)), 0)
            assert [len(s) for s in c.sequences()] == got["length"].tolist()


def test_kind_32_is_still_refused_and_the_step_takes_any_limits():
    R = _mdbg()
    c = SG.BY_NAME["braid"]
    m, nodes, ul = built(R, c.reads, c.k, c.A)
    with m:
        for bad in ([(32, 1, 0)], [SB, (32, 0, 0)], [(96, 0, 0)]):
            with pytest.raises(R.MdbgError) as e:
                m.graph_simplify(bad)
            assert e.value.code == E_PARAM
        assert m.graph_simplify([SB])["stats"]["nodes_removed"] == [6]
    with R.Mdbg(3, G.L, G.D, 2) as m:                                              # an empty context: the empty list, no error
        assert m.graph_simplify([SB])["n_unitigs"] == 0


def test_magic_superbubble_steps_give_one_contig_in_base_space(tmp_path):
    """an error-free genome at high coverage and two variants at low coverage whose differences lie less than k minimizers apart: MAGIC_SIMPLIFY_STEPS leaves the
    braid, MAGIC_SUPERBUBBLE_STEPS one contig that is an exact piece of the genome — through the library, run_file and the C program's -B"""
    from oracle import oracle as O
    from rust_mdbg_amd import api, pipeline
    from test_gpu_unitigs import build_cli, read_fasta
    R = _mdbg()
    k, l, d, A = BASE_PARAMS
    genome, h1, h2 = braid_genomes()
    reads = tiled_reads(genome) + tiled_reads(h1, step=1000) + tiled_reads(h2, step=1000)
    b, o = O.concat_reads(reads)
    with R.Mdbg(k, l, d, A, reads_already_hpc=True, keep_reads=True) as m:
        m.ingest(b, o, 0)
        nodes = m.finalize()
        edges = m.graph_edges(0.0)
        plain = m.graph_simplify(api.MAGIC_SIMPLIFY_STEPS)
        assert plain["n_unitigs"] >= 5 and plain["stats"]["total_nodes_removed"] == 0
        got, log, exp = check(R, m, nodes, edges, api.MAGIC_SUPERBUBBLE_STEPS, reads)
        assert got["n_unitigs"] == 1 and pieces_of(genome, exp["seqs"]) and len(exp["seqs"][0]) > int(plain["length"].max())
        ctg = m.graph_contigs(0)
        offs = ctg["offsets"].tolist()
        assert [bytes(ctg["bases"][x:y]).decode("latin-1") for x, y in zip(offs, offs[1:])] == exp["seqs"]
    src = str(tmp_path / "reads.fa")
    with open(src, "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, r.decode()) for i, r in enumerate(reads)))
    pre = str(tmp_path / "p")
    res = pipeline.run_file(src, pre, k, l, d, A, reads_already_hpc=True, contigs=True, simplify=[(SUPERBUBBLES, 0, 100000)])
    assert open(pre + ".msimpl.fa").read() == U.fasta_text(exp) and res["n_simplified"] == 1
    exe = build_cli(tmp_path)
    cpre = str(tmp_path / "c")
    out = subprocess.run([exe, src, "-k", str(k), "-l", str(l), "--density", str(d), "--minabund", str(A), "--skiphpc", "-B", "0,100000", "--prefix", cpre],
                         check=True, capture_output=True, text=True).stdout
    assert "simplify step 1 (superbubbles 0,100000): %d unitigs, %d nodes removed\n" % (res["simplify"]["unitigs_removed"][0], res["simplify"]["nodes_removed"][0]) in out
    assert open(pre + ".msimpl.fa", "rb").read() == open(cpre + ".msimpl.fa", "rb").read()
    names, cseqs = read_fasta(cpre + ".msimpl.fa")
    assert len(cseqs) == 1 and pieces_of(genome, cseqs)
    # the k sweep's built-in producer: the contigs of round k are what round k + 1 is fed
    multi = pipeline.run_multik(src, str(tmp_path / "mk"), [k, k + 1], l, d, A, reads_already_hpc=True, contigs_fn="simplified", min_contig_len=300,
                                simplify_steps=api.MAGIC_SUPERBUBBLE_STEPS)
    usual = pipeline.run_multik(src, str(tmp_path / "mu"), [k, k + 1], l, d, A, reads_already_hpc=True, contigs_fn="simplified", min_contig_len=300)
    assert multi[k + 1]["n_contigs"] == 1 < usual[k + 1]["n_contigs"]


# ---- under MDBG_GUARD: no kernel of the step writes outside its blocks -------------------------------------------------------------------------------------------
GUARD_LINE = re.compile(r"^GUARD_OK calls=(\d+) blocks=(\d+) bytes=(\d+)$", re.M)


def child_main():
    import rust_mdbg_amd as R
    from rust_mdbg_amd import api
    assert api.GUARD and api.load_library().mdbg_guard_selftest() == 0
    print("SELFTEST_OK", flush=True)
    for name in SG.CASE_IDS:
        run_catalogue_case(R, name)
    api.guard_check()
    print("GUARD_OK calls=%d blocks=%d bytes=%d" % (api.GUARD_SEEN["calls"], api.GUARD_SEEN["blocks"], api.GUARD_SEEN["bytes"]))


def test_catalogue_under_guard():
    base = {k: v for k, v in os.environ.items() if k not in ("MDBG_GUARD", "MDBG_POISON")}
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_superbubbles as T; T.child_main()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(base, MDBG_GUARD="1"), timeout=600)
    print(r.stdout[-2500:])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    got = GUARD_LINE.search(r.stdout)
    assert got is not None and r.stdout.startswith("SELFTEST_OK\n"), (r.stdout[-1500:], r.stderr[-3000:])
    assert all(int(x) > 0 for x in got.groups()), got.group(0)
