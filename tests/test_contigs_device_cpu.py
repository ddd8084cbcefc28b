"""CPU-side checks of the GPU contig stitching's boundary (no device needed): declarations, export lists, the ctypes mirror of mdbg_contig_seqs, the host
entry point that takes GPU-stitched sequences (mdbg_emit_contigs_set_sequences), and the C example."""
import os
import re
import subprocess

import numpy as np
import pytest

import unitig_restatement as U
from conftest import ROOT
from oracle import oracle as O
from test_unitigs_cpu import emit_case, plan_of


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_new_symbols_are_declared_exported_and_listed():
    from rust_mdbg_amd import api, emit
    h = header("mdbg_hip.h")
    assert re.search(r"#define\s+MDBG_FLAG_KEEP_READS\s+2u", h) and api.FLAG_KEEP_READS == 2
    L = api.load_library()
    for s in ("mdbg_graph_contigs", "mdbg_graph_contigs_device", "mdbg_kept_reads"):
        assert re.search(r"\b%s\s*\(" % s, h) and s in api.EXPORTS and hasattr(L, s), s
    assert re.search(r"\bmdbg_emit_contigs_set_sequences\s*\(", header("mdbg_emit.h")) and "mdbg_emit_contigs_set_sequences" in emit.EXPORTS
    assert hasattr(emit.load_library(), "mdbg_emit_contigs_set_sequences")
    assert L.mdbg_abi_version() == 3                                   # an addition: the ABI version stays
    import inspect
    for fn, arg in ((api.Mdbg.__init__, "keep_reads"), (api.Mdbg.graph_contigs, "min_len"), (api.Mdbg.graph_contigs, "device")):
        assert arg in inspect.signature(fn).parameters
    from rust_mdbg_amd import pipeline
    for fn in (pipeline.run_file, pipeline.run_multik):
        assert inspect.signature(fn).parameters["keep_reads"].default is False
    assert callable(api.Mdbg.kept_reads)


def test_set_sequences_fills_a_handle_like_add_batch(tmp_path):
    from rust_mdbg_amd import emit as E
    reads, nodes, u = emit_case()
    plan = plan_of(u, nodes)
    b, o = O.concat_reads(reads)
    g1, f1, g2, f2 = (str(tmp_path / x) for x in ("a.gfa", "a.fa", "b.gfa", "b.fa"))
    with E.Emitter().contigs(plan, [(b, o, 0)], g1, f1) as c:
        seqs = c.sequences()
    assert [s.decode() for s in seqs] == u["seqs"] and len(seqs) > 3
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    with E.Contigs(plan) as c:
        with pytest.raises(E.MdbgError) as ei:                         # nothing filled yet
            c.write_gfa(g2)
        assert ei.value.code == -6
        wrong = offs.copy()
        wrong[1] += 1                                                  # one length off (the total still fits)
        for bad_b, bad_o in ((bases, offs[:-1]), (bases, wrong), (bases, np.concatenate([offs, offs[-1:]])), (bases, offs + np.uint64(1))):
            with pytest.raises(E.MdbgError) as ei:
                c.set_sequences(bad_b, bad_o)
            assert ei.value.code == -1
        with pytest.raises(E.MdbgError):                               # a rejected call fills nothing
            c.sequences()
        c.set_sequences(bases, offs)
        assert c.sequences() == seqs
        c.write_gfa(g2)
        c.write_fasta(f2)
    assert open(g1, "rb").read() == open(g2, "rb").read() == U.gfa_text(u).encode()
    assert open(f1, "rb").read() == open(f2, "rb").read() == U.fasta_text(u).encode()


def test_cli_example_is_pedantic_c99_and_knows_the_flag(tmp_path):
    lib = os.path.join(ROOT, "rust_mdbg_amd")
    exe = str(tmp_path / "mdbg_cli")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mdbg_cli.c"), "-L" + lib, "-lmdbg_hip", "-lmdbg_emit", "-lpthread", "-Wl,-rpath," + lib, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--keep-reads" in r.stderr
    src = open(os.path.join(ROOT, "examples", "mdbg_cli.c")).read()
    assert "MDBG_FLAG_KEEP_READS" in src and "mdbg_graph_contigs" in src and "mdbg_emit_contigs_set_sequences" in src
