"""The host half of ".sequences from the kept reads", without a GPU: mdbg_seqfile_write_nodes (ready, already oriented sequences in, lines out) against
the writer that exists without it, mdbg_seqfile_write_batch[_part] over the reads; and the new keyword arguments and the CLI flag.  The sequences fed here are
built in plain Python from the oracle's node table (slice, then reversed through the switch_base map of src/utils.rs:10-24).  The GPU half is
tests/test_gpu_node_seqs.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O
from rust_mdbg_amd import emit as E
from test_unitigs_cpu import fuzz_case, oracle_graph

SWITCH = dict(zip(b"acgtuACGTU", b"tgcaaTGCAA"))      # every other byte -> N


def oriented(reads, nodes, i):
    """the sequence field of row i, by the host rule"""
    s = reads[int(nodes["src_read"][i])][int(nodes["src_start"][i]):int(nodes["src_end"][i])]
    return bytes(SWITCH.get(c, ord("N")) for c in reversed(s)) if nodes["reversed"][i] else s


def write_nodes(path, nt, l, chunks, part=0, n_parts=1):
    """chunks: [(first_row, [sequence, ...])] -> the return code of the first failing mdbg_seqfile_write_nodes call (0: none failed)"""
    L = E.load_library()
    err = C.c_int()
    f = L.mdbg_seqfile_open(path.encode(), nt.c.k, l, C.byref(err))
    assert f, err.value
    rc = 0
    try:
        for first, seqs in chunks:
            bases, offs = O.concat_reads(seqs)
            bases = np.concatenate([bases, np.zeros(1, np.uint8)])      # (never an empty buffer's null pointer)
            rc = L.mdbg_seqfile_write_nodes(f, C.byref(nt.c), part, n_parts, first, len(seqs), bases.ctypes.data, offs.ctypes.data)
            if rc:
                break
    finally:
        assert L.mdbg_seqfile_close(f) == 0
    return rc


@pytest.mark.parametrize("seed,hpc", [(1, False), (1, True), (3, False), (3, True)], ids=lambda v: str(v))
def test_write_nodes_equals_the_batch_writer(seed, hpc, tmp_path):
    """hpc here = reads_already_hpc (True: homopolymer compression off)"""
    k, l, d, A, reads = fuzz_case(seed)
    nodes, _ = oracle_graph(reads, k, l, d, A, 0.01, hpc=hpc)
    n = int(nodes["n_nodes"])
    assert n > 20 and 0 < int(np.count_nonzero(nodes["reversed"])) < n
    seqs = [oriented(reads, nodes, i) for i in range(n)]
    b, o = O.concat_reads(reads)
    em, nt = E.Emitter(), E.NodeTable(nodes)
    want = str(tmp_path / "want.0.sequences")
    em.write_sequences(want, nodes, l, [(b, o, 0)])
    want = open(want, "rb").read()
    for step in (n, 1, 7):
        p = str(tmp_path / ("got%d.0.sequences" % step))
        assert write_nodes(p, nt, l, [(f, seqs[f:f + step]) for f in range(0, n, step)]) == 0
        assert open(p, "rb").read() == want, step
    parts = em.write_sequences_parallel(str(tmp_path / "par"), nodes, l, [(b, o, 0)], 3)
    for t in range(3):
        for step in (n, 7):
            p = str(tmp_path / ("got_part%d_%d" % (t, step)))
            assert write_nodes(p, nt, l, [(f, seqs[f:f + step]) for f in range(0, n, step)], t, 3) == 0
            assert open(p, "rb").read() == open(parts[t], "rb").read(), (t, step)
    # a chunk whose offsets disagree with src_end - src_start; a chunk outside the table; a part outside the parts
    bad = list(seqs[:5])
    bad[2] = bad[2] + b"A"
    assert write_nodes(str(tmp_path / "bad"), nt, l, [(0, bad)]) == -1
    assert write_nodes(str(tmp_path / "bad"), nt, l, [(n - 2, seqs[n - 2:] + [b""])]) == -1
    assert write_nodes(str(tmp_path / "bad"), nt, l, [(0, seqs[:5])], 3, 3) == -1
    gfa_only = E.NodeTable({f: nodes[f] for f in ("index", "seqlen", "abundance")} | {"k": k})
    assert write_nodes(str(tmp_path / "bad"), gfa_only, l, [(0, seqs[:5])]) == -1


def test_new_arguments_and_the_cli_flag(tmp_path):
    from rust_mdbg_amd import api, pipeline
    assert inspect.signature(pipeline.run_file).parameters["sequences_from_kept"].default is False
    p = inspect.signature(api.Mdbg.graph_node_seqs).parameters
    assert [p[f].default for f in ("first_row", "max_rows", "max_bases", "device")] == [0, 0, 0, False]
    assert callable(api.Mdbg.node_seqs_ms)
    p = inspect.signature(E.Emitter.write_sequences_from_kept).parameters
    assert list(p)[:5] == ["self", "prefix", "nodes", "l", "m"] and p["threads"].default == 1 and p["chunk_bases"].default == 256 << 20
    assert "mdbg_seqfile_write_nodes" in E.EXPORTS and {"mdbg_graph_node_seqs", "mdbg_graph_node_seqs_device", "mdbg_node_seqs_ms"} <= set(api.EXPORTS)
    lib = os.path.join(ROOT, "rust_mdbg_amd")
    exe = str(tmp_path / "mdbg_cli")
    subprocess.run(["gcc", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mdbg_cli.c"), "-L" + lib, "-lmdbg_hip", "-lmdbg_emit",
                    "-lpthread", "-Wl,-rpath," + lib, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--sequences-from-kept" in r.stderr and "--keep-reads" in r.stderr
