"""The oracle, the second restatement and the host emulation of the sketch kernel against the two `.sequences` lines the reference tree itself holds
(tests/golden/reference_held_vectors.json, made by tests/golden/make_reference_held_vectors.py): hashes, positions, shift pair, span, orientation, line text.
The expected values are the reference's own output; every comparison is exact.  Both lines reproduce with homopolymer compression OFF (oracle/PIN.md)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import reference_held as H
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from test_emit_cpu import read_lz4_frame
from test_emu_cpu import emu  # noqa: F401  (the fixture that builds and loads tests/emu/sketch_emu.cpp)

VEC = pytest.mark.parametrize("v", H.VECTORS, ids=repr)


def generator():
    spec = importlib.util.spec_from_file_location("make_reference_held_vectors", os.path.join(GOLDEN, "make_reference_held_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_regenerates_from_the_reference_tree():
    """the ONE test that opens the reference tree: the committed file is, byte for byte, what the generator makes of it"""
    gen = generator()
    if not all(os.path.exists(os.path.join(gen.REFERENCE, v["file"])) for v in gen.VECTORS):
        pytest.skip("no reference tree at %s" % gen.REFERENCE)
    assert gen.text(gen.derive()) == open(H.FIXTURE).read()


def test_fixture_holds_data_only_and_the_generator_holds_no_line():
    raw = open(H.FIXTURE).read()
    assert len(raw) < 8192
    src = open(os.path.join(GOLDEN, "make_reference_held_vectors.py")).read()
    for v in H.VECTORS:
        assert set(v.seq) <= set(b"ACGT") and v.n == (409 if v.name == "A" else 303) and v.k == (10 if v.name == "A" else 7)
        assert v.seq[:40].decode() not in src and str(v.key[0]) not in src
        # what the derived positions owe the printed line: first and last gap, and the span ending with the last l-mer
        assert v.pos[0] == 0 and (v.pos[1] - v.pos[0], v.pos[-1] - v.pos[-2]) == v.shift and v.pos[-1] + v.l == v.n
        assert v.pos == sorted(set(v.pos))
    assert [(v.name, v.index, v.shift, v.l) for v in H.VECTORS] == [("A", 16606, (24, 33), 12), ("B", 1740, (29, 5), 10)]


def test_tile_stride_is_the_header_s():
    txt = open(os.path.join(ROOT, "rust_mdbg_amd", "csrc", "mdbg_dev.h")).read()
    c = {n: int(re.search(r"constexpr int %s = (\d+);" % n, txt).group(1)) for n in ("TILE_WPT", "TILE_THREADS", "TILE_HALO")}
    assert re.search(r"TILE_STRIDE = TILE_RAW_WORDS \* 32 - TILE_HALO;", txt) and re.search(r"TILE_RAW_WORDS = TILE_WPT \* TILE_THREADS;", txt)
    assert c["TILE_WPT"] * c["TILE_THREADS"] * 32 - c["TILE_HALO"] == H.TILE_STRIDE


def smaller_set(v, d):
    """what the listed hashes say on their own about a density below the exact range: those <= floor(d * 2^64) stay (src/read.rs:183,196)"""
    bound = int(d * 18446744073709551616.0)
    return [h for h in v.key if h <= bound]


@VEC
def test_oracle_sketch(v):
    b, o = O.concat_reads([v.seq])
    for d, hashes, pos in v.densities():
        sk = O.sketch(b, o, v.l, d, already_hpc=True)
        assert sk["err"] == 0 and sk["off"].tolist() == [0, len(hashes)]
        assert sk["hashes"].tolist() == hashes and sk["pos"].tolist() == pos, d
    for d, hashes, pos in v.outside:
        assert hashes != v.key
        if len(hashes) < v.k:
            assert hashes == smaller_set(v, d) and O.hash_bound(d) == int(d * 18446744073709551616.0)
        else:                                      # a larger set: the listed minimizers, in order, and others between them
            assert [h for h, p in zip(hashes, pos) if p in v.pos] == v.key and [p for p in pos if p in v.pos] == v.pos
    for d in v.exact:
        assert smaller_set(v, d) == v.key


def test_the_lines_reproduce_with_homopolymer_compression_off_only():
    """neither printed sequence is homopolymer-compressed (409 -> 307 and 303 -> 224 bases if it were), and with compression on the oracle selects other l-mers,
    none of them listed (oracle/PIN.md): the vectors pin the hash and the window loop, not compression together with hashing"""
    for v, n_hpc, pos in zip(H.VECTORS, (307, 224), ([24, 311], [6, 56, 74, 133])):
        assert len(O.encode_rle(v.seq)[0]) == n_hpc < v.n
        sk = O.sketch(*O.concat_reads([v.seq]), v.l, 0.01, already_hpc=False)
        assert sk["pos"].tolist() == pos and not set(sk["hashes"].tolist()) & set(v.key)


def test_vector_a_pins_the_density_bound_from_both_sides():
    """largest selected hash 0.0099452 * 2^64, smallest unselected 0.0103603 * 2^64: hash_bound(0.01) lies between them"""
    v = H.VECTORS[0]
    d, hashes, pos = [o for o in v.outside if len(o[1]) > v.k][0]
    extra = [(h, p) for h, p in zip(hashes, pos) if p not in v.pos]
    assert [p for h, p in extra] == [53]
    assert max(v.key) <= O.hash_bound(0.01) < extra[0][0]
    assert round(max(v.key) / 2.0 ** 64, 7) == 0.0099452 and round(extra[0][0] / 2.0 ** 64, 7) == 0.0103603


@VEC
def test_second_restatement_sketch(v):
    from golden.independent_restatement import sketch_read
    for d, hashes, pos in v.densities():
        h, p = sketch_read(v.seq, v.l, d, already_hpc=True)
        assert [int(x) for x in h] == hashes and [int(x) for x in p] == pos, d
    for rev in (False, True):
        s, hashes, pos = v.strand(rev)
        h, p = sketch_read(s, v.l, v.exact[0], already_hpc=True)
        assert [int(x) for x in h] == hashes and [int(x) for x in p] == pos


def emu_sketch(L, reads, l, d):
    b, o = O.concat_reads(reads)
    cap = len(b) + 16
    h, p, r = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    ns, nc = C.c_uint64(0), C.c_uint64(0)
    n = L.emu_sketch(b.ctypes.data, len(b), o.ctypes.data, len(o) - 1, l, d, 0, h.ctypes.data, p.ctypes.data, r.ctypes.data, cap, C.byref(ns), C.byref(nc))
    assert n >= 0
    return h[:n], p[:n], r[:n]


@VEC
def test_host_emulation_of_the_kernel(emu, v):   # noqa: F811
    for d, hashes, pos in v.densities():
        h, p, r = emu_sketch(emu, [v.seq], v.l, d)
        assert h.tolist() == hashes and p.tolist() == pos and not r.any(), d
    # across the first tile boundaries, on both strands: the listed minimizers, and the whole sketch the oracle's
    for start in H.placements(v):
        for rev in (False, True):
            s, hashes, pos = v.strand(rev)
            read = H.placed_read(v, start, rev)
            h, p, r = emu_sketch(emu, [read], v.l, 0.01)
            b, o = O.concat_reads([read])
            exp = O.sketch(b, o, v.l, 0.01, already_hpc=True)
            assert H.inside(exp, 0, start, start + v.n, v.l) == (hashes, pos), (start, rev)
            assert h.tolist() == exp["hashes"].tolist() and p.tolist() == exp["pos"].tolist(), (start, rev)


@VEC
def test_oracle_sketch_of_the_embedded_vector(v):
    """the minimizers lying wholly inside the embedded interval are the listed ones wherever the vector sits in a read, next to whatever"""
    for rev in (False, True):
        s, hashes, pos = v.strand(rev)
        for start in [127, 128, 32103, 32312, 32501, 32512, 32513, 64924]:
            b, o = O.concat_reads([H.placed_read(v, start, rev)])
            assert H.inside(O.sketch(b, o, v.l, 0.01, already_hpc=True), 0, start, start + v.n, v.l) == (hashes, pos), (start, rev)
        for reads, r, start in H.neighbour_cases(v, rev):
            b, o = O.concat_reads(reads)
            assert H.inside(O.sketch(b, o, v.l, 0.01, already_hpc=True), r, start, start + v.n, v.l) == (hashes, pos), (r, rev)


def oracle_nodes(reads, k, l, A=1, d=0.01):
    g = O.Graph(k, l, d, A, already_hpc=True)
    b, o = O.concat_reads(reads)
    assert g.ingest(b, o) == 0
    return g.finalize(with_edges=False)


@VEC
def test_oracle_graph_row_and_line_text(v):
    fwd = v.seq + H.flank(v)
    for read, rev, start in ((fwd, 0, 0), (H.revcomp(fwd), 1, H.FLANK), (H.revcomp(v.seq) + H.flank(v), 1, 0)):
        r = oracle_nodes([read], v.k, v.l)
        assert r["n_windows"] == r["n_nodes"] >= 2
        i = H.row_of_key(r, v.key)
        assert (int(r["src_read"][i]), int(r["src_start"][i]), int(r["src_end"][i])) == (0, start, start + v.n)
        assert tuple(int(x) for x in r["shift_full"][i]) == v.shift and int(r["reversed"][i]) == rev and int(r["abundance"][i]) == 1
        assert tuple(int(x) for x in r["shift"][i]) == v.shift
        # the line, built from the oracle's row as tests/test_emit_cpu.py builds its expected fields: the reference's line from the second field on
        seq = read[start:start + v.n]
        assert H.line_tail(r["keys"][i], O.revcomp(seq) if rev else seq, r["shift_full"][i]) == v.line_tail
        assert H.row_sequence([read], r, i) == v.seq


@VEC
def test_host_sequences_writer_prints_the_reference_line(v, tmp_path):
    """Emitter.write_sequences (the second pass over the reads) on the oracle's table: the listed node's line, forward and through the reverse-complement branch"""
    from rust_mdbg_amd import emit as E
    fwd = v.seq + H.flank(v)
    for n, read in enumerate((fwd, H.revcomp(fwd))):
        r = oracle_nodes([read], v.k, v.l)
        i = H.row_of_key(r, v.key)
        p = str(tmp_path / ("%s%d.0.sequences" % (v.name, n)))
        b, o = O.concat_reads([read])
        E.Emitter().write_sequences(p, r, v.l, [(b, o, 0)])
        body = [x for x in read_lz4_frame(p).decode().split("\n") if x and not x.startswith("#")]
        assert len(body) == r["n_nodes"]
        assert body[i] == "%d\t%s" % (r["index"][i], v.line_tail)


@VEC
def test_strict_window_rule_without_a_flank(v):
    """a read needs MORE than k minimizers (src/main.rs:756): the vector alone has exactly k"""
    for read in (v.seq, H.revcomp(v.seq)):
        at_k, below = oracle_nodes([read], v.k, v.l), oracle_nodes([read], v.k - 1, v.l)
        assert at_k["n_minimizers"] == below["n_minimizers"] == v.k
        assert (at_k["n_windows"], at_k["n_nodes"]) == (0, 0) and (below["n_windows"], below["n_nodes"]) == (2, 2)


def test_vector_a_repeats_one_pair_the_source_is_the_second_sighting():
    """A's key holds three hashes twice; at k = 2, minabund = 2 exactly one 2-min-mer is seen twice, and the entry describes the A-th sighting (src/main.rs:676-684)"""
    v = H.VECTORS[0]
    r = oracle_nodes([v.seq], 2, v.l, A=2)
    assert r["n_nodes"] == 1 and r["n_nodes_before"] == 8 and r["n_windows"] == 9
    assert tuple(int(x) for x in r["keys"][0]) == (83024137861838436, 183455804785478733) == tuple(v.key[8:10]) == tuple(v.key[2:4])
    assert (int(r["abundance"][0]), int(r["reversed"][0]), int(r["src_start"][0]), int(r["src_end"][0])) == (2, 0, 364, 409)
    assert tuple(int(x) for x in r["shift_full"][0]) == (33, 33)
