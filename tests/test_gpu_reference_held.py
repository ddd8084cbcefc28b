"""The HIP path against the two `.sequences` lines the reference tree itself holds (tests/golden/reference_held_vectors.json; tests/test_reference_held_cpu.py
pins the oracle, the second restatement and the host emulation on the same file): sketch kernels at l = 12 and l = 10 on both input layouts and both strands,
across the tile boundaries; the node row; the three places a node's sequence line is made.  The first assertion of every check is against the reference's own
values; where the oracle is consulted as well, that is a second assertion.  Exact equality of integers and bytes throughout; inputs are the fixture plus seeded
random bases, homopolymer compression off (oracle/PIN.md)."""
import numpy as np
import pytest

import reference_held as H
from oracle import oracle as O
from test_emit_cpu import read_lz4_frame
from test_gpu_parity import _mdbg, assert_nodes_equal, assert_sketch_equal

pytestmark = pytest.mark.gpu

VEC = pytest.mark.parametrize("v", H.VECTORS, ids=repr)
LAYOUT = pytest.mark.parametrize("packed", [False, True], ids=["ascii", "packed"])
STRAND = pytest.mark.parametrize("rev", [False, True], ids=["fwd", "rc"])
D = 0.01          # both lines reproduce at this density (the fixture's `exact` lists)
HINT = 64         # table_capacity_hint: a few rows per context


def gpu_sketch(m, reads, packed):
    """the sketch of one batch on the context `m`: mdbg_sketch_only on the ASCII bases, or a packed ingest read back from the store (which is then emptied)"""
    from rust_mdbg_amd import emit as E
    b, o = O.concat_reads(reads)
    if not packed:
        return m.sketch(b, o)
    m.ingest_packed(E.pack_reads(b, o), 0)
    sk = m.store_sketch()
    m.reset(0)
    return sk


def as_lists(sk):
    return sk["hashes"].tolist(), sk["pos"].tolist(), sk["off"].tolist()


@VEC
@pytest.mark.parametrize("path", ["ascii", "packed", "generic"])
def test_sketch_of_the_vector_alone_at_every_density(v, path):
    R = _mdbg()
    for d, hashes, pos in v.densities():
        with R.Mdbg(v.k, v.l, d, 1, reads_already_hpc=True, flags=R.api.FLAG_FORCE_GENERIC if path == "generic" else 0, table_capacity_hint=HINT) as m:
            assert as_lists(gpu_sketch(m, [v.seq], path == "packed")) == (hashes, pos, [0, len(hashes)]), d
            if path == "generic":
                assert as_lists(gpu_sketch(m, [v.seq], True)) == (hashes, pos, [0, len(hashes)]), d


@VEC
@LAYOUT
@STRAND
def test_sketch_of_the_vector_placed_in_a_read(v, packed, rev):
    """13 start offsets around the 32-base words and across the first two tile boundaries, then the read boundaries: the minimizers inside the embedded
    interval are the listed ones (mirrored on the other strand), and the whole sketch is the oracle's"""
    R = _mdbg()
    s, hashes, pos = v.strand(rev)
    assert H.TILE_STRIDE - v.n in H.placements(v) and 2 * H.TILE_STRIDE - 100 in H.placements(v)
    with R.Mdbg(v.k, v.l, D, 1, reads_already_hpc=True, table_capacity_hint=HINT) as m:
        for start in H.placements(v):
            read = H.placed_read(v, start, rev)
            assert read[start:start + v.n] == s and len(read) < 66000
            sk = gpu_sketch(m, [read], packed)
            assert H.inside(sk, 0, start, start + v.n, v.l) == (hashes, pos), start
            assert_sketch_equal(sk, O.sketch(*O.concat_reads([read]), v.l, D, already_hpc=True))
        for reads, r, start in H.neighbour_cases(v, rev):
            sk = gpu_sketch(m, reads, packed)
            assert H.inside(sk, r, start, start + v.n, v.l) == (hashes, pos), (r, start)
            assert_sketch_equal(sk, O.sketch(*O.concat_reads(reads), v.l, D, already_hpc=True))


def gpu_nodes(m, reads, packed):
    from rust_mdbg_amd import emit as E
    b, o = O.concat_reads(reads)
    if packed:
        m.ingest_packed(E.pack_reads(b, o), 0)
    else:
        m.ingest(b, o, 0)
    return m.finalize()


def oracle_nodes(reads, k, l, A=1):
    g = O.Graph(k, l, D, A, already_hpc=True)
    assert g.ingest(*O.concat_reads(reads)) == 0
    return g.finalize(with_edges=False)


def row_facts(nodes, i):
    return ((int(nodes["src_read"][i]), int(nodes["src_start"][i]), int(nodes["src_end"][i])), tuple(int(x) for x in nodes["shift_full"][i]),
            tuple(int(x) for x in nodes["shift"][i]), int(nodes["reversed"][i]), int(nodes["abundance"][i]))


@VEC
@LAYOUT
@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep_reads"])
def test_node_row_of_the_listed_k_min_mer(v, packed, keep):
    R = _mdbg()
    fwd = v.seq + H.flank(v)
    for read, rev, start in ((fwd, 0, 0), (H.revcomp(fwd), 1, H.FLANK)):
        with R.Mdbg(v.k, v.l, D, 1, reads_already_hpc=True, keep_reads=keep, table_capacity_hint=HINT) as m:
            got = gpu_nodes(m, [read], packed)
        i = H.row_of_key(got, v.key)
        assert row_facts(got, i) == ((0, start, start + v.n), v.shift, v.shift, rev, 1)
        assert H.line_tail(got["keys"][i], H.row_sequence([read], got, i), got["shift_full"][i]) == v.line_tail
        assert_nodes_equal(got, oracle_nodes([read], v.k, v.l))


@VEC
@LAYOUT
def test_strict_window_rule_without_a_flank(v, packed):
    """the vector alone holds exactly k minimizers: no window at k (src/main.rs:756 wants MORE than k), two at k - 1"""
    R = _mdbg()
    for read in (v.seq, H.revcomp(v.seq)):
        for k, n in ((v.k, 0), (v.k - 1, 2)):
            with R.Mdbg(k, v.l, D, 1, reads_already_hpc=True, table_capacity_hint=HINT) as m:
                got = gpu_nodes(m, [read], packed)
                st = m.stats()
            assert (got["n_nodes"], st["n_windows"], st["n_minimizers"]) == (n, n, v.k)
            assert_nodes_equal(got, oracle_nodes([read], k, v.l))


@LAYOUT
@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep_reads"])
def test_vector_a_second_sighting_is_the_source(packed, keep):
    """A's key holds one adjacent pair twice: at k = 2, minabund = 2 that pair is the one node, and it describes its SECOND sighting (src/main.rs:676-684)"""
    R = _mdbg()
    v = H.VECTORS[0]
    with R.Mdbg(2, v.l, D, 2, reads_already_hpc=True, keep_reads=keep, table_capacity_hint=HINT) as m:
        got = gpu_nodes(m, [v.seq], packed)
    assert got["n_nodes"] == 1 and got["n_nodes_before"] == 8
    assert tuple(int(x) for x in got["keys"][0]) == (83024137861838436, 183455804785478733) == tuple(v.key[8:10])
    assert row_facts(got, 0) == ((0, 364, 409), (33, 33), (33, 33), 0, 2)
    assert_nodes_equal(got, oracle_nodes([v.seq], 2, v.l, A=2))


def body_lines(path):
    return [x for x in read_lz4_frame(path).decode().split("\n") if x and not x.startswith("#")]


@VEC
@LAYOUT
@pytest.mark.parametrize("strand", ["fwd", "rc", "rc_read"])
@pytest.mark.parametrize("at", [0, 1, 15, 16, 17, 31])
def test_sequences_line_of_the_listed_node(v, packed, strand, at, tmp_path):
    """the vector starts `at` bases into the kept batch, behind a read of that many bases (too few to form a window): the gather kernel's 16-byte groups then
    start at every kind of position inside a 32-base word.  fwd: vector + flank; rc: the vector's reverse complement + flank, at the same place; rc_read: the
    reverse complement of the whole fwd read, the vector FLANK bases further on.  The second pass over the reads, the writer fed from the kept reads, and the
    device rows of graph_node_seqs all give the reference's line from the second field on."""
    from rust_mdbg_amd import emit as E
    R = _mdbg()
    rev = strand != "fwd"
    read, start = (H.revcomp(v.seq + H.flank(v)), H.FLANK) if strand == "rc_read" else (v.strand(rev)[0] + H.flank(v), 0)
    assert (H.revcomp(read[start:start + v.n]) if rev else read[start:start + v.n]) == v.seq
    reads = ([H.rnd_bases(at, at)] if at else []) + [read]
    b, o = O.concat_reads(reads)
    with R.Mdbg(v.k, v.l, D, 1, reads_already_hpc=True, keep_reads=True, table_capacity_hint=HINT) as m:
        nodes = gpu_nodes(m, reads, packed)                      # (a packed batch is kept as it came, an ASCII batch is packed on the device)
        i = H.row_of_key(nodes, v.key)
        assert row_facts(nodes, i) == ((len(reads) - 1, start, start + v.n), v.shift, v.shift, int(rev), 1)
        want = "%d\t%s" % (nodes["index"][i], v.line_tail)
        em = E.Emitter()
        second_pass = str(tmp_path / "pass.0.sequences")
        em.write_sequences(second_pass, nodes, v.l, [(b, o, 0)])
        lines = body_lines(second_pass)
        assert len(lines) == nodes["n_nodes"] and lines[i] == want
        (kept,) = em.write_sequences_from_kept(str(tmp_path / "kept"), nodes, v.l, m)
        lines = body_lines(kept)
        assert len(lines) == nodes["n_nodes"] and lines[i] == want
        for first, rows in ((0, 0), (i, 1)):                     # the row inside a whole-table chunk, and as a chunk of its own
            dv = m.graph_node_seqs(first, rows, 0, device=True)
            assert dv["first_row"] == first and dv["n_rows"] == (rows or nodes["n_nodes"])
            off = m.to_host(dv["offsets"], 8 * (dv["n_rows"] + 1), np.uint64).astype(np.int64)
            row = m.to_host(dv["bases"], dv["n_bases"]).tobytes()[off[i - first]:off[i - first + 1]]
            assert row == v.seq
            assert H.line_tail(nodes["keys"][i], row, nodes["shift_full"][i]) == v.line_tail
    assert_nodes_equal(nodes, oracle_nodes(reads, v.k, v.l))
