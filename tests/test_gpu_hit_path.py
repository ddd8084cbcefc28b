"""What follows a confirmed match in the insertion kernels (csrc/table.hip, record_hit): the reject test on the slot's current A-th smallest ordinal, the atomicMin cascade
and the count, in that order — in insert_windows_kernel, insert_records_kernel and the two listed-insertion kernels of csrc/owner.hip.

Everything goes through the C ABI and is compared with the CPU oracle on the same reads, node for node and field by field (index, abundance, seqlen, shift, shift_full,
src_read / src_start / src_end, reversed; the keys too).  The shapes are the smallest at which a wrong reject, or a count lost to the order of the memory operations, would
show: ONE read of ~4 kb with a few dozen windows, ingested c = 1 ... A + 2 times under distinct read ordinals, so that every slot sees exactly c sightings and the A-th
is one particular copy; the copies arrive in one launch, in ascending and in DESCENDING ordinal order (every later hit then carries a smaller ordinal than anything the
slot holds: nothing may be rejected, the whole cascade runs), with and without a finalize in between; and dozens of racing hits on the same slots inside one launch."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, TESTS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

K, L, D = 5, 8, 0.008
NODE_FIELDS = ("keys", "index", "abundance", "seqlen", "shift", "shift_full", "src_read", "src_start", "src_end", "reversed")


def the_read():
    rnd = random.Random(1205)
    return bytes(rnd.choice(b"ACGT") for _ in range(4000))


def racing_reads():
    """64 copies of the read and 64 copies with one substituted base each (at 64 different places): most windows of a mutated copy are still the read's"""
    r = the_read()
    rnd = random.Random(77)
    out = [r] * 64
    for p in sorted(rnd.sample(range(100, len(r) - 100), 64)):
        s = bytearray(r)
        s[p] = ord("ACGT"[("ACGT".index(chr(s[p])) + 1 + rnd.randrange(3)) % 4])
        out.append(bytes(s))
    return out


def oracle_nodes(batches, A):
    """batches: [(reads, first ordinal)].  The reference's semantics are those of the reads in ordinal order, whatever the order of the calls."""
    g = O.Graph(K, L, D, A)
    for reads, first in sorted(batches, key=lambda b: b[1]):
        b, o = O.concat_reads(reads)
        assert g.ingest(b, o, first) == 0
    return g.finalize(with_edges=False)


def assert_nodes_equal(got, exp, what):
    assert got["n_nodes_before"] == exp["n_nodes_before"], what
    assert got["n_nodes"] == exp["n_nodes"], what
    for f in NODE_FIELDS:
        assert np.array_equal(np.asarray(got[f]), np.asarray(exp[f])), (what, f)


def ingest_all(m, batches):
    for reads, first in batches:
        m.ingest_reads(reads, first)


def n_windows_of_the_read():
    b, o = O.concat_reads([the_read()])
    n = len(O.sketch(b, o, L, D)["hashes"])
    return n - K + 1 if n > K else 0


def test_the_read_has_a_few_dozen_windows():
    """the premise of the cases below (no GPU work, but it belongs with them)"""
    assert 24 <= n_windows_of_the_read() <= 72


@pytest.mark.parametrize("A", [1, 2, 3, 5])
def test_copies_one_to_a_plus_two_in_every_arrival_order(A):
    """c copies of one read under ordinals 0 ... c - 1: as one batch (one launch, the copies race), as c batches in ascending order (every later hit is larger than what
    the slot holds: rejected once the slot is full) and as c batches in DESCENDING order (every later hit is smaller: the whole cascade).  Same table every time."""
    import rust_mdbg_amd as R
    r = the_read()
    with R.Mdbg(K, L, D, A) as m:
        for c in range(1, A + 3):
            exp = oracle_nodes([([r] * c, 0)], A)
            assert exp["n_nodes_before"] >= 24 and (exp["n_nodes"] == exp["n_nodes_before"] if c >= A else exp["n_nodes"] == 0)
            if c >= A:
                assert set(np.asarray(exp["abundance"]).tolist()) == {c} and set(np.asarray(exp["src_read"]).tolist()) == {A - 1}      # the A-th sighting is copy A - 1's
            orders = {"one batch": [([r] * c, 0)],
                      "ascending": [([r], j) for j in range(c)],
                      "descending": [([r], j) for j in reversed(range(c))]}
            for name, batches in orders.items():
                m.reset(0)
                ingest_all(m, batches)
                got = m.finalize()
                assert_nodes_equal(got, exp, (A, c, name))


@pytest.mark.parametrize("A", [1, 2, 3, 5])
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_finalize_between_the_batches(A, order):
    """the same copies, one per batch, with a finalize after every batch: the table is read in between and the slot's A-th smallest changes from round to round; every
    intermediate table is the oracle's for the ordinals seen so far"""
    import rust_mdbg_amd as R
    r = the_read()
    c = A + 2
    ords = list(range(c)) if order == "ascending" else list(reversed(range(c)))
    with R.Mdbg(K, L, D, A) as m:
        for j in range(c):
            m.ingest_reads([r], ords[j])
            got = m.finalize()
            assert_nodes_equal(got, oracle_nodes([([r], x) for x in ords[:j + 1]], A), (A, order, j))


def racing_case():
    """one launch, 128 reads, every slot of the read hit ~127 times (also run in a child process under MDBG_WEAK_FP)"""
    import rust_mdbg_amd as R
    reads = racing_reads()
    nd = {}
    for A in (1, 2, 3, 5):
        exp = oracle_nodes([(reads, 0)], A)
        assert exp["n_nodes"] >= 24 and int(np.max(exp["abundance"])) >= 100
        with R.Mdbg(K, L, D, A) as m:
            m.ingest_reads(reads, 0)
            assert_nodes_equal(m.finalize(), exp, ("racing", A))
            # and once more behind itself: 128 further hits per slot, every one of them larger than the A smallest — all rejected, all counted
            m.ingest_reads(reads, len(reads))
            assert_nodes_equal(m.finalize(), oracle_nodes([(reads, 0), (reads, len(reads))], A), ("racing twice", A))
        nd[A] = exp["n_nodes"]
    return nd


def test_many_racing_hits_in_one_launch():
    racing_case()


def test_many_racing_hits_behind_a_weak_fingerprint():
    """MDBG_WEAK_FP (read once per process, hence the child): a two-bit fingerprint, most probes meet another key first, and matches confirmed after the plain walk
    feed record_hit too"""
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_hit_path as t; print('RACING_OK', t.racing_case())" % (ROOT, TESTS)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, MDBG_WEAK_FP="1"), timeout=600)
    assert r.returncode == 0 and "RACING_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def dilution_reads():
    """reads with exactly K minimizers (one too few for a window: src/main.rs:756): they add window STARTS to a sketch and no windows"""
    r = the_read()
    b, o = O.concat_reads([r])
    pos = O.sketch(b, o, L, D)["pos"]
    short = r[:int(pos[K])]                      # ends in front of minimizer K's first base
    b, o = O.concat_reads([short])
    assert len(O.sketch(b, o, L, D)["hashes"]) == K
    return short


@pytest.mark.parametrize("A", [2, 3])
@pytest.mark.parametrize("sparse", [False, True])
def test_listed_kernels_on_a_partitioned_table(A, sparse):
    """the same multiset of reads through two partitioned tables (mdbg_set_partition, world 2, both ranks on this GPU): a rank's own windows go through
    insert_windows_kernel, its share of the peer's sketch through the listed kernels — the span kernel when the list is dense, the per-entry kernel when fewer than 150
    windows are listed per 2048 window starts (owner.hip, LISTED_SPAN_MIN), which `sparse` arranges with reads that start no window.  The union of the two partitions is
    the one-context table, which is the oracle's."""
    from test_distributed_cpu import check_against_oracle
    from test_gpu_distributed import run
    reads = racing_reads()
    if sparse:
        # n windows and n + K - 1 starts per copy; 400 short reads per copy add 400 K starts: n / (n + 4 + 2000) < 150 / 2048 for every n <= 72, whichever rank owns them
        short = dilution_reads()
        reads = [x for r in reads for x in [r] + [short] * 400]
    parts = run(2, reads, K, L, D, A, batches_per_rank=2, mode="replicate")
    check_against_oracle(parts, reads, K, L, D, A)
    assert sum(p["n_local"] for p in parts) == parts[0]["n_nodes"] >= 24


@pytest.mark.parametrize("A", [2, 3])
def test_routed_records(A):
    """the same reads as routed records (insert_records_kernel), two ranks"""
    from test_distributed_cpu import check_against_oracle
    from test_gpu_distributed import run
    reads = racing_reads()
    parts = run(2, reads, K, L, D, A, batches_per_rank=2, mode="route")
    check_against_oracle(parts, reads, K, L, D, A)
    assert parts[0]["n_nodes"] >= 24
