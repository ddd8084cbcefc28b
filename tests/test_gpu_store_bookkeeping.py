"""Bookkeeping of the resident sketch store (csrc/store.inc): temporary batches (sketch / query) leave nothing behind, rewind and reset(0) cut
the store back to what a fresh context holds, a gap left by an imported region survives the cut, and both host entry points refuse bad offsets
the same way.  Seeded reads, the CPU oracle as comparator; every context here holds about 60 reads of 300 - 3,000 bases."""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import assert_nodes_equal, assert_sketch_equal, oracle_graph, rand_reads

pytestmark = pytest.mark.gpu

K, L, D, A = 7, 10, 0.05, 2
TIMERS = ("ms_sketch", "ms_insert", "ms_finalize")
COUNTERS = ("n_reads", "n_bases", "n_minimizers", "n_tiles", "n_slow_tiles", "n_sketch_tile_launches", "n_sketch_tile_bases")


def _reads():
    """batch A (30 reads), batch B and B' (30 reads each, overlapping A so that some nodes are solid, and different from each other)"""
    base = rand_reads(1234, 30, 300, 3000)
    b1 = [r[20:] for r in base[:20]] + rand_reads(1235, 10, 300, 3000)
    b2 = [r[35:] for r in base[5:25]] + rand_reads(1236, 10, 300, 3000)
    return base, b1, b2


def _oracle_batches(batches):
    """node table of the oracle over [(reads, first ordinal)]"""
    g = O.Graph(K, L, D, A)
    for reads, first in sorted(batches, key=lambda t: t[1]):
        b, o = O.concat_reads(reads)
        assert g.ingest(b, o, first) == 0
    return g.finalize(with_edges=False)


def test_temporary_batches_leave_nothing_behind():
    import rust_mdbg_amd as R
    ra, rb, _ = _reads()
    with R.Mdbg(K, L, D, A) as m:
        m.ingest_reads(ra, 0)
        st0, mk0 = m.stats(), m.mark()
        bad = [ra[3], ra[4][:200] + b"R" + ra[4][200:], ra[5]]
        with pytest.raises(R.MdbgError) as ei:
            m.sketch(*O.concat_reads(bad))
        assert ei.value.code == R.api.MDBG_E_ALPHABET
        qb, qo = O.concat_reads(rb)
        exp_sk = O.sketch(qb, qo, L, D)
        assert exp_sk["err"] == 0 and len(exp_sk["hashes"]) > 30 * K
        assert_sketch_equal(m.sketch(qb, qo), exp_sk)                  # the context is still usable
        # query: reads of A against the filtered table of A
        nodes_a = oracle_graph(ra, K, L, D, A)
        table = {tuple(int(x) for x in nodes_a["keys"][i]): int(nodes_a["abundance"][i]) for i in range(nodes_a["n_nodes"])}
        ab, ao = O.concat_reads(ra[:10])
        sk = O.sketch(ab, ao, L, D)
        exp_counts, exp_off = [], [0]
        for r in range(10):
            h = [int(x) for x in sk["hashes"][int(sk["off"][r]):int(sk["off"][r + 1])]]
            if len(h) > K:
                for i in range(len(h) - K + 1):
                    w = tuple(h[i:i + K]); rv = w[::-1]
                    exp_counts.append(table.get(w if w < rv else rv, 0))
            exp_off.append(len(exp_counts))
        counts, off = m.query(ab, ao)
        assert off.tolist() == exp_off and counts.tolist() == exp_counts and len(exp_counts) > 100
        st1 = m.stats()
        for f in COUNTERS:
            assert st1[f] == st0[f], f
        assert {f: v for f, v in st1.items() if f not in TIMERS} == {f: v for f, v in st0.items() if f not in TIMERS}
        assert m.mark() == mk0
        m.ingest_reads(rb, 30)
        got = m.finalize()
    exp = oracle_graph(ra + rb, K, L, D, A)
    assert exp["n_nodes"] > 20
    assert_nodes_equal(got, exp)


@pytest.fixture(scope="module")
def fresh_a_b2():
    """what a fresh context holds after A + B': (oracle node table, stats, kept_reads of a keep_reads context)"""
    import rust_mdbg_amd as R
    ra, _, rb2 = _reads()
    with R.Mdbg(K, L, D, A, keep_reads=True) as m:
        m.ingest_reads(ra, 0)
        m.ingest_reads(rb2, 30)
        st, kept = m.stats(), m.kept_reads()
    exp = oracle_graph(ra + rb2, K, L, D, A)
    assert exp["n_nodes"] > 20
    return exp, st, kept


@pytest.mark.parametrize("cut,keep", [("rewind", False), ("reset0", False), ("rewind", True), ("reset0", True)])
def test_rewind_and_reset0_cut_back_to_a_fresh_context(fresh_a_b2, cut, keep):
    import rust_mdbg_amd as R
    ra, rb, rb2 = _reads()
    exp, st_fresh, kept_fresh = fresh_a_b2
    with R.Mdbg(K, L, D, A, keep_reads=keep) as m:
        m.ingest_reads(ra, 0)
        mk = m.mark()
        m.ingest_reads(rb, 30)
        if cut == "rewind":
            m.rewind(mk)
            m.reset(K)
            assert m.mark() == mk
        else:
            m.reset(0)
            assert m.mark() == 0 and m.stats()["n_minimizers"] == 0
            m.ingest_reads(ra, 0)
        if keep:
            assert m.kept_reads()["n_reads"] == len(ra)
        m.ingest_reads(rb2, 30)
        got, st = m.finalize(), m.stats()
        if keep:
            assert m.kept_reads() == kept_fresh
        else:
            assert m.kept_reads() == dict(n_reads=0, n_bases=0, bytes=0)
    assert_nodes_equal(got, exp)
    for f in ("n_reads", "n_bases", "n_minimizers"):
        assert st[f] == st_fresh[f], f


def test_a_gap_in_the_store_survives_truncation():
    """a region reserved before and committed after a batch of the context's own leaves unused boundary slots between the batches (next_slot0);
    a rewind to a mark behind them keeps them, and what is ingested afterwards lands behind everything that stayed"""
    import torch
    import rust_mdbg_amd as R
    from rust_mdbg_amd import dist as D_
    ra, rb, rb2 = _reads()
    parts = [(ra[:15], 0), (ra[15:], 15), (rb[:10], 30), (rb[10:20], 40)]          # own, imported, own (sketched while the region is pending), own
    dev = torch.device("cuda", 0)
    with R.Mdbg(K, L, D, A, device=0) as src, R.Mdbg(K, L, D, A, device=0) as dst:
        es, ed = D_.GpuEngine(src, torch, dev), D_.GpuEngine(dst, torch, dev)
        dst.store_reserve(1 << 18, 1 << 10)
        dst.ingest_reads(*parts[0])
        es.sketch_host(*O.concat_reads(parts[1][0]), parts[1][1])
        h, p, off, first, n = es.last_sketch()
        (hv, pv, token), = ed.reserve_import([h.shape[0]])
        ed.sketch_host(*O.concat_reads(parts[2][0]), parts[2][1])        # not adjacent to the last registered batch: one unused slot
        hv.copy_(h); pv.copy_(p)
        torch.cuda.synchronize()
        ed.commit_import(token, off.clone(), first)                      # registered behind a batch that lies above it in the store: another one
        ed.insert_owned()
        dst.ingest_reads(*parts[3])
        v = dst.sketch_view()
        assert int(v.n_reads) == sum(len(r) for r, _ in parts) + 3      # three gaps
        mk = dst.mark()
        assert mk == 4
        dst.ingest_reads(rb[20:], 50)
        dst.rewind(mk)
        dst.reset(K)
        assert int(dst.sketch_view().n_reads) == int(v.n_reads) and dst.mark() == mk
        dst.ingest_reads(rb2, 50)
        got = dst.finalize()
        st = dst.stats()
    exp = _oracle_batches(parts + [(rb2, 50)])
    assert exp["n_nodes"] > 20
    assert_nodes_equal(got, exp)
    assert st["n_minimizers"] == exp["n_minimizers"]


@pytest.mark.parametrize("what,message", [("first", "offsets[0] must be 0"), ("decreasing", "offsets must be non-decreasing")])
def test_offsets_validation_is_the_same_on_both_host_entry_points(what, message):
    import rust_mdbg_amd as R
    from rust_mdbg_amd import emit as E
    ra, _, _ = _reads()
    b, o = O.concat_reads(ra[:8])
    bad = np.array(o, dtype=np.uint64)
    if what == "first":
        bad[0] = 1
    else:
        bad[4] = bad[3] - 1
    packed = dict(E.pack_reads(b, o))
    packed["offsets"] = bad
    with R.Mdbg(K, L, D, A) as m:
        errs = []
        for call in (lambda: m.ingest(b, bad, 0), lambda: m.ingest_packed(packed, 0)):
            with pytest.raises(R.MdbgError) as ei:
                call()
            errs.append((ei.value.code, str(ei.value)))
        assert errs[0] == errs[1] == (R.api.MDBG_E_PARAM, "mdbg error %d: %s" % (R.api.MDBG_E_PARAM, message))
        assert m.stats()["n_reads"] == 0 and m.mark() == 0
        m.ingest(b, o, 0)                                                # refused, not poisoned
        assert m.stats()["n_reads"] == 8
