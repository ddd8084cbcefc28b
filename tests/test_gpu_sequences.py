"""Finalize between batches that arrive in any ordinal order: one context walked through a seeded sequence of operations (ingest through three entry points,
the three finalize variants, edges, reset(k), reset(0), mark / rewind, temporary batches) beside the plain model of tests/sequence_model.py, and directed
sequences for what a context keeps from one finalize to the next: the marks of the claim-map finalize, the speculative row count, the ranks of wrapped
slots.  After EVERY finalize the node table equals the table of a fresh oracle graph fed the resident batches in ascending ordinal order, bit for bit, with the
claim-map finalize and with MDBG_NO_CLAIMS (read per finalize).  tests/test_sequences_cpu.py checks that the inputs hit what they are meant to hit."""
import ctypes

import numpy as np
import pytest

import sequence_model as S
from oracle import oracle as O
from test_gpu_parity import _mdbg, assert_nodes_equal, assert_sketch_equal

pytestmark = pytest.mark.gpu

GFA_FIELDS = ("index", "seqlen", "abundance")


def _claims(monkeypatch, no_claims):
    if no_claims:
        monkeypatch.setenv("MDBG_NO_CLAIMS", "1")
    else:
        monkeypatch.delenv("MDBG_NO_CLAIMS", raising=False)


def nodes_from_device(m, nd):
    """the device table of finalize_device() copied back field by field -> the dict finalize() returns"""
    n, k = int(nd.n), int(nd.k)

    def col(p, count, dt):
        return m.to_host(ctypes.cast(p, ctypes.c_void_p).value, count * np.dtype(dt).itemsize, dt) if count else np.zeros(0, dt)
    return dict(n_nodes=n, n_nodes_before=int(nd.n_distinct), keys=col(nd.keys, n * k, np.uint64).reshape(n, k), index=col(nd.index, n, np.uint32),
                abundance=col(nd.abundance, n, np.uint16), seqlen=col(nd.seqlen, n, np.uint32), shift=col(nd.shift, 2 * n, np.uint16).reshape(n, 2),
                shift_full=col(nd.shift_full, 2 * n, np.uint64).reshape(n, 2), src_read=col(nd.src_read, n, np.uint64), src_start=col(nd.src_start, n, np.uint64),
                src_end=col(nd.src_end, n, np.uint64), reversed=col(nd.reversed, n, np.uint8))


def check_finalize(m, exp, variant="host"):
    if variant == "gfa":
        got = m.finalize(gfa_only=True)
        assert got["n_nodes"] == exp["n_nodes"] and got["n_nodes_before"] == exp["n_nodes_before"]
        for f in GFA_FIELDS:
            assert np.array_equal(got[f], exp[f]), f
    else:
        assert_nodes_equal(m.finalize() if variant == "host" else nodes_from_device(m, m.finalize_device()), exp)


def ingest(m, op, keep):
    from rust_mdbg_amd import emit as E
    b, o = O.concat_reads(op["reads"])
    if op["entry"] == "reads":
        m.ingest_reads(op["reads"], op["first"])
    elif op["entry"] == "packed":
        m.ingest_packed(E.pack_reads(b, o), op["first"])
    else:                                                   # sketch stage and insertion as two calls, from device buffers
        import torch
        tb = torch.from_numpy(b).cuda() if len(b) else torch.zeros(16, dtype=torch.uint8, device="cuda")
        to = torch.from_numpy(o.view(np.int64)).cuda()
        torch.cuda.synchronize()                            # (the copies ran on torch's stream, the sketch runs on the context's)
        m.sketch_device(tb.data_ptr(), to.data_ptr(), len(op["reads"]), len(b), op["first"])
        m.insert_resident()
        m.sync()
        keep += [tb, to]


def walk(m, R, k, l, d, A, ops):
    """the operations on the context and on the model; every finalize against the oracle"""
    model = S.Model(k, l, d, A)
    keep, edges_live, n_checked = [], False, 0
    for op in ops:
        what = op["op"]
        if what == "ingest":
            ingest(m, op, keep)
            if edges_live:                                  # the edge list belongs to a table that is no longer current
                with pytest.raises(R.MdbgError) as ei:
                    m.graph_unitigs()
                assert ei.value.code == R.api.MDBG_E_STATE == -6
                edges_live = False
        elif what == "finalize":
            edges_live = False
            exp = model.expected(with_edges=op["edges"])
            check_finalize(m, exp, op["variant"])
            n_checked += 1
            if op["twice"]:
                check_finalize(m, exp, "host")
            if op["edges"] and exp["n_nodes"]:
                pe = m.graph_edges(S.PRESIMP)
                assert sorted(zip(pe["n1"].tolist(), pe["o1"].tolist(), pe["n2"].tolist(), pe["o2"].tolist(), pe["overlap"].tolist())) == S.edge_rows(exp)
                assert len(pe["n1"]) == exp["n_edges"] and pe["presimp_removed"] == exp["presimp_removed"]
                edges_live = True
        elif what == "reset":
            m.reset(op["k"]); edges_live = False
        elif what == "reset0":
            m.reset(0); edges_live = False
            assert m.mark() == 0 and m.stats()["n_minimizers"] == 0
        elif what == "mark":
            assert m.mark() == op["mark"] == len(model.batches)
        elif what == "rewind":
            m.rewind(op["mark"]); m.reset(op["k"]); edges_live = False
            assert m.mark() == op["mark"]
        else:                                               # temporary batches: nothing of them stays
            st0, mk0 = m.stats(), m.mark()
            b, o = O.concat_reads(op["reads"])
            if what == "sketch":
                assert_sketch_equal(m.sketch(b, o), O.sketch(b, o, l, d))
            else:
                counts, off = m.query(b, o)
                assert len(off) == len(op["reads"]) + 1 and int(off[-1]) == len(counts)
            st1 = m.stats()
            assert {f: v for f, v in st1.items() if f not in S.TIMERS} == {f: v for f, v in st0.items() if f not in S.TIMERS}
            assert m.mark() == mk0 == len(model.batches)
        model.apply(op)
    return n_checked


@pytest.mark.parametrize("seed", range(S.N_SEEDS))
def test_seeded_sequences_equal_the_oracle_after_every_finalize(seed, monkeypatch):
    R = _mdbg()
    seq = S.gen_sequence(seed)
    _claims(monkeypatch, seq["no_claims"])
    with R.Mdbg(seq["k"], seq["l"], seq["d"], seq["A"], table_capacity_hint=seq["hint"]) as m:
        assert walk(m, R, seq["k"], seq["l"], seq["d"], seq["A"], seq["ops"]) >= 2


@pytest.mark.parametrize("no_claims", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(S.DIRECTED))
def test_first_sightings_that_move_between_two_finalize_calls(name, A, no_claims, monkeypatch):
    """descending triple (2000, 1000, finalize, 0, finalize), ascending pair then two batches below it, and 3000 / 1000 / 4000 / 0 / 2000 with a finalize after
    each: a key of every batch has its first sighting moved by each later, lower batch.  Until the ordinal rule of fin_setup the claim-map finalize left the
    mark of the sighting in between standing (at least 1,187 / 1,411 / 1,348 keys counted twice at the last finalize of the three inputs:
    sequence_model.certain_stale_marks)."""
    R = _mdbg()
    steps = S.DIRECTED[name]()
    assert S.certain_stale_marks(steps, S.K, S.L, S.D)[-1] >= S.MIN_STALE
    _claims(monkeypatch, no_claims)
    with R.Mdbg(S.K, S.L, S.D, A) as m:
        assert walk(m, R, S.K, S.L, S.D, A, S._steps_to_ops(steps)) == sum(1 for s in steps if s[0] == "finalize")


@pytest.mark.parametrize("no_claims", [False, True])
@pytest.mark.parametrize("direction", ["up", "down"])
def test_row_estimate_of_an_earlier_finalize_far_from_the_table(direction, no_claims, monkeypatch):
    """fin_rows_guess: a second table far larger than the rows the first finalize makes the second write ahead (the plain path runs after all), and, through
    rewind + reset, a far smaller one"""
    R = _mdbg()
    k, l, d, A = S.SPEC
    ops = S._steps_to_ops(S.speculation_up()) if direction == "up" else S.speculation_down()
    _claims(monkeypatch, no_claims)
    with R.Mdbg(k, l, d, A) as m:
        assert walk(m, R, k, l, d, A, ops) == sum(1 for op in ops if op["op"] == "finalize")


@pytest.fixture(scope="module")
def wrap_case():
    """the wrap input and the oracle's two tables (computed once for both finalize modes)"""
    k, l, d, A = S.WRAP
    read, steps = S.wrap_leftovers()
    model, tables = S.Model(k, l, d, A), []
    for st in steps:
        if st[0] == "ingest":
            model.batches.append((st[1], st[2]))
        else:
            tables.append(model.expected())
    return steps, tables


@pytest.mark.parametrize("no_claims", [False, True])
def test_wrapped_slots_then_a_lower_batch_with_their_keys(wrap_case, no_claims, monkeypatch):
    """one read 65,536 + A times: wrap_list_kernel leaves ranks in Slot.pad at the first finalize; then a batch BELOW it holds the same keys, so their first
    sightings move and the wrapped nodes describe another sighting (src/main.rs:676-684)"""
    R = _mdbg()
    k, l, d, A = S.WRAP
    steps, tables = wrap_case
    assert tables[0]["n_nodes"] >= 5 and tables[1]["n_nodes"] > tables[0]["n_nodes"]
    _claims(monkeypatch, no_claims)
    with R.Mdbg(k, l, d, A) as m:
        it = iter(tables)
        for st in steps:
            if st[0] == "ingest":
                m.ingest_reads(st[1], st[2])
            else:
                exp = next(it)
                assert_nodes_equal(m.finalize(), exp)
                assert_nodes_equal(m.finalize(), exp)
