"""The inputs of tests/test_gpu_sequences.py, checked with the oracle alone: every directed input hits the case it is named after, the seeded sequences
never put two batches on overlapping ordinals, and each of them holds a finalize that sees a batch which arrived out of order after an earlier finalize.
Without this the GPU test could pass on sequences that exercise nothing."""
import pytest

import sequence_model as S


def _walk(seq, max_reads=None):
    """the model through a sequence -> the oracle's table at every finalize"""
    model = S.Model(seq["k"], seq["l"], seq["d"], seq["A"])
    tables = []
    for op in seq["ops"]:
        model.apply(op)
        assert not S.spans_overlap(model.batches)
        assert max_reads is None or sum(len(r) for r, _ in model.batches) <= max_reads
        if op["op"] == "finalize":
            tables.append(model.expected(with_edges=op["edges"]))
        if op["op"] in ("mark", "rewind"):
            assert op["mark"] <= len(model.batches)
    return tables


@pytest.mark.parametrize("seed", range(5))
def test_seeded_sequences_are_not_trivial(seed):
    seq = S.gen_sequence(seed)
    assert 8 <= len(seq["ops"]) <= 14
    assert S.out_of_order_finalizes(seq["ops"]) >= 1
    tables = _walk(seq, S.MAX_READS)
    assert max(t["n_nodes"] for t in tables) > 20          # keys repeat across the batches: something is solid


def test_the_seeds_cover_every_mode():
    seqs = [S.gen_sequence(s) for s in range(S.N_SEEDS)]
    for seq in seqs:
        assert S.out_of_order_finalizes(seq["ops"]) >= 1
    for hint in (0, 16):
        for nc in (False, True):
            assert sum(1 for q in seqs if q["hint"] == hint and q["no_claims"] == nc) == S.N_SEEDS // 4
    assert {q["policy"] for q in seqs} == {"asc", "desc", "rand"}
    assert {(q["k"], q["l"], q["d"], q["A"]) for q in seqs} == set(S.PARAMS)
    ops = [op for q in seqs for op in q["ops"]]
    assert {op["op"] for op in ops} == {"ingest", "finalize", "reset", "reset0", "mark", "rewind", "sketch", "query"}
    assert {op["entry"] for op in ops if op["op"] == "ingest"} == {"reads", "packed", "resident"}
    fins = [op for op in ops if op["op"] == "finalize"]
    assert {op["variant"] for op in fins} == {"host", "device", "gfa"} and any(op["twice"] for op in fins) and any(op["edges"] for op in fins)


@pytest.mark.parametrize("name", sorted(S.DIRECTED))
@pytest.mark.parametrize("A", [1, 2, 3])
def test_directed_inputs_move_first_sightings_between_finalize_calls(name, A):
    steps = S.DIRECTED[name]()
    ops = S._steps_to_ops(steps)
    assert S.out_of_order_finalizes(ops) >= 1
    assert len(S.shared_in_all(steps, S.K, S.L, S.D)) >= S.MIN_STALE      # in every batch, so first seen in the batch with the smallest ordinals
    stale = S.certain_stale_marks(steps, S.K, S.L, S.D)
    assert stale[0] == 0 and stale[-1] >= S.MIN_STALE                       # what a claim map whose marks are only ever moved would count twice
    tables = _walk(dict(k=S.K, l=S.L, d=S.D, A=A, ops=ops))
    assert tables[-1]["n_nodes"] > 20 and tables[-1]["n_nodes_before"] > tables[0]["n_nodes_before"]


def test_descending_triple_first_sightings_lie_in_the_last_batch():
    steps = S.descending_triple()
    (b2, o2), (b1, o1), (b0, o0) = [(s[1], s[2]) for s in steps if s[0] == "ingest"]
    assert (o2, o1, o0) == (2000, 1000, 0)
    k2, k1, k0 = (S.window_keys(b, S.K, S.L, S.D) for b in (b2, b1, b0))
    assert len(k2 & k1 & k0) >= 50


def test_speculation_inputs_leave_the_row_estimate_behind():
    k, l, d, A = S.SPEC
    up = _walk(dict(k=k, l=l, d=d, A=A, ops=S._steps_to_ops(S.speculation_up())))
    guess = S.guess_of(up[0]["n_nodes"])
    assert 0 < up[0]["n_nodes"] and up[1]["n_nodes"] > guess + guess // 4 + 1024
    down = _walk(dict(k=k, l=l, d=d, A=A, ops=S.speculation_down()))
    assert down[0]["n_nodes"] == up[1]["n_nodes"] and down[1]["n_nodes"] == up[0]["n_nodes"]      # the same two tables, the large one first
    assert S.guess_of(down[1]["n_nodes"]) + 1024 < down[0]["n_nodes"] and down[2]["n_nodes"] >= down[1]["n_nodes"]


def test_wrap_input_wraps_and_is_shared_by_the_lower_batch():
    k, l, d, A = S.WRAP
    read, steps = S.wrap_leftovers()
    assert len(read) == 420
    keys = S.window_keys([read], k, l, d)
    assert len(keys) >= 5                                                   # the read has windows, each at least 65,536 + A times in the first batch
    first, low = steps[0], steps[2]
    assert len(first[1]) - A >= 65536 and set(first[1]) == {read}           # count - A >= 65536: wrap_list_kernel ranks the slot
    assert low[2] < first[2] and low[2] + len(low[1]) <= first[2]
    assert keys <= S.window_keys(low[1], k, l, d)                           # the batch below holds every one of them
