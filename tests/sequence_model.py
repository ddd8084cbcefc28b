"""Operation sequences on ONE context and the plain model beside them (tests/test_gpu_sequences.py walks them on the GPU, tests/test_sequences_cpu.py with the
oracle alone).  The model is the list of (reads, first ordinal) that is resident, in call order, plus the current k; the expected node table at any point is a
FRESH oracle graph fed the model's batches in ascending ordinal order.  Everything here is seeded data: a sequence is a dict of parameters and a list of
operations, each a dict, so that both tests walk exactly the same operations.

What the sequences are after is the state a context keeps from one finalize to the next (the claim map's marks, the speculative row count, the ranks
wrap_list_kernel leaves in the slots, the cached batch table): finalize and ingest alternate, and the ordinals arrive in any order."""
import random

import numpy as np

from oracle import oracle as O
from test_gpu_fuzz import fuzz_reads
from test_gpu_parity import rand_reads

PARAMS = [(3, 8, 0.05, 2), (5, 10, 0.03, 1), (7, 10, 0.05, 2), (4, 6, 0.05, 3)]      # (k, l, density, minabund): the small sets of the fuzz tests
RESET_KS = [3, 4, 5, 7]
N_SEEDS = 40
SPAN = 1000                    # span i holds the ordinals [1000 i, 1000 i + 1000): a batch has at most 10 reads, so spans never touch
MAX_READS = 60                 # resident reads per context
PRESIMP = 0.01
TIMERS = ("ms_sketch", "ms_insert", "ms_finalize")


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, k, l, d, A):
        self.k, self.l, self.d, self.A = k, l, d, A
        self.batches = []          # (reads, first ordinal) in call order

    def expected(self, with_edges=False):
        """the oracle's table of what is resident: a fresh graph, the batches in ascending ordinal order"""
        g = O.Graph(self.k, self.l, self.d, self.A, presimp=PRESIMP)
        for reads, first in sorted(self.batches, key=lambda t: t[1]):
            b, o = O.concat_reads(reads)
            assert g.ingest(b, o, first) == 0
        return g.finalize(with_edges=with_edges)

    def apply(self, op):
        """what the operation does to the resident batches (finalize, sketch, query, mark: nothing)"""
        what = op["op"]
        if what == "ingest":
            self.batches.append((op["reads"], op["first"]))
        elif what == "reset":
            self.k = op["k"]
        elif what == "reset0":
            self.batches = []
        elif what == "rewind":                         # rewind(mark) + reset(k): the batches registered after the mark are gone
            self.batches = self.batches[:op["mark"]]


def spans_overlap(batches):
    """two resident batches whose ordinal ranges [first, first + n) meet"""
    iv = sorted((first, first + len(reads)) for reads, first in batches)
    return any(iv[i][1] > iv[i + 1][0] for i in range(len(iv) - 1))


def edge_rows(exp):
    """the oracle's edges (finalize(with_edges=True)) as sorted rows, like the rows of graph_edges()"""
    return sorted(zip(exp["edge_n1"].tolist(), exp["edge_o1"].tolist(), exp["edge_n2"].tolist(), exp["edge_o2"].tolist(), exp["edge_overlap"].tolist()))


def window_keys(reads, k, l, d):
    """canonical k-min-mers of a batch as a plain set of tuples (reads with MORE than k minimizers only: src/main.rs:950)"""
    b, o = O.concat_reads(reads)
    sk = O.sketch(b, o, l, d)
    assert sk["err"] == 0
    out = set()
    for r in range(len(reads)):
        h = [int(x) for x in sk["hashes"][int(sk["off"][r]):int(sk["off"][r + 1])]]
        if len(h) > k:
            for i in range(len(h) - k + 1):
                w = tuple(h[i:i + k]); rv = w[::-1]
                out.add(w if w < rv else rv)
    return out


def out_of_order_finalizes(ops):
    """finalize calls that see a batch which arrived, in the life of one table, AFTER an earlier finalize and BELOW a batch that finalize had seen: the
    combination in which a first sighting can move between two finalize calls.  (A table's life ends with reset, reset(0) and rewind.)"""
    resident, seen_top, pending, hits = [], None, False, 0
    for op in ops:
        what = op["op"]
        if what == "ingest":
            if seen_top is not None and op["first"] < seen_top:
                pending = True
            resident.append(op["first"])
        elif what == "finalize":
            if pending:
                hits += 1
            if resident:
                seen_top = max(resident)
        elif what in ("reset", "reset0", "rewind"):
            seen_top, pending = None, False
            if what == "reset0":
                resident = []
            elif what == "rewind":
                resident = resident[:op["mark"]]
    return hits


def certain_stale_marks(steps, k, l, d):
    """The claim map as the finalize BEFORE the ordinal rule kept it, at the grain of batches: steps = [("ingest", reads, first) | ("finalize",)] in call
    order, one table life.  A key's claimer lies in the first batch (call order) that holds it; a finalize clears the claimer's byte and marks the key's earliest
    sighting = a window of the resident batch with the smallest ordinal that holds it.  A mark an earlier finalize left in a batch that is neither the claimer's
    nor the one marked now stays for good: the key is counted twice.  -> per finalize, the number of keys with such a mark (marks inside the claimer's own batch
    depend on which window won the claim and are not counted: the result is a lower bound)."""
    claimer, marks, holders, out = {}, {}, {}, []
    for st in steps:
        if st[0] == "ingest":
            for key in window_keys(st[1], k, l, d):
                claimer.setdefault(key, st[2])
                holders.setdefault(key, set()).add(st[2])
        else:
            stale = 0
            for key, hs in holders.items():
                at = min(hs)
                ms = marks.setdefault(key, set())
                ms.discard(claimer[key])                  # by_first[ic] = 0 ...
                ms.add(at)                                # ... by_first[at] = 1 | 3
                stale += 1 if len(ms) > 1 else 0
            out.append(stale)
    return out


# ---- seeded sequences ------------------------------------------------------------------------------------------------------------------------------------
def gen_sequence(seed):
    """-> dict(k, l, d, A, hint, no_claims, policy, ops).  8 - 14 operations; at most MAX_READS resident reads of up to 3,000 bases, sampled from a 20 - 40 kb
    genome in both orientations with 1 % errors so that keys repeat across batches; every sequence holds a finalize that out_of_order_finalizes() counts."""
    rnd = random.Random(90000 + seed)
    k, l, d, A = PARAMS[(seed // 4) % len(PARAMS)]
    hint = 16 if seed % 2 == 0 else 0                   # half the seeds: a table that grows and is rehashed between finalize calls
    no_claims = (seed // 2) % 2 == 1                    # half the seeds (of either half above): the byte-map finalize
    policy = ("asc", "desc", "rand")[seed % 3]
    pool = [r[:3000] for r in fuzz_reads(rnd, n_reads=160, genome_len=rnd.randint(20000, 40000), mean_len=1500, err=0.01, p_lower=0.0, p_n=0.0, p_hp=0.0)]
    used, resident, ops = set(), [], []                 # resident: (span, n_reads) in call order
    state = dict(k=k, mark=None, next_read=0, cursor=rnd.randint(20, 30) if policy != "desc" else rnd.randint(30, 35))

    def take(n):
        reads = pool[state["next_read"]:state["next_read"] + n]
        state["next_read"] += n
        return reads

    def pick_span(below=None):
        if below is not None:
            s = below - 1 - rnd.randint(0, 1)
            while s in used:
                s -= 1
        elif policy == "asc":
            s = state["cursor"]; state["cursor"] += 1 + rnd.randint(0, 2)
        elif policy == "desc":
            s = state["cursor"]; state["cursor"] -= 1 + rnd.randint(0, 2)
        else:
            s = rnd.choice([x for x in range(5, 56) if x not in used])
        assert s >= 0 and s not in used
        used.add(s)
        return s

    def ingest(below=None):
        n = rnd.randint(4, 10)
        s = pick_span(below)
        resident.append((s, n))
        ops.append(dict(op="ingest", reads=take(n), first=s * SPAN, entry=rnd.choice(["reads", "packed", "resident"])))

    def finalize():
        ops.append(dict(op="finalize", variant=rnd.choice(["host", "host", "device", "gfa"]), twice=rnd.random() < 0.3, edges=rnd.random() < 0.3))

    ingest()
    n_ops = rnd.randint(8, 10)
    while len(ops) < n_ops:
        r = rnd.random()
        n_res = sum(n for _, n in resident)
        if r < 0.38:
            if n_res + 10 > MAX_READS:
                finalize()
            else:
                ingest()
        elif r < 0.66:
            finalize()
        elif r < 0.72:
            state["k"] = rnd.choice(RESET_KS)
            ops.append(dict(op="reset", k=state["k"]))
        elif r < 0.76:
            resident, state["mark"] = [], None
            ops.append(dict(op="reset0"))
        elif r < 0.83 or (r < 0.90 and state["mark"] is None):
            state["mark"] = len(resident)
            ops.append(dict(op="mark", mark=state["mark"]))
        elif r < 0.90:
            resident = resident[:state["mark"]]
            ops.append(dict(op="rewind", mark=state["mark"], k=state["k"]))
        elif r < 0.95 or not resident:
            ops.append(dict(op="sketch", reads=[rnd.choice(pool) for _ in range(rnd.randint(1, 6))]))
        else:
            ops.append(dict(op="query", reads=[rnd.choice(pool) for _ in range(rnd.randint(1, 6))]))
    if not out_of_order_finalizes(ops):                # up to four more: (a batch,) a finalize, a batch below everything resident, a finalize
        if not resident:
            ingest()
        finalize()
        ingest(below=min(s for s, _ in resident))
        finalize()
    assert 8 <= len(ops) <= 14 and out_of_order_finalizes(ops)
    return dict(k=k, l=l, d=d, A=A, hint=hint, no_claims=no_claims, policy=policy, ops=ops)


# ---- directed inputs -------------------------------------------------------------------------------------------------------------------------------------
K, L, D = 7, 10, 0.05          # as tests/test_gpu_store_bookkeeping.py


def _shifted(base, cut, seed, n_fresh=10):
    """the reads of `base` without their first `cut` bases (the same minimizers behind them) plus fresh reads"""
    return [r[cut:] for r in base] + rand_reads(seed, n_fresh, 300, 3000)


def _steps_to_ops(steps):
    return [dict(op="ingest", reads=s[1], first=s[2], entry="reads") if s[0] == "ingest" else dict(op="finalize", variant="host", twice=False, edges=False) for s in steps]


def descending_triple():
    """B2 at 2000, B1 at 1000, finalize, B0 at 0, finalize: the claimer of a shared key lies in B2, the first finalize moves its mark into B1, the second into B0"""
    base = rand_reads(1234, 30, 300, 3000)
    b2, b1, b0 = base, _shifted(base[:20], 20, 1235), _shifted(base[5:25], 35, 1236)
    return [("ingest", b2, 2000), ("ingest", b1, 1000), ("finalize",), ("ingest", b0, 0), ("finalize",)]


def mode1_then_mode2():
    """ascending B0, B1 and a finalize (dense order = store order), then two batches below them, each followed by a finalize"""
    base = rand_reads(2234, 20, 300, 3000)
    return [("ingest", base, 2000), ("ingest", _shifted(base[:14], 20, 2235, 6), 3000), ("finalize",),
            ("ingest", _shifted(base[3:17], 35, 2236, 6), 1000), ("finalize",), ("ingest", _shifted(base[5:19], 50, 2237, 6), 0), ("finalize",)]


def interleaved():
    """ordinals 3000, 1000, 4000, 0, 2000, a finalize after every ingest"""
    base = rand_reads(3234, 12, 300, 3000)
    steps = []
    for i, first in enumerate((3000, 1000, 4000, 0, 2000)):
        steps += [("ingest", base if i == 0 else _shifted(base, 15 * i, 3235 + i, 4), first), ("finalize",)]
    return steps


DIRECTED = dict(descending_triple=descending_triple, mode1_then_mode2=mode1_then_mode2, interleaved=interleaved)
MIN_STALE = 50                 # keys that the move-only claim map counts twice at the last finalize of a directed input


def shared_in_all(steps, k, l, d):
    """keys present in every batch of the steps"""
    sets = [window_keys(s[1], k, l, d) for s in steps if s[0] == "ingest"]
    return set.intersection(*sets)


SPEC = (3, 8, 0.05, 2)         # the speculation cases


def guess_of(n):
    """fin_rows_guess after a finalize of n rows (finalize_end_impl)"""
    return n + n // 4 + 1024


def speculation_up():
    """a handful of reads, finalize; then enough duplicated reads that the second table is far larger than the rows the first one makes the second write ahead"""
    few = rand_reads(4234, 3, 2000, 3000)
    many = rand_reads(4235, 28, 2900, 3000)
    return [("ingest", few + few, 0), ("finalize",), ("ingest", many + many, 1000), ("finalize",)]


def speculation_down():
    """the reverse: the large table first, then rewind + reset to the handful of reads in front of the mark, finalize, a few more, finalize"""
    few = rand_reads(4234, 3, 2000, 3000)
    many = rand_reads(4235, 28, 2900, 3000)
    return [dict(op="ingest", reads=few + few, first=0, entry="reads"), dict(op="mark", mark=1), dict(op="ingest", reads=many + many, first=1000, entry="reads"),
            dict(op="finalize", variant="host", twice=False, edges=False), dict(op="rewind", mark=1, k=SPEC[0]), dict(op="finalize", variant="host", twice=False, edges=False),
            dict(op="ingest", reads=few[:2], first=2000, entry="reads"), dict(op="finalize", variant="host", twice=False, edges=False)]


WRAP = (3, 8, 0.05, 2)         # as the wrap test of tests/test_gpu_round6.py


def wrap_leftovers():
    """one 420-base read 65,536 + A times (its nodes' u16 abundance wraps: wrap_list_kernel ranks their slots), finalize, then a batch BELOW it that holds the
    read once more and others, finalize"""
    rnd = random.Random(3)
    read = bytes(rnd.choice(b"ACGT") for _ in range(420))
    other = [bytes(rnd.choice(b"ACGT") for _ in range(900)) for _ in range(6)]
    return read, [("ingest", [read] * (65536 + WRAP[3]), 1000), ("finalize",), ("ingest", other + other + [read], 0), ("finalize",)]
