"""Hand-built graphs in MINIMIZER SPACE and the plain model beside them (tests/test_sketch_graphs_cpu.py checks the catalogue against the references without a
GPU, tests/test_gpu_sketch_graphs.py feeds it to Mdbg.ingest_sketch and runs the graph stages on the result).

A read is a list of minimizer hashes with chosen positions, repeated to set abundances; the stages behind the node table (edges, unitigs, simplify,
components) never look at bases, so the graph is exactly the one written down: palindromic (k-1)-mers, self-neighbours, hubs, ties and limit boundaries on
purpose instead of by ntHash's luck.  nodes_from_sketch is written from oracle/mdbg_oracle.cpp (add_kminmer, process_read, filter) and from nothing else.

Every sketch stays within what a real one can be: hashes nonzero and below HASH_LIMIT (= the oracle's hash_bound(D), asserted in the CPU test), positions
strictly ascending and below 2^32, offsets from 0 and non-decreasing.  Small integers written out in a case go through remap(), which keeps their order:
the canonical orientation of a k-min-mer depends on it."""
import itertools
import random

import numpy as np

L, D = 10, 0.01                                # l and density of every context here (the (5, 10, 0.01, 2) set of tests/test_gpu_edges.py)
HASH_LIMIT = int(D * 18446744073709551616.0)   # hash_bound(D)
REMAP_STRIDE, REMAP_BASE, REMAP_MAX = 2_000_000_000_000_003, 977, 90
TIPS, BUBBLES, COMPONENTS = 1, 2, 4


def remap(v):
    """a written-out small integer (1 .. REMAP_MAX) as a hash: injective, order-preserving, nonzero, below HASH_LIMIT"""
    assert 1 <= v <= REMAP_MAX
    return REMAP_BASE + REMAP_STRIDE * v


def fresh(seed, n):
    """n distinct random hashes in [1, HASH_LIMIT)"""
    rnd = random.Random(seed)
    out = []
    while len(out) < n:
        h = rnd.randrange(1, HASH_LIMIT)
        if h not in out:
            out.append(h)
    return out


def mread(hashes, step=100, rev=False):
    """a minimizer-space read -> (hashes, ascending positions).  step: the distance between neighbours, or the list of positions itself;
    rev: the read as sequenced from the other strand (the hashes in reverse order: a minimizer hash is canonical)"""
    hashes = [int(h) for h in hashes]
    pos = [step * j for j in range(len(hashes))] if isinstance(step, int) else [int(p) for p in step]
    assert len(pos) == len(hashes) and all(a < b for a, b in zip(pos, pos[1:])) and (not pos or pos[-1] < 1 << 32)
    if rev:
        hashes = hashes[::-1]
        pos = [pos[-1] - p for p in reversed(pos)]
    return (tuple(hashes), tuple(pos))


def nodes_from_sketch(reads, k, l, A):
    """the node table of reads [(hashes, positions)] with ordinals 0, 1, ...: the dict of oracle.Graph.finalize(with_edges=False) without the edge and
    .sequences entries.  mdbg_oracle.cpp: process_read (windows only when a read has MORE than k minimizers; a window equal to its reverse counts as
    reversed), add_kminmer (the entry describes the sighting whose previous abundance is A - 1; the abundance is a u16 that wraps), filter (only when A > 1;
    rows in first-sighting order)."""
    table = {}
    wrap = 0xFFFF
    for ordinal, (H, P) in enumerate(reads):
        if len(H) <= k:
            continue
        for i in range(len(H) - k + 1):
            w = tuple(H[i:i + k])
            r = w[::-1]
            rev = not (w < r)
            first, last = P[i + 1] - P[i], P[i + k - 1] - P[i + k - 2]
            sighting = (P[i + k - 1] + 1 - P[i] + 1, last if rev else first, first if rev else last, ordinal, P[i], P[i + k - 1] + l, rev)
            e = table.get(r if rev else w)
            if e is None:
                e = table[r if rev else w] = [len(table), 0, sighting]
            if e[1] == ((A - 1) & wrap):
                e[2] = sighting
            e[1] = (e[1] + 1) & wrap
    rows = [(key, e) for key, e in table.items() if A <= 1 or e[1] >= A]          # dict order = index order
    n = len(rows)
    col = lambda f, t: np.array([f(key, e) for key, e in rows], dtype=t)
    return dict(n_nodes=n, n_nodes_before=len(table),
                keys=np.array([key for key, _ in rows], dtype=np.uint64).reshape(n, k),
                index=col(lambda key, e: e[0], np.uint32), abundance=col(lambda key, e: e[1], np.uint16),
                seqlen=col(lambda key, e: e[2][0] & 0xFFFFFFFF, np.uint32),
                shift=np.array([(e[2][1] & wrap, e[2][2] & wrap) for _, e in rows], dtype=np.uint16).reshape(n, 2),
                shift_full=np.array([(e[2][1], e[2][2]) for _, e in rows], dtype=np.uint64).reshape(n, 2),
                src_read=col(lambda key, e: e[2][3], np.uint64), src_start=col(lambda key, e: e[2][4], np.uint64),
                src_end=col(lambda key, e: e[2][5], np.uint64), reversed=col(lambda key, e: int(e[2][6]), np.uint8))


def fake_bases(reads, l, seed):
    """one ACGT string per read, of length positions[-1] + l (empty for a read without minimizers): the stages cut node sequences by position only.
    A read object that occurs several times gets the same string every time."""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    made, out = {}, []
    for rd in reads:
        if id(rd) not in made:
            made[id(rd)] = acgt[rs.randint(0, 4, rd[1][-1] + l)].tobytes() if rd[1] else b""
        out.append(made[id(rd)])
    return out


def sketch_arrays(reads):
    """-> (hashes u64, positions u32, offsets u64[n + 1]) of a list of reads, as mdbg_ingest_sketch takes them"""
    n = sum(len(h) for h, _ in reads)
    hashes = np.fromiter(itertools.chain.from_iterable(h for h, _ in reads), dtype=np.uint64, count=n)
    pos = np.fromiter(itertools.chain.from_iterable(p for _, p in reads), dtype=np.uint32, count=n)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(h) for h, _ in reads], dtype=np.uint64)
    return hashes, pos, off


def length_of_walk(nodes):
    """a walk's base length from seqlen-free fields alone (for the cases that skip the string side): the first node whole, every later node the shift_full
    on its far side (unitig_restatement.stitch); a node's sequence has src_end - src_start bases"""
    at = {int(i): r for r, i in enumerate(nodes["index"])}

    def length(walk):
        total = 0
        for j, (idx, o) in enumerate(walk):
            r = at[idx]
            ln = int(nodes["src_end"][r]) - int(nodes["src_start"][r])
            total += ln if j == 0 else min(ln, int(nodes["shift_full"][r][1 if o == "+" else 0]))
        return total
    return length


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """k, A, reads (in ordinal order), the presimp values to build edges with, the schedules to run (on the edges of presimps[0]), and what the references give:
    expect = dict(nodes=, edges={presimp: (rows, presimp_removed)}, unitigs=[(nodes, bases)] in unitig order,
                  removed={schedule: [sorted node indices per step]}, components=dict(nodes=, bases=, circular=), shifts=, overlaps=)
    split: the reads go in as two ingest_sketch batches, cut in front of read `split`; strings: False = no fake bases (the 65,535-abundance rows)"""

    def __init__(self, name, k, A, reads, presimps=(0.0,), schedules=(), expect=None, split=None, strings=True):
        self.name, self.k, self.A, self.reads = name, k, A, list(reads)
        self.presimps, self.schedules, self.expect, self.split, self.strings = tuple(presimps), [list(s) for s in schedules], dict(expect or {}), split, strings


def rm(values):
    return [remap(v) for v in values]


def _fork_cases():
    h = fresh(101, 23)
    spine, arm, head = h[:14], h[14:17], h[17:20]
    long_read, short_read = mread(spine), mread(spine[:6] + arm)
    T = TIPS
    tips = [[(T, 2, 0)], [(T, 3, 0)], [(T, 0, 0)], [(T, 0, 410)], [(T, 0, 1000)], [(T, 0, 409)], [(T, 3, 410)], [(T, 3, 409)], [(T, 2, 410)]]
    gone = {((T, 2, 0),): [[]], ((T, 3, 0),): [[12, 13, 14]], ((T, 0, 0),): [[12, 13, 14]], ((T, 0, 410),): [[12, 13, 14]], ((T, 0, 1000),): [[12, 13, 14]],
            ((T, 0, 409),): [[]], ((T, 3, 410),): [[12, 13, 14]], ((T, 3, 409),): [[]], ((T, 2, 410),): [[]]}
    shape = dict(nodes=15, edges={0.0: (28, 0)}, unitigs=[(4, 510), (8, 910), (3, 410)])
    yield Case("fork", 3, 2, [long_read] * 5 + [short_read] * 2, schedules=tips, expect=dict(shape, removed=gone), split=5)
    yield Case("fork, equal abundance", 3, 2, [long_read] * 5 + [short_read] * 5, schedules=[[(T, 0, 0)]],
               expect=dict(shape, removed={((T, 0, 0),): [[12, 13, 14]]}), split=3)
    # the same fork sequenced from the other strand: the rows come in another order (the trunk is seen last), the graph is the same
    yield Case("fork, mirrored", 3, 2, [mread(spine, rev=True)] * 5 + [mread(spine[:6] + arm, rev=True)] * 2, schedules=tips,
               expect=dict(nodes=15, edges={0.0: (28, 0)}, unitigs=[(8, 910), (4, 510), (3, 410)], removed=gone))
    # an arm that ENDS in the trunk: the dead end is the arm's first vertex (rows 0..11 the spine, 12..14 the arm: [h0 h1 h2], [h1 h2 s8], [h2 s8 s9])
    yield Case("fork, arm ends in the trunk", 3, 2, [long_read] * 5 + [mread(head + spine[8:])] * 2, schedules=tips,
               expect=dict(nodes=15, edges={0.0: (28, 0)}, unitigs=[(8, 910), (4, 510), (3, 410)], removed=gone))


def _bubble_cases():
    h = fresh(202, 24)
    a, c, b1, b2, b3, b4 = h[:6], h[6:12], h[12:14], h[14:16], h[16:18], h[18:21]
    one, two, three = mread(a + b1 + c), mread(a + b2 + c, rev=True), mread(a + b3 + c)
    B = BUBBLES
    shape = dict(nodes=16, edges={0.0: (32, 0)}, unitigs=[(4, 510)] * 4)
    for n1, n2, gone in ((7, 3, [12, 13, 14, 15]), (3, 7, [4, 5, 6, 7]), (5, 5, [12, 13, 14, 15])):
        yield Case("bubble %d/%d" % (n1, n2), 3, 2, [one] * n1 + [two] * n2, schedules=[[(B, 0, 0)]], expect=dict(shape, removed={((B, 0, 0),): [gone]}),
                   split=n1 - 1)
    # the limits sit exactly on both branches (4 nodes, 510 bases): one node or one base less and neither is small
    yield Case("bubble at the limits", 3, 2, [one] * 7 + [two] * 3, schedules=[[(B, 4, 510)], [(B, 3, 510)], [(B, 4, 509)], [(B, 4, 0)], [(B, 3, 0)], [(B, 0, 510)], [(B, 0, 509)]],
               expect=dict(shape, removed={((B, 4, 510),): [[12, 13, 14, 15]], ((B, 3, 510),): [[]], ((B, 4, 509),): [[]], ((B, 4, 0),): [[12, 13, 14, 15]], ((B, 3, 0),): [[]],
                                           ((B, 0, 510),): [[12, 13, 14, 15]], ((B, 0, 509),): [[]]}))
    # the WEAKER branch is the larger one (5 nodes, 610 bases): the limits sit on it alone, the stronger branch is small either way
    yield Case("bubble, weaker branch at the limits", 3, 2, [one] * 7 + [mread(a + b4 + c)] * 3,
               schedules=[[(B, 5, 610)], [(B, 4, 610)], [(B, 5, 609)], [(B, 5, 0)], [(B, 4, 0)], [(B, 0, 610)], [(B, 0, 609)]],
               expect=dict(nodes=17, edges={0.0: (34, 0)}, unitigs=[(4, 510), (4, 510), (4, 510), (5, 610)],
                           removed={((B, 5, 610),): [[12, 13, 14, 15, 16]], ((B, 4, 610),): [[]], ((B, 5, 609),): [[]], ((B, 5, 0),): [[12, 13, 14, 15, 16]], ((B, 4, 0),): [[]],
                                    ((B, 0, 610),): [[12, 13, 14, 15, 16]], ((B, 0, 609),): [[]]}))
    # three branches: the most abundant stays, whichever read order brought it in
    yield Case("bubble, three branches", 3, 2, [one] * 3 + [two] * 6 + [three] * 4, schedules=[[(B, 0, 0)]],
               expect=dict(nodes=20, edges={0.0: (42, 0)}, unitigs=[(4, 510)] * 5, removed={((B, 0, 0),): [[4, 5, 6, 7, 16, 17, 18, 19]]}))
    yield Case("bubble, three branches, tie", 3, 2, [one] * 4 + [two] * 4 + [three] * 4, schedules=[[(B, 0, 0)]],
               expect=dict(nodes=20, edges={0.0: (42, 0)}, unitigs=[(4, 510)] * 5, removed={((B, 0, 0),): [[12, 13, 14, 15, 16, 17, 18, 19]]}))


def _presimp_cases():
    h = fresh(303, 11)
    hub, x, y = h[:5], h[5:8], h[8:11]
    big_read, small_read = mread(hub + x), mread(hub + y)
    for big, small, p, rows, removed in ((100, 1, 0.01, 16, 0), (200, 1, 0.01, 14, 1), (99, 1, 0.01, 16, 0), (4, 2, 0.5, 16, 0), (5, 2, 0.5, 14, 1),
                                         (65535, 656, 0.01, 16, 0), (65535, 655, 0.01, 16, 0),
                                         # 0.01f and 0.5f times a u16 never round ACROSS an integer (0.01f lies below 0.01: the exact product is below the integer the f32
                                         # product rounds to, and `<` says the same for both).  0.1f and 0.3f lie above 0.1 and 0.3: at 10/1 and 10/3 the f32 product is
                                         # exactly 1.0 and 3.0 (the edge stays), the exact product is 1.000000015 and 3.00000012 (it would go)
                                         (10, 1, 0.1, 16, 0), (11, 1, 0.1, 14, 1), (10, 3, 0.3, 16, 0), (10, 2, 0.3, 14, 1)):
        yield Case("presimp %d/%d at %g" % (big, small, p), 3, 1, [big_read] * big + [small_read] * small, presimps=(p, 0.0),
                   expect=dict(nodes=9, edges={p: (rows, removed), 0.0: (16, 0)}), strings=big < 1000)
    # the hub's three nodes are seen 65,536 times: their u16 abundance is 0.  With A = 1 nothing is filtered (mdbg_oracle.cpp, filter(): only when minabund > 1,
    # as src/main.rs:922-929 says on purpose), so they STAY, with abundance 0, and the edge rules see aref = min(amax, 0) = 0: nothing is removed
    yield Case("presimp 65535/1 at 0.01", 3, 1, [big_read] * 65535 + [small_read], presimps=(0.01, 0.0), expect=dict(nodes=9, edges={0.01: (16, 0), 0.0: (16, 0)}, n_unitigs=3),
               strings=False)


ODD = [(3, [5, 7, 7, 5, 9, 11, 13], 4, 8, 1), (3, [5, 5, 5, 5, 5, 5], 1, 16, 1), (4, [1, 2, 3, 3, 2, 1, 4, 5], 4, 12, 2), (3, [1, 2, 1, 2, 1, 2, 1, 3], 3, 40, 3),
       (4, [1, 2, 3, 2, 1, 2, 3, 2, 1], 2, 6, 1), (2, [1, 2, 1, 3, 1, 4, 1, 1], 4, 58, 4)]


def odd_name(k, written):
    return "odd k=%d %s" % (k, "-".join(str(v) for v in written))


def _odd_cases():
    """palindromic (k-1)-mers and k-min-mers, a node that is its own neighbour in all four orientations, pairs of nodes joined by several edges"""
    for k, written, n_nodes, n_edges, n_unitigs in ODD:
        yield Case(odd_name(k, written), k, 1, [mread(rm(written)), mread(rm(written), rev=True)], presimps=(0.0, 0.5),
                   schedules=[[(TIPS, 0, 0), (BUBBLES, 0, 0)]], expect=dict(nodes=n_nodes, edges={0.0: (n_edges, 0), 0.5: (n_edges, 0)}, n_unitigs=n_unitigs))


GAP_HASHES = [9, 3, 8, 5, 6, 2, 4, 7]          # the order of the values fixes the orientation of every window, and with it the recorded shifts


def _gap_case():
    h = rm(GAP_HASHES)
    yield Case("gaps", 3, 1, [mread(h, [0, 70000, 70100, 140100, 140200, 140300, 300000, 300100]), mread(h[2:][::-1], [0, 100, 200, 70000, 70100, 140200])],
               presimps=(0.0, 0.5), expect=dict(nodes=6, edges={0.0: (10, 0)}, shifts=[[100, 4464]] * 3 + [[100, 100]] + [[28628, 100]] * 2,
                                                overlaps=[65638, 70002, 65638, 70002, 201, 102, 102, 201, 159702, 159702]))


def _hub_case():
    """40 reads around one shared (k-1)-mer: both listings of it are dozens of nodes long, and every node before it meets every node behind it"""
    h = fresh(404, 2 + 40 * 6)
    shared, own = h[:2], h[2:]
    reads = [mread(own[6 * i:6 * i + 3] + shared + own[6 * i + 3:6 * i + 6], step=[100, 1, 70000][i % 3] if i % 5 == 0 else 100, rev=i % 4 == 1) for i in range(40)]
    yield Case("hub", 3, 1, reads, presimps=(0.0, 0.01, 0.5), schedules=[[(TIPS, 0, 0)], [(TIPS, 2, 0), (BUBBLES, 0, 0)]], expect=dict(nodes=240, edges={0.0: (3520, 0), 0.01: (3520, 0), 0.5: (3520, 0)}, n_unitigs=80))


def _island_cases():
    h = fresh(505, 24)
    p9, p5, p4, ring = h[:9], h[9:14], h[14:18], h[18:24]
    reads = [mread(p9)] * 2 + [mread(p5)] * 2 + [mread(p4)] * 3 + [mread(ring + ring[:3])] * 2
    K = COMPONENTS
    cc = dict(nodes=[7, 3, 2, 6], bases=[810, 410, 310, 710], circular=[False, False, False, True])
    sched = [[(K, 2, 0)], [(K, 3, 0)], [(K, 1, 0)], [(K, 0, 310)], [(K, 0, 309)], [(K, 2, 310)], [(K, 2, 309)], [(K, 1, 310)], [(K, 0, 1000)], [(TIPS, 0, 0), (K, 3, 410), (BUBBLES, 0, 0)]]
    gone = {((K, 2, 0),): [[10, 11]], ((K, 3, 0),): [[7, 8, 9, 10, 11]], ((K, 1, 0),): [[]], ((K, 0, 310),): [[10, 11]], ((K, 0, 309),): [[]], ((K, 2, 310),): [[10, 11]],
            ((K, 2, 309),): [[]], ((K, 1, 310),): [[]], ((K, 0, 1000),): [list(range(12))], ((TIPS, 0, 0), (K, 3, 410), (BUBBLES, 0, 0)): [[], [7, 8, 9, 10, 11], []]}
    yield Case("islands", 3, 2, reads, schedules=sched, expect=dict(nodes=18, unitigs=[(7, 810), (3, 410), (2, 310), (6, 710)], components=cc, removed=gone), split=4)


def _short_read_case():
    """an empty read, a read of exactly k minimizers (no window: the reference asks for MORE than k) and one of k + 1 (two windows)"""
    h = fresh(606, 12)
    k = 3
    reads = [mread([]), mread(h[:k]), mread(h[:k + 1]), mread([]), mread(h[4:5]), mread(h[1:k + 3]), mread(h[5:5 + k]), mread([])]
    yield Case("short reads", k, 1, reads, presimps=(0.0, 0.01), schedules=[[(TIPS, 0, 0)]], expect=dict(nodes=4, edges={0.0: (6, 0), 0.01: (6, 0)}, unitigs=[(4, 510)], removed={((TIPS, 0, 0),): [[]]}), split=3)


def _all_cases():
    for make in (_fork_cases, _bubble_cases, _presimp_cases, _odd_cases, _gap_case, _hub_case, _island_cases, _short_read_case):
        yield from make()


CASES = list(_all_cases())
CASE_IDS = [c.name for c in CASES]


# ---- random minimizer-space graphs -----------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = list(range(8))                  # all admissible: asserted in tests/test_sketch_graphs_cpu.py


def random_case(seed):
    """a 'genome' of 300 hashes over an alphabet of only 40 values (repeats, palindromes and hubs are dense), 120 reads as random slices of it, half of them
    reversed; neighbouring minimizers lie 1, 100 or 70,000 bases apart (70,000 for one gap in a hundred: the reads stay small enough to have strings).
    -> (k, A, presimp, reads)"""
    rnd = random.Random(9100 + seed)
    k, A, presimp = [2, 3, 4][seed % 3], [1, 2][(seed // 3) % 2], [0.0, 0.01, 0.5][(seed + seed // 3) % 3]
    genome = [remap(rnd.randint(1, 40)) for _ in range(300)]
    at = [0]
    for _ in range(299):
        r = rnd.random()
        at.append(at[-1] + (70000 if r < 0.01 else 1 if r < 1 / 3 else 100))
    reads = []
    for _ in range(120):
        n = rnd.randint(0, 60)
        a = rnd.randrange(0, 300 - n + 1)
        reads.append(mread(genome[a:a + n], [p - at[a] for p in at[a:a + n]], rev=rnd.random() < 0.5))
    return k, A, presimp, reads
