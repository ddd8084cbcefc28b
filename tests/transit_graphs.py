"""Hand-built repeats in MINIMIZER SPACE for the transit tests (tests/test_transits_cpu.py, tests/test_gpu_transits.py), made with sketch_graphs.mread and
sketch_graphs.fresh; k = 3 throughout.  Every case carries expectations written down by hand from the definition of include/mdbg_hip.h (mdbg_graph_transits):
the number of keys, the passes, the sorted counts, the repeats, and per min_support the number of resolved repeats.

A flank is a run of fresh hashes that occurs in one place of the 'genome'; a repeat R of r hashes is shared by several paths.  With k = 3 a repeat of r = 2 = k - 1
hashes is the 2 x 2 cross of edges (no unitig of its own); r >= 3 gives a repeat unitig of r - k + 1 entries."""
import random

import sketch_graphs as G

EDGES = 8
K = 3


class TCase:
    """k, A, reads (in ordinal order), the presimp the edges are built with, the schedule to run first (or None: the plain list), split (the reads go in as two
    batches, cut in front of read `split`) and expect = dict(transits=, passes=, counts=[sorted], repeats=, resolved={min_support: n_resolved}[, walks=sorted
    entry counts of the unitigs][, selfs=number of SELF verdicts][, missing=True: the junctions report n_missing > 0])"""

    def __init__(self, name, reads, expect, A=1, presimp=0.0, steps=None, split=None, k=K):
        self.name, self.k, self.A, self.reads, self.presimp, self.steps, self.split, self.expect = name, k, A, list(reads), presimp, steps, split, dict(expect)


def flanks(seed, n, r, size=6):
    """n flanks of `size` fresh hashes each and a repeat of r"""
    h = G.fresh(seed, n * size + r)
    return [h[i * size:(i + 1) * size] for i in range(n)], h[n * size:]


def cross_reads(seed, r, times=3):
    (a, b, c, d), rep = flanks(seed, 4, r)
    return [G.mread(a + rep + b)] * times + [G.mread(c + rep + d, rev=True)] * times, (a, b, c, d), rep


def _cross_cases():
    # r = 2 = k - 1: the repeat is no node's interior, the four flanks meet in a 2 x 2 cross of edges; nothing is walked from end to end
    yield TCase("cross r=2", cross_reads(701, 2)[0], dict(transits=0, passes=0, counts=[], repeats=0, resolved={1: 0, 2: 0, 4: 0}))
    # r = 3: ONE window lies inside the repeat; both crossings of a transit sit on neighbouring indices.  A..R and C..R take 6 entries each (4 windows inside the
    # flank and 2 that reach into R), so do R..B and R..D
    yield TCase("cross r=3", cross_reads(702, 3)[0], dict(transits=2, passes=6, counts=[3, 3], repeats=1, resolved={1: 1, 2: 1, 3: 1, 4: 0}, walks=[1, 6, 6, 6, 6]))
    yield TCase("cross r=8", cross_reads(703, 8)[0], dict(transits=2, passes=6, counts=[3, 3], repeats=1, resolved={1: 1, 2: 1, 3: 1, 4: 0}, walks=[6, 6, 6, 6, 6]), split=3)
    # one read that takes A's entrance and D's exit: a third key of count 1 shares p with one strong key and q with the other at min_support 1, and is weak at 2
    reads, (a, b, c, d), rep = cross_reads(704, 5)
    yield TCase("mixed", reads + [G.mread(a + rep + d)], dict(transits=3, passes=7, counts=[1, 3, 3], repeats=1, resolved={1: 0, 2: 1, 3: 1, 4: 0}), split=4)
    # no read reaches from one end of the repeat (2 entries) to the other
    (a, b, c, d), rep = flanks(705, 4, 4)
    yield TCase("unspanned", [G.mread(a + rep[:3]), G.mread(rep[1:] + b), G.mread(c + rep[:3], rev=True), G.mread(rep[1:] + d)],
                dict(transits=0, passes=0, counts=[], repeats=1, resolved={1: 0, 2: 0}))


def _three_way_cases():
    f, rep = flanks(706, 6, 4)
    yield TCase("three-way", [G.mread(f[i] + rep + f[3 + i], rev=i == 1) for i in range(3) for _ in range(2)],
                dict(transits=3, passes=6, counts=[2, 2, 2], repeats=1, resolved={1: 1, 2: 1, 3: 0}))
    # the third path leaves by the second path's exit: 3 entrances, 2 exits
    yield TCase("three-way, one exit fewer", [G.mread(f[i] + rep + f[3 + min(i, 1)]) for i in range(3) for _ in range(2)],
                dict(transits=3, passes=6, counts=[2, 2, 2], repeats=1, resolved={1: 0, 2: 0}))


def _ring_case():
    # 6 hashes in a ring give 6 nodes; three and a half turns of the ring are 21 minimizers, 19 windows: the read's first window is entry 0, the walk runs
    # against the read, so the pairs 0, 6 and 12 wrap (0 -> 5): 3 crossings on the closing record's key, 2 transits a read
    ring = G.fresh(707, 6)
    read = G.mread((ring * 4)[:21])
    yield TCase("ring", [read, read], dict(transits=1, passes=4, counts=[4], repeats=0, resolved={1: 0}, walks=[6]))


def _break_cases():
    # A = 2: the windows that hold the changed middle hash are seen once and are no nodes; that read's chain breaks inside R
    reads, (a, b, c, d), rep = cross_reads(708, 5)
    other = rep[:2] + G.fresh(7080, 1) + rep[3:]
    yield TCase("break by an unplaced window", reads + [G.mread(a + other + b)], dict(transits=2, passes=6, counts=[3, 3], repeats=1, resolved={1: 1, 3: 1, 4: 0}), A=2)
    # read 6 ends on the first window of R (the window behind its crossing into R), read 7 starts on the second and leaves: no transit between them
    reads, (a, b, c, d), rep = cross_reads(709, 8)
    for split in (None, 7):
        yield TCase("break at a read boundary" + ("" if split is None else ", batches split there"), reads + [G.mread(a + rep[:3]), G.mread(rep[1:] + b)],
                    dict(transits=2, passes=6, counts=[3, 3], repeats=1, resolved={1: 1, 3: 1, 4: 0}), split=split)
    # two repeats S1 and S2 of one entry each with a 2 x 2 cross (r = 2) between them.  The one read that changes sides in the cross is crossed by fewer than 2
    # reads there: the EDGES step removes that record, and the read's chain  P1 -> S1 -> A ... [missing] ... D -> S2 -> Q1  breaks between S1's exit and S2's
    # entrance.  It still passes S1 and S2: counts 4 and 3 on each
    (p1, p2, e1, a, b, c, d, e2, q1, q2), h = flanks(710, 10, 8)
    s1, rr, s2 = h[:3], h[3:5], h[5:8]
    reads = [G.mread(p1 + s1 + a + rr + b)] * 3 + [G.mread(p2 + s1 + e1, rev=True)] * 3 + [G.mread(c + rr + d + s2 + q1)] * 3 + [G.mread(e2 + s2 + q2)] * 3
    reads.append(G.mread(p1 + s1 + a + rr + d + s2 + q1))
    yield TCase("break by a missing crossing", reads, dict(transits=4, passes=14, counts=[3, 3, 4, 4], repeats=2, resolved={1: 2, 3: 2, 4: 0}, missing=True),
                steps=[(EDGES, 2, 0)], split=6)


def _long_case():
    # the two crossings of a transit lie 5,000 - k + 1 windows apart: in different workgroups of every kernel and different blocks of the scan
    reads = cross_reads(711, 5000, times=1)[0]
    yield TCase("long", reads, dict(transits=2, passes=2, counts=[1, 1], repeats=1, resolved={1: 1, 2: 0}, walks=[6, 6, 6, 6, 4998]))


def _all():
    for make in (_cross_cases, _three_way_cases, _ring_case, _break_cases, _long_case):
        yield from make()


CASES = list(_all())
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
SELF_CASE = "odd k=3 5-5-5-5-5-5"          # of sketch_graphs.CASES: one unitig that is its own neighbour; random seed 0: every unitig is


def many_crosses(n, seed=712):
    """n crosses of r = 3 side by side, flanks of 4: 2 n distinct transit keys of count 1, n resolved repeats (for more keys than one block of the sort holds)"""
    h = random.Random(seed).sample(range(1, G.HASH_LIMIT), 19 * n)
    reads = []
    for i in range(n):
        g = h[19 * i:19 * i + 19]
        a, b, c, d, rep = g[:4], g[4:8], g[8:12], g[12:16], g[16:]
        reads += [G.mread(a + rep + b), G.mread(c + rep + d, rev=i % 2 == 1)]
    return reads
