"""Hand-built NESTED repeats in MINIMIZER SPACE for the nested-repeat tests (tests/test_nested_cpu.py, tests/test_gpu_nested.py), made with sketch_graphs.mread
and sketch_graphs.fresh in the style of tests/transit_graphs.py; k = 3 throughout.  Every case names a schedule and the sorted entry counts of the unitigs
that are left, worked out by hand from include/mdbg_hip.h (MDBG_SIMPLIFY_NESTED), and every case is SHARP: it names a second run (another schedule, or the
reads without the ones in question) and what must differ between the two —
  "list":       the checker's unitig list.  Used wherever the rule under test can change a list at all;
  "placement":  the checker's four placement counts (ambiguous, resolved, conflicts, unanchored).  Used for the rules that by the definition itself can never
                change a list: a candidate lies in its anchor's unitig, so the windows of an ambiguous run sit inside one unitig between their anchors and
                are links there, and a read that starts, ends or breaks inside the run crosses nothing with them.  What a wrong placement would change is
                exactly those counts, which the library prints for the GPU test (MDBG_NESTED_STATS).

With k = 3 a stretch of r hashes shared by several paths is a unitig of r - 2 entries; a flank of f fresh hashes in front of it takes f entries (its last two
windows reach into the stretch).

The nested family.  R = x u y occurs twice (A1 R B1, A2 R B2), its middle u a third time (Cin u Cout).  On the plain list u has two ways in and two out, while
the x part has two in and ONE out: plain.  [(REPEATS)] copies u; x + u + y is then one unitig of |x| + |u| - 2 + |y| entries with two ways in and two out, half
of whose rows belong to two entries.  [(REPEATS), (NESTED)] resolves it.

The tail family.  A x u y B1, Cin u Cout, and E joining on the last two hashes of u: E u[-2:] y B2.  The unitig Y starts right behind u and has two ways in (u,
E) and two out (B1, B2).  The REPEATS step runs at min_support 3 and resolves u only (Y's keys are seen twice); then W = A x u ends with the copied stretch, and
Y's key from W needs the crossing W -> Y, whose first window is ambiguous.  A read that starts in x places it by its LEFT anchor alone (the right one lies in Y,
another unitig); one that starts inside u has no anchor and must not count.  Reversed reads make it the right anchor and a read that ENDS inside.
The last window of E, (e, u3, u4), overlaps the first window of Cout, (u3, u4, d), as well: the graph holds the edge E -> Cout that no read takes (the 2 x 2 cross
of tests/transit_graphs.py), so Cout keeps two ways in and E two ways out, and both stay unitigs of their own unless an EDGES step in front prunes that edge."""
import sketch_graphs as G

TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS, NESTED = 1, 2, 4, 8, 16, 128
K = 3
PW_SPAN = 1024                                  # minimizer indices per workgroup of place_windows_kernel


class NCase:
    """reads in ordinal order, the schedule, expect = the sorted entry counts of the unitigs left, counts = the checker's placement counts summed over the
    NESTED steps on a graph with copies (or None: not pinned), and the second run: other_steps / other_reads (None: the same) with differs = "list" | "placement"
    and other_counts = the second run's placement counts (or None: only required to differ)"""

    def __init__(self, name, reads, steps, expect, differs, other_steps=None, other_reads=None, counts=None, A=1, split=None, other_counts=None):
        assert differs in ("list", "placement") and (other_steps is not None or other_reads is not None) and (differs == "list" or counts is not None)
        self.name, self.k, self.A, self.reads, self.steps, self.expect, self.counts, self.other_counts = name, K, A, list(reads), list(steps), list(expect), counts, other_counts
        self.differs, self.other_steps, self.other_reads, self.split, self.presimp = differs, other_steps, other_reads, split, 0.0


def pieces(seed, *sizes):
    h = G.fresh(seed, sum(sizes))
    out, at = [], 0
    for n in sizes:
        out.append(h[at:at + n])
        at += n
    return out


# ---- the nested family ---------------------------------------------------------------------------------------------------------------------------------------
def nested_family(seed, nu=5, flank=6, cflank=6):
    a1, a2, b1, b2, cin, cout, x, u, y = pieces(seed, flank, flank, flank, flank, cflank, cflank, 4, nu, 4)
    return dict(a1=a1, a2=a2, b1=b1, b2=b2, cin=cin, cout=cout, x=x, u=u, y=y, p1=a1 + x + u + y + b1, p2=a2 + x + u + y + b2, p3=cin + u + cout)


def spanning(f, times=2, strands=(False, True, True)):
    return [G.mread(f[p], rev=r) for p, r in zip(("p1", "p2", "p3"), strands) for _ in range(times)]


def _nested_cases():
    f = nested_family(801)
    reads = spanning(f)
    # after REPEATS: the four flanks, x u y = 4 + 3 + 4, Cin u Cout = 6 + 3 + 6; after NESTED: A x u y B = 6 + 11 + 6 twice.  Each of the four spanning reads of
    # x u y has its 3 windows of u between two anchors
    yield NCase("nested", reads, [(REPEATS, 1, 0), (NESTED, 1, 0)], [15, 23, 23], "list", other_steps=[(REPEATS, 1, 0)], counts=(18, 18, 0, 0))
    yield NCase("nested, one strand", spanning(f, strands=(False, False, False)), [(REPEATS, 2, 0), (NESTED, 2, 0)], [15, 23, 23], "list",
                other_steps=[(REPEATS, 2, 0), (NESTED, 3, 0)], counts=(18, 18, 0, 0))
    yield NCase("nested, the second step alone sees no copies", reads, [(NESTED, 1, 0), (NESTED, 1, 0)], [15, 23, 23], "list", other_steps=[(NESTED, 1, 0)], counts=(18, 18, 0, 0))
    # x u y copied once more needs its own round: S = p (x u y) q occurs twice, x u y a third time, u a fourth
    a1, a2, b1, b2, d1, d2, c1, c2, p, x, u, y, q = pieces(802, 6, 6, 6, 6, 6, 6, 6, 6, 4, 4, 5, 4, 4)
    paths = [a1 + p + x + u + y + q + b1, a2 + p + x + u + y + q + b2, d1 + x + u + y + d2, c1 + u + c2]
    reads = [G.mread(h, rev=i % 2 == 1) for i, h in enumerate(paths) for _ in range(2)]
    # first NESTED step: the 3 windows of u in each of the 8 reads; second: the 11 windows of x u y in 6 reads and the 3 of u in the other 2
    yield NCase("doubly nested", reads, [(REPEATS, 1, 0), (NESTED, 1, 0), (NESTED, 1, 0)], [15, 23, 31, 31], "list", other_steps=[(REPEATS, 1, 0), (NESTED, 1, 0)],
                counts=(24 + 72, 24 + 72, 0, 0))
    # where row(e) alone decides.  C1 u y D2 follows C1 u C2 into u and leaves it as D1 x u y D2 does, at a COPY inside a unitig: every window from u to y3 is
    # ambiguous in the second NESTED step, with the left anchor (c1[5], u0, u1) on entry 5 of C1 u' C2 (15 entries) and the right one (y2, y3, d2[0]) in
    # D1 x u y D2.  The 3 windows of u have a valid candidate from each side, in two unitigs: conflicts, in both steps (in the first the right anchor is
    # (u3, u4, y0), still unique).  The 4 windows behind them, (u3, u4, y0) to (y1, y2, y3), have left candidates on entries 9 to 12 of C1 u' C2: inside the
    # unitig, but those entries are (u3, u4, c2[0]) and on, OTHER rows: not valid, so the right candidate places all 4.  Without the row test only the strand
    # test stands in the way, and between a window and an entry of another row that is a coin's toss on the hashes: with these, 3 of the 4 would be conflicts
    # (tests/test_nested_cpu.py runs that wrong rule).  All steps at min_support 2: that read's crossings are weak
    chimera = [G.mread(c1 + u + y + d2)]
    yield NCase("a candidate on another row", reads + chimera, [(REPEATS, 2, 0), (NESTED, 2, 0), (NESTED, 2, 0)], [15, 23, 31, 31], "placement", other_reads=reads,
                counts=(96 + 3 + 7, 96 + 4, 3 + 3, 0), other_counts=(96, 96, 0, 0))
    # reads that start, end or lie wholly inside the copied stretch: placed by one anchor, or by none; they cross nothing, so only the counts can tell
    f = nested_family(803, nu=7)
    extra = [G.mread(f["u"][1:] + f["y"] + f["b1"]), G.mread(f["a2"] + f["x"] + f["u"][:-1], rev=True), G.mread(f["u"])]
    yield NCase("one anchor and none, inside one unitig", spanning(f) + extra, [(REPEATS, 1, 0), (NESTED, 1, 0)], [17, 25, 25], "placement", other_reads=spanning(f),
                counts=(30 + 4 + 4 + 5, 30 + 4 + 4, 0, 5))
    # A1 x u Cout: its u windows have a valid candidate from each side, in two different unitigs.  (The REPEATS step runs at 2: that read's key of u is weak.)
    f = nested_family(804)
    chimera = [G.mread(f["a1"] + f["x"] + f["u"] + f["cout"])]
    yield NCase("conflict", spanning(f) + chimera, [(REPEATS, 2, 0), (NESTED, 2, 0)], [15, 23, 23], "placement", other_reads=spanning(f), counts=(18 + 3, 18, 3, 0))
    # A = 2: the windows that hold a changed hash are seen once and are no rows.  The read ends inside the run: of its nine windows in u the first three are
    # placed by the left anchor, three are no rows, and the three behind them have no right anchor and must not take the left one from across the gap.  A
    # second read, with another changed hash and sequenced from the other strand, tests the other side.  The six spanning reads have ten windows each in u
    f = nested_family(805, nu=12)
    broken = [f["a1"] + f["x"] + f["u"][:5] + G.fresh(seed, 1) + f["u"][6:11] for seed in (8050, 8051)]
    yield NCase("an unplaced window inside the run", spanning(f) + [G.mread(broken[0]), G.mread(broken[1], rev=True)], [(REPEATS, 2, 0), (NESTED, 2, 0)], [22, 30, 30], "placement",
                other_reads=spanning(f), counts=(60 + 2 * (3 + 3), 60 + 2 * 3, 0, 2 * 3), A=2)
    # two reads back to back in the store: the first ends on windows of x, the second starts on windows of u and is placed by its right anchor alone
    f = nested_family(806)
    pair = [G.mread(f["a1"] + f["x"]), G.mread(f["u"] + f["y"] + f["b1"])]
    yield NCase("two reads back to back", spanning(f) + pair, [(REPEATS, 1, 0), (NESTED, 1, 0)], [15, 23, 23], "placement", other_reads=spanning(f) + pair[:1], counts=(18 + 3, 18 + 3, 0, 0))


# ---- the tail family ---------------------------------------------------------------------------------------------------------------------------------------------
def tail_family(seed, flank=6, attach=False):
    a, b1, b2, e, cin, cout, x, u, y, g1, g2 = pieces(seed, flank, flank, flank, flank, 3 if attach else 6, 3 if attach else 6, 4, 5, 4, 20, 20)
    return dict(a=a, b1=b1, b2=b2, e=e, x=x, u=u, y=y, pa=a + x + u + y[:2], pe=e + u[-2:] + y + b2, pc=(g1[-3:] if attach else []) + cin + u + cout, pg=g1 + g2,
                from_x=x[1:] + u + y + b1, from_u=u[1:] + y + b1)


def tail_reads(f, which, rev, attach=False):
    reads = [G.mread(f["pa"], rev=rev)] * 3 + [G.mread(f["pc"], rev=not rev)] * 3 + [G.mread(f["pe"], rev=rev)] * 2 + [G.mread(f[which], rev=rev)] * 2
    return reads + ([G.mread(f["pg"])] * 3 if attach else [])


def _tail_cases():
    steps = [(REPEATS, 3, 0), (NESTED, 2, 0)]
    f = tail_family(811)
    for rev, side, verb in ((False, "left", "starts"), (True, "right", "ends")):
        # W = A x u = 6 + 4 + 3, Y = 4, Cin u' = 6 + 3, and E, Cout, B1, B2 = 6 each.  Resolved: W Y B1 = 23, Y' B2 = 10.  The windows of u in the three reads of
        # A x u, the three of Cin u Cout and the two reads in question are ambiguous: 3 each, or 2 in a read that starts on u[1]
        yield NCase("the %s anchor alone" % side, tail_reads(f, "from_x", rev), steps, [6, 6, 9, 10, 23], "list", other_reads=tail_reads(f, "from_u", rev), counts=(24, 24, 0, 0))
        yield NCase("a read that %s inside the copied stretch has no anchor" % verb, tail_reads(f, "from_u", rev), steps, [4, 6, 6, 6, 6, 9, 13], "list",
                    other_reads=tail_reads(f, "from_x", rev), counts=(22, 18, 0, 4))
    # An EDGES step in front prunes E -> Cout; Cin u' Cout (2 + 3 + 3 + 3 entries) then hangs on another contig G by one end, and a TIPS step between the two
    # repeat steps clips it: the rows of u belong to one entry again, and the read that starts inside u IS placed.  Flanks of 16 and a limit of 14 entries keep
    # every other dead end.  Left: A x u Y B1 = 16 + 4 + 3 + 4 + 16, E Y' B2 = 16 + 4 + 16, G = 38
    f = tail_family(812, flank=16, attach=True)
    reads = tail_reads(f, "from_u", False, attach=True)
    yield NCase("a TIPS step removes a copy", reads, [(EDGES, 1, 0), (REPEATS, 3, 0), (TIPS, 14, 0), (NESTED, 2, 0)], [36, 38, 43], "list",
                other_steps=[(EDGES, 1, 0)] + steps)


# ---- long runs and a ring -------------------------------------------------------------------------------------------------------------------------------------------
def _long_cases():
    # u has 1,203 hashes: 1,201 ambiguous windows in a row, the anchors in other workgroups.  A filler read in front puts the run's first window on index 1,023
    # of the store, the last index of the first workgroup (the runs of the other two reads start wherever they fall)
    f = nested_family(821, nu=1203)
    filler = G.fresh(8210, PW_SPAN - 1 - (6 + 4 - 2))
    reads = [G.mread(filler)] + spanning(f, times=1)
    yield NCase("a run longer than a workgroup", reads, [(REPEATS, 1, 0), (NESTED, 1, 0)], [1013, 1213, 1221, 1221], "list", other_steps=[(REPEATS, 1, 0)], counts=(3603, 3603, 0, 0))
    # u has 4 hashes: a run of two windows, on indices 1,023 and 1,024: one index on either side of the boundary
    f = nested_family(822, nu=4)
    reads = [G.mread(filler)] + spanning(f, times=1)
    yield NCase("a run across a workgroup boundary", reads, [(REPEATS, 1, 0), (NESTED, 1, 0)], [14, 22, 22, 1013], "list", other_steps=[(REPEATS, 1, 0)], counts=(6, 6, 0, 0))


def _ring_cases():
    # a ring r1 u r2 u of 23 hashes: 23 windows, the 3 inside u seen at two places.  The REPEATS step makes it ONE circular unitig of 23 entries that holds
    # the rows of u twice.  A circular unitig's walk starts at its entry with the lowest index, and indices go by first sighting: the FIRST read of the store,
    # u[1:5], gives the middle window of u index 0, so the walk starts INSIDE the occurrence of u that kept the originals, call it O.  Whichever way the walk
    # runs, O then lies in entries 22, 0, 1 (or 1, 0, 22) and the other occurrence in the middle of the walk.
    #   the first read: 2 windows of u, no anchor: 2 unanchored.
    #   `turns`: three turns of the ring in one read, twice: 2 * 3 * 2 * 3 = 36 windows of u, each between two anchors.  In O one of the two candidates falls
    #   off the walk's end, the other is valid: all 36 resolved, with or without a wrap.
    #   `one_sided`: four reads that hold all of u and three hashes of ONE flank, one per side of each occurrence: 12 windows with one anchor each.  The two at
    #   the other occurrence place all 6.  Of the two at O, the one whose anchor lies on the side of entry 22 reaches 1 window before the walk ends and the one
    #   on the side of entry 1 reaches 2 (walked the other way round it is 2 and 1): 3 resolved, and 3 that only a WRAP round the walk's end would reach (there
    #   it would find the right row in the right strand): unanchored.  Which occurrence is O and which way the walk runs need not be known: 9 and 3.
    # In all 50 ambiguous, 45 resolved, 5 unanchored.  The second run puts four hashes of r1 in front as the first read: index 0 is then a window of r1, the walk
    # starts there, no stretch of u lies across its end and only the two windows of u[1:5] stay unanchored: 50, 48, 0, 2.  A placement that wraps gives that in both
    r1, r2, u = pieces(831, 6, 7, 5)
    ring = r1 + u + r2 + u
    turns = [G.mread((ring * 4)[:3 * len(ring) + 4])] * 2
    one_sided = [G.mread(r1[-3:] + u), G.mread(u + r2[:3], rev=True), G.mread(r2[-3:] + u, rev=True), G.mread(u + r1[:3])]
    reads = [G.mread(u[1:5])] + turns + one_sided
    yield NCase("a circular unitig that holds copies", reads, [(REPEATS, 1, 0), (NESTED, 1, 0)], [23], "placement", other_reads=[G.mread(r1[:4])] + reads,
                counts=(50, 45, 0, 5), other_counts=(50, 48, 0, 2))


def _all():
    for make in (_nested_cases, _tail_cases, _long_cases, _ring_cases):
        yield from make()


def many_nested(n, seed=841):
    """n nested families side by side, flanks of 4, x, u, y of 4, 5, 4 hashes, one read per path: after a REPEATS step n unitigs x u y of 11 entries wait for the
    NESTED step, which places 3 n ambiguous runs of 3 windows and leaves 3 n unitigs (for more resolved unitigs and more ambiguous runs than one workgroup holds)"""
    import random
    h = random.Random(seed).sample(range(1, G.HASH_LIMIT), 37 * n)
    reads = []
    for i in range(n):
        g = h[37 * i:37 * i + 37]
        a1, a2, b1, b2, cin, cout, x, u, y = g[:4], g[4:8], g[8:12], g[12:16], g[16:20], g[20:24], g[24:28], g[28:33], g[33:]
        reads += [G.mread(a1 + x + u + y + b1), G.mread(a2 + x + u + y + b2, rev=i % 2 == 1), G.mread(cin + u + cout, rev=i % 3 == 1)]
    return reads


CASES = list(_all())
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
