"""Hand-built bubbles with branching insides, in MINIMIZER SPACE (the way of tests/sketch_graphs.py, whose Case, mread and fresh they use): the smallest shapes at
which the SUPERBUBBLES step (include/mdbg_hip.h, MDBG_SIMPLIFY_SUPERBUBBLES) can go wrong, each with the node indices the step removes written out by hand.
tests/test_superbubbles_cpu.py checks them against the restatement, tests/test_gpu_superbubbles.py feeds them to the library.

Every case has k = 3 and min_abundance 2.  A read is a path of hashes; P and S are six hashes in front of and behind the place where the reads differ.  Node
indices count the windows in first-sighting order, so the first read fixes 0 .. 11 wherever it has 14 hashes: 0 .. 3 the source, 8 .. 11 the sink, 4 .. 7 the
windows that hold a changed place."""
import sketch_graphs as G

K, A = 3, 2
TIPS, BUBBLES, SUPERBUBBLES = 1, 2, 64
SB = (SUPERBUBBLES, 0, 0)


def case(name, reads, removed, **kw):
    """removed: {schedule (tuple of steps): [sorted node indices per step]}"""
    return G.Case(name, K, A, reads, schedules=[list(s) for s in removed], expect=dict(removed=dict(removed), **kw))


def braid_reads(h, n_g, n_h1, n_h2, rev=False):
    """a genome and two variants whose differences lie one minimizer apart: five interior unitigs between one source and one sink.
    G: 4 = aG, 5 6 = bG, 7 = cG; H1: 12 13 14 (it joins cG); H2: 15 16 17 (it leaves aG and ends in the sink)"""
    P, S, x, y, x1, y1 = h[:6], h[6:12], h[12], h[13], h[14], h[15]
    return [G.mread(P + [x, y] + S, rev=rev)] * n_g + [G.mread(P + [x1, y] + S, rev=rev)] * n_h1 + [G.mread(P + [x, y1] + S, rev=rev)] * n_h2


def _braids():
    h = G.fresh(6401, 16)
    # G 6, H1 3, H2 2: the means are aG 8, bG 6, cG 9, H1 3, H2 2; the path through G has the weakest unitig 6
    yield case("braid", braid_reads(h, 6, 3, 2), {(SB,): [[12, 13, 14, 15, 16, 17]], ((BUBBLES, 0, 0),): [[]], ((TIPS, 0, 0), (BUBBLES, 0, 0), (TIPS, 0, 0), (BUBBLES, 0, 0)): [[], [], [], []]})
    # G 2, H1 6, H2 3: aG 5, bG 2, cG 8, H1 6, H2 3; through H1 and cG the weakest is 6
    yield case("braid, a variant wins", braid_reads(h, 2, 6, 3), {(SB,): [[4, 5, 6, 15, 16, 17]]})
    # the limits count the inside: 1 + 2 + 1 + 3 + 3 = 10 entries, 210 + 310 + 210 + 410 + 410 = 1550 bases
    yield case("braid at the limits", braid_reads(h, 6, 3, 2),
               {((SUPERBUBBLES, 10, 1550),): [[12, 13, 14, 15, 16, 17]], ((SUPERBUBBLES, 9, 0),): [[]], ((SUPERBUBBLES, 0, 1549),): [[]], ((SUPERBUBBLES, 10, 0),): [[12, 13, 14, 15, 16, 17]],
                ((SUPERBUBBLES, 0, 1550),): [[12, 13, 14, 15, 16, 17]]})
    # every abundance equal: aG 3 + 3 = 6, bG 3, cG 6, H1 3, H2 3.  All three paths have the weakest unitig 3; best(t) = cG (mean 6 beats H2's 3), best(cG): bG and
    # H1 tie at 3 and H1 is the longer unitig (410 bases against 310)
    yield case("braid, all equal", braid_reads(h, 3, 3, 3), {(SB,): [[4, 5, 6, 15, 16, 17]]})
    # sequenced from the other strand only: the same windows in the same sighting order
    yield case("braid, minus side", braid_reads(h, 6, 3, 2, rev=True), {(SB,): [[12, 13, 14, 15, 16, 17]]})
    # half the reads from each strand.  MIRROR RECORDS: in every case here each edge record u -> v stands beside its mirror comp(v) -> comp(u) (38 records, 19 arcs
    # and their mirrors, in this one); the step reads the arcs of both and must count each pair of readings as one bubble
    mixed = braid_reads(h, 3, 2, 1) + braid_reads(h, 3, 1, 1, rev=True)
    yield case("braid, both strands", mixed, {(SB,): [[12, 13, 14, 15, 16, 17]]})
    # DUPLICATE RECORDS.  A record occurs twice only where a (k-1)-mer is its own reverse, here a minimizer v twice in a row: the window (v, v, p) then follows its own
    # complement, a record that is its own mirror and is listed twice.  In front of the source (one more hash: 0 .. 4 source, 5 = aG, 6 7 = bG, 8 = cG, 9 .. 12 sink,
    # H1 13 14 15, H2 16 17 18) the doubled record is an in-arc of s, which no condition looks at: the braid pops
    P, rest = h[:6], h[6:]
    doubled = lambda front, n_g, n_h1, n_h2: braid_reads(front + rest, n_g, n_h1, n_h2)
    yield case("braid, duplicate record in front of the source", [G.mread((P[0],) + rd[0]) for rd in braid_reads(h, 6, 3, 2)], {(SB,): [[13, 14, 15, 16, 17, 18]]})
    # the same v v as the last two hashes in front of the changed place: now aG, H1 (and the source, for the mirror reading) each follow their own complement by a
    # doubled record, so s reaches the complement of a member (d): nothing is a bubble, and the run the lanes read holds the duplicate
    yield case("braid, duplicate records at the source's end", doubled(P[:4] + [P[4], P[4]], 6, 3, 2), {(SB,): [[]]})


def _ladder_and_chains():
    h = G.fresh(6402, 24)
    P, S, a, b, c, d, M = h[:6], h[6:12], h[12], h[13], h[14], h[15], h[16:18]
    rd = lambda first, second: G.mread(P + [first] + M + [second] + S)
    # s -> a, b; a -> c, d; b -> c, d; c, d -> t: the shared (k-1)-mer M joins both left branches to both right ones.  Read a-c (5) fixes 0 .. 3 source, 4 5 6 = a,
    # 7 8 9 = c, 10 .. 13 sink; b-d (4): 14 15 16 = b, 17 18 19 = d; a-d and b-c (2 each) add no window.  a 7, b 6, c 7, d 6: a and c stay
    yield case("ladder", [rd(a, c)] * 5 + [rd(b, d)] * 4 + [rd(a, d)] * 2 + [rd(b, c)] * 2, {(SB,): [[14, 15, 16, 17, 18, 19]], ((BUBBLES, 0, 0),): [[]]})
    # two simple bubbles back to back, four hashes between them: the unitig in the middle is the sink of the first and the source of the second
    M4 = h[16:20]
    rd4 = lambda first, second, n: [G.mread(P + [first] + M4 + [second] + S)] * n
    yield case("back to back", rd4(a, c, 5) + rd4(b, d, 3), {(SB,): [[16, 17, 18, 19, 20, 21]], ((BUBBLES, 0, 0),): [[16, 17, 18, 19, 20, 21]]})


def _nested():
    h = G.fresh(6403, 24)
    P, S, o, z, v = h[:6], h[6:12], h[12:19], h[19:22], h[22]
    inner = o[:3] + [v] + o[4:]
    # an outer bubble (o against z) whose o branch holds a bubble of its own (o[3] against v).  0 .. 3 source, 4 .. 6 the way in, 7 8 9 = o[3], 10 .. 12 the way out,
    # 13 .. 16 sink; 17 18 19 = v; 20 .. 24 = z.  Means: o side 7, o[3] 4, v 3, z 6: the outer bubble keeps z (weakest 6 against 4)
    reads = [G.mread(P + o + S)] * 4 + [G.mread(P + inner + S)] * 3 + [G.mread(P + z + S)] * 6
    outer, inner_only = list(range(4, 13)) + [17, 18, 19], [17, 18, 19]
    # inside the outer bubble: 3 + 3 + 3 + 3 + 5 = 17 entries; inside the inner one 6.  Once the inner one has popped, the o side is ONE unitig of nine entries with
    # mean (21 + 12 + 21) / 9 = 6, as z's: the longer one stays, z goes
    yield case("nested", reads, {(SB,): [outer], ((SUPERBUBBLES, 17, 0),): [outer], ((SUPERBUBBLES, 16, 0),): [inner_only], ((SUPERBUBBLES, 6, 0),): [inner_only], ((SUPERBUBBLES, 5, 0),): [[]],
                                 ((SUPERBUBBLES, 16, 0), SB): [inner_only, [20, 21, 22, 23, 24]]})


def _left_alone():
    h = G.fresh(6404, 40)
    base = braid_reads(h, 6, 3, 2)
    P, S, x, y, x1, y1 = h[:6], h[6:12], h[12], h[13], h[14], h[15]
    q = h[16:22]
    nothing = {(SB,): [[]]}
    # a read that leaves the inside and ends: an interior dead end (the TIPS step's business; behind it the braid pops)
    yield case("interior dead end", base + [G.mread(P[3:] + [x1] + q[:3])] * 2, {(SB,): [[]], ((TIPS, 0, 0), SB): [[18, 19, 20], [12, 13, 14, 15, 16, 17]]})
    # a read that comes from elsewhere into the inside
    yield case("in-arc from outside", base + [G.mread(q[:3] + [x1, y] + S[:3])] * 2, nothing)
    # and one that leaves the inside for elsewhere and goes on (no dead end: it ends in a unitig of its own that is long)
    yield case("out-arc to outside", base + [G.mread(P[3:] + [x1] + q)] * 2, {(SB,): [[]]})
    # one branch is the other read backwards: its windows are the same k-min-mers on the other strand
    r = h[22:25]
    yield case("inversion", [G.mread(P + r + S)] * 3 + [G.mread(P + r[::-1] + S)] * 3, nothing)
    # a branch that runs three times through the same three hashes: a cycle inside
    yield case("interior cycle", [G.mread(P + [x] + S)] * 4 + [G.mread(P + r + r + r + S)] * 3, nothing)
    # a ring with one changed place: the rest of the ring is the source and the sink at once
    ring = h[25:35]
    other = ring[:4] + [h[35]] + ring[5:]
    yield case("sink is the source", [G.mread(ring + ring[:6])] * 3 + [G.mread(other + other[:6])] * 3, nothing)


def fan_reads(n):
    h = G.fresh(6405, 12 + n)
    return [rd for i in range(n) for rd in [G.mread(h[:6] + [h[12 + i]] + h[6:12])] * (3 if i == 0 else 2)]


def _fans():
    # n branches of three nodes each: the first read has 13 hashes: 0 .. 3 source, 4 5 6 branch 0 (seen three times), 7 .. 10 sink; branch i >= 1 is 8 + 3 i .. 10 + 3 i.  64 fit one bubble, 65 do not
    yield case("fan of 64", fan_reads(64), {(SB,): [list(range(11, 11 + 3 * 63))], ((BUBBLES, 0, 0),): [list(range(11, 11 + 3 * 63))]})
    yield case("fan of 65", fan_reads(65), {(SB,): [[]], ((BUBBLES, 0, 0),): [list(range(11, 11 + 3 * 64))]})


def _all():
    for make in (_braids, _ladder_and_chains, _nested, _left_alone, _fans):
        yield from make()
    by = {c.name: c for c in G.CASES}
    hub = by["hub"]                                # a source with dozens of ways out, again and again: nothing removed, no defect
    yield G.Case("hub", hub.k, hub.A, hub.reads, schedules=[[SB]], expect=dict(removed={(SB,): [[]]}))
    h = G.fresh(6406, 2 + 70 * 6)                 # the same with 70 reads round the shared (k-1)-mer: every source has 70 ways out, more than one bubble may hold
    wide = [G.mread(h[2 + 6 * i:5 + 6 * i] + h[:2] + h[5 + 6 * i:8 + 6 * i], rev=i % 4 == 1) for i in range(70)]
    yield G.Case("hub of 70", 3, 1, wide, schedules=[[SB]], expect=dict(removed={(SB,): [[]]}))
    simple = by["bubble 7/3"]                     # a closed simple bubble: both kinds remove the same unitig
    yield G.Case("simple bubble", simple.k, simple.A, simple.reads, schedules=[[SB], [(BUBBLES, 0, 0)]], expect=dict(removed={(SB,): [[12, 13, 14, 15]], ((BUBBLES, 0, 0),): [[12, 13, 14, 15]]}))
    for name in G.CASE_IDS:                        # palindromes, self-neighbours, several records between two nodes (duplicates and mirrors): against the restatement only
        if name.startswith("odd "):
            c = by[name]
            yield G.Case(name, c.k, c.A, c.reads, schedules=[[SB], [(TIPS, 0, 0), SB]], expect={})


CASES = list(_all())
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


# ---- random graphs ----------------------------------------------------------------------------------------------------------------------------------------------
def random_braids(seed):
    """a genome of 36 distinct hashes and two or three variants of it whose changed places mostly lie within a few minimizers of one site: braids, ladders and
    nested bubbles, with simple bubbles, tips (a variant read that stops early) and untouched graphs among them.  -> reads (k = 3, A = 2)"""
    import random
    rnd = random.Random(7300 + seed)
    n = 36
    pool = G.fresh(7300 + seed, n + 12)
    genome, spare = pool[:n], pool[n:]
    site = rnd.randrange(8, n - 12)
    haps = [genome]
    for _ in range(rnd.randint(2, 3)):
        hap = list(rnd.choice(haps))
        at = site + rnd.randint(0, 4) if rnd.random() < 0.8 else rnd.randrange(6, n - 8)
        hap[at] = spare.pop()
        if rnd.random() < 0.3:
            hap[at + rnd.randint(1, 2)] = spare.pop()
        haps.append(hap if rnd.random() < 0.85 else hap[:at + 3])
    return [G.mread(hap, rev=rnd.random() < 0.3) for hap in haps for _ in range(rnd.randint(2, 4))]
