"""Hand-built minimizer-space cases for the chain stage (include/mdbg_chain.h), in the style of tests/sketch_graphs.py: k = 3, A = 2, so that a k-min-mer seen once —
every window that holds a spoilt minimizer — is no node and the window is unplaced.  Every case names the reads it is about (`probe`) and says, per
(max_skew, max_gap), what their alignments' bridges must be, written out by hand from the definition: (kind, entries) per alignment, kind "-" not bridged, "I"
INSIDE, "R" over a record.  tests/test_chains_cpu.py holds the restatement against these, tests/test_gpu_chains.py the GPU against the restatement."""
import random

import sketch_graphs as G

K, A = 3, 2
NO = ("-", 0)


class Case:
    def __init__(self, name, reads, probe, expect, presimp=0.0, split=None):
        self.name, self.k, self.A, self.reads, self.probe, self.expect, self.presimp, self.split = name, K, A, list(reads), probe, expect, presimp, split


def spoil(h, at, seed=1):
    """the hashes with those at the given positions replaced by fresh ones"""
    new = G.fresh(9000 + seed, len(at))
    return [new[at.index(i)] if i in at else v for i, v in enumerate(h)]


def drop(h, i):
    return h[:i] + h[i + 1:]


def insert(h, i, seed=2):
    return h[:i] + G.fresh(9100 + seed, 1) + h[i:]


def _linear_cases():
    """one linear unitig of 18 entries (20 minimizers, the read twice); the third read carries the error.  Substituted at 8: windows 6, 7, 8 unplaced, dw = 4 between
    entries 5 and 9: de = 4.  Removed at 8: windows 6, 7 unplaced, window 8 is entry 9: dw = 3, de = 4.  Inserted in front of 9: windows 7, 8, 9 unplaced, window 10 is
    entry 9 behind entry 6: dw = 4, de = 3"""
    h = G.fresh(701, 20)
    clean = G.mread(h)
    for rev in (False, True):
        tag = ", other strand" if rev else ""
        yield Case("substituted" + tag, [clean] * 2 + [G.mread(spoil(h, [8]), rev=rev)], [2], {(0, 0): [[NO, ("I", 4)]], (1, 0): [[NO, ("I", 4)]]})
        yield Case("removed" + tag, [clean] * 2 + [G.mread(drop(h, 8), rev=rev)], [2], {(0, 0): [[NO, NO]], (1, 0): [[NO, ("I", 4)]], (2, 0): [[NO, ("I", 4)]]})
        yield Case("inserted" + tag, [clean] * 2 + [G.mread(insert(h, 9), rev=rev)], [2], {(0, 0): [[NO, NO]], (1, 0): [[NO, ("I", 3)]]})
    # two errors closer than k are ONE gap (windows 6 .. 9, dw = 5 between entries 5 and 10); two far apart give a chain of three
    yield Case("two errors in one gap", [clean] * 2 + [G.mread(spoil(h, [8, 9]))], [2], {(0, 0): [[NO, ("I", 5)]]})
    yield Case("two errors far apart", [clean] * 2 + [G.mread(spoil(h, [5, 14]))], [2], {(0, 0): [[NO, ("I", 4), ("I", 4)]], (0, 2): [[NO, NO, NO]], (0, 3): [[NO, ("I", 4), ("I", 4)]]})
    # max_gap cuts exactly at dw - 1 = 3
    yield Case("max_gap", [clean] * 2 + [G.mread(spoil(h, [8]))], [2], {(0, 3): [[NO, ("I", 4)]], (0, 2): [[NO, NO]], (5, 1): [[NO, NO]], (0, 4): [[NO, ("I", 4)]]})
    # a read that goes BACK on the unitig (entries 10 .. 13, then 2 .. 5), and one that comes back on the other strand: neither candidate exists
    junk = G.fresh(702, 1)
    yield Case("backwards", [clean] * 2 + [G.mread(h[10:16] + junk + h[2:8])], [2], {(9, 0): [[NO, NO]]})
    yield Case("other strand of the same unitig", [clean] * 2 + [G.mread(h[2:8] + junk + h[10:16][::-1])], [2], {(9, 0): [[NO, NO]]})


def _fork_cases():
    """hub + x ten times, hub + y twice: u0 = the hub's 3 nodes, u1 = the x branch, u2 = the y branch (3 nodes each).  The probe is hub + y with hub[3] spoilt: windows
    1, 2, 3 unplaced, x = entry 0 of u0 (tail 2), y = entry 1 of u2 (head 1): de = 4 = dw over the record u0 -> u2.  At presimp 0.5 that record is gone (the x
    branch is five times as abundant) and nothing bridges"""
    h = G.fresh(703, 11)
    hub, x, y = h[:5], h[5:8], h[8:11]
    reads = [G.mread(hub + x)] * 10 + [G.mread(hub + y)] * 2 + [G.mread(spoil(hub, [3]) + y)]
    yield Case("gap over a fork", reads, [12], {(0, 0): [[NO, ("R", 4)]]})
    yield Case("gap over a fork, record removed", reads, [12], {(0, 0): [[NO, NO]], (9, 0): [[NO, NO]]}, presimp=0.5)


def _bubble_case():
    """a + b1 + c and a + b2 + c three times each: four unitigs of 4 nodes.  The probe is the first with BOTH minimizers of b1 spoilt: windows 4 .. 7, all of the
    branch, are unplaced; the gap would need the records a -> b1 and b1 -> c: not bridged at any skew"""
    h = G.fresh(704, 16)
    a, c, b1, b2 = h[:6], h[6:12], h[12:14], h[14:16]
    yield Case("gap swallows a short unitig", [G.mread(a + b1 + c)] * 3 + [G.mread(a + b2 + c)] * 3 + [G.mread(a + spoil(b1, [0, 1]) + c)], [6], {(0, 0): [[NO, NO]], (9, 0): [[NO, NO]]})


def _ring_cases():
    """a ring of 6 (its hashes ascending: the first window is canonical as read and the ring starts there on strand 0), walked twice: 12 minimizers, 10 windows on
    entries 0 .. 5, 0 .. 3.  Spoilt at 3: windows 1, 2, 3 unplaced, entries 0 -> 4 in one turn: INSIDE, de = 4 (the closing record would give 10).  Spoilt at 6:
    windows 4, 5, 6 unplaced, entries 3 -> 1 of the next turn: no INSIDE (no modulo), the closing record gives tail 2 + head 1 + 1 = 4"""
    r6 = sorted(G.fresh(705, 6))
    turn = [G.mread(r6 + r6[:3])] * 2
    yield Case("ring, inside a turn", turn + [G.mread(spoil(r6 * 2, [3]))], [2], {(0, 0): [[NO, ("I", 4)]]})
    yield Case("ring, over the closing record", turn + [G.mread(spoil(r6 * 2, [6]))], [2], {(0, 0): [[NO, ("R", 4)]]})
    yield Case("ring, other strand", turn + [G.mread(spoil(r6 * 2, [6]), rev=True)], [2], {(0, 0): [[NO, ("R", 4)]]})
    # a ring of 4 walked three times, spoilt at 3 and 4: windows 1 .. 4 unplaced, entry 0 -> entry 1 of the NEXT turn, dw = 5.  Both candidates exist: INSIDE de = 1
    # (skew 4), RECORD de = 3 + 1 + 1 = 5 (skew 0): the nearer one wins, whatever max_skew is
    r4 = sorted(G.fresh(706, 4))
    turn = [G.mread(r4 + r4[:3])] * 2
    yield Case("ring, both candidates, the nearer wins", turn + [G.mread(spoil(r4 * 3, [3, 4]))], [2], {(0, 0): [[NO, ("R", 5)]], (9, 0): [[NO, ("R", 5)]]})
    # entry 0, two windows that are no nodes, entry 1: dw = 3, INSIDE de = 1 and RECORD de = 5 are both 2 away: the tie goes to INSIDE
    yield Case("ring, a tie goes to INSIDE", turn + [G.mread(r4[:3] + r4[1:4])], [2], {(1, 0): [[NO, NO]], (2, 0): [[NO, ("I", 1)]]})


def _missing_case():
    """presimp 200/1 at 0.01 of the catalogue with A = 1: the read that takes the small branch crosses a key on no record, dw == 1: never bridged"""
    h = G.fresh(303, 11)
    hub, x, y = h[:5], h[5:8], h[8:11]
    c = Case("dw == 1 on no record", [G.mread(hub + x)] * 200 + [G.mread(hub + y)], [200], {(0, 0): [[NO, NO]], (9, 0): [[NO, NO]]}, presimp=0.01)
    c.A = 1
    yield c


def _short_case():
    """empty reads, reads of exactly k and k + 1 minimizers, between reads that chain; the last read's chain ends at the range's last index"""
    h = G.fresh(707, 20)
    clean, bad = G.mread(h), G.mread(spoil(h, [8]))
    reads = [G.mread([]), clean, G.mread(h[:3]), bad, G.mread([]), G.mread(h[:4]), clean, G.mread([]), G.mread(spoil(h, [5, 14]), rev=True)]
    yield Case("short and empty reads", reads, [3, 8], {(0, 0): [[NO, ("I", 4)], [NO, ("I", 4), ("I", 4)]]}, split=4)


CASES = [c for make in (_linear_cases, _fork_cases, _bubble_case, _ring_cases, _missing_case, _short_case) for c in make()]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


def mutated(reads, rate, seed):
    """the reads with every minimizer substituted, removed or preceded by a fresh one with probability `rate` each (seeded) -> reads with positions 100 apart"""
    rnd = random.Random(seed)
    out = []
    for hs, _ in reads:
        new = []
        for v in hs:
            r = rnd.random()
            if r < rate:
                new.append(rnd.randrange(1, G.HASH_LIMIT))
            elif r < 2 * rate:
                continue
            elif r < 3 * rate:
                new += [rnd.randrange(1, G.HASH_LIMIT), v]
            else:
                new.append(v)
        out.append(G.mread(new))
    return out
