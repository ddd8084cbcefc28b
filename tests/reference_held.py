"""The two reference-produced .sequences lines of tests/golden/reference_held_vectors.json, and the inputs the CPU and GPU tests build around them.
Everything a test EXPECTS comes from the fixture (the reference's own hashes, sequence and shift pair; the derived positions, which the fixture's generator
checked against the printed shift pair and length); nothing here calls the code under test.  Test infrastructure only."""
import json
import os

import numpy as np

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "reference_held_vectors.json")
TILE_STRIDE = 32512          # rust_mdbg_amd/csrc/mdbg_dev.h (tests/test_reference_held_cpu.py reads the header and checks this number)
FLANK = 300                  # seeded random bases behind a vector, so that its read holds more than k minimizers (the strict `> k` rule, src/main.rs:756)
REVCOMP = bytes(dict(zip(b"acgtuACGTU", b"tgcaaTGCAA")).get(c, ord("N")) for c in range(256))      # switch_base, src/utils.rs:10-24


class Vector:
    def __init__(self, v):
        extra = v["not_printed_by_the_reference"]
        self.name, self.index, self.key, self.shift = v["name"], v["index"], [int(x) for x in v["key"]], tuple(v["shift"])
        self.seq = v["seq"].encode()
        self.k, self.n = len(self.key), len(self.seq)
        self.l, self.exact, self.pos = extra["l"], extra["exact"], extra["pos"]
        self.outside = [(o["density"], o["hashes"], o["pos"]) for o in extra["outside"]]
        # the reference's line from the second field on (src/main.rs:702)
        self.line_tail = "[%s]\t%s\t*\t*\t(%d, %d)" % (", ".join(str(x) for x in self.key), self.seq.decode(), self.shift[0], self.shift[1])

    def __repr__(self):
        return self.name

    def densities(self):
        """-> [(density, expected hashes, expected positions)] for the vector alone: the exact ones, then the ones outside"""
        return [(d, self.key, self.pos) for d in self.exact] + self.outside

    def strand(self, rev):
        """-> (bases of the vector on that strand, hashes in the order that strand shows them, positions of their l-mers on that strand)"""
        if not rev:
            return self.seq, self.key, self.pos
        return revcomp(self.seq), self.key[::-1], [self.n - self.l - p for p in self.pos[::-1]]


def vectors():
    return [Vector(v) for v in json.load(open(FIXTURE))["vectors"]]


VECTORS = vectors()


def revcomp(s):
    return s[::-1].translate(REVCOMP)


def rnd_bases(seed, n):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()


def flank(v, n=FLANK):
    return rnd_bases(1000 + v.index, n)


def line_tail(key, seq, shift_full):
    """fields 2 - 6 of a .sequences line from a node row's minimizers, sequence and un-truncated shift pair, formatted as src/main.rs:702 does"""
    return "[%s]\t%s\t*\t*\t(%d, %d)" % (", ".join(str(int(x)) for x in key), seq.decode(), int(shift_full[0]), int(shift_full[1]))


def row_of_key(nodes, key):
    """index of the one row of a node table whose minimizer list is `key`"""
    hit = [i for i in range(nodes["n_nodes"]) if [int(x) for x in nodes["keys"][i]] == list(key)]
    assert len(hit) == 1, "the listed k-min-mer is in %d rows" % len(hit)
    return hit[0]


def row_sequence(reads, nodes, i):
    """what the row's .sequences line prints: reads[src_read][src_start:src_end], through utils::revcomp where `reversed`"""
    s = reads[int(nodes["src_read"][i])][int(nodes["src_start"][i]):int(nodes["src_end"][i])]
    return revcomp(s) if nodes["reversed"][i] else s


def inside(sk, read, lo, hi, l):
    """the minimizers of read `read` of a sketch whose l-mers lie wholly in [lo, hi) -> (hashes, positions relative to lo)"""
    a, b = int(sk["off"][read]), int(sk["off"][read + 1])
    h, p = sk["hashes"][a:b], sk["pos"][a:b].astype(np.int64)
    m = (p >= lo) & (p + l <= hi)
    return [int(x) for x in h[m]], [int(x) - lo for x in p[m]]


def placements(v):
    """start offsets of the vector in one random read: around the 32-base words, and across the halo and the ownership of l-mer ends of the first tiles"""
    return [0, 1, 31, 32, 33, 127, 128, TILE_STRIDE - v.n, TILE_STRIDE - 200, TILE_STRIDE - (v.l - 1), TILE_STRIDE, TILE_STRIDE + 1, 2 * TILE_STRIDE - 100]


def placed_read(v, start, rev, tail=257):
    """one read: `start` seeded random bases, the vector on the given strand, `tail` random bases"""
    return rnd_bases(7 * start + v.index + rev, start) + v.strand(rev)[0] + rnd_bases(3 * start + v.index + 2 + rev, tail)


def neighbour_cases(v, rev):
    """-> [(reads, read that holds the vector, its start there)]: the vector as the last bases of a read that another follows directly, as the first bases of a
    read that follows another, and both at once"""
    s = v.strand(rev)[0]
    a, b = rnd_bases(v.index + 11, 700), rnd_bases(v.index + 12, 500)
    return [([a + s, b], 0, 700), ([b, s + a], 1, 0), ([a + s, s + b], 0, 700), ([a + s, s + b], 1, 0)]
