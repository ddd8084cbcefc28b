#!/usr/bin/env python3
"""The two .sequences lines the reference tree holds, as a fixture: tests/golden/reference_held_vectors.json.

rust-mdbg cannot be built where this project is built (Rust, no cargo), but its tree QUOTES two lines of real `.sequences` files as comments, each an example of
what the code next to it parses:

  A   experiments/661k_genomes/scan_genomes_minmers.py   a node of a k = 10 graph (the script asserts len(kminmer) == 10); the sequence is broken by blanks
  B   src/to_basespace.rs                                a node of a k = 7 graph, beside the code that reads the line back

A line is  <node>  [m1, ..., mk]  <sequence>  *  *  (s0, s1)   (src/main.rs:702): the k minimizer hashes of a k-min-mer in normalized order, the bases from the
first minimizer's first base to the last minimizer's last base, and the two outer minimizer distances.  Everything on it was computed by the reference: ntHash
values, the canonical minimum, the density filter, the positions (through the shift pair and the length), the orientation, the line format.

This script finds each line by its SHAPE (it holds neither line), and writes DATA only: the node name, the hashes, the sequence with the blanks removed, the
shift pair.  What the reference does not print is added per vector and marked as such in the file:
  l             the l-mer length at which the line reproduces (A: 12, B: 10; the reference's example settings);
  exact         densities at which the sketch of the sequence alone is exactly the listed hashes;
  outside       densities just outside that range, each with the smaller or larger sketch expected there;
  pos           the positions of the listed minimizers in the sequence.
`pos` and `outside` are DERIVED here with tests/golden/independent_restatement.py (the plain definition of ntHash, homopolymer compression off: neither printed
sequence is homopolymer-compressed), and the script refuses to write a file unless that derivation gives exactly the listed hashes at every `exact` density, the
printed shift pair, and pos[-1] + l == len(seq).  A smaller `outside` set is, besides, what the listed hashes give on their own: those <= floor(d * 2^64).

Run by hand where the reference tree is:  python tests/golden/make_reference_held_vectors.py [reference root]
tests/test_reference_held_cpu.py re-derives the fixture the same way when the tree is present and compares it with the committed file, byte for byte.
"""
import importlib.util
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
OUT = os.path.join(HERE, "reference_held_vectors.json")

# comment mark, node name, [integers], runs of ACGT possibly broken by blanks, *, *, (s0, s1)
LINE = re.compile(r"^\s*(?://|#)\s*(\d+)\s+\[(\d+(?:,\s*\d+)*)\]\s+([ACGT]+(?:\s+[ACGT]+)*)\s+\*\s+\*\s+\((\d+),\s*(\d+)\)\s*$")

VECTORS = [
    dict(name="A", file="experiments/661k_genomes/scan_genomes_minmers.py", l=12, exact=[0.00995, 0.01], outside=[0.0095, 0.0104]),
    dict(name="B", file="src/to_basespace.rs", l=10, exact=[0.0079, 0.008, 0.01, 0.012, 0.0125], outside=[0.0075]),
]


def held_line(path):
    """-> (line number, match) of the one line of the file that has the shape of a .sequences line inside a comment"""
    hits = [(no, m) for no, m in ((no, LINE.match(text)) for no, text in enumerate(open(path, encoding="utf-8", errors="replace"), 1)) if m]
    if len(hits) != 1:
        raise SystemExit("%s: %d lines of the expected shape, want exactly one" % (path, len(hits)))
    return hits[0]


def derive(root=REFERENCE):
    spec = importlib.util.spec_from_file_location("independent_restatement", os.path.join(HERE, "independent_restatement.py"))
    restatement = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(restatement)
    sketch_read = restatement.sketch_read
    out = []
    for v in VECTORS:
        no, m = held_line(os.path.join(root, v["file"]))
        key = [int(x) for x in m.group(2).split(",")]
        seq = "".join(m.group(3).split())
        shift = [int(m.group(4)), int(m.group(5))]
        l = v["l"]
        pos = None
        for d in v["exact"]:
            h, p = sketch_read(seq.encode(), l, d, already_hpc=True)
            if [int(x) for x in h] != key:
                raise SystemExit("%s: density %r does not reproduce the listed hashes" % (v["name"], d))
            pos = [int(x) for x in p]
        if [pos[1] - pos[0], pos[-1] - pos[-2]] != shift or pos[0] != 0 or pos[-1] + l != len(seq):
            raise SystemExit("%s: positions %r do not give the printed shift %r and length %d" % (v["name"], pos, shift, len(seq)))
        outside = []
        for d in v["outside"]:
            h, p = sketch_read(seq.encode(), l, d, already_hpc=True)
            h, p = [int(x) for x in h], [int(x) for x in p]
            if h == key:
                raise SystemExit("%s: density %r is not outside" % (v["name"], d))
            outside.append(dict(density=d, hashes=h, pos=p))
        out.append(dict(name=v["name"], source=dict(file=v["file"], line=no), index=int(m.group(1)), key=key, seq=seq, shift=shift,
                        not_printed_by_the_reference=dict(l=l, exact=v["exact"], pos=pos, outside=outside)))
    return dict(provenance="two .sequences lines quoted as comments in the rust-mdbg tree, taken by tests/golden/make_reference_held_vectors.py; index, key, seq "
                           "and shift are the reference's own output, the rest is derived (see the script)", vectors=out)


def text(fixture):
    return json.dumps(fixture, indent=1) + "\n"


if __name__ == "__main__":
    fx = derive(sys.argv[1] if len(sys.argv) > 1 else REFERENCE)
    open(OUT, "w").write(text(fx))
    for v in fx["vectors"]:
        print("%s: node %d, k = %d, %d bases, shift %r, l = %d, positions %r" % (v["name"], v["index"], len(v["key"]), len(v["seq"]), v["shift"],
                                                                                  v["not_printed_by_the_reference"]["l"], v["not_printed_by_the_reference"]["pos"]))
