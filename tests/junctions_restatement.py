"""A plain, slow statement of the junction-support definition of include/mdbg_hip.h (mdbg_graph_junctions), working on dictionaries and tuples: one read at a
time, one pair of neighbouring windows at a time.  It is the CHECKER of the junction tests and shares nothing with the code under test — no packed keys, no
sort, no search, no codes.  Written from the rule.

Inputs: those of read_paths_restatement.read_paths (the reads as lists of minimizer hashes in slot order, k, the node table's `keys` and `index` columns, the
unitig list as walks [[(index, '+' / '-')]]) and the list's edge records as (n1, o1, n2, o2[, overlap]) tuples with '+' / '-' characters.
A vertex is (unitig, entry, strand)."""
from read_paths_restatement import canonical


def mirror(pair):
    (xu, xj, xs), (yu, yj, ys) = pair
    return ((yu, yj, 1 - ys), (xu, xj, 1 - xs))


def key_of(pair):
    """the smaller of the pair and its mirror; tuples compare as the definition orders vertices, by (u, j, s), and pairs, by (x, y)"""
    return min(pair, mirror(pair))


def record_key(rec, walks):
    n1, o1, n2, o2 = rec[:4]
    x = (n1, len(walks[n1]) - 1 if o1 == "+" else 0, int(o1 == "-"))
    y = (n2, 0 if o2 == "+" else len(walks[n2]) - 1, int(o2 == "-"))
    return key_of((x, y))


def placements(reads, k, keys, index, walks):
    """per read, per window: the vertex (u, j, s) it is placed on, or None"""
    where = {}
    for u, walk in enumerate(walks):
        for j, (idx, o) in enumerate(walk):
            assert int(idx) not in where, "an index occurs in two entries: the unitigs do not partition the nodes"
            where[int(idx)] = (u, j, o)
    row = {tuple(int(v) for v in key): int(i) for key, i in zip(keys, index)}
    out = []
    for H in reads:
        H = [int(h) for h in H]
        W = len(H) - k + 1 if len(H) > k else 0
        placed = []
        for w in range(W):
            key, rev = canonical(tuple(H[w:w + k]))
            at = where.get(row.get(key, -1))
            placed.append(None if at is None else (at[0], at[1], int(rev != (at[2] == "-"))))
        out.append(placed)
    return out


def is_link(x, y):
    """same unitig, same strand, the entry one further in the read's direction — never wrapped"""
    return x[0] == y[0] and x[2] == y[2] and y[1] == (x[1] + 1 if x[2] == 0 else x[1] - 1)


def junctions(reads, k, keys, index, walks, edges):
    """-> dict(n_adjacent, n_links, n_crossings, n_explained, n_missing_crossings, n_records, n_missing, support: per record, missing: {key: count},
    missing_rows: [(u1, j1, s1, u2, j2, s2, count)] in key order, keys: per record)"""
    rkeys = [record_key(e, walks) for e in edges]
    known = set(rkeys)
    seen, missing = {}, {}
    n_adjacent = n_links = 0
    for placed in placements(reads, k, keys, index, walks):
        for x, y in zip(placed, placed[1:]):
            if x is None or y is None:
                continue
            n_adjacent += 1
            if is_link(x, y):
                n_links += 1
                continue
            key = key_of((x, y))
            book = seen if key in known else missing
            book[key] = book.get(key, 0) + 1
    rows = [x + y + (missing[(x, y)],) for x, y in sorted(missing)]
    return dict(n_adjacent=n_adjacent, n_links=n_links, n_crossings=n_adjacent - n_links, n_explained=sum(seen.values()), n_missing_crossings=sum(missing.values()),
                n_records=len(rkeys), n_missing=len(missing), support=[seen.get(key, 0) for key in rkeys], missing=missing, missing_rows=rows, keys=rkeys)


def name(i, circular):
    return "utg%07d%s" % (i + 1, "c" if circular else "l")


def tsv_text(edges, j, circular):
    """one L line per edge record (n1, o1, n2, o2, overlap) in list order — the record's L line of the .gfa with its support appended —, then one X line per
    missing key in key order"""
    lines = ["L\t%s\t%s\t%s\t%s\t%dM\t%d\n" % (name(a, circular[a]), oa, name(b, circular[b]), ob, ov, sup) for (a, oa, b, ob, ov), sup in zip(edges, j["support"])]
    for u1, j1, s1, u2, j2, s2, count in j["missing_rows"]:
        lines.append("X\t%s\t%s\t%d\t%s\t%s\t%d\t%d\n" % (name(u1, circular[u1]), "-" if s1 else "+", j1, name(u2, circular[u2]), "-" if s2 else "+", j2, count))
    return "".join(lines)
