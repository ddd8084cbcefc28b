"""A plain, slow statement of the transit definition of include/mdbg_hip.h (mdbg_graph_transits), working on dictionaries and tuples: one read at a time, one
pair of neighbouring windows at a time, the chain of explained crossings extended or broken.  It is the CHECKER of the transit tests and shares nothing with
the code under test — no packed keys, no scan, no sort, no counters.  Written from the rule.

Inputs: those of junctions_restatement.junctions (the reads as lists of minimizer hashes in slot order, k, the node table's `keys` and `index` columns, the
unitig list as walks [[(index, '+' / '-')]], the list's edge records as (n1, o1, n2, o2[, overlap]) tuples) and the call's min_support.
A vertex is (unitig, entry, strand); a transit key is (u, p, q) with p and q vertices."""
from junctions_restatement import is_link, key_of, mirror, placements, record_key

PLAIN, RESOLVED, UNRESOLVED, SELF = 0, 1, 2, 3
VERDICT_NAMES = ("plain", "resolved", "unresolved", "self")


def transits_of_read(placed, known, walks):
    """the transits of one read, canonical: [(u, p, q)] in window order.  `last` is the explained crossing (w, pair) the chain hangs on, or None"""
    out, last = [], None
    for w, (x, y) in enumerate(zip(placed, placed[1:])):
        if x is None or y is None:                       # an unplaced window ends the chain
            last = None
            continue
        if is_link(x, y):
            continue
        c = (x, y)
        if key_of(c) not in known:                       # a missing crossing ends the chain
            last = None
            continue
        if last is not None:
            w0, c0 = last
            (_, y0), (x1, _) = c0, c
            u, s = y0[0], y0[2]
            m = len(walks[u])
            assert (x1[0], x1[2]) == (u, s) and w - w0 == m, "a transit does not walk all of one unitig"
            first, second = (c0, c) if s == 0 else (mirror(c), mirror(c0))
            assert first[1] == (u, 0, 0) and second[0] == (u, m - 1, 0), "the canonical form has another shape"
            out.append((u, first[0], second[1]))
        last = (w, c)
    return out


def verdict_of(u, n_in, n_out, is_self, counts, min_support):
    """counts: {(p, q): count} of unitig u"""
    if n_in < 2 or n_out < 2:
        return PLAIN
    if is_self:
        return SELF
    strong = [pq for pq, n in counts.items() if n >= min_support]
    if n_in == n_out == len(strong) and len({p for p, _ in strong}) == len(strong) and len({q for _, q in strong}) == len(strong):
        return RESOLVED
    return UNRESOLVED


def transits(reads, k, keys, index, walks, edges, min_support=1):
    """-> dict(n_crossings, n_explained, n_passes, n_transits, n_unitigs, n_repeats, n_resolved, counts: {(u, p, q): count},
    rows: [(u, pu, pj, ps, qu, qj, qs, in_record, out_record, count)] in key order, n_in, n_out, passes, verdict: per unitig)"""
    assert min_support >= 1
    rkeys = [record_key(e, walks) for e in edges]
    known = set(rkeys)
    first_record = {}
    for r, key in enumerate(rkeys):
        first_record.setdefault(key, r)
    counts = {}
    n_crossings = n_explained = 0
    for placed in placements(reads, k, keys, index, walks):
        for x, y in zip(placed, placed[1:]):
            if x is not None and y is not None and not is_link(x, y):
                n_crossings += 1
                n_explained += key_of((x, y)) in known
        for t in transits_of_read(placed, known, walks):
            counts[t] = counts.get(t, 0) + 1
    rows = []
    for (u, p, q) in sorted(counts):
        m = len(walks[u])
        rows.append((u,) + p + q + (first_record[key_of((p, (u, 0, 0)))], first_record[key_of(((u, m - 1, 0), q))], counts[(u, p, q)]))
    U = len(walks)
    pairs = set()
    for e in edges:
        n1, o1, n2, o2 = e[:4]
        pair = ((n1, len(walks[n1]) - 1 if o1 == "+" else 0, int(o1 == "-")), (n2, 0 if o2 == "+" else len(walks[n2]) - 1, int(o2 == "-")))
        pairs.add(pair)
        pairs.add(mirror(pair))
    by_target, by_source = {}, {}                       # the distinct keys of the pairs that end on, and that start from, a vertex
    for pr in pairs:
        by_source.setdefault(pr[0], set()).add(key_of(pr))
        by_target.setdefault(pr[1], set()).add(key_of(pr))
    n_in = [len(by_target.get((u, 0, 0), ())) for u in range(U)]
    n_out = [len(by_source.get((u, len(walks[u]) - 1, 0), ())) for u in range(U)]
    selfs = {e[0] for e in edges if e[0] == e[2]}
    passes = [0] * U
    per_unitig = [{} for _ in range(U)]
    for (u, p, q), n in counts.items():
        passes[u] += n
        per_unitig[u][(p, q)] = n
    verdict = [verdict_of(u, n_in[u], n_out[u], u in selfs, per_unitig[u], min_support) for u in range(U)]
    repeats = [u for u in range(U) if n_in[u] >= 2 and n_out[u] >= 2]
    return dict(n_crossings=n_crossings, n_explained=n_explained, n_passes=sum(counts.values()), n_transits=len(counts), n_unitigs=U, n_repeats=len(repeats),
                n_resolved=sum(verdict[u] == RESOLVED for u in repeats), counts=counts, rows=rows, n_in=n_in, n_out=n_out, passes=passes, verdict=verdict,
                self_flags=[int(u in selfs) for u in range(U)])


def at_min_support(t, min_support):
    """a transits() result -> the same range at another min_support: only the verdicts and n_resolved depend on it"""
    assert min_support >= 1
    per_unitig = [{} for _ in range(t["n_unitigs"])]
    for (u, p, q), n in t["counts"].items():
        per_unitig[u][(p, q)] = n
    verdict = [verdict_of(u, t["n_in"][u], t["n_out"][u], t["self_flags"][u], per_unitig[u], min_support) for u in range(t["n_unitigs"])]
    return dict(t, verdict=verdict, n_resolved=sum(v == RESOLVED for v in verdict))


def name(i, circular):
    return "utg%07d%s" % (i + 1, "c" if circular else "l")


def tsv_text(t, circular):
    """one T line per key in key order, then one U line per unitig with n_in >= 2 and n_out >= 2 in unitig order"""
    sign = lambda s: "-" if s else "+"
    lines = ["T\t%s\t%s\t%s\t+\t%s\t%s\t%d\n" % (name(pu, circular[pu]), sign(ps), name(u, circular[u]), name(qu, circular[qu]), sign(qs), n)
             for u, pu, _, ps, qu, _, qs, _, _, n in t["rows"]]
    for u in range(t["n_unitigs"]):
        if t["n_in"][u] >= 2 and t["n_out"][u] >= 2:
            lines.append("U\t%s\t%d\t%d\t%d\t%s\n" % (name(u, circular[u]), t["n_in"][u], t["n_out"][u], t["passes"][u], VERDICT_NAMES[t["verdict"][u]]))
    return "".join(lines)
