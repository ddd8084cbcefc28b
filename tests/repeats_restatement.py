"""A plain, slow statement of the REPEATS step of include/mdbg_hip.h (mdbg_graph_simplify, MDBG_SIMPLIFY_REPEATS) and of a schedule that mixes it with tip,
bubble, component and edge-pruning steps, on dictionaries, sets and tuples.  It is the CHECKER of the repeat tests, written from the rule, in the pattern of
edge_prune_restatement.simplify.

The state of a schedule is (columns, records, alive, dead_arcs, origin): the node columns and the edge records, both of which a REPEATS step extends by its
copies; the surviving node indices; the removed arcs; and for every copy's index the index of its original.  The unitigs of every step come from
unitig_restatement.unitigs, the verdicts from transits_restatement.transits over all reads.  Nothing here numbers vertices, scans or keeps a mask."""
import components_restatement as C
import edge_prune_restatement as EP
import simplify_restatement as S
import transits_restatement as T
import unitig_restatement as U

TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS = 1, 2, 4, 8, 16
COLUMNS = ("index", "abundance", "src_read", "src_start", "src_end", "reversed", "shift_full")


def as_steps(steps):
    """the limits of the header: (EDGES | REPEATS, min_support >= 1, 0), at most one REPEATS step, no EDGES step behind it"""
    out, seen = [], False
    for kind, a, b in steps:
        kind, a, b = int(kind), int(a), int(b)
        assert kind in (TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS), kind
        assert kind not in (EDGES, REPEATS) or (a >= 1 and b == 0), "an EDGES or REPEATS step is (kind, min_support >= 1, 0)"
        assert kind != COMPONENTS or a or b, "a component step without a limit would remove the whole graph"
        assert not (seen and kind in (EDGES, REPEATS)), "one REPEATS step, and no EDGES step behind it"
        seen |= kind == REPEATS
        out.append((kind, a, b))
    return out


def list_vertices(walks):
    """node vertex (index, o) -> the vertex (u, j, s) of the list"""
    out = {}
    for u, w in enumerate(walks):
        for j, (idx, o) in enumerate(w):
            out[(idx, o)] = (u, j, 0)
            out[(idx, U.flip(o))] = (u, j, 1)
    return out


def flipped(v):
    return (v[0], v[1], 1 - v[2])


def strong_keys(t, min_support):
    """resolved unitig -> its strong keys (p, q) in key order"""
    out = {}
    for u, verdict in enumerate(t["verdict"]):
        if verdict == T.RESOLVED:
            keys = sorted((p, q) for (uu, p, q), n in t["counts"].items() if uu == u and n >= min_support)
            assert len(keys) == t["n_in"][u] == t["n_out"][u] >= 2
            assert len({p for p, _ in keys}) == len(keys) == len({q for _, q in keys})
            out[u] = keys
    return out


def the_one(found):
    assert len(found) == 1, "exactly one strong key takes an end of a record at a resolved unitig: %r" % (found,)
    return found[0]


def duplicate(cols, records, in_graph, walks, keys, first_index, origin):
    """the step itself.  cols, records and origin are extended in place; in_graph: per record, whether it is a record of the current graph; keys: strong_keys().
    -> the number of copies"""
    copy, c = {}, 0
    row_of = {int(x): r for r, x in enumerate(cols["index"])}
    for u in sorted(keys):
        for i in range(1, len(keys[u])):
            for j, (idx, _) in enumerate(walks[u]):
                copy[(u, i, j)] = first_index + c
                origin[first_index + c] = idx
                for f in cols:
                    cols[f].append(first_index + c if f == "index" else cols[f][row_of[idx]])
                c += 1
    at = list_vertices(walks)
    interior = set()
    for w in walks:
        for a, b in zip(w, w[1:]):
            interior.add((a, b))
            interior.add((U.comp(b), U.comp(a)))
    added = []
    for r, (a, oa, b, ob, ov) in enumerate(records):
        if not in_graph[r]:
            continue
        x, y = at[(a, oa)], at[(b, ob)]
        if ((a, oa), (b, ob)) in interior:
            assert x[0] == y[0]
            for i in range(1, len(keys.get(x[0], ()))):
                added.append((copy[(x[0], i, x[1])], oa, copy[(x[0], i, y[1])], ob, ov))
            continue
        if x[0] in keys:                                 # the source end
            u, m = x[0], len(walks[x[0]])
            if x == (u, m - 1, 0):
                i = the_one([i for i, (p, q) in enumerate(keys[u]) if q == y])
            else:
                assert x == (u, 0, 1)
                i = the_one([i for i, (p, q) in enumerate(keys[u]) if p == flipped(y)])
            if i:
                a = copy[(u, i, x[1])]
        if y[0] in keys:                                 # the target end
            u, m = y[0], len(walks[y[0]])
            if y == (u, 0, 0):
                i = the_one([i for i, (p, q) in enumerate(keys[u]) if p == x])
            else:
                assert y == (u, m - 1, 1)
                i = the_one([i for i, (p, q) in enumerate(keys[u]) if q == flipped(x)])
            if i:
                b = copy[(u, i, y[1])]
        records[r] = (a, oa, b, ob, ov)
    records.extend(added)
    return c


def simplify(nodes, edges, steps, hashes, k, reads=None, length_of=None):
    """hashes: every resident read as its list of minimizer hashes, in slot order; reads / length_of: as edge_prune_restatement.simplify (length_of sees the
    ORIGINALS' indices)
    -> (per step: the dict of edge_prune_restatement.simplify, a REPEATS step with copies = the entries it added and resolved = the unitigs it duplicated;
    unitigs(...) of what is left, with walks holding the COPIES' indices, walks_original the originals' (what the list's node[] reports), origin and copies)"""
    cols = {f: [x for x in nodes[f]] for f in COLUMNS if nodes.get(f) is not None}
    cols["index"] = [int(x) for x in cols["index"]]
    records = [(u[0], u[1], v[0], v[1], ov) for u, v, ov in U.as_records(edges)]
    first_index = 1 + max(cols["index"]) if cols["index"] else 0
    alive, dead_arcs, origin = set(cols["index"]), set(), {}
    originals = lambda w: [(origin.get(i, i), o) for i, o in w]
    length = None if length_of is None else (lambda w: length_of(originals(w)))
    log = []
    for kind, a, b in as_steps(steps):
        cur, recs = EP.current(cols, records, alive, dead_arcs, reads, length)
        if kind == EDGES:
            assert not origin
            dead, gone, weak, support = EP.edges_to_remove(cur, hashes, k, nodes, a)
            assert not (dead & dead_arcs)
            n_records = sum(((r[0], r[1]), (r[2], r[3])) in dead for r in recs)
            assert n_records == len(gone)
            dead_arcs |= dead
            log.append(dict(kind=kind, unitigs=[], nodes=set(), edges=n_records, weak=len(weak), support=support))
            continue
        if kind == REPEATS:
            keys = {}
            if hashes and cur["walks"]:
                t = T.transits(hashes, k, nodes["keys"].tolist(), nodes["index"].tolist(), cur["walks"], [e[:4] for e in cur["edges"]], a)
                keys = strong_keys(t, a)
            in_graph = [r[0] in alive and r[2] in alive and ((r[0], r[1]), (r[2], r[3])) not in dead_arcs for r in records]
            n_before = len(records)
            copies = duplicate(cols, records, in_graph, cur["walks"], keys, first_index, origin) if keys else 0
            assert len(records) >= n_before and all(i not in alive for i in origin)
            alive |= set(origin)
            log.append(dict(kind=kind, unitigs=[], nodes=set(), edges=0, copies=copies, resolved=sorted(keys)))
            continue
        if kind == COMPONENTS:
            gone = C.components_to_remove(cur, a, b)
        else:
            succ, pred = S.arcs_of(recs)
            gone = (S.tips_to_remove if kind == TIPS else S.bubbles_to_remove)(cur, succ, pred, a, b)
        removed = {n for i in gone for n, _ in cur["walks"][i]}
        log.append(dict(kind=kind, unitigs=[cur["walks"][i] for i in sorted(gone)], nodes=removed, edges=0))
        alive -= removed
    final, _ = EP.current(cols, records, alive, dead_arcs, reads, length)
    final.update(walks_original=[originals(w) for w in final["walks"]], origin=dict(origin), copies=len(origin))
    return log, final
