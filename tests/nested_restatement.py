"""A plain, slow statement of the NESTED step of include/mdbg_hip.h (mdbg_graph_simplify, MDBG_SIMPLIFY_NESTED): the placement of the resident reads on a
unitig list that holds copies, the transits over those placements, and a schedule that mixes TIPS, BUBBLES, COMPONENTS, EDGES (in front), REPEATS and NESTED
steps, on dictionaries, lists and tuples.  It is the CHECKER of the nested-repeat tests, written from the header's text: one read at a time, one window at a
time, each ambiguous window looking along its own read for its two anchors.  No codes, no scans, no maps from rows to entries.

It imports the existing restatements and leaves them as they are: the unitigs of every step come from unitig_restatement.unitigs (through
edge_prune_restatement.current), the transit rule from transits_restatement (handed the placements below in place of the plain ones), the copy and arc rule
from repeats_restatement.duplicate.  The state of a schedule is that of repeats_restatement.simplify, with origin[] naming the TABLE ROW's index for every copy."""
import components_restatement as C
import edge_prune_restatement as EP
import repeats_restatement as RR
import simplify_restatement as S
import transits_restatement as T
from read_paths_restatement import canonical

TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS, NESTED = 1, 2, 4, 8, 16, 128
UNPLACED, UNIQUE, AMBIGUOUS = "unplaced", "unique", "ambiguous"


def as_steps(steps):
    """the limits of the header: (EDGES | REPEATS | NESTED, min_support >= 1, 0); a REPEATS step stands on a graph without copies, so behind no REPEATS and no
    NESTED step; no EDGES step behind either"""
    out, repeats, nested = [], False, False
    for kind, a, b in steps:
        kind, a, b = int(kind), int(a), int(b)
        assert kind in (TIPS, BUBBLES, COMPONENTS, EDGES, REPEATS, NESTED), kind
        assert kind not in (EDGES, REPEATS, NESTED) or (a >= 1 and b == 0), "an EDGES, REPEATS or NESTED step is (kind, min_support >= 1, 0)"
        assert kind != COMPONENTS or a or b, "a component step without a limit would remove the whole graph"
        assert not ((repeats or nested) and kind in (EDGES, REPEATS)), "no EDGES and no REPEATS step behind a step that may copy"
        repeats |= kind == REPEATS
        nested |= kind == NESTED
        out.append((kind, a, b))
    return out


def entries_of_rows(walks, origin):
    """row (named by its table index) -> the entries (u, j, ori) of the list that descend from it"""
    out = {}
    for u, walk in enumerate(walks):
        for j, (idx, o) in enumerate(walk):
            out.setdefault(origin.get(int(idx), int(idx)), []).append((u, j, o))
    return out


def candidate(anchor, distance, behind, row, rev, walks, origin):
    """the entry `distance` windows behind (or in front of) the anchor's vertex along the read, if it is valid for a window of `row` read in orientation `rev`"""
    u, j, s = anchor
    j2 = j + distance if behind == (s == 0) else j - distance
    if not 0 <= j2 < len(walks[u]):                      # the same unitig, never wrapped
        return None
    idx, o = walks[u][j2]
    if origin.get(int(idx), int(idx)) != row or int(rev != (o == "-")) != s:
        return None
    return (u, j2, s)


def classify(H, k, row_of_key, entries):
    """per window of one read: (class, row, rev, the vertex of a UNIQUE window)"""
    out = []
    for w in range(len(H) - k + 1 if len(H) > k else 0):
        key, rev = canonical(tuple(H[w:w + k]))
        row = row_of_key.get(key)
        at = entries.get(row, []) if row is not None else []
        if len(at) == 0:
            out.append((UNPLACED, row, rev, None))
        elif len(at) == 1:
            u, j, o = at[0]
            out.append((UNIQUE, row, rev, (u, j, int(rev != (o == "-")))))
        else:
            out.append((AMBIGUOUS, row, rev, None))
    return out


def place_read(H, k, row_of_key, entries, walks, origin, tally=None):
    """one read -> per window the vertex it is placed on, or None.  tally: a dict that counts ambiguous / resolved / conflicts / unanchored"""
    cls = classify(H, k, row_of_key, entries)
    placed = []
    for w, (what, row, rev, at) in enumerate(cls):
        if what != AMBIGUOUS:
            placed.append(at)
            continue
        found = []
        for step, behind in ((-1, True), (1, False)):    # the left anchor, then the right one
            a = w + step
            while 0 <= a < len(cls) and cls[a][0] == AMBIGUOUS:
                a += step
            if 0 <= a < len(cls) and cls[a][0] == UNIQUE:  # the nearest window that is not ambiguous, provided it is unique
                c = candidate(cls[a][3], abs(w - a), behind, row, rev, walks, origin)
                if c is not None:
                    found.append(c)
        verdict = found[0] if found and all(c == found[0] for c in found) else None
        placed.append(verdict)
        if tally is not None:
            tally["ambiguous"] = tally.get("ambiguous", 0) + 1
            name = "resolved" if verdict is not None else "conflicts" if len(found) == 2 else "unanchored"
            tally[name] = tally.get(name, 0) + 1
    return placed


def placements(reads, k, keys, index, walks, origin, tally=None):
    """per read, per window: the vertex (u, j, s) it is placed on, or None — junctions_restatement.placements on a list that holds copies"""
    row_of_key = {tuple(int(v) for v in key): int(i) for key, i in zip(keys, index)}
    entries = entries_of_rows(walks, origin)
    return [place_read([int(h) for h in H], k, row_of_key, entries, walks, origin, tally) for H in reads]


def brute_force_placements(reads, k, keys, index, walks, origin):
    """the same by another road: every ambiguous window tries EVERY entry of its row and keeps those that an anchor reaches by stepping one entry per window
    along the read, the anchors found by walking the read outwards one window at a time"""
    row_of_key = {tuple(int(v) for v in key): int(i) for key, i in zip(keys, index)}
    entries = entries_of_rows(walks, origin)
    out = []
    for H in reads:
        H = [int(h) for h in H]
        cls = classify(H, k, row_of_key, entries)
        placed = []
        for w, (what, row, rev, at) in enumerate(cls):
            if what != AMBIGUOUS:
                placed.append(at)
                continue
            reached = []
            for step in (-1, 1):
                a = w
                while True:
                    a += step
                    if not 0 <= a < len(cls) or cls[a][0] == UNPLACED:
                        a = None
                        break
                    if cls[a][0] == UNIQUE:
                        break
                if a is None:
                    continue
                au, aj, s = cls[a][3]
                hits = [(u, j, s) for (u, j, o) in entries[row]
                        if u == au and int(rev != (o == "-")) == s and (j - aj) * (1 if s == 0 else -1) == w - a]
                assert len(hits) <= 1
                reached += hits
            placed.append(reached[0] if reached and len(set(reached)) == 1 else None)
        out.append(placed)
    return out


def transits(reads, k, keys, index, walks, edges, min_support, origin, tally=None):
    """transits_restatement.transits over the placements above.  Without copies these ARE the plain placements (every row has at most one entry), and the
    plain function is called as it stands"""
    if not origin:
        return T.transits(reads, k, keys, index, walks, edges, min_support)
    plain = T.placements
    T.placements = lambda reads_, k_, keys_, index_, walks_: placements(reads_, k_, keys_, index_, walks_, origin, tally)
    try:
        return T.transits(reads, k, keys, index, walks, edges, min_support)
    finally:
        T.placements = plain


def simplify(nodes, edges, steps, hashes, k, reads=None, length_of=None, tally=None):
    """repeats_restatement.simplify with NESTED steps: the same arguments, the same result.  A REPEATS or NESTED step's log entry has copies = the entries it
    added and resolved = the unitigs it duplicated; final has walks (the copies' indices), walks_original (the ORIGINS' indices, what node[] reports), origin
    (copy's index -> its table row's index) and copies (all of the schedule).  tally: a dict that collects the four placement counts of the steps that ran
    on a graph with copies"""
    import unitig_restatement as U
    cols = {f: [x for x in nodes[f]] for f in RR.COLUMNS if nodes.get(f) is not None}
    cols["index"] = [int(x) for x in cols["index"]]
    records = [(u[0], u[1], v[0], v[1], ov) for u, v, ov in U.as_records(edges)]
    first_index = 1 + max(cols["index"]) if cols["index"] else 0      # X: of the node TABLE, for the whole schedule
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
        if kind in (REPEATS, NESTED):
            assert kind == NESTED or not origin
            keys = {}
            if hashes and cur["walks"]:
                t = transits(hashes, k, nodes["keys"].tolist(), nodes["index"].tolist(), cur["walks"], [e[:4] for e in cur["edges"]], a, origin, tally)
                keys = RR.strong_keys(t, a)
            in_graph = [r[0] in alive and r[2] in alive and ((r[0], r[1]), (r[2], r[3])) not in dead_arcs for r in records]
            n_before, copied_from = len(records), {}
            copies = RR.duplicate(cols, records, in_graph, cur["walks"], keys, first_index + len(origin), copied_from) if keys else 0
            assert len(records) >= n_before and copies == len(copied_from) and all(i not in alive and i not in origin for i in copied_from)
            assert sorted(copied_from) == list(range(first_index + len(origin), first_index + len(origin) + copies))      # behind all earlier copies
            for new in sorted(copied_from):              # the origin of a copy of a copy is the table row's
                origin[new] = origin.get(copied_from[new], copied_from[new])
            alive |= set(copied_from)
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
