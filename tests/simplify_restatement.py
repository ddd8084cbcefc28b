"""A plain, slow statement of the tip and simple-bubble rules of include/mdbg_hip.h (mdbg_graph_simplify) on dictionaries, sets and tuples.
It is the CHECKER of the simplification tests.  The current unitigs of every step come from unitig_restatement.unitigs on the induced graph;
nothing here numbers vertices, sorts by a key or keeps a mask.  The rules are this project's own, order-free definition — not gfatools' passes."""
import unitig_restatement as U

TIPS, BUBBLES = 1, 2


def as_steps(steps):
    """[(kind, max_nodes, max_bases)] or [dict(kind=, max_nodes=, max_bases=)] -> list of tuples"""
    out = []
    for s in steps:
        if isinstance(s, dict):
            s = (s["kind"], s.get("max_nodes", 0), s.get("max_bases", 0))
        kind, mn, mb = (int(x) for x in s)
        assert kind in (TIPS, BUBBLES), kind
        out.append((kind, mn, mb))
    return out


def induced(nodes, edges, alive):
    """the node table and the edge records restricted to the surviving node indices, records in their order"""
    keep = [i for i, x in enumerate(nodes["index"]) if int(x) in alive]
    sub = {f: [v[i] for i in keep] for f, v in nodes.items() if f in ("index", "abundance", "src_read", "src_start", "src_end", "reversed", "shift_full") and v is not None}
    recs = [(u[0], u[1], v[0], v[1], ov) for u, v, ov in U.as_records(edges) if u[0] in alive and v[0] in alive]
    return sub, recs


def arcs_of(recs):
    succ, pred = {}, {}
    for a, oa, b, ob, _ in recs:
        u, v = (a, oa), (b, ob)
        for x, y in ((u, v), (U.comp(v), U.comp(u))):
            succ.setdefault(x, set()).add(y)
            pred.setdefault(y, set()).add(x)
    return succ, pred


def beats(a, b, cur):
    """unitig a ranks above unitig b: mean abundance (exactly), then length, then the smaller number"""
    na, nb = len(cur["walks"][a]), len(cur["walks"][b])
    ma, mb = cur["kc_sum"][a] * nb, cur["kc_sum"][b] * na
    if ma != mb:
        return ma > mb
    if cur["length"][a] != cur["length"][b]:
        return cur["length"][a] > cur["length"][b]
    return a < b


def small(i, cur, max_nodes, max_bases):
    return (not cur["circular"][i]) and (max_nodes == 0 or len(cur["walks"][i]) <= max_nodes) and (max_bases == 0 or cur["length"][i] <= max_bases)


def tip_candidates(cur, succ, pred, max_nodes, max_bases):
    """unitig -> its attached vertex (the last vertex of the one orientation whose first vertex has no in-arc)"""
    att = {}
    for i, w in enumerate(cur["walks"]):
        if not small(i, cur, max_nodes, max_bases):
            continue
        fwd = not pred.get(w[0])                      # as written: nothing enters the first vertex
        rev = not succ.get(w[-1])                     # mirrored: nothing enters comp(last), i.e. nothing leaves last
        if fwd != rev:
            att[i] = w[-1] if fwd else U.comp(w[0])
    return att


def tips_to_remove(cur, succ, pred, max_nodes, max_bases):
    att = tip_candidates(cur, succ, pred, max_nodes, max_bases)
    owner = {x: i for i, x in att.items()}
    gone = set()
    for i, x in att.items():
        def other_way_in(w):
            return any(y != x and (y not in owner or beats(owner[y], i, cur)) for y in pred[w])
        if all(other_way_in(w) for w in succ[x]):
            gone.add(i)
    return gone


def branches(cur, succ, pred, max_nodes, max_bases):
    """unitig -> key of the simple bubble it is a branch of (a set of the two readings of (entry, exit): one per strand)"""
    out = {}
    for i, w in enumerate(cur["walks"]):
        if not small(i, cur, max_nodes, max_bases):
            continue
        ins, outs = pred.get(w[0], set()), succ.get(w[-1], set())
        if len(ins) != 1 or len(outs) != 1:
            continue
        (p,), (q,) = ins, outs
        on = {n for n, _ in w}
        if p[0] in on or q[0] in on or q == U.comp(p):
            continue
        out[i] = frozenset([(p, q), (U.comp(q), U.comp(p))])
    return out


def bubbles_to_remove(cur, succ, pred, max_nodes, max_bases):
    groups = {}
    for i, key in branches(cur, succ, pred, max_nodes, max_bases).items():
        groups.setdefault(key, []).append(i)
    gone = set()
    for members in groups.values():
        if len(members) < 2:
            continue
        best = [a for a in members if all(a == b or beats(a, b, cur) for b in members)]
        assert len(best) == 1
        gone.update(m for m in members if m != best[0])
    return gone


def current(nodes, edges, alive, reads, length_of):
    sub, recs = induced(nodes, edges, alive)
    cur = U.unitigs(sub, recs, reads)
    if reads is None:
        assert length_of is not None, "without reads the caller says what a walk's length is"
        cur["length"] = [length_of(w) for w in cur["walks"]]
    return cur, recs


def simplify(nodes, edges, steps, reads=None, length_of=None):
    """-> (per step: dict(kind, unitigs = the removed unitigs' walks, nodes = set of removed node indices), unitigs(...) of what is left)"""
    alive = {int(i) for i in nodes["index"]}
    log = []
    for kind, mn, mb in as_steps(steps):
        cur, recs = current(nodes, edges, alive, reads, length_of)
        succ, pred = arcs_of(recs)
        gone = (tips_to_remove if kind == TIPS else bubbles_to_remove)(cur, succ, pred, mn, mb)
        removed = {n for i in gone for n, _ in cur["walks"][i]}
        log.append(dict(kind=kind, unitigs=[cur["walks"][i] for i in sorted(gone)], nodes=removed))
        alive -= removed
    final, _ = current(nodes, edges, alive, reads, length_of)
    return log, final
