"""A plain, slow statement of the SUPERBUBBLES rule of include/mdbg_hip.h (mdbg_graph_simplify, MDBG_SIMPLIFY_SUPERBUBBLES) on dictionaries, sets and tuples, on
top of simplify_restatement.current / beats and components_restatement.  It is the CHECKER of the superbubble tests.  A vertex is (unitig number, '+' / '-');
per source the interior is the forward closure that stops at the candidate sink, and (a) .. (f) are tested on it one by one as the header writes them: no queue
of ready vertices, no in-degree counters, no topological sort.  The driver asserts on every call what the rule claims about applied bubbles."""
import components_restatement as CR
import simplify_restatement as S
import unitig_restatement as U

TIPS, BUBBLES, COMPONENTS, SUPERBUBBLES = S.TIPS, S.BUBBLES, CR.COMPONENTS, 64
MAX_UNITIGS = 64                               # MDBG_SUPERBUBBLE_MAX_UNITIGS
INF = None                                     # val(s)


def as_steps(steps):
    out = []
    for s in steps:
        if isinstance(s, dict):
            s = (s["kind"], s.get("max_nodes", 0), s.get("max_bases", 0))
        kind, mn, mb = (int(x) for x in s)
        assert kind in (TIPS, BUBBLES, COMPONENTS, SUPERBUBBLES), kind
        assert kind != COMPONENTS or mn or mb
        out.append((kind, mn, mb))
    return out


def unitig_arcs(cur):
    """the arcs between oriented unitigs: every unitig edge record and its mirror, parallel records and duplicates as one arc"""
    succ, pred = {}, {}
    for a, oa, b, ob, _ in cur["edges"]:
        for x, y in (((a, oa), (b, ob)), ((b, U.flip(ob)), (a, U.flip(oa)))):
            succ.setdefault(x, set()).add(y)
            pred.setdefault(y, set()).add(x)
    return succ, pred


def closure(s, t, succ):
    """what can be reached from s without leaving t, without s and t; None: more than MAX_UNITIGS (f), or s itself comes back (s is not in I)"""
    seen, todo = set(), [s]
    while todo:
        for y in succ.get(todo.pop(), ()):
            if y == t or y in seen:
                continue
            if y == s or len(seen) == MAX_UNITIGS:
                return None
            seen.add(y)
            todo.append(y)
    return seen


def has_cycle(members, succ):
    """(c) by removing, again and again, a vertex that no remaining arc enters"""
    left = set(members)
    while left:
        free = [x for x in left if not any(x in succ.get(y, ()) for y in left)]
        if not free:
            return True
        left -= set(free)
    return False


def bounds(s, t, I, succ, pred):
    """(a) .. (d) and (f), literally; (e) is the caller's"""
    if not I or s in I or t in I or t == s or len(I) > MAX_UNITIGS:
        return False
    if not all(succ.get(x, set()) <= I | {t} for x in I | {s}) or not all(succ.get(x) for x in I):                  # (a)
        return False
    if not all(pred.get(x, set()) <= I | {s} for x in I | {t}) or not all(pred.get(x) for x in I):                  # (b)
        return False
    members = I | {s, t}
    if has_cycle(members, succ):                                                                                      # (c)
        return False
    return len({x[0] for x in members}) == len(members)                                                               # (d)


def superbubble_from(s, succ, pred):
    """-> (t, I) or None"""
    if len(succ.get(s, ())) < 2:
        return None
    reach, todo = set(), [s]
    while todo:                                                        # every vertex s reaches is a candidate sink
        for y in succ.get(todo.pop(), ()):
            if y not in reach:
                reach.add(y)
                todo.append(y)
    found = {}
    for t in reach:
        I = closure(s, t, succ)
        if I is not None and bounds(s, t, I, succ, pred):
            found[t] = I
    first = [t for t, I in found.items() if not any(t2 in I and found[t2] <= I for t2 in found)]                     # (e)
    assert len(first) <= 1, (s, first)
    return (first[0], found[first[0]]) if first else None


def fits(I, cur, max_nodes, max_bases):
    return (max_nodes == 0 or sum(len(cur["walks"][u]) for u, _ in I) <= max_nodes) and (max_bases == 0 or sum(cur["length"][u] for u, _ in I) <= max_bases)


def mean_of(x, cur):
    return (cur["kc_sum"][x[0]], len(cur["walks"][x[0]]))


def above(a, b):
    """val a > val b, by cross products"""
    if a is INF or b is INF:
        return a is INF and b is not INF
    return a[0] * b[1] > b[0] * a[1]


def kept_path(s, t, I, pred, cur):
    val, best = {s: INF}, {}

    def settle(x):
        if x in val:
            return
        for y in pred[x]:
            settle(y)
        top = None
        for y in pred[x]:
            if top is None or above(val[y], val[top]) or (not above(val[top], val[y]) and S.beats(y[0], top[0], cur)):
                top = y
        best[x] = top
        val[x] = val[top] if above(mean_of(x, cur), val[top]) else mean_of(x, cur)
    settle(t)
    path = [t]
    while path[-1] != s:
        path.append(best[path[-1]])
        assert len(path) <= len(I) + 2
    return path[::-1]


def comp_set(I):
    return {U.comp(x) for x in I}


def order_key(v):
    return (v[0], 0 if v[1] == "+" else 1)


def find_bubbles(cur, max_nodes, max_bases):
    """-> (succ, pred, the fitting bubbles in their canonical reading: [(s, t, I)])"""
    succ, pred = unitig_arcs(cur)
    out = []
    for s in sorted(succ, key=order_key):
        got = superbubble_from(s, succ, pred)
        if got is None or not fits(got[1], cur, max_nodes, max_bases):
            continue
        t, I = got
        mirror = superbubble_from(U.comp(t), succ, pred)
        assert mirror == (U.comp(s), comp_set(I)), (s, t, mirror)                  # the two readings are one bubble
        if order_key(s) < order_key(U.comp(t)):
            out.append((s, t, I))
    return succ, pred, out


def paths(s, t, succ, gone):
    """the number of paths from s to t among the unitigs that are left"""
    if s == t:
        return 1
    return sum(paths(y, t, succ, gone) for y in succ.get(s, ()) if y[0] not in gone)


def superbubbles_to_remove(cur, max_nodes, max_bases, report=None, nested_ok=False):
    succ, pred, fitting = find_bubbles(cur, max_nodes, max_bases)
    J = set()
    for _, _, I in fitting:
        J |= I | comp_set(I)
    applied = [(s, t, I, kept_path(s, t, I, pred, cur)) for s, t, I in fitting if s not in J and U.comp(t) not in J]
    gone = set()
    for s, t, I, keep in applied:
        gone |= {x[0] for x in I - set(keep)}
    # what the rule claims
    for i, (s, t, I, keep) in enumerate(applied):
        for s2, t2, I2, _ in applied[i + 1:]:
            assert not ({x[0] for x in I} & {x[0] for x in I2}), ("applied bubbles share a unitig", s, t, s2, t2)
        assert not ({x[0] for x in keep} & gone), ("a kept path lost a unitig", s, t)
        assert paths(s, t, succ, gone) == 1, ("not exactly one path is left", s, t)
    for a, (s, t, I) in enumerate(fitting):                                         # fitting bubbles are nested or disjoint
        for s2, t2, I2 in fitting[a + 1:]:
            A, B = {x[0] for x in I}, {x[0] for x in I2}
            assert not (A & B) or A <= B or B <= A, ("fitting bubbles overlap without nesting", s, t, s2, t2)
    if report is not None:
        report.append(dict(fitting=[(s, t, sorted(I, key=order_key)) for s, t, I in fitting], applied=[(s, t, sorted(I, key=order_key), keep) for s, t, I, keep in applied]))
    return gone


def simplify(nodes, edges, steps, reads=None, length_of=None, report=None):
    """the step loop of simplify_restatement.simplify with kinds 4 and 64 added; same return value.  report (a list): one dict(fitting, applied) per SUPERBUBBLES step"""
    alive = {int(i) for i in nodes["index"]}
    log = []
    for kind, mn, mb in as_steps(steps):
        cur, recs = S.current(nodes, edges, alive, reads, length_of)
        if kind == SUPERBUBBLES:
            gone = superbubbles_to_remove(cur, mn, mb, report)
        elif kind == COMPONENTS:
            gone = CR.components_to_remove(cur, mn, mb)
        else:
            succ, pred = S.arcs_of(recs)
            gone = (S.tips_to_remove if kind == TIPS else S.bubbles_to_remove)(cur, succ, pred, mn, mb)
        removed = {n for i in gone for n, _ in cur["walks"][i]}
        log.append(dict(kind=kind, unitigs=[cur["walks"][i] for i in sorted(gone)], nodes=removed))
        alive -= removed
    final, _ = S.current(nodes, edges, alive, reads, length_of)
    return log, final
