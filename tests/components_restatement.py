"""A plain, slow statement of the component definition of include/mdbg_hip.h (mdbg_graph_components) and of the small-component step of
mdbg_graph_simplify, on dictionaries and sets over the output of unitig_restatement.unitigs.  It is the CHECKER of the component tests: sets of
unitig numbers, merged whenever an edge joins two of them — no parent array, no path compression, no scan."""
import simplify_restatement as S

TIPS, BUBBLES, COMPONENTS = S.TIPS, S.BUBBLES, 4


def classes(cur):
    """the components as sets of unitig numbers, ordered by their smallest member"""
    where = {i: {i} for i in range(len(cur["walks"]))}                         # unitig -> the set it lies in
    for e in cur["edges"]:
        a, b = e[0], e[2]                                                      # orientation ignored; "u + u +" joins nothing
        if where[a] is not where[b]:
            merged = where[a] | where[b]
            for u in merged:
                where[u] = merged
    sets = {id(s): s for s in where.values()}.values()
    return sorted(sets, key=min)


def components(cur):
    """-> dict(component = the component number of every unitig, and per component first_unitig, unitigs, nodes, bases (None without lengths), kc_sum, circular)"""
    cls = classes(cur)
    comp = [None] * len(cur["walks"])
    for c, s in enumerate(cls):
        for u in s:
            comp[u] = c
    has_len = "length" in cur
    return dict(component=comp, n_components=len(cls), first_unitig=[min(s) for s in cls], unitigs=[len(s) for s in cls],
                nodes=[sum(len(cur["walks"][u]) for u in s) for s in cls], bases=[sum(cur["length"][u] for u in s) for s in cls] if has_len else None,
                kc_sum=[sum(cur["kc_sum"][u] for u in s) for s in cls], circular=[any(cur["circular"][u] for u in s) for s in cls])


def small_component(c, cc, max_nodes, max_bases):
    return (not cc["circular"][c]) and (max_nodes == 0 or cc["nodes"][c] <= max_nodes) and (max_bases == 0 or cc["bases"][c] <= max_bases)


def components_to_remove(cur, max_nodes, max_bases):
    cc = components(cur)
    return {u for u, c in enumerate(cc["component"]) if small_component(c, cc, max_nodes, max_bases)}


def as_steps(steps):
    """simplify_restatement.as_steps with kind 4 allowed; a component step needs a limit"""
    out = []
    for s in steps:
        if isinstance(s, dict):
            s = (s["kind"], s.get("max_nodes", 0), s.get("max_bases", 0))
        kind, mn, mb = (int(x) for x in s)
        assert kind in (TIPS, BUBBLES, COMPONENTS), kind
        assert kind != COMPONENTS or mn or mb, "a component step without a limit would remove the whole graph"
        out.append((kind, mn, mb))
    return out


def simplify(nodes, edges, steps, reads=None, length_of=None):
    """the step loop of simplify_restatement.simplify with the component kind added; same return value"""
    alive = {int(i) for i in nodes["index"]}
    log = []
    for kind, mn, mb in as_steps(steps):
        cur, recs = S.current(nodes, edges, alive, reads, length_of)
        if kind == COMPONENTS:
            gone = components_to_remove(cur, mn, mb)
        else:
            succ, pred = S.arcs_of(recs)
            gone = (S.tips_to_remove if kind == TIPS else S.bubbles_to_remove)(cur, succ, pred, mn, mb)
        removed = {n for i in gone for n, _ in cur["walks"][i]}
        log.append(dict(kind=kind, unitigs=[cur["walks"][i] for i in sorted(gone)], nodes=removed))
        alive -= removed
    final, _ = S.current(nodes, edges, alive, reads, length_of)
    return log, final
