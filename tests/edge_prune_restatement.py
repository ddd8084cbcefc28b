"""A plain, slow statement of the EDGES step of include/mdbg_hip.h (mdbg_graph_simplify, MDBG_SIMPLIFY_EDGES) and of a schedule that mixes it with tip and
bubble steps, on dictionaries, sets and tuples.  It is the CHECKER of the edge-pruning tests, written from the rule.

The state of a schedule is (alive, dead_arcs): the surviving node indices and the removed arcs, a set of ((index, o), (index, o)) pairs closed under
mirroring.  Per step the edge records are filtered by both; TIPS / BUBBLES decide with simplify_restatement's tips_to_remove / bubbles_to_remove on the
unitigs of the filtered records, EDGES with unitig_restatement.unitigs plus junctions_restatement.junctions over all reads.  Nothing here numbers vertices or
keeps a mask."""
import junctions_restatement as J
import simplify_restatement as S
import unitig_restatement as U

TIPS, BUBBLES, EDGES = 1, 2, 8


def as_steps(steps):
    out = []
    for kind, a, b in steps:
        kind, a, b = int(kind), int(a), int(b)
        assert kind in (TIPS, BUBBLES, EDGES), kind
        assert kind != EDGES or (a >= 1 and b == 0), "an EDGES step is (EDGES, min_support >= 1, 0)"
        out.append((kind, a, b))
    return out


def current(nodes, edges, alive, dead_arcs, reads, length_of):
    """the current graph: the records whose two nodes survive and whose arc is not removed, and its unitigs -> (unitigs, records as (n1, o1, n2, o2, overlap))"""
    sub, recs = S.induced(nodes, edges, alive)
    recs = [r for r in recs if ((r[0], r[1]), (r[2], r[3])) not in dead_arcs]
    cur = U.unitigs(sub, recs, reads)
    if reads is None:
        assert length_of is not None, "without reads the caller says what a walk's length is"
        cur["length"] = [length_of(w) for w in cur["walks"]]
    return cur, recs


def arc_of(rec, walks):
    """the node-level arc x -> y of a unitig edge record: x the last vertex of n1 in orientation o1, y the first vertex of n2 in orientation o2"""
    n1, o1, n2, o2 = rec[:4]
    x = walks[n1][-1] if o1 == "+" else U.comp(walks[n1][0])
    y = walks[n2][0] if o2 == "+" else U.comp(walks[n2][-1])
    return x, y


def edges_to_remove(cur, hashes, k, nodes, min_support):
    """-> (the arcs that join the removed set, the unitig edge records removed, the weak ones, the supports)"""
    walks, recs = cur["walks"], cur["edges"]
    support = J.junctions(hashes, k, nodes["keys"].tolist(), nodes["index"].tolist(), walks, [e[:4] for e in recs])["support"] if hashes else [0] * len(recs)
    arcs = [arc_of(r, walks) for r in recs]
    strong_exit = set()
    for (x, y), sup in zip(arcs, support):
        if sup >= min_support:
            strong_exit.add(x)                     # the arc leaves x,
            strong_exit.add(U.comp(y))             # its mirror leaves comp(y)
    weak = [i for i, sup in enumerate(support) if sup < min_support]
    gone = [i for i in weak if arcs[i][0] in strong_exit and U.comp(arcs[i][1]) in strong_exit]
    dead = set()
    for i in gone:
        x, y = arcs[i]
        dead.add((x, y))
        dead.add((U.comp(y), U.comp(x)))
    return dead, gone, weak, support


def simplify(nodes, edges, steps, hashes, k, reads=None, length_of=None):
    """hashes: every resident read as its list of minimizer hashes, in slot order; reads: the base strings (or None with length_of, as simplify_restatement)
    -> (per step: dict(kind, unitigs = the removed unitigs' walks, nodes = set of removed node indices, edges = node-level edge records removed,
    and for an EDGES step weak = its weak unitig edge records, support = per record of the list the step saw), unitigs(...) of what is left)"""
    alive = {int(i) for i in nodes["index"]}
    dead_arcs = set()
    log = []
    for kind, a, b in as_steps(steps):
        cur, recs = current(nodes, edges, alive, dead_arcs, reads, length_of)
        if kind == EDGES:
            dead, gone, weak, support = edges_to_remove(cur, hashes, k, nodes, a)
            assert not (dead & dead_arcs)
            n_records = sum(((r[0], r[1]), (r[2], r[3])) in dead for r in recs)
            assert n_records == len(gone)          # a unitig edge record is one node-level record; mirrors and duplicates are records of their own
            dead_arcs |= dead
            log.append(dict(kind=kind, unitigs=[], nodes=set(), edges=n_records, weak=len(weak), support=support))
            continue
        succ, pred = S.arcs_of(recs)
        gone = (S.tips_to_remove if kind == TIPS else S.bubbles_to_remove)(cur, succ, pred, a, b)
        removed = {n for i in gone for n, _ in cur["walks"][i]}
        log.append(dict(kind=kind, unitigs=[cur["walks"][i] for i in sorted(gone)], nodes=removed, edges=0))
        alive -= removed
    final, _ = current(nodes, edges, alive, dead_arcs, reads, length_of)
    return log, final
