"""A plain, slow statement of the read-path definition of include/mdbg_hip.h (mdbg_graph_read_paths), working on dictionaries and lists: one read at a
time, one window at a time, the current step extended or closed.  It is the CHECKER of the read-path tests and shares nothing with the code under test —
no hash table, no bitmaps, no codes, no head flags, no scan.  Written from the rule.

Inputs: the reads as lists of minimizer hashes (slot order), k, the node table as its `keys` (one k-tuple per row) and `index` columns, and the unitig list
as walks [[(index, '+' / '-')]] with their circular flags (walks_of turns the arrays of graph_unitigs into that)."""


def canonical(w):
    """KmerVec::normalize (src/kmer_vec.rs:34-39) -> (key, rev); a window equal to its reverse counts as reversed"""
    r = w[::-1]
    rev = not (w < r)
    return (r if rev else w), rev


def walks_of(u):
    """the arrays of Mdbg.graph_unitigs / graph_simplify -> (walks, circular)"""
    off = [int(x) for x in u["offsets"]]
    node, ori = [int(x) for x in u["node"]], [chr(int(x)) for x in u["ori"]]
    n = int(u["n_unitigs"]) if "n_unitigs" in u else len(off) - 1
    return [list(zip(node[off[i]:off[i + 1]], ori[off[i]:off[i + 1]])) for i in range(n)], [bool(c) for c in list(u["circular"])[:n]]


def read_paths(reads, k, keys, index, walks, circular):
    """-> dict(steps: per read [(first_window, n_windows, unitig, first_entry, strand)], windows: per read W, placed: per read,
    support_windows, support_steps: per unitig, n_windows, n_placed, n_steps)"""
    where = {}
    for u, walk in enumerate(walks):
        for j, (idx, o) in enumerate(walk):
            assert int(idx) not in where, "an index occurs in two entries: the unitigs do not partition the nodes"
            where[int(idx)] = (u, j, o)
    row = {tuple(int(v) for v in key): int(i) for key, i in zip(keys, index)}
    assert len(row) == len(list(index))
    sup_w, sup_s = [0] * len(walks), [0] * len(walks)
    out = dict(steps=[], windows=[], placed=[])
    for H in reads:
        H = [int(h) for h in H]
        W = len(H) - k + 1 if len(H) > k else 0          # src/main.rs:756-759: strictly more than k minimizers
        steps, cur, placed = [], None, 0
        for w in range(W):
            key, rev = canonical(tuple(H[w:w + k]))
            at = where.get(row.get(key, -1))
            if at is None:                                # not a row, or a row that is in no entry: ends a run
                cur = None
                continue
            u, j, o = at
            s = int(rev != (o == "-"))
            placed += 1
            sup_w[u] += 1
            if cur is not None and (cur["u"], cur["s"]) == (u, s):
                nxt = cur["j"] + (1 if s == 0 else -1)
                if circular[u]:
                    nxt %= len(walks[u])
                if nxt == j:                              # (a linear unitig: -1 and len are no entries, it never continues onto itself)
                    cur["n"] += 1
                    cur["j"] = j
                    continue
            cur = dict(w=w, n=1, u=u, j0=j, s=s, j=j)
            steps.append(cur)
            sup_s[u] += 1
        out["steps"].append([(c["w"], c["n"], c["u"], c["j0"], c["s"]) for c in steps])
        out["windows"].append(W)
        out["placed"].append(placed)
    out.update(support_windows=sup_w, support_steps=sup_s, n_windows=sum(out["windows"]), n_placed=sum(out["placed"]), n_steps=sum(len(s) for s in out["steps"]))
    return out


def name(i, circular):
    return "utg%07d%s" % (i + 1, "c" if circular else "l")


def tsv_text(paths, ordinals, circular):
    """one line per read in slot order: ordinal, windows, placed, path; path = `*` or the steps joined by `,`, each first_window:n_windows:>NAME:first_entry
    (`<` for strand 1)"""
    lines = []
    for o, W, placed, steps in zip(ordinals, paths["windows"], paths["placed"], paths["steps"]):
        path = ",".join("%d:%d:%s%s:%d" % (w, n, "<" if s else ">", name(u, circular[u]), j) for w, n, u, j, s in steps) or "*"
        lines.append("%d\t%d\t%d\t%s\n" % (o, W, placed, path))
    return "".join(lines)
