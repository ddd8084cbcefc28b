"""A plain, slow statement of the unitig definition of include/mdbg_hip.h (mdbg_graph_unitigs) and of the stitching rule of
src/to_basespace.rs, working on dictionaries, sets and strings: node sequence cut from the read, reverse complement, slice,
concatenate.  It is the CHECKER of the unitig tests and deliberately shares nothing with the code under test — no vertex
numbering, no sort, no pointer jumping, no copy plan.  Written from the rule, not transcribed from the Rust."""

COMPLEMENT = {"a": "t", "c": "g", "t": "a", "g": "c", "u": "a", "A": "T", "C": "G", "T": "A", "G": "C", "U": "A"}


def revcomp(s):
    """src/utils.rs:3-24: anything outside ACGTU / acgtu becomes N"""
    return "".join(COMPLEMENT.get(c, "N") for c in reversed(s))


def flip(o):
    return "-" if o == "+" else "+"


def comp(v):
    return (v[0], flip(v[1]))


def as_records(edges):
    """dict of arrays (n1, o1, n2, o2, overlap; o as ASCII codes) or a list of tuples -> [((n1, o1), (n2, o2), overlap)] with '+' / '-' characters"""
    if isinstance(edges, dict):
        edges = zip(*(list(edges[f]) for f in ("n1", "o1", "n2", "o2", "overlap")))
    ch = lambda o: o if isinstance(o, str) else chr(int(o))
    return [((int(a), ch(oa)), (int(b), ch(ob)), int(ov)) for a, oa, b, ob, ov in edges]


def compact(node_indices, edges):
    """-> (walks, circular flags, unitig edges [(unitig, o, unitig, o, overlap)] with the overlap NOT yet fixed); unitigs ordered by the index of their first node"""
    recs = as_records(edges)
    succ, pred = {}, {}
    for u, v, _ in recs:
        for a, b in ((u, v), (comp(v), comp(u))):
            succ.setdefault(a, set()).add(b)
            pred.setdefault(b, set()).add(a)
    nxt = {}
    for u, outs in succ.items():
        if len(outs) == 1:
            (v,) = outs
            if len(pred[v]) == 1 and v[0] != u[0]:
                nxt[u] = v
    prv = {v: u for u, v in nxt.items()}
    seen, found = set(), []
    for idx in sorted(int(i) for i in node_indices):
        for v in ((idx, "+"), (idx, "-")):
            if v in seen:
                continue
            cur, circular = v, False
            while cur in prv:                       # back to the start of the chain, or once round the cycle
                cur = prv[cur]
                if cur == v:
                    circular = True
                    break
            chain = [cur]
            while chain[-1] in nxt and nxt[chain[-1]] != cur:
                chain.append(nxt[chain[-1]])
            mirror = [comp(x) for x in reversed(chain)]
            assert not (set(chain) & set(mirror)), "a chain holds a vertex and its complement"
            seen.update(chain)
            seen.update(mirror)
            if circular:
                low = min(x[0] for x in chain)
                keep = chain if (low, "+") in chain else mirror
                at = keep.index((low, "+"))
                keep = keep[at:] + keep[:at]
            elif len(chain) == 1:
                keep = chain if chain[0][1] == "+" else mirror
            else:
                keep = chain if chain[0][0] < chain[-1][0] else mirror
            found.append((keep, circular))
    found.sort(key=lambda t: t[0][0][0])
    walks = [w for w, _ in found]
    circ = [c for _, c in found]
    interior, leaves, enters = set(), {}, {}
    for i, w in enumerate(walks):
        for a, b in zip(w, w[1:]):
            interior.add((a, b))
            interior.add((comp(b), comp(a)))
        leaves[w[-1]] = (i, "+")
        leaves[comp(w[0])] = (i, "-")
        enters[w[0]] = (i, "+")
        enters[comp(w[-1])] = (i, "-")
    uedges = []
    for u, v, ov in recs:
        if (u, v) in interior:
            continue
        (a, oa), (b, ob) = leaves[u], enters[v]
        uedges.append((a, oa, b, ob, ov))
    return walks, circ, uedges


def node_sequences(nodes, reads):
    """index -> (the node's .sequences sequence: the read's slice, reverse-complemented when `reversed` (main.rs:700-701); shift_full pair)"""
    out = {}
    for i in range(len(nodes["index"])):
        r = reads[int(nodes["src_read"][i])]
        s = bytes(r[int(nodes["src_start"][i]):int(nodes["src_end"][i])]).decode("latin-1")
        if int(nodes["reversed"][i]):
            s = revcomp(s)
        out[int(nodes["index"][i])] = (s, int(nodes["shift_full"][i][0]), int(nodes["shift_full"][i][1]))
    return out


def stitch(walk, seqs):
    """to_basespace.rs:132-153, 203-262: the first node whole ('-': reverse-complemented), every later node its last s1 bases ('+') or the reverse
    complement of its first s0 bases ('-')"""
    parts = []
    for j, (idx, o) in enumerate(walk):
        s, s0, s1 = seqs[idx]
        if j == 0:
            parts.append(s if o == "+" else revcomp(s))
        elif o == "+":
            parts.append(s[len(s) - s1:] if s1 <= len(s) else s)
        else:
            parts.append(revcomp(s[:s0]))
    return "".join(parts)


def name(i, circular):
    return "utg%07d%s" % (i + 1, "c" if circular else "l")


def unitigs(nodes, edges, reads=None):
    """-> dict(walks, circular, names, kc_sum, edges, and with reads: seqs, length, and the edges' overlaps fixed by to_basespace.rs:312-320)"""
    walks, circ, ue = compact(nodes["index"], edges)
    ab = {int(i): int(a) for i, a in zip(nodes["index"], nodes["abundance"])}
    out = dict(walks=walks, circular=circ, names=[name(i, c) for i, c in enumerate(circ)], kc_sum=[sum(ab[i] for i, _ in w) for w in walks], edges=ue)
    if reads is not None:
        ns = node_sequences(nodes, reads)
        out["seqs"] = [stitch(w, ns) for w in walks]
        out["length"] = [len(s) for s in out["seqs"]]
        fixed = []
        for a, oa, b, ob, ov in ue:
            la, lb = out["length"][a], out["length"][b]
            if ov > la or ov > lb:
                ov = min(la - 1, lb - 1)
            fixed.append((a, oa, b, ob, ov))
        out["edges"] = fixed
    return out


def gfa_text(u):
    lines = ["H\tVN:Z:1.0"]
    for i, s in enumerate(u["seqs"]):
        lines.append("S\t%s\t%s\tLN:i:%d\tmc:f:%.1f" % (u["names"][i], s, len(s), u["kc_sum"][i] / len(u["walks"][i])))
    for a, oa, b, ob, ov in u["edges"]:
        lines.append("L\t%s\t%s\t%s\t%s\t%dM" % (u["names"][a], oa, u["names"][b], ob, ov))
    return "\n".join(lines) + "\n"


def fasta_text(u, min_len=0):
    return "".join(">%s\n%s\n" % (n, s) for n, s in zip(u["names"], u["seqs"]) if len(s) >= min_len)
