"""A plain, slow statement of the chain definition of include/mdbg_chain.h (mdbg_graph_chains) on top of alignments_restatement.alignments: one read at a time,
one pair of consecutive alignments at a time.  It is the CHECKER of the chain tests and shares nothing with the code under test — both candidates are built by
WALKING the unitigs' entry lists one entry at a time (no closed formula for tail, head or the distance inside a unitig), the record is looked up in a dictionary of
the edge tuples' keys, and a chain's path is laid out occurrence by occurrence, each starting where the one in front ends minus the bases the two share: no sum of
path lengths minus overlaps.

Inputs: those of alignments_restatement.alignments, and max_skew, max_gap.  Also here: gaf_lines for chains, from the column list of include/mdbg_chain.h alone."""
import alignments_restatement as AL
import junctions_restatement as J
import read_paths_restatement as RP

NOT_BRIDGED, INSIDE = 0xFFFFFFFF, 0xFFFFFFFE


def walk_on(x, m):
    """the vertex one entry further in walk direction inside a unitig of m entries, or None at its end (no wrap)"""
    u, j, s = x
    nj = j + 1 if s == 0 else j - 1
    return (u, nj, s) if 0 <= nj < m else None


def candidates(x, y, walks, first_record):
    """-> (entries of INSIDE or None, (entries, record) of RECORD or None) for the placements x of the last window in front of a gap and y of the first behind it"""
    mx, my = len(walks[x[0]]), len(walks[y[0]])
    inside, at, n = None, x, 0
    while at is not None:                                          # walk on from x: is y further on in the same unitig, on the same strand?
        at, n = walk_on(at, mx), n + 1
        if at == y:
            inside = n
            break
    tail, at = 0, walk_on(x, mx)                                   # the entries behind x, to the end of its unitig
    while at is not None:
        tail, at = tail + 1, walk_on(at, mx)
    end_x = (x[0], 0 if x[2] else mx - 1, x[2])                    # the last vertex of u_x in direction s_x
    start_y = (y[0], my - 1 if y[2] else 0, y[2])                  # the first vertex of u_y in direction s_y
    head, at = 0, start_y
    while at != y:
        head, at = head + 1, walk_on(at, my)
    rec = first_record.get(J.key_of((end_x, start_y)))
    return inside, None if rec is None else (tail + head + 1, rec)


def occurrences(steps, walks, closing):
    """the occurrences of an alignment's steps, window by window -> [(unitig, strand, the record that joins it to the one in front; None for the first)]"""
    out = []
    for fw, n, u, j0, s, rec in steps:
        m, j = len(walks[u]), j0
        out.append((u, s, rec if out else None))
        for _ in range(n - 1):
            nj = (j + (1 if s == 0 else -1)) % m
            if (s == 0 and nj == 0) or (s == 1 and j == 0):
                out.append((u, s, closing[u]))
            j = nj
    return out


def chains(reads, k, l, nodes, lay, max_skew, max_gap):
    """-> dict(a: the alignments() result; bridges: per read, per alignment (bridge_record, bridge_entries); chains: per read [(first alignment, n alignments,
    windows, gap windows, query_begin, query_end, path [(unitig, strand)], path_length, path_begin, path_end, steps)]; n_bridges, n_bridges_inside,
    n_bridges_record, n_chains, n_gap_windows)"""
    walks = lay["walks"]
    a = AL.alignments(reads, k, l, nodes, lay)
    keys, index = [tuple(int(v) for v in key) for key in nodes["keys"].tolist()], [int(i) for i in nodes["index"]]
    placed = J.placements([[int(h) for h in hs] for hs, _ in reads], k, keys, index, walks)
    first_record, overlap = {}, [e[4] for e in lay["edges"]]
    for r, e in enumerate(lay["edges"]):
        first_record.setdefault(J.record_key(e, walks), r)
    closing = {u: first_record.get(J.key_of(((u, len(w) - 1, 0), (u, 0, 0)))) for u, w in enumerate(walks)}
    out = dict(a=a, bridges=[], chains=[], n_bridges_inside=0, n_bridges_record=0, n_gap_windows=0)
    for q, rows in enumerate(a["alns"]):
        steps, bridges, made, cur = a["steps"][q], [], [], None
        for i, (first, n, windows, qb, qe, occ, plen, pb, pe) in enumerate(rows):
            w0 = steps[first][0]
            w1 = steps[first + n - 1][0] + steps[first + n - 1][1] - 1
            kind, entries, gap = NOT_BRIDGED, 0, 0
            if i:
                x, y, dw = placed[q][cur["last_window"]], placed[q][w0], w0 - cur["last_window"]
                inside, record = candidates(x, y, walks, first_record)
                best = None
                if inside is not None:
                    best = (INSIDE, inside)
                if record is not None and (best is None or abs(record[0] - dw) < abs(best[1] - dw)):      # a tie goes to INSIDE
                    best = (record[1], record[0])
                if best is not None and dw >= 2 and abs(best[1] - dw) <= max_skew and (max_gap == 0 or dw - 1 <= max_gap):
                    kind, entries, gap = best[0], best[1], dw - 1
            bridges.append((kind, entries))
            mine = occurrences(steps[first:first + n], walks, closing)
            assert [(u, s) for u, s, _ in mine] == occ
            if kind == NOT_BRIDGED:
                cur = dict(first=i, n=0, windows=0, gap=0, qb=qb, occ=[], starts=[], begin=pb, steps=0)
                made.append(cur)
            else:
                out["n_bridges_inside" if kind == INSIDE else "n_bridges_record"] += 1
            # lay the alignment's occurrences out behind what the chain has: each starts where the one in front ends, minus the bases the two share
            for t, (u, s, rec) in enumerate(mine):
                if not cur["occ"]:
                    start = 0
                elif t == 0 and kind == INSIDE:
                    assert cur["occ"][-1] == (u, s)
                    continue                                       # merged: the last occurrence in front IS this one
                else:
                    r = kind if t == 0 else rec
                    start = cur["starts"][-1] + lay["length"][cur["occ"][-1][0]] - (overlap[r] + l - 2)
                cur["occ"].append((u, s))
                cur["starts"].append(start)
            # where the alignment's last window ends inside its last occurrence: its path_end minus where that occurrence starts on the alignment's own path
            within = pe - (plen - lay["length"][occ[-1][0]])
            cur.update(n=cur["n"] + 1, windows=cur["windows"] + windows, gap=cur["gap"] + gap, qe=qe, last_window=w1, end=cur["starts"][-1] + within, steps=cur["steps"] + n)
            out["n_gap_windows"] += gap
        out["bridges"].append(bridges)
        out["chains"].append([(c["first"], c["n"], c["windows"], c["gap"], c["qb"], c["qe"], c["occ"], c["starts"][-1] + lay["length"][c["occ"][-1][0]], c["begin"], c["end"], c["steps"])
                              for c in made])
    out.update(n_bridges=out["n_bridges_inside"] + out["n_bridges_record"], n_chains=sum(len(c) for c in out["chains"]))
    return out


def gaf_lines(res, ordinals, read_lengths, circular):
    """one GAF line per chain of a chains() result, in read order: the 12 columns and the nw / ns / ng / gw tags of include/mdbg_chain.h (mdbg_gaf_append_chains)"""
    lines = []
    for o, qlen, rows in zip(ordinals, read_lengths, res["chains"]):
        for _, n, windows, gap, qb, qe, occ, plen, pb, pe, n_steps in rows:
            path = "".join("%s%s" % ("<" if s else ">", RP.name(u, circular[u])) for u, s in occ)
            block = (qe - qb, pe - pb)
            lines.append("\t".join(str(x) for x in (o, qlen, qb, qe, "+", path, plen, pb, pe, min(block), max(block), 255, "nw:i:%d" % windows, "ns:i:%d" % n_steps,
                                                    "ng:i:%d" % (n - 1), "gw:i:%d" % gap)) + "\n")
    return lines
