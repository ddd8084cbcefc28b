"""A plain, slow statement of the alignment definition of include/mdbg_align.h (mdbg_graph_alignments), built from the read-path restatement and the junction
keys: one read at a time, one step at a time, the path laid out occurrence by occurrence.  It is the CHECKER of the alignment tests and shares nothing with the code
under test — no scan, no atomics, no closed formula for the wraps (they are counted window by window), and the coordinates come from where each occurrence STARTS
on the path, not from sums of lengths minus overlaps and a tail.

Inputs: the reads as (hashes, positions) in slot order, k, l, the node table's keys / index / src_start / src_end columns, and the unitig list as a LAYOUT:
dict(walks [[(index, '+' / '-')]], circular, length per unitig, ends per unitig [E(e) per entry], edges [(n1, o1, n2, o2, overlap)]).  layout_of_arrays turns the
arrays of graph_unitigs / graph_simplify into one, layout_of_model the unitig restatement's result and the model's node table.

Also here: gaf_lines, a GAF formatter written from the column list of include/mdbg_align.h alone."""
import junctions_restatement as J
import read_paths_restatement as RP

NO_RECORD = 0xFFFFFFFF


def layout_of_arrays(ul):
    walks, circular = RP.walks_of(ul)
    off = [int(x) for x in ul["offsets"]]
    end = [int(d) + int(n) for d, n in zip(ul["dst_offset"], ul["len"])]
    e = ul["edges"]
    edges = list(zip([int(x) for x in e["n1"]], [chr(int(o)) for o in e["o1"]], [int(x) for x in e["n2"]], [chr(int(o)) for o in e["o2"]], [int(x) for x in e["overlap"]]))
    return dict(walks=walks, circular=circular, length=[int(x) for x in ul["length"]], ends=[end[off[i]:off[i + 1]] for i in range(len(walks))], edges=edges)


def layout_of_model(nodes, u):
    """u: unitig_restatement.unitigs(nodes, edges[, reads]); the pieces as unitig_restatement.stitch cuts them: the first node whole, a later node its far shift_full"""
    at = {int(i): r for r, i in enumerate(nodes["index"])}
    ends, length = [], []
    for walk in u["walks"]:
        total, row = 0, []
        for j, (idx, o) in enumerate(walk):
            r = at[idx]
            ln = int(nodes["src_end"][r]) - int(nodes["src_start"][r])
            total += ln if j == 0 else min(ln, int(nodes["shift_full"][r][1 if o == "+" else 0]))
            row.append(total)
        ends.append(row)
        length.append(total)
    return dict(walks=u["walks"], circular=u["circular"], length=length, ends=ends, edges=[tuple(e) for e in u["edges"]])


def alignments(reads, k, l, nodes, lay):
    """-> dict(per read: steps [(first_window, n_windows, unitig, first_entry, strand, record)], alns [(first step, n_steps, windows, query_begin, query_end, path
    [(unitig, strand)], path_length, path_begin, path_end)]; n_windows, n_placed, n_steps, n_chained, n_alignments, n_wraps)"""
    walks, circular = lay["walks"], lay["circular"]
    keys, index = [tuple(int(v) for v in key) for key in nodes["keys"].tolist()], [int(i) for i in nodes["index"]]
    seq_len = {i: int(e) - int(s) for i, s, e in zip(index, nodes["src_start"], nodes["src_end"])}      # node index -> bases of its sequence
    H = [[int(h) for h in hs] for hs, _ in reads]
    rp = RP.read_paths(H, k, keys, index, walks, circular)
    placed = J.placements(H, k, keys, index, walks)
    first_record, overlap = {}, [e[4] for e in lay["edges"]]
    for r, e in enumerate(lay["edges"]):
        first_record.setdefault(J.record_key(e, walks), r)

    def span(u, j):                                                # [B, E) of entry j's node inside unitig u
        E = lay["ends"][u][j]
        return max(0, E - seq_len[walks[u][j][0]]), E

    out = dict(steps=[], alns=[], n_chained=0, n_wraps=0)
    for q, (hs, pos) in enumerate(reads):
        steps, alns, cur = [], [], None
        for fw, n, u, j0, s in rp["steps"][q]:
            m = len(walks[u])
            # the step window by window: where it is, and the ring closures it makes
            occ, j = [(u, s)], j0
            for w in range(fw + 1, fw + n):
                nj = (j + (1 if s == 0 else -1)) % m
                assert placed[q][w] == (u, nj, s)
                if (s == 0 and nj == 0) or (s == 1 and j == 0):    # m - 1 -> 0, or 0 -> m - 1 against the walk
                    assert circular[u]
                    occ.append((u, s))
                j = nj
            wraps = len(occ) - 1
            out["n_wraps"] += wraps
            rec = NO_RECORD
            if cur is not None and cur["next_window"] == fw:
                key = J.key_of((placed[q][fw - 1], placed[q][fw]))
                assert not J.is_link(placed[q][fw - 1], placed[q][fw])
                rec = first_record.get(key, NO_RECORD)
            if rec == NO_RECORD:
                cur = dict(first_step=len(steps), n_steps=0, windows=0, first_window=fw, occ=[], starts=[], first=(u, j0, s))
                alns.append(cur)
            else:
                out["n_chained"] += 1
            # lay the step's occurrences out on the path: each starts where the one in front ends, minus the bases the two share
            for i, (ou, os) in enumerate(occ):
                if not cur["occ"]:
                    start = 0
                else:
                    r = rec if i == 0 else first_record[J.key_of(((u, m - 1, 0), (u, 0, 0)))]
                    pu = cur["occ"][-1][0]
                    start = cur["starts"][-1] + lay["length"][pu] - (overlap[r] + l - 2)
                cur["occ"].append((ou, os))
                cur["starts"].append(start)
            cur.update(n_steps=cur["n_steps"] + 1, windows=cur["windows"] + n, next_window=fw + n, last=(u, j, s))
            steps.append((fw, n, u, j0, s, rec))
        rows = []
        for a in alns:
            w0, w1 = a["first_window"], a["next_window"] - 1
            (u0, j0, s0), (u1, j1, s1) = a["first"], a["last"]
            b0, e0 = span(u0, j0)
            b1, e1 = span(u1, j1)
            L0, L1 = lay["length"][u0], lay["length"][u1]
            begin = a["starts"][0] + (b0 if s0 == 0 else L0 - e0)
            end = a["starts"][-1] + (e1 if s1 == 0 else L1 - b1)
            rows.append((a["first_step"], a["n_steps"], a["windows"], int(pos[w0]), int(pos[w1 + k - 1]) + l, a["occ"], a["starts"][-1] + L1, begin, end))
        out["steps"].append(steps)
        out["alns"].append(rows)
    out.update(n_windows=rp["n_windows"], n_placed=rp["n_placed"], n_steps=rp["n_steps"], windows=rp["windows"], placed=rp["placed"],
               n_alignments=sum(len(a) for a in out["alns"]))
    return out


def gaf_lines(res, ordinals, read_lengths, circular):
    """one GAF line per alignment of an alignments() result, in read order: the 12 columns and the nw / ns tags of include/mdbg_align.h (mdbg_gaf_append)"""
    lines = []
    for o, qlen, rows in zip(ordinals, read_lengths, res["alns"]):
        for _, n_steps, windows, qb, qe, occ, plen, pb, pe in rows:
            path = "".join("%s%s" % ("<" if s else ">", RP.name(u, circular[u])) for u, s in occ)
            block = (qe - qb, pe - pb)
            lines.append("\t".join(str(x) for x in (o, qlen, qb, qe, "+", path, plen, pb, pe, min(block), max(block), 255, "nw:i:%d" % windows, "ns:i:%d" % n_steps)) + "\n")
    return lines
