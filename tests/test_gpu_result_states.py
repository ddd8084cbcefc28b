"""Which derived results (node table -> edge list -> unitig list, and what hangs on them) a context holds after each call that makes or ends one: one scripted
walk over ONE context, every reader probed after every event, "works / MDBG_E_STATE" compared with the table written out below (include/mdbg_hip.h; where the
header is silent, what the library did before the results got one owner).  Then every list's host and device variant column for column, and the refusals of a
context that keeps no reads.  Input: the example reads at (k, l, d, A) = (7, 10, 0.0008, 2), 206 edges (tests/golden/example_cfg1.json)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import _mdbg

pytestmark = pytest.mark.gpu

K, L, D, A = 7, 10, 0.0008, 2
OK, ST = "ok", "state"

# The probes of one step, in this order.  The first four change nothing.  `unitigs0` asks for the list BEFORE the edge probe has made an edge list (it ends the unitig
# list whether it works or not), `edges` ends the unitig list, `unitigs` and `simplify` (an empty schedule) make it again, and the last three ask once more with the list
# the probes themselves made.  So every step starts from the state the probes of the step before left: edge list and unitig list current wherever they can be.
PROBES = ("components", "contigs", "read_paths", "node_seqs", "unitigs0", "edges", "unitigs", "simplify", "components+", "contigs+", "read_paths+")
ALL_ST = (ST,) * 11
ALL_OK = (OK,) * 11
EMPTY = (ST, ST, ST, ST, OK, OK, OK, OK, OK, OK, OK)       # nothing resident and no finalize since: empty lists, but no node table to take sequences from
TABLE = (ST, ST, ST, OK, ST, OK, OK, OK, OK, OK, OK)       # a finalize has just run: a node table, nothing on it yet
NO_LIST = (ST, ST, ST, OK, OK, OK, OK, OK, OK, OK, OK)     # node table and edge list current, the unitig list ended
# a batch sketched but not inserted ends the unitig list only: the table and its edge list are what they were.  The store then holds reads the table has not seen, so
# the list the probes rebuild is not threaded, stitched or grouped here (None: not probed)
SKETCHED = (ST, ST, ST, OK, OK, OK, OK, OK, None, None, None)

# (event, the reads the results describe afterwards, expected outcome of every probe)
WALK = (
    ("fresh", "empty", EMPTY),
    ("finalize", "empty", ALL_OK),                          # the finalize of an empty context: a table of no rows, and it ends nothing
    ("ingest", "full", ALL_ST),
    ("finalize", "full", TABLE),
    ("edges", "full", NO_LIST),
    ("unitigs", "full", ALL_OK),
    ("simplify", "full", ALL_OK),
    ("finalize_gfa", "full", TABLE),
    ("mark", "full", ALL_OK),
    ("sketch_device", "full", SKETCHED),
    ("insert_resident", "more", ALL_ST),
    ("finalize", "more", TABLE),
    ("reset_k", "more", ALL_ST),
    ("finalize", "more", TABLE),
    ("rewind", "full", ALL_ST),
    ("reset_k", "full", ALL_ST),
    ("finalize", "full", TABLE),
    ("reset_0", "empty", EMPTY),
    ("finalize", "empty", ALL_OK),
    ("ingest", "full", ALL_ST),
    ("reset_0", "empty", EMPTY),
)
SCHEDULE = [(1, 10, 50000), (2, 0, 100000)]                 # one tip step, one bubble step (MDBG_SIMPLIFY_TIPS / _BUBBLES)


def _addr(p):
    return p if isinstance(p, int) else C.cast(p, C.c_void_p).value or 0


def _counts(kind, r):
    if kind == "edges":
        return (len(r["n1"]), r["presimp_removed"])
    if kind == "unitigs":
        return (r["n_unitigs"], r["n_entries"], len(r["edges"]["n1"]))
    if kind == "components":
        return (r["n_unitigs"], r["n_components"])
    if kind == "contigs":
        return (r["n_contigs"], r["n_bases"])
    if kind == "node_seqs":
        return (r["n_rows"], r["n_bases"])
    return (r["n_reads"], r["n_windows"], r["n_placed"], r["n_steps"], r["n_unitigs"])


def test_every_reader_after_every_event(example_reads):
    import torch
    R = _mdbg()
    more = example_reads[:10]
    mb = np.frombuffer(b"".join(more), dtype=np.uint8).copy()
    mo = np.zeros(len(more) + 1, dtype=np.uint64)
    mo[1:] = np.cumsum([len(r) for r in more])
    tb, to = torch.from_numpy(mb).cuda(), torch.from_numpy(mo.view(np.int64)).cuda()
    torch.cuda.synchronize()                                 # (torch's stream; the sketch runs on the context's)
    first_seen = {}                                          # (reader, reads, list) -> counts, the first time the reader worked there
    with R.Mdbg(K, L, D, A, keep_reads=True) as m:
        mark = [None]
        events = dict(
            fresh=lambda: None,
            ingest=lambda: m.ingest_reads(example_reads, 0),
            finalize=lambda: m.finalize(),
            finalize_gfa=lambda: m.finalize(gfa_only=True),
            edges=lambda: m.graph_edges(0.01),
            unitigs=lambda: m.graph_unitigs(),
            simplify=lambda: m.graph_simplify(SCHEDULE),
            mark=lambda: mark.__setitem__(0, m.mark()),
            sketch_device=lambda: m.sketch_device(tb.data_ptr(), to.data_ptr(), len(more), len(mb), len(example_reads)),
            insert_resident=lambda: m.insert_resident(),
            reset_k=lambda: m.reset(K),
            reset_0=lambda: m.reset(0),
            rewind=lambda: m.rewind(mark[0]),
        )
        readers = {
            "components": ("components", m.graph_components), "contigs": ("contigs", m.graph_contigs), "read_paths": ("read_paths", m.graph_read_paths),
            "node_seqs": ("node_seqs", m.graph_node_seqs), "unitigs0": ("unitigs", m.graph_unitigs), "edges": ("edges", lambda: m.graph_edges(0.01)),
            "unitigs": ("unitigs", m.graph_unitigs), "simplify": ("unitigs", lambda: m.graph_simplify([])),
        }
        for step, (event, reads, expect) in enumerate(WALK):
            events[event]()
            lst = "simplified" if event == "simplify" else "plain"      # which list the readers of the list see: the probes only ever make the plain one
            for probe, want in zip(PROBES, expect):
                if want is None:
                    continue
                where = "step %d (%s), probe %s" % (step, event, probe)
                kind, call = readers[probe.rstrip("+")]
                try:
                    got, cnt = OK, _counts(kind, call())
                except R.MdbgError as e:
                    assert e.code == R.api.MDBG_E_STATE, where
                    got, cnt = ST, None
                print(where, got, cnt)
                assert got == want, where
                if probe in ("unitigs0", "unitigs", "simplify"):
                    lst = "plain"
                if got == OK:
                    if reads == "empty":
                        assert not any(cnt), where
                    key = (kind, reads, lst if kind in ("components", "contigs", "read_paths") else None)
                    assert first_seen.setdefault(key, cnt) == cnt, where
    assert first_seen[("edges", "full", None)][0] == 206
    assert first_seen[("read_paths", "full", "plain")][0] == len(example_reads) and first_seen[("read_paths", "more", "plain")][0] == len(example_reads) + len(more)
    assert all(first_seen[(kind, "full", lst)][0] > 0 for kind, lst in (("unitigs", None), ("components", "plain"), ("components", "simplified"), ("contigs", "plain"),
                                                                         ("node_seqs", None)))


def test_host_and_device_variants_name_the_same_columns(example_reads):
    R = _mdbg()
    api = R.api
    with R.Mdbg(K, L, D, A, keep_reads=True) as m:
        def same(what, host, dev, n, dtype):
            got = m.to_host(_addr(dev), n * np.dtype(dtype).itemsize, dtype) if n else np.zeros(0, dtype)
            assert np.asarray(host).size == n and np.array_equal(np.asarray(host).reshape(-1), got), what

        def same_unitigs(what, h, d):
            assert (h["n_unitigs"], h["n_entries"], h["n_rounds"]) == (int(d.n_unitigs), int(d.n_entries), int(d.n_rounds)) and h["n_unitigs"] > 0, what
            cnt = api.unitig_counts(d)
            for f, t in api.UNITIG_FIELDS:
                same(what + "." + f, h[f], getattr(d, f), cnt[f], t)
            for f, t in api.EDGE_FIELDS:
                same(what + ".edges." + f, h["edges"][f], getattr(d.edges, f), int(d.edges.n), t)

        m.ingest_reads(example_reads, 0)
        h = m.finalize()
        d = m.finalize_device()
        n = int(d.n)
        assert n == h["n_nodes"] > 0 and (int(d.k), int(d.n_distinct), int(d.n_wrapped)) == (K, h["n_nodes_before"], h["n_wrapped"])
        cols = (("keys", "keys", K, np.uint64), ("index", "index", 1, np.uint32), ("abundance", "abundance", 1, np.uint16), ("seqlen", "seqlen", 1, np.uint32),
                ("shift", "shift", 2, np.uint16), ("shift_full", "shift_full", 2, np.uint64), ("src_read", "src_read", 1, np.uint64),
                ("src_start", "src_start", 1, np.uint64), ("src_end", "src_end", 1, np.uint64), ("reversed", "reversed", 1, np.uint8))
        for f, field, per, t in cols:
            same("nodes." + f, h[f], getattr(d, field), n * per, t)
        g = m.finalize(gfa_only=True)                        # its three host columns; the rest stay on the device and are not handed out
        assert g["n_nodes"] == n and all(g[f] is None for f in ("keys", "shift", "shift_full", "src_read", "src_start", "src_end", "reversed"))
        for f in ("index", "seqlen", "abundance"):
            assert np.array_equal(g[f], h[f]), f
        h, d = m.graph_edges(0.01), m.graph_edges_device(0.01)
        assert len(h["n1"]) == int(d.n) == 206 and h["presimp_removed"] == int(d.presimp_removed)
        for f, t in api.EDGE_FIELDS:
            same("edges." + f, h[f], getattr(d, f), int(d.n), t)
        h, (d, st) = m.graph_simplify(SCHEDULE), m.graph_simplify_device(SCHEDULE)
        assert h["stats"] == st
        same_unitigs("simplify", h, d)
        same_unitigs("unitigs", m.graph_unitigs(), m.graph_unitigs_device())
        h, d = m.graph_components(), m.graph_components_device()
        assert (h["n_unitigs"], h["n_components"]) == (int(d.n_unitigs), int(d.n_components)) and h["n_components"] > 0
        for f, t, per_unitig in api.COMPONENT_FIELDS:
            same("components." + f, h[f], getattr(d, f), h["n_unitigs"] if per_unitig else h["n_components"], t)
        h, d = m.graph_contigs(), m.graph_contigs(device=True)
        assert (h["n_contigs"], h["n_bases"]) == (int(d.n_contigs), int(d.n_bases)) and h["n_bases"] > 0
        for f, cnt, t in (("bases", h["n_bases"], np.uint8), ("offsets", h["n_contigs"] + 1, np.uint64), ("unitig", h["n_contigs"], np.uint64)):
            same("contigs." + f, h[f], getattr(d, f), cnt, t)
        h, d = m.graph_node_seqs(3, 40), m.graph_node_seqs(3, 40, device=True)
        assert (h["first_row"], h["n_rows"], h["n_bases"]) == (d["first_row"], d["n_rows"], d["n_bases"]) == (3, 40, h["n_bases"]) and h["n_bases"] > 0
        same("node_seqs.bases", h["bases"], d["bases"], h["n_bases"], np.uint8)
        same("node_seqs.offsets", h["offsets"], d["offsets"], 41, np.uint64)
        h, d = m.graph_read_paths(5, 300), m.graph_read_paths_device(5, 300)
        heads = ("first_read", "n_reads", "n_windows", "n_placed", "n_steps", "n_unitigs")
        assert tuple(h[f] for f in heads) == tuple(int(getattr(d, f)) for f in heads) and h["n_reads"] == 300 and h["n_steps"] > 0
        per = dict(read=h["n_reads"], step=h["n_steps"], unitig=h["n_unitigs"])
        for f, t, what in api.READ_PATH_FIELDS:
            same("read_paths." + f, h[f], getattr(d, f), per[what], t)
        same("read_paths.step_offsets", h["step_offsets"], d.step_offsets, h["n_reads"] + 1, np.uint64)


def test_a_context_without_kept_reads_refuses_the_two_gathers(example_reads):
    R = _mdbg()
    with R.Mdbg(K, L, D, A) as m:
        m.ingest_reads(example_reads, 0)
        m.finalize()
        m.graph_edges(0.01)
        assert m.graph_unitigs()["n_unitigs"] > 0            # everything else the two calls ask for is there
        for call in (m.graph_contigs, lambda: m.graph_contigs(device=True), m.graph_node_seqs, lambda: m.graph_node_seqs(device=True)):
            with pytest.raises(R.MdbgError) as ei:
                call()
            assert ei.value.code == R.api.MDBG_E_STATE and "does not keep its reads" in str(ei.value)
        assert m.graph_components()["n_components"] > 0 and m.graph_read_paths()["n_reads"] == len(example_reads)      # and the refusals ended nothing
