"""The counting pre-filter (MDBG_FLAG_PREFILTER) restated from the definition in include/mdbg_hip.h alone: plain Python integers, no code of the library.

Input: the oracle's node table at min_abundance = 1 — every distinct k-min-mer of the reads with its canonical key, its number of occurrences (abundance) and the
rank of its first sighting (index) — and n_cells.  Output: which keys the table holds, and what follows from that."""
import numpy as np

M64 = (1 << 64) - 1
SALT = 0x9E3779B97F4A7C15
HMUL = 0x9E3779B97F4A7C15
SEEDS = (0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89)
DEFAULT_CELLS = 1 << 32


def fmix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    return x ^ (x >> 33)


def rol64(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def key_hash(key):
    """h of a canonical key: four multiply-xorshift chains over j mod 4, folded through fmix64"""
    h = list(SEEDS)
    for j, v in enumerate(key):
        x = ((h[j & 3] ^ int(v)) * HMUL) & M64
        h[j & 3] = x ^ (x >> 29)
    return fmix64(h[0] ^ rol64(h[1], 17) ^ rol64(h[2], 31) ^ rol64(h[3], 47))


def cell_of(key, n_cells):
    return (fmix64(key_hash(key) ^ SALT) * n_cells) >> 64


def restate(all_nodes, n_cells):
    """all_nodes: oracle node table at min_abundance = 1 (keys, abundance, index).  ->
    dict(admitted: bool per row of all_nodes, n_distinct, n_windows_admitted, new_index: {exact index -> index in the pre-filtered table},
         promoted / rejected: number of keys seen once that are / are not in the table)"""
    n_cells = n_cells or DEFAULT_CELLS
    keys, ab, idx = all_nodes["keys"], np.asarray(all_nodes["abundance"]).astype(np.int64), np.asarray(all_nodes["index"]).astype(np.int64)
    assert len(set(idx.tolist())) == len(idx) and int(ab.max(initial=0)) < 65535          # (no wrapped abundance: the counts are the occurrences)
    cells = [cell_of(k, n_cells) for k in keys]
    total = {}
    for c, a in zip(cells, ab.tolist()):
        total[c] = total.get(c, 0) + a
    admitted = np.array([min(2, total[c]) == 2 for c in cells], dtype=bool)
    order = sorted(int(i) for i in idx[admitted])
    return dict(admitted=admitted, n_distinct=int(admitted.sum()), n_windows_admitted=int(ab[admitted].sum()),
                new_index={e: r for r, e in enumerate(order)},
                promoted=int((admitted & (ab == 1)).sum()), rejected=int((~admitted & (ab == 1)).sum()))


def expected_nodes(exact_nodes, all_nodes, n_cells):
    """the node table of a pre-filtered context at min_abundance A >= 2 from the exact one at the same A: the same rows, `index` renumbered, n_distinct replaced"""
    r = restate(all_nodes, n_cells)
    out = dict(exact_nodes)
    out["index"] = np.array([r["new_index"][int(i)] for i in exact_nodes["index"]], dtype=np.uint32)
    out["n_nodes_before"] = r["n_distinct"]
    return out, r
