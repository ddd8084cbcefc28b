"""The restatement of the counting pre-filter (tests/prefilter_restatement.py) on its own, and the conditions the inputs of tests/test_gpu_prefilter.py must meet:
no GPU.  The reads are the GPU tests' reads, the table of all keys is the oracle's at min_abundance = 1."""
import numpy as np
import pytest

import prefilter_restatement as PR
from oracle import oracle as O

K, L, D = 5, 8, 0.008
MEDIUM_CELLS = (1024, 16384)          # sizes at which some singletons share a cell and some do not
HUGE_CELLS = 1 << 36                  # the largest filter the header allows


def synth_set(n_reads):
    from rust_mdbg_amd import synth
    return synth.synth_reads(7, 20000, n_reads, mean_len=3000, sd_len=300, min_len=1500, max_len=4500, err_ppm=10000)


def all_keys(reads, first=0):
    g = O.Graph(K, L, D, 1)
    b, o = O.concat_reads(reads)
    assert g.ingest(b, o, first) == 0
    return g.finalize(with_edges=False)


@pytest.fixture(scope="module")
def small():
    return all_keys(synth_set(60))


@pytest.fixture(scope="module")
def large():
    return all_keys(synth_set(240))


def test_the_small_set_is_the_one_the_cases_were_sized_for(small):
    ab = np.asarray(small["abundance"])
    assert (small["n_windows"], small["n_nodes"], int((ab == 1).sum()), int((ab >= 2).sum())) == (1679, 871, 649, 222)
    # one workgroup's span of window starts, and several for the large set: 2048 starts per workgroup
    assert small["n_minimizers"] <= 2048


def test_the_large_set_covers_several_spans(large):
    assert large["n_minimizers"] > 3 * 2048


def test_key_hash_is_the_headers_on_hand_computed_cases():
    """k = 1 and k = 5 by hand from the header's formula: chain 0 takes elements 0 and 4, the chains without an element keep their seed"""
    M = PR.M64
    mix = lambda h, v: (lambda x: x ^ (x >> 29))(((h ^ v) * PR.HMUL) & M)
    fold = lambda h: PR.fmix64(h[0] ^ PR.rol64(h[1], 17) ^ PR.rol64(h[2], 31) ^ PR.rol64(h[3], 47))
    s = PR.SEEDS
    assert PR.key_hash([7]) == fold([mix(s[0], 7), s[1], s[2], s[3]])
    assert PR.key_hash([1, 2, 3, 4, 5]) == fold([mix(mix(s[0], 1), 5), mix(s[1], 2), mix(s[2], 3), mix(s[3], 4)])
    assert PR.fmix64(0) == 0 and PR.fmix64(1) == 0xb456bcfc34c2cb2c          # MurmurHash3's finaliser
    assert PR.cell_of([1, 2, 3, 4, 5], 1) == 0 and 0 <= PR.cell_of([1, 2, 3, 4, 5], 1000) < 1000


@pytest.mark.parametrize("which", ["small", "large"])
def test_one_cell_admits_everything(which, request):
    a = request.getfixturevalue(which)
    r = PR.restate(a, 1)
    assert r["admitted"].all() and r["n_distinct"] == a["n_nodes"] and r["n_windows_admitted"] == a["n_windows"] and r["rejected"] == 0
    assert r["new_index"] == {int(i): int(i) for i in a["index"]}


def test_a_filter_without_shared_cells_admits_exactly_the_keys_seen_twice(small):
    cells = [PR.cell_of(k, HUGE_CELLS) for k in small["keys"]]
    assert len(set(cells)) == len(cells)                                    # the premise: no two keys share a cell
    r = PR.restate(small, HUGE_CELLS)
    ab = np.asarray(small["abundance"])
    assert np.array_equal(r["admitted"], ab >= 2) and r["promoted"] == 0 and r["rejected"] == 649
    assert r["n_distinct"] == 222 and r["n_windows_admitted"] == int(ab[ab >= 2].sum())
    # the index is the rank among the admitted keys, in the order of the first sightings
    solid = sorted(int(i) for i in np.asarray(small["index"])[ab >= 2])
    assert [r["new_index"][i] for i in solid] == list(range(222))


@pytest.mark.parametrize("which", ["small", "large"])
@pytest.mark.parametrize("n_cells", MEDIUM_CELLS)
def test_medium_sizes_promote_some_singletons_and_reject_others(which, n_cells, request):
    """the condition on the GPU tests' inputs (not a tolerance): at each medium size at least one promoted and one rejected singleton, and fewer keys than the exact table"""
    a = request.getfixturevalue(which)
    r = PR.restate(a, n_cells)
    assert r["promoted"] >= 1 and r["rejected"] >= 1 and r["n_distinct"] < a["n_nodes"]
    assert r["n_distinct"] == int((np.asarray(a["abundance"]) >= 2).sum()) + r["promoted"]
    vals = [r["new_index"][e] for e in sorted(r["new_index"])]
    assert vals == list(range(len(vals))) and all(v <= e for e, v in r["new_index"].items())      # strictly increasing, <= the exact value


def test_the_promoted_singletons_of_the_small_set(small):
    assert [PR.restate(small, n)["promoted"] for n in (1024, 16384, 1 << 20, 0)] == [388, 36, 0, 0]


def test_expected_nodes_renumbers_the_index_and_nothing_else(small):
    g = O.Graph(K, L, D, 2)
    b, o = O.concat_reads(synth_set(60))
    assert g.ingest(b, o, 0) == 0
    exact = g.finalize(with_edges=False)
    exp, r = PR.expected_nodes(exact, small, 16384)
    assert exp["n_nodes"] == exact["n_nodes"] == 222 and exp["n_nodes_before"] == r["n_distinct"] == 258
    assert (np.diff(exp["index"].astype(np.int64)) > 0).all() and (exp["index"] <= exact["index"]).all() and (exp["index"] < exact["index"]).any()
    for f in ("keys", "abundance", "seqlen", "src_read"):
        assert exp[f] is exact[f]
