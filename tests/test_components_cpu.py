"""Connected components of the unitig graph and the small-component step without a GPU: the checker (tests/components_restatement.py) is itself
checked on hand-made graphs with the answer written out and, on the fuzz graphs, against a flood fill over the NODE-level edge records that knows
nothing of unitigs; the constants and the ctypes mirror are checked against the header.  The GPU side is tests/test_gpu_components.py."""
import os

import pytest

import components_restatement as CR
import simplify_restatement as S
import unitig_restatement as U
from conftest import ROOT
from test_simplify_cpu import FORK, FORK_AB, hand, path
from test_unitigs_cpu import fuzz_case, oracle_graph

P, M = "+", "-"
K = CR.COMPONENTS


def test_constants():
    from rust_mdbg_amd import api
    assert api.MDBG_SIMPLIFY_COMPONENTS == K == 4
    h = open(os.path.join(ROOT, "include", "mdbg_hip.h")).read()
    assert "#define MDBG_SIMPLIFY_COMPONENTS 4u" in h and "#define MDBG_ABI_VERSION 3 " in h
    assert {"mdbg_graph_components", "mdbg_graph_components_device"} <= set(api.EXPORTS)
    assert [f for f, _, _ in api.COMPONENT_FIELDS] == [f for f, _ in api.ComponentList._fields_[2:]]
    assert all(s[0] != K for s in api.MAGIC_SIMPLIFY_STEPS)                   # the default schedule is what it was


def hand_components(abund, edges, length=None):
    nodes, edges, length_of = hand(abund, edges, length)
    cur, _ = S.current(nodes, edges, {int(i) for i in nodes["index"]}, None, length_of)
    return cur, CR.components(cur)


def run_hand(abund, edges, steps, length=None):
    nodes, edges, length_of = hand(abund, edges, length)
    log, final = CR.simplify(nodes, edges, steps, length_of=length_of)
    return [sorted(st["nodes"]) for st in log], final["walks"]


FORK2 = [(a + 20, oa, b + 20, ob, ov) for a, oa, b, ob, ov in FORK]             # the same fork on the nodes 21..28
FORK2_AB = {n + 20: a for n, a in FORK_AB.items()}


def test_two_paths_and_a_singleton_give_three_components():
    cur, cc = hand_components({n: 3 for n in (1, 2, 3, 5, 6, 9)}, path(1, 2, 3) + path(5, 6))
    assert cur["walks"] == [[(1, P), (2, P), (3, P)], [(5, P), (6, P)], [(9, P)]]
    assert cc == dict(component=[0, 1, 2], n_components=3, first_unitig=[0, 1, 2], unitigs=[1, 1, 1], nodes=[3, 2, 1], bases=[300, 200, 100], kc_sum=[9, 6, 3],
                      circular=[False] * 3)


def test_unitigs_joined_by_edges_form_one_component():
    """two forks (three unitigs each: the trunk and two arms) with a singleton between them in unitig order"""
    ab = {**FORK_AB, **FORK2_AB, **{10: 7}}
    cur, cc = hand_components(ab, FORK + FORK2)
    assert [w[0][0] for w in cur["walks"]] == [1, 4, 8, 10, 21, 24, 28]
    assert cc["component"] == [0, 0, 0, 1, 2, 2, 2] and cc["first_unitig"] == [0, 3, 4] and cc["unitigs"] == [3, 1, 3]
    assert cc["nodes"] == [8, 1, 8] and cc["bases"] == [800, 100, 800] and cc["kc_sum"] == [sum(FORK_AB.values()), 7, sum(FORK_AB.values())]
    # the singleton branches into the two arms of the second fork (no link: the unitigs stay): numbering follows the smallest unitig of a component
    cur, cc = hand_components(ab, FORK + FORK2 + [(10, P, 28, P, 5), (10, P, 24, P, 5)])
    assert [w[0][0] for w in cur["walks"]] == [1, 4, 8, 10, 21, 24, 28]
    assert cc["component"] == [0, 0, 0, 1, 1, 1, 1] and cc["first_unitig"] == [0, 3] and cc["unitigs"] == [3, 4] and cc["nodes"] == [8, 9]


def test_a_record_from_a_unitig_to_itself_joins_nothing():
    cycle = path(1, 2, 3) + [(3, P, 1, P, 5)]                                   # one circular unitig: its closing link is the record "u + u +"
    loop = [(7, P, 7, P, 5)]                                                    # a node with an arc to itself: a unitig of one node with the record "u + u +"
    cur, cc = hand_components({1: 2, 2: 2, 3: 2, 7: 4, 9: 1}, cycle + loop)
    assert cur["edges"] == [(0, P, 0, P, 5), (1, P, 1, P, 5)] and cur["circular"] == [True, False, False]
    assert cc["component"] == [0, 1, 2] and cc["unitigs"] == [1, 1, 1] and cc["circular"] == [True, False, False] and cc["nodes"] == [3, 1, 1]


def test_a_record_given_on_the_other_strand_joins_the_same_pair():
    flip = lambda o: P if o == M else M
    _, want = hand_components({**FORK_AB, **{10: 7}}, FORK)
    for pick in (lambda i: True, lambda i: i % 2 == 0, lambda i: i % 3 == 1):
        edges = [(b, flip(ob), a, flip(oa), ov) if pick(i) else (a, oa, b, ob, ov) for i, (a, oa, b, ob, ov) in enumerate(FORK)]
        assert hand_components({**FORK_AB, **{10: 7}}, edges)[1] == want
    assert want["component"] == [0, 0, 0, 1]


def test_component_step_limits_at_the_boundary():
    """the fork is a component of 8 nodes and 800 bases in three unitigs: the limits apply to those sums, not to one unitig"""
    ab = {**FORK_AB, **{10: 7}}
    assert run_hand(ab, FORK, [(K, 8, 0)])[0] == [list(range(1, 9)) + [10]]
    assert run_hand(ab, FORK, [(K, 7, 0)])[0] == [[10]]
    assert run_hand(ab, FORK, [(K, 0, 800)])[0] == [list(range(1, 9)) + [10]]
    assert run_hand(ab, FORK, [(K, 0, 799)])[0] == [[10]]
    assert run_hand(ab, FORK, [(K, 8, 800)])[0] == [list(range(1, 9)) + [10]] and run_hand(ab, FORK, [(K, 8, 799)])[0] == [[10]] and run_hand(ab, FORK, [(K, 7, 800)])[0] == [[10]]
    assert run_hand(ab, FORK, [(K, 1, 99)]) == ([[]], hand_components(ab, FORK)[0]["walks"])
    assert run_hand(ab, FORK, [(K, 0, 801)], length={8: 102})[0] == [[10]]
    removed, walks = run_hand(ab, FORK, [(S.TIPS, 2, 0), (K, 7, 0)])             # the tip step removes node 8: 7 nodes are left, and the next step sees them
    assert removed == [[8], list(range(1, 8)) + [10]] and walks == []
    for bad in ([(K, 0, 0)], [(3, 1, 1)], [(5, 1, 1)]):
        with pytest.raises(AssertionError):
            CR.simplify(*hand(ab, FORK)[:2], bad, length_of=len)


def test_a_component_with_a_circular_unitig_stays():
    cycle = path(1, 2, 3) + [(3, P, 1, P, 5)]
    removed, walks = run_hand({1: 2, 2: 2, 3: 2, 5: 1, 6: 1}, cycle + path(5, 6), [(K, 0, 10 ** 9)])
    assert removed == [[5, 6]] and walks == [[(1, P), (2, P), (3, P)]]
    # a cycle with a branch hanging on it is no circular unitig: the component is an ordinary one
    removed, walks = run_hand({1: 2, 2: 2, 3: 2, 4: 1}, cycle + [(2, P, 4, P, 5)], [(K, 0, 10 ** 9)])
    assert removed == [[1, 2, 3, 4]] and walks == []


def test_a_step_that_removes_everything_leaves_the_empty_list():
    nodes, edges, length_of = hand(FORK_AB, FORK)
    log, final = CR.simplify(nodes, edges, [(K, 0, 10 ** 9), (S.TIPS, 10, 0), (K, 1, 0)], length_of=length_of)
    assert [sorted(st["nodes"]) for st in log] == [list(range(1, 9)), [], []]
    assert final["walks"] == [] and final["edges"] == [] and final["kc_sum"] == [] and final["length"] == []
    assert CR.components(final) == dict(component=[], n_components=0, first_unitig=[], unitigs=[], nodes=[], bases=[], kc_sum=[], circular=[])


# ---- the fuzz graphs ------------------------------------------------------------------------------------------------------------------------
def node_flood_fill(nodes, edges):
    """node index -> the smallest node index it can reach over the node-level edge records, orientation ignored (nothing here knows of unitigs)"""
    nb = {int(i): set() for i in nodes["index"]}
    for (a, _), (b, _), _ in U.as_records(edges):
        nb[a].add(b)
        nb[b].add(a)
    label = {}
    for start in sorted(nb):
        if start in label:
            continue
        todo = [start]
        label[start] = start
        while todo:
            for y in nb[todo.pop()]:
                if y not in label:
                    label[y] = start
                    todo.append(y)
    return label


MORE_THAN_ONE = {(0, 0.0), (1, 0.0), (3, 0.01)}                                 # where the fuzz graphs are known to fall apart (measured with this checker)
STEP = [(K, 10, 5000)]


@pytest.mark.parametrize("presimp", [0.0, 0.01])
@pytest.mark.parametrize("seed", range(6))
def test_components_of_the_fuzz_graphs(seed, presimp):
    k, l, d, A, reads = fuzz_case(seed)
    nodes, edges = oracle_graph(reads, k, l, d, A, presimp)
    cur = U.unitigs(nodes, edges, reads)
    cc = CR.components(cur)
    label = node_flood_fill(nodes, edges)
    of_unitig = []
    for w in cur["walks"]:
        assert len({label[n] for n, _ in w}) == 1                               # a unitig lies in one node-level component
        of_unitig.append(label[w[0][0]])
    order = {}
    for x in of_unitig:                                                         # numbered by first appearance in unitig order = by the smallest unitig
        order.setdefault(x, len(order))
    assert cc["component"] == [order[x] for x in of_unitig] and cc["n_components"] == len(order) == len(set(label.values()))
    assert cc["first_unitig"] == [of_unitig.index(x) for x in order]
    assert sum(cc["unitigs"]) == len(cur["walks"]) and sum(cc["nodes"]) == len(nodes["index"]) and sum(cc["bases"]) == sum(cur["length"])
    assert sum(cc["kc_sum"]) == sum(int(a) for a in nodes["abundance"]) and any(cc["circular"]) == any(cur["circular"])
    sizes = sorted(zip(cc["nodes"], cc["bases"]))
    print("seed %d presimp %g: %d components, %d of one node, smallest %s" % (seed, presimp, cc["n_components"], sum(n == 1 for n in cc["nodes"]), sizes[0]))
    if (seed, presimp) in MORE_THAN_ONE:
        assert cc["n_components"] > 1
    # the small-component step
    log, final = CR.simplify(nodes, edges, STEP, reads)
    small = {c for c in range(cc["n_components"]) if CR.small_component(c, cc, *STEP[0][1:])}
    gone_nodes = {n for u, w in enumerate(cur["walks"]) if cc["component"][u] in small for n, _ in w}
    assert log[0]["nodes"] == gone_nodes                                        # every removed node belonged to a small component, and all of those went
    assert final["walks"] == [w for u, w in enumerate(cur["walks"]) if cc["component"][u] not in small]      # the survivors' walks are unchanged
    after = CR.components(final)
    assert not any(CR.small_component(c, after, *STEP[0][1:]) for c in range(after["n_components"]))
    assert after["n_components"] == cc["n_components"] - len(small)
    if seed in (0, 1) and presimp == 0.0:
        assert gone_nodes
