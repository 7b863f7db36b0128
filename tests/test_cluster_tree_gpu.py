"""ms_cluster_tree on the GPU against its sequential restatement (cluster_tree_case.cluster_tree_np: Kruskal in the header's order): the
SET of (a, b, weight bits) exactly, the edge count, `saturated`, and the promised bound on the rounds -- on the smallest inputs, on pure
tie-breaking with deep hook chains (a shuffled path, rings), on one hot root (a star), on a bridge, on random graphs with everything
that is no edge, on the same entries split between lists and extras, on a reused workspace and run after run.  Then the cut on the
device: ms_cluster_components over the forest's edges equals ms_cluster_components over the graph, threshold by threshold."""
import math

import numpy as np
import pytest

import cluster_case as cc
import cluster_complete_case as ccc
import cluster_components_case as cpc
import cluster_tree_case as ctc

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu(idx, score, extras, lengths, min_score, mincov, **kw):
    from merizo_search_amd import ops
    src, dst, esc = extras if extras is not None else (None, None, None)
    pairs, weight, info = ops.cluster_tree(_dev(idx), _dev(score), _dev(src), _dev(dst), _dev(esc), lengths, min_score, mincov, **kw)
    return pairs.cpu().numpy(), weight.cpu().numpy(), info


def _check(idx, score, extras, lengths, min_score, mincov, **kw):
    """One call compared with the restatement -> (forest set, pairs, weight, info) of the GPU."""
    pairs, weight, info = _gpu(idx, score, extras, lengths, min_score, mincov, **kw)
    src, dst, esc = extras if extras is not None else (None, None, None)
    a, b, w, want = ctc.cluster_tree_np(idx, score, src, dst, esc, lengths, min_score, mincov)
    n = len(lengths)
    assert pairs.shape == (n, 2) and pairs.dtype == np.int32 and weight.shape == (n,) and weight.dtype == np.float32
    got = ctc.forest_set(*ctc.slots_as_forest(pairs, weight))
    expected = ctc.forest_set(a, b, w)
    assert got == expected, (sorted(got - expected)[:5], sorted(expected - got)[:5])
    assert info["n_edges"] == want["n_edges"] == len(got) and info["saturated"] == want["saturated"]
    assert 1 <= info["rounds"] <= int(math.floor(math.log2(n))) + 1, info["rounds"]
    return got, pairs, weight, info


def test_smallest_inputs():
    one = np.array([7], np.int32)
    for idx, score in (cc.empty_lists(1, 1), (np.array([[0]], np.int64), np.array([[0.9]], np.float32))):     # padding; a self-loop
        got, pairs, weight, info = _check(idx, score, None, one, 0.5, 0.0)
        assert got == set() and pairs.tolist() == [[-1, -1]] and info["n_edges"] == 0 and info["rounds"] == 1
    _check(None, None, (np.array([0]), np.array([0]), np.array([0.9], np.float32)), one, 0.5, 0.0)
    # n = 2: the two directions at different scores; the weight is the larger one; the larger row hooks
    idx, score = cc.lists_from_edges(2, 1, [(0, 1, 0.6), (1, 0, 0.9)])
    got, pairs, weight, info = _check(idx, score, None, np.array([5, 6], np.int32), 0.5, 0.0)
    assert got == {(0, 1, int(ccc.bits(np.float32(0.9))[0]))} and pairs.tolist() == [[-1, -1], [0, 1]] and info["rounds"] == 2
    got, _pairs, _weight, info = _check(idx, score, None, np.array([5, 6], np.int32), 0.7, 0.0)           # one direction below the cut
    assert len(got) == 1 and info["saturated"] == 1
    assert _check(idx, score, None, np.array([5, 6], np.int32), 0.5, 0.9)[3]["n_edges"] == 0              # 5 < 0.9 * 6
    zero = cc.lists_from_edges(2, 1, [(0, 1, -0.0)])
    assert _check(zero[0], zero[1], None, np.array([5, 5], np.int32), 0.0, 0.0)[0] == {(0, 1, 0)}           # -0.0 counts as +0.0


def test_shuffled_path_of_equal_weights_ends_within_the_promised_rounds():
    """1,000 rows, every weight 0.8: pure tie-breaking, hook chains across many trees.  rounds <= floor(log2 1000) + 1 = 10 (what
    _check asserts) is what a sequential degeneration -- one hook per round -- would miss by far."""
    order = np.random.default_rng(4).permutation(1000)
    idx, score, lengths = cpc.path_lists(order)
    got, _pairs, _weight, info = _check(idx, score, None, lengths, 0.5, 0.0)
    assert len(got) == 999 and info["rounds"] <= 10
    for order in (np.arange(1000), np.arange(1000)[::-1].copy()):          # every row hooks at once: one chain of 1,000 hooks
        idx, score, lengths = cpc.path_lists(order)
        assert _check(idx, score, None, lengths, 0.5, 0.0)[3]["rounds"] == 2


@pytest.mark.parametrize("n", [64, 257])
def test_ring_of_equal_weights_drops_the_last_edge_of_the_order(n):
    idx, score, lengths = ctc.ring_lists(n)
    got, _pairs, _weight, info = _check(idx, score, None, lengths, 0.5, 0.0)
    bits = int(ccc.bits(np.float32(0.8))[0])
    ring = {(min(t, (t + 1) % n), max(t, (t + 1) % n), bits) for t in range(n)}
    assert ring - got == {(n - 2, n - 1, bits)} and info["n_edges"] == n - 1


def test_star_of_70000_leaves_on_one_hot_root():
    idx, score, lengths = ctc.star_lists(70000)
    got, pairs, _weight, info = _check(idx, score, None, lengths, 0.5, 0.0)
    assert info["n_edges"] == 70000 and info["rounds"] == 2 and pairs[0].tolist() == [-1, -1] and np.all(pairs[1:, 0] == 0)


def test_two_cliques_and_a_weaker_bridge():
    idx, score, extras, lengths = ctc.two_cliques()
    got, _pairs, _weight, info = _check(idx, score, extras, lengths, 0.5, 0.0)
    weak = int(ccc.bits(np.float32(0.7))[0])
    assert info["n_edges"] == 79 and [e for e in got if e[2] == weak] == [(39, 40, weak)]
    assert _check(idx, score, extras, lengths, 0.8, 0.0)[3]["n_edges"] == 78                                # the bridge is below the cut


@pytest.fixture(scope="module")
def graph():
    return ctc.random_graph(5000, 8, 3000, 21)


def test_random_graph_with_everything_that_is_no_edge(graph):
    idx, score, extras, lengths = graph
    full = _check(idx, score, extras, lengths, ctc.TREE_CUT, 0.7)
    assert 1000 < full[3]["n_edges"] < 4999
    lists_only = _check(idx, score, None, lengths, ctc.TREE_CUT, 0.7)                                       # m = 0
    extras_only = _check(None, None, extras, lengths, ctc.TREE_CUT, 0.7)                                    # k = 0
    assert extras_only[3]["saturated"] == 0 and extras_only[3]["n_edges"] < lists_only[3]["n_edges"] <= full[3]["n_edges"]
    _check(idx, score, extras, lengths, float("-inf"), 1.0)                                                 # no cut; equal lengths only


def test_same_entries_split_between_lists_and_extras_with_duplicates(graph):
    idx, score, _extras, lengths = graph
    base = _check(idx, score, None, lengths, ctc.TREE_CUT, 0.7)
    k = idx.shape[1]
    splits = [([0, 1, 2, 3], [4, 5, 6, 7]), ([1, 3, 5, 7], [0, 2, 4, 6]), ([], list(range(k))), (list(range(k)), [0, 0, 3, 7])]
    for t, (keep, move) in enumerate(splits):
        lists = (np.ascontiguousarray(idx[:, keep]), np.ascontiguousarray(score[:, keep])) if keep else (None, None)
        got = _check(lists[0], lists[1], cpc.lists_as_extras(idx, score, move, 40 + t), lengths, ctc.TREE_CUT, 0.7)
        assert got[0] == base[0] and got[3]["rounds"] == base[3]["rounds"]
        assert np.array_equal(got[1], base[1]) and np.array_equal(ccc.bits(got[2]), ccc.bits(base[2]))     # the slots too


def test_second_call_on_one_workspace_with_fewer_rows(graph):
    import torch
    from merizo_search_amd import _lib
    idx, score, extras, lengths = graph
    ws = torch.empty(int(_lib.load().ms_cluster_tree_workspace_bytes(5000)), dtype=torch.uint8, device="cuda")
    first = _check(idx, score, extras, lengths, ctc.TREE_CUT, 0.7, workspace=ws)
    idx2, score2, extras2, lengths2 = ctc.random_graph(1234, 6, 500, 22)
    out = (torch.full((1234, 2), 9, dtype=torch.int32, device="cuda"), torch.full((1234,), 9.0, dtype=torch.float32, device="cuda"))
    second = _check(idx2, score2, extras2, lengths2, ctc.TREE_CUT, 0.7, workspace=ws, out=out)
    assert np.array_equal(out[0].cpu().numpy(), second[1])
    again = _check(idx, score, extras, lengths, ctc.TREE_CUT, 0.7, workspace=ws)
    assert again[0] == first[0] and np.array_equal(again[1], first[1])


def test_twenty_calls_give_identical_outputs_rounds_included(graph):
    idx, score, extras, lengths = graph
    from merizo_search_amd import ops
    args = (_dev(idx), _dev(score), _dev(extras[0]), _dev(extras[1]), _dev(extras[2]), _dev(lengths))
    first = None
    for _call in range(20):
        pairs, weight, info = ops.cluster_tree(*args, ctc.TREE_CUT, 0.7)
        got = (pairs.cpu().numpy().tobytes(), weight.cpu().numpy().tobytes(), info)
        first = first or got
        assert got == first


def test_components_of_the_forest_are_the_components_of_the_graph_at_every_threshold(graph):
    """The cut on the device: ms_cluster_components over the forest's edges as extras (k = 0) against ms_cluster_components over the
    full graph, at the cut itself and at three of the score values above it."""
    import torch
    from merizo_search_amd import ops
    idx, score, extras, lengths = graph
    full = (_dev(idx), _dev(score), _dev(extras[0]), _dev(extras[1]), _dev(extras[2]))
    L = _dev(lengths)
    pairs, weight, info = ops.cluster_tree(*full, L, ctc.TREE_CUT, 0.7)
    filled = pairs[:, 0] >= 0
    a, b, w = pairs[filled, 0].to(torch.int64).contiguous(), pairs[filled, 1].to(torch.int64).contiguous(), weight[filled].contiguous()
    assert int(filled.sum()) == info["n_edges"]
    counts = []
    for level in (float(ctc.TREE_CUT), float(ctc.TREE_SCORES[2]), float(ctc.TREE_SCORES[4]), float(ctc.TREE_SCORES[7])):
        want_rep, want_link, want = ops.cluster_components(*full, L, level, 0.7)
        rep, link, got = ops.cluster_components(None, None, a, b, w, L, level, 0.7)
        assert torch.equal(rep, want_rep) and torch.equal(link.view(torch.int32), want_link.view(torch.int32)), level
        assert got["n_components"] == want["n_components"]
        counts.append(got["n_components"])
    assert counts == sorted(counts) and counts[0] == 5000 - info["n_edges"] and counts[0] < counts[-1]
