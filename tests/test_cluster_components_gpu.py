"""ms_cluster_components on the GPU against its sequential restatement (cluster_components_case.cluster_components_np): `rep`
exactly, the link score bit for bit, both counts -- on the smallest inputs, on everything a list or an extra entry may hold that is
not an edge, on long paths in three numberings (many hook / compress rounds, deep trees), on a star (one hot root), on the same
entries split between lists and extras in different ways, and twice on one workspace."""
import numpy as np
import pytest

import cluster_case as cc
import cluster_complete_case as ccc
import cluster_components_case as cpc

pytestmark = pytest.mark.gpu


def _gpu(idx, score, extras, lengths, min_score, mincov, **kw):
    import torch
    from merizo_search_amd import ops
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src, dst, esc = extras if extras is not None else (None, None, None)
    rep, link, info = ops.cluster_components(dev(idx), dev(score), dev(src), dev(dst), dev(esc), lengths, min_score, mincov, **kw)
    return rep.cpu().numpy(), link.cpu().numpy(), info


def _check(idx, score, extras, lengths, min_score, mincov, **kw):
    """One call compared with the restatement -> (rep, link, info) of the GPU."""
    rep, link, info = _gpu(idx, score, extras, lengths, min_score, mincov, **kw)
    src, dst, esc = extras if extras is not None else (None, None, None)
    want_rep, want_link, want = cpc.cluster_components_np(idx, score, src, dst, esc, lengths, min_score, mincov)
    n = len(lengths)
    assert np.array_equal(rep, want_rep), np.nonzero(rep != want_rep)[0][:10]
    assert np.array_equal(ccc.bits(link), ccc.bits(want_link)), np.nonzero(ccc.bits(link) != ccc.bits(want_link))[0][:10]
    assert info["n_components"] == want["n_components"] and info["saturated"] == want["saturated"]
    assert 1 <= info["rounds"] <= n
    return rep, link, info


def test_smallest_inputs():
    one = np.array([7], np.int32)
    for idx, score in (cc.empty_lists(1, 1), (np.array([[0]], np.int64), np.array([[0.9]], np.float32))):     # padding; a self-loop
        rep, link, info = _check(idx, score, None, one, 0.5, 0.0)
        assert rep.tolist() == [0] and link.tolist() == [1.0] and info["n_components"] == 1 and info["rounds"] == 1
    rep, link, info = _check(None, None, (np.array([0]), np.array([0]), np.array([0.9], np.float32)), one, 0.5, 0.0)
    assert rep.tolist() == [0] and info["saturated"] == 0
    # k = 1: the edge is held by the higher row only; equal lengths, then the longer row second
    idx, score = cc.lists_from_edges(2, 1, [(1, 0, 0.8)])
    assert _check(idx, score, None, np.array([5, 5], np.int32), 0.5, 0.0)[0].tolist() == [0, 0]
    rep, link, info = _check(idx, score, None, np.array([5, 6], np.int32), 0.5, 0.0)
    assert rep.tolist() == [1, 1] and link.tolist() == [np.float32(0.8), 1.0] and info == dict(info, n_components=1, saturated=1)
    assert _check(idx, score, None, np.array([5, 6], np.int32), 0.5, 0.9)[2]["n_components"] == 2           # 5 < 0.9 * 6


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_garbage_mix_in_lists_and_extras(seed):
    """cluster_case.random_lists and cluster_complete_case.random_extras: padding, rows n, 2^40 + r and negative, self-loops, NaN,
    -inf, scores one ulp below the cut, coverage failures (70 / 100 passes, 70 / 130 does not), a src that is no row, -0.0 next to
    +0.0, duplicates.  n = 777 is no multiple of the workgroup; with k = 5 a workgroup's entries straddle rows."""
    n, k = 777, 5
    idx, score, lengths = cc.random_lists(n, k, seed)
    extras = ccc.random_extras(n, 2000, idx, score, seed + 10)
    full = _check(idx, score, extras, lengths, cc.CUT, 0.7)
    assert 1 < full[2]["n_components"] < n
    _check(idx, score, None, lengths, cc.CUT, 0.7)                         # extras absent
    _check(None, None, extras, lengths, cc.CUT, 0.7)                       # k = 0 with extras
    zero = _check(idx, score, extras, lengths, 0.0, 0.0)                   # -0.0 >= 0.0: a valid edge of weight +0.0
    assert zero[2]["n_components"] < full[2]["n_components"]
    _check(idx, score, extras, lengths, float("-inf"), 1.0)                # no cut; equal lengths only


_PATH = 4096
_ORDERS = {"ascending": lambda: np.arange(_PATH), "descending": lambda: np.arange(_PATH)[::-1].copy(),
           "shuffled": lambda: np.random.default_rng(4).permutation(_PATH)}


@pytest.mark.parametrize("decreasing", [False, True])
@pytest.mark.parametrize("numbering", list(_ORDERS))
def test_long_paths(numbering, decreasing):
    """One path of 4,096 rows: the call returns, with one component and its longest (or, on equal lengths, smallest) row on top."""
    order = _ORDERS[numbering]()
    idx, score, lengths = cpc.path_lists(order, 10000 - np.arange(_PATH) if decreasing else None)
    rep, link, info = _check(idx, score, None, lengths, 0.5, 0.0)
    assert info["n_components"] == 1 and info["saturated"] == _PATH - 1
    assert np.all(rep == (order[0] if decreasing else 0))
    print("path %s, lengths %s: %d rounds" % (numbering, "decreasing" if decreasing else "equal", info["rounds"]))
    if decreasing:                                                         # cut in the middle by coverage: 100 / 7000 < 0.5 at the joint
        lengths = np.full(_PATH, 7000, np.int32)
        lengths[order[_PATH // 2:]] = 100
        rep, _link, info = _check(idx, score, None, lengths, 0.5, 0.5)
        assert info["n_components"] == 2 and set(rep.tolist()) == {int(order[:_PATH // 2].min()), int(order[_PATH // 2:].min())}


def test_star_held_by_the_leaves_and_by_the_centre():
    """5,000 leaves around the highest row.  Each edge held by its leaf only (lists of k = 1); then by the centre only, as extras."""
    n = 5001
    leaves = np.arange(n - 1, dtype=np.int64)
    idx, score = cc.empty_lists(n, 1)
    idx[:n - 1, 0], score[:n - 1, 0] = n - 1, (0.6 + 0.3 * (leaves % 7) / 7).astype(np.float32)
    lengths = np.full(n, 80, np.int32)
    rep, link, info = _check(idx, score, None, lengths, 0.5, 0.0)
    assert info["n_components"] == 1 and np.all(rep == 0) and link[n - 1] == score[:, 0].max()
    extras = (np.full(n - 1, n - 1, np.int64), leaves, score[:n - 1, 0].copy())
    rep2, link2, info2 = _check(None, None, extras, lengths, 0.5, 0.0)
    assert np.array_equal(rep, rep2) and np.array_equal(ccc.bits(link), ccc.bits(link2)) and info2["saturated"] == 0
    lengths[n - 1] = 81                                                    # the centre is the longest: it represents the star
    assert np.all(_check(None, None, extras, lengths, 0.5, 0.0)[0] == n - 1)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("maker", ["random", "family"])
def test_same_entries_split_between_lists_and_extras(maker, seed):
    """n = 3,000, k = 8: all entries as lists; columns 0..3 as lists and 4..7 as extras; odd columns as lists and even ones as extras in
    another order; everything as extras.  `rep`, the link score and the component count are identical (`saturated` is the lists')."""
    n, k = 3000, 8
    idx, score, lengths = (cc.random_lists(n, k, seed) if maker == "random" else cc.family_lists(n, k, seed)[:3])
    base = _check(idx, score, None, lengths, cc.CUT, 0.7)
    splits = [([0, 1, 2, 3], [4, 5, 6, 7]), ([1, 3, 5, 7], [0, 2, 4, 6]), ([], list(range(k)))]
    for t, (keep, move) in enumerate(splits):
        lists = (np.ascontiguousarray(idx[:, keep]), np.ascontiguousarray(score[:, keep])) if keep else (None, None)
        got = _check(lists[0], lists[1], cpc.lists_as_extras(idx, score, move, seed + t), lengths, cc.CUT, 0.7)
        assert np.array_equal(got[0], base[0]) and np.array_equal(ccc.bits(got[1]), ccc.bits(base[1]))
        assert got[2]["n_components"] == base[2]["n_components"]
    if maker == "family":                                                  # families of at most 12 at k = 8: each is one component
        family = cc.family_lists(n, k, seed)[3]
        assert base[2]["n_components"] == np.unique(family).size and np.array_equal(family[base[0]], family)


def test_second_call_on_one_workspace_with_fewer_rows():
    """Stale parents, keys, links and flags of a larger problem must not show in a smaller one on the same workspace and outputs."""
    import torch
    from merizo_search_amd import _lib
    n1, n2, k = 3000, 1234, 6
    ws = torch.empty(int(_lib.load().ms_cluster_components_workspace_bytes(n1)), dtype=torch.uint8, device="cuda")
    idx, score, lengths = cc.random_lists(n1, k, 5)
    first = _check(idx, score, ccc.random_extras(n1, 500, idx, score, 6), lengths, cc.CUT, 0.7, workspace=ws)
    idx2, score2, lengths2 = cc.random_lists(n2, k, 7)
    out = (torch.full((n2,), -7, dtype=torch.int64, device="cuda"), torch.full((n2,), 9.0, dtype=torch.float32, device="cuda"))
    second = _check(idx2, score2, None, lengths2, cc.CUT, 0.7, workspace=ws, out=out)
    assert np.array_equal(out[0].cpu().numpy(), second[0]) and second[2]["n_components"] != first[2]["n_components"]
    again = _check(idx, score, ccc.random_extras(n1, 500, idx, score, 6), lengths, cc.CUT, 0.7, workspace=ws)
    assert np.array_equal(again[0], first[0]) and np.array_equal(ccc.bits(again[1]), ccc.bits(first[1]))
