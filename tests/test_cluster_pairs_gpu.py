"""ms_cluster_pairs, ms_cluster_pairs_apply and ms_cluster_pairs_find on the GPU against their sequential restatements
(cluster_tm_case): the pair SET and both counts on random graphs with every kind of entry that is no edge, duplicates between lists
and extras, equal lengths, list widths and extra counts around the wave size, one pair named by every entry, a star, a cap below
the count with guard slots behind it, a reused workspace; the edited lists and extras bit for bit; slots found in either order;
and what the ops refuse."""
import numpy as np
import pytest

import cluster_case as cc
import cluster_complete_case as ccc
import cluster_components_case as cpc
import cluster_tm_case as ct

pytestmark = pytest.mark.gpu
CUT, COV = float(cc.CUT), 0.7


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pairs_gpu(idx, score, src, dst, esc, lengths, min_score=CUT, mincov=COV, **kw):
    """-> (pairs as the GPU wrote them [min(count, cap),2], count, saturated, the device tensors of the graph, workspace)."""
    from merizo_search_amd import ops
    graph = tuple(_dev(x) for x in (idx, score, src, dst, esc))
    pairs, counts, ws = ops.cluster_pairs(*graph, lengths, min_score, mincov, **kw)
    count, saturated = (int(c) for c in counts.cpu().numpy())
    return pairs.cpu().numpy()[:min(count, pairs.shape[0])], count, saturated, graph, ws


def _check_set(idx, score, src, dst, esc, lengths, min_score=CUT, mincov=COV, what=None):
    """The GPU's pairs are the restatement's as a SET, without a duplicate, with both counts."""
    want, want_sat = ct.cluster_pairs_np(idx, score, src, dst, esc, lengths, min_score, mincov)
    got, count, saturated, graph, ws = _pairs_gpu(idx, score, src, dst, esc, lengths, min_score, mincov)
    assert got.dtype == np.int32 and count == want.shape[0] == got.shape[0], (what, count, want.shape)
    assert saturated == want_sat, (what, saturated, want_sat)
    as_set = {tuple(p) for p in got.tolist()}
    assert len(as_set) == count and as_set == {tuple(p) for p in want.tolist()}, what
    return got, graph, ws


def _reciprocal(idx, score, seed):
    """Every third edge of the lists also in the other endpoint's list (its last column), where that endpoint is a row."""
    rng = np.random.default_rng(seed)
    n, k = idx.shape
    for i in rng.permutation(n)[:n // 3]:
        j = int(idx[i, 0])
        if 0 <= j < n and j != i:
            idx[j, k - 1], score[j, k - 1] = i, score[i, 0]
    return idx, score


# ------------------------------------------------------------------ the set ----
def test_random_lists_with_reciprocal_entries_extras_and_every_kind_of_invalid_entry():
    n, k = 300, 7
    idx, score, lengths = cc.random_lists(n, k, seed=41)
    idx, score = _reciprocal(idx, score, 42)
    src, dst, esc = ccc.random_extras(n, 500, idx, score, seed=43)
    again = cpc.lists_as_extras(idx, score, [0, 3], seed=44)             # extras that repeat list entries, and each other
    src, dst, esc = (np.concatenate([a, b, b]) for a, b in zip((src, dst, esc), again))
    i, j, s, _k = ct._entries(idx, score, src, dst, esc, n)
    valid = cpc.valid_entries(i, j, s, lengths, CUT, COV)
    with np.errstate(invalid="ignore"):
        kinds = dict(negative=j < 0, beyond=j >= n, loop=i == j, nan=np.isnan(s), low=s < np.float32(CUT), src_out=(i < 0) | (i >= n),
                     coverage=~valid & (i >= 0) & (i < n) & (j >= 0) & (j < n) & (i != j) & (s >= np.float32(CUT)))
    assert all(v.any() for v in kinds.values()), {name: int(v.sum()) for name, v in kinds.items()}
    _check_set(idx, score, src, dst, esc, lengths, what="lists + extras")
    _check_set(idx, score, None, None, None, lengths, what="lists")
    # the set does not depend on how the entries are split between lists and extras, nor on their order
    want = {tuple(p) for p in ct.cluster_pairs_np(idx, score, src, dst, esc, lengths, CUT, COV)[0].tolist()}
    moved = cpc.lists_as_extras(idx, score, list(range(k)), seed=45)
    all_src, all_dst, all_esc = (np.concatenate([a, b]) for a, b in zip((src, dst, esc), moved))
    got, _g, _w = _check_set(None, None, all_src, all_dst, all_esc, lengths, what="extras only (k == 0)")
    assert {tuple(p) for p in got.tolist()} == want
    # no cut at all, and equal lengths: orientation by row alone
    _check_set(idx, score, src, dst, esc, lengths, -np.inf, 0.0, what="no cut")
    got, _g, _w = _check_set(idx, score, src, dst, esc, np.full(n, 90, np.int32), what="equal lengths")
    assert (got[:, 0] < got[:, 1]).all()


@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_list_widths_around_the_wave_size(k):
    idx, score, lengths = cc.random_lists(130, k, seed=500 + k)
    _check_set(idx, score, None, None, None, lengths, what=k)


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 1000])
def test_extra_counts_around_the_wave_size(m):
    n = 200
    idx, score, lengths = cc.random_lists(n, 3, seed=600 + m)
    extras = ccc.random_extras(n, m, idx, score, seed=700 + m) if m else (None, None, None)
    _check_set(idx, score, *extras, lengths, what=m)
    if m:
        _check_set(None, None, *extras, lengths, what=("extras only", m))


def test_a_single_row_has_no_pair():
    idx, score = np.array([[0, -1, 5]], np.int64), np.array([[0.9, -np.inf, 0.9]], np.float32)
    got, _g, _w = _check_set(idx, score, np.array([0, 0]), np.array([0, 1]), np.array([0.9, 0.9], np.float32), np.array([50], np.int32))
    assert got.shape == (0, 2)


def test_every_entry_names_one_pair():
    """Every lane of every wave fights for one position: one pair, both orientations of the entry, lists and extras."""
    n, k = 400, 64
    lengths = np.full(n, 80, np.int32)
    lengths[7] = 90
    idx, score = cc.empty_lists(n, k)
    idx[7], score[7] = 3, 0.9
    idx[3], score[3] = 7, 0.8
    src = np.where(np.arange(5000) % 2 == 0, 3, 7).astype(np.int64)
    got, _g, _w = _check_set(idx, score, src, 10 - src, np.full(5000, 0.7, np.float32), lengths)
    assert got.tolist() == [[7, 3]]


def test_a_star():
    n, hub = 3001, 11
    leaves = np.array([r for r in range(n) if r != hub])
    idx, score = cc.empty_lists(n, 1)
    idx[leaves, 0], score[leaves, 0] = hub, 0.9
    lengths = np.full(n, 60, np.int32)
    got, _g, _w = _check_set(idx, score, leaves[::2], np.full(leaves[::2].shape, hub), np.full(leaves[::2].shape, 0.8, np.float32), lengths)
    assert got.shape[0] == n - 1 and sorted(np.where(got[:, 0] == hub, got[:, 1], got[:, 0]).tolist()) == leaves.tolist()


def test_a_cap_below_the_count_and_cap_zero():
    import torch
    from merizo_search_amd import ops
    n, k = 300, 7
    idx, score, lengths = cc.random_lists(n, k, seed=81)
    want, want_sat = ct.cluster_pairs_np(idx, score, None, None, None, lengths, CUT, COV)
    count, cap, G = want.shape[0], want.shape[0] // 3, 64
    assert cap > 10
    buf = torch.full((cap + G, 2), -77, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    graph = (_dev(idx), _dev(score), None, None, None)
    pairs, counts, ws = ops.cluster_pairs(*graph, lengths, CUT, COV, out=(buf[:cap], counts))
    assert counts.cpu().tolist() == [count, want_sat]                     # exact whatever the cap
    got = buf.cpu().numpy()
    assert (got[cap:] == -77).all()                                       # nothing at or behind slot cap
    kept = {tuple(p) for p in got[:cap].tolist()}
    assert len(kept) == cap and kept <= {tuple(p) for p in want.tolist()}
    # find knows the pairs that were written, and only those; apply removes the rest, keep or not (fail closed)
    slots = ops.cluster_pairs_find(want[:, 0], want[:, 1], lengths, ws).cpu().numpy()
    written = np.array([tuple(p) in kept for p in want.tolist()])
    assert (slots[written] >= 0).all() and (slots[written] < cap).all() and (slots[~written] == -1).all()
    assert np.array_equal(got[slots[written]], want[written])
    removed = ops.cluster_pairs_apply(*graph, lengths, CUT, COV, torch.ones(count, dtype=torch.uint8, device="cuda"), ws)
    new_idx, new_score, _d, _e, want_removed = ct.pairs_apply_np(idx, score, None, None, None, lengths, CUT, COV, got[:cap], np.ones(count))
    assert int(removed.item()) == want_removed > 0
    assert np.array_equal(graph[0].cpu().numpy(), new_idx) and np.array_equal(ccc.bits(graph[1].cpu().numpy()), ccc.bits(new_score))
    # cap == 0 only counts
    pairs, counts, _ws = ops.cluster_pairs(_dev(idx), _dev(score), None, None, None, lengths, CUT, COV, cap=0)
    assert pairs.shape == (0, 2) and counts.cpu().tolist() == [count, want_sat]


def test_one_workspace_serves_two_graphs_without_clean_up():
    import torch
    from merizo_search_amd import ops
    big = cc.random_lists(300, 7, seed=91)
    small = cc.random_lists(120, 3, seed=92)
    need = int(ops._lib.load().ms_cluster_pairs_workspace_bytes(300, 7, 0))
    G = 256
    ws_buf = torch.full((need + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    for idx, score, lengths in (big, small, big):
        want, want_sat = ct.cluster_pairs_np(idx, score, None, None, None, lengths, CUT, COV)
        got, count, saturated, _graph, _ws = _pairs_gpu(idx, score, None, None, None, lengths, workspace=ws_buf[G:G + need])
        assert (count, saturated) == (want.shape[0], want_sat) and {tuple(p) for p in got.tolist()} == {tuple(p) for p in want.tolist()}
        assert bool((ws_buf[:G] == 0x5A).all()) and bool((ws_buf[-G:] == 0x5A).all())


# ------------------------------------------------------------------ apply ----
@pytest.mark.parametrize("n,k,m", [(300, 7, 800), (200, 0, 600), (130, 65, 0)])
def test_apply_edits_lists_and_extras_as_the_restatement_does(n, k, m):
    import torch
    from merizo_search_amd import ops
    rng = np.random.default_rng(n + k + m)
    idx, score, lengths = cc.random_lists(n, max(k, 1), seed=n + k)
    extras = ccc.random_extras(n, m, idx, score, seed=n + m) if m else (None, None, None)
    if k == 0:
        idx = score = None
    got, graph, ws = _check_set(idx, score, *extras, lengths)
    assert got.shape[0] > 20
    keep = (rng.random(got.shape[0]) < 0.5).astype(np.uint8)
    removed = ops.cluster_pairs_apply(*graph, lengths, CUT, COV, _dev(keep), ws)
    new_idx, new_score, new_dst, new_esc, want_removed = ct.pairs_apply_np(idx, score, *extras, lengths, CUT, COV, got, keep)
    assert int(removed.item()) == want_removed > 0
    for dev, want in ((graph[0], new_idx), (graph[3], new_dst)):
        assert (dev is None) == (want is None) and (dev is None or np.array_equal(dev.cpu().numpy(), want))
    for dev, want in ((graph[1], new_score), (graph[4], new_esc)):        # bit for bit: invalid entries keep theirs, NaN payloads too
        assert dev is None or np.array_equal(ccc.bits(dev.cpu().numpy()), ccc.bits(want))
    if extras[0] is not None:
        assert np.array_equal(graph[2].cpu().numpy(), extras[0])
    # the cluster calls now see the graph without the rejected pairs, in both directions
    left, _sat = ct.cluster_pairs_np(new_idx, new_score, extras[0], new_dst, new_esc, lengths, CUT, COV)
    assert {tuple(p) for p in left.tolist()} == {tuple(p) for p, kp in zip(got.tolist(), keep) if kp}
    pairs2, counts2, _ws2 = ops.cluster_pairs(*graph, lengths, CUT, COV)
    assert int(counts2[0].item()) == int(keep.sum())


def test_apply_removes_a_pair_the_set_does_not_hold_and_a_slot_behind_keep():
    import torch
    from merizo_search_amd import ops
    n = 200
    idx, score, lengths = cc.random_lists(n, 5, seed=7)
    got, graph, ws = _check_set(idx, score, None, None, None, lengths)
    # the same workspace, a graph with one more valid entry between two rows of one length that were not adjacent
    same = np.nonzero(lengths == lengths[0])[0]
    a, b = next((int(x), int(y)) for x in same for y in same if x < y and (x, y) not in {tuple(p) for p in got.tolist()})
    src, dst, esc = np.array([b]), np.array([a]), np.array([0.9], np.float32)
    extra = tuple(_dev(x) for x in (src, dst, esc))
    ws2 = torch.empty(int(ops._lib.load().ms_cluster_pairs_workspace_bytes(n, 5, 1)), dtype=torch.uint8, device="cuda")
    pairs2, counts2, ws2 = ops.cluster_pairs(graph[0], graph[1], None, None, None, lengths, CUT, COV, workspace=ws2)
    # (n k and n k + 1 entries take the same number of positions here: the set built without the extra serves the call with it)
    assert ws2.numel() == ws.numel()
    count = int(counts2[0].item())
    keep = torch.ones(count - 3, dtype=torch.uint8, device="cuda")       # the last three slots have no verdict
    removed = ops.cluster_pairs_apply(graph[0], graph[1], *extra, lengths, CUT, COV, keep, ws2)
    new_idx, new_score, new_dst, new_esc, want_removed = ct.pairs_apply_np(idx, score, src, dst, esc, lengths, CUT, COV,
                                                                           pairs2.cpu().numpy()[:count], np.ones(count - 3))
    assert int(removed.item()) == want_removed >= 4
    assert extra[1].cpu().tolist() == [-1] and extra[2].cpu().tolist() == [-np.inf] and new_dst.tolist() == [-1]
    assert np.array_equal(graph[0].cpu().numpy(), new_idx) and np.array_equal(ccc.bits(graph[1].cpu().numpy()), ccc.bits(new_score))


# ------------------------------------------------------------------ find ----
def test_find_in_both_orders_absent_pairs_rows_out_of_range_and_equal_rows():
    from merizo_search_amd import ops
    n = 300
    idx, score, lengths = cc.random_lists(n, 7, seed=17)
    got, _graph, ws = _check_set(idx, score, None, None, None, lengths)
    count = got.shape[0]
    slots = np.arange(count)
    assert np.array_equal(ops.cluster_pairs_find(got[:, 0], got[:, 1], lengths, ws).cpu().numpy(), slots)
    assert np.array_equal(ops.cluster_pairs_find(got[:, 1], got[:, 0], lengths, ws).cpu().numpy(), slots)
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.integers(0, n, 2000), [-1, n, 1 << 40, 5, 5, 0]]).astype(np.int64)
    b = np.concatenate([rng.integers(0, n, 2000), [3, 3, 3, 5, -7, n + 2]]).astype(np.int64)
    want = ct.pairs_find_np(a, b, lengths, got)
    assert (want >= 0).any() and (want[:2000] == -1).sum() > 1000 and (want[2000:] == -1).all()
    assert np.array_equal(ops.cluster_pairs_find(a, b, lengths, ws).cpu().numpy(), want)
    assert ops.cluster_pairs_find(a[:0], b[:0], lengths, ws).shape == (0,)
    # a workspace that holds the set of a graph of another n finds nothing
    assert (ops.cluster_pairs_find(got[:, 0] % 10, got[:, 1] % 10, lengths[:10], ws).cpu().numpy() == -1).all()


# ------------------------------------------------------------------ refusals, through ops ----
def test_what_the_ops_refuse():
    import torch
    from merizo_search_amd import ops
    from merizo_search_amd._lib import MerizoHipError
    n, k = 100, 4
    idx, score, lengths = cc.random_lists(n, k, seed=3)
    d_idx, d_score = _dev(idx), _dev(score)
    pairs, counts, ws = ops.cluster_pairs(d_idx, d_score, None, None, None, lengths, CUT, COV)
    keep = torch.ones(int(counts[0].item()), dtype=torch.uint8, device="cuda")
    with pytest.raises(MerizoHipError, match="workspace"):
        ops.cluster_pairs(d_idx, d_score, None, None, None, lengths, CUT, COV, workspace=ws[:ws.numel() - 1])
    with pytest.raises(MerizoHipError, match="workspace"):
        ops.cluster_pairs_apply(d_idx, d_score, None, None, None, lengths, CUT, COV, keep, ws[:ws.numel() - 1])
    with pytest.raises(MerizoHipError, match="workspace"):
        ops.cluster_pairs_apply(d_idx, d_score, None, None, None, lengths, CUT, COV, keep, None)
    with pytest.raises(MerizoHipError, match="workspace"):
        ops.cluster_pairs_find([0], [1], lengths, ws[:100])
    with pytest.raises(MerizoHipError, match="16-byte aligned"):
        ops.cluster_pairs(d_idx, d_score, None, None, None, lengths, CUT, COV, workspace=torch.empty(ws.numel() + 8, dtype=torch.uint8, device="cuda")[8:])
    with pytest.raises(MerizoHipError, match="lengths"):
        ops.cluster_pairs(d_idx, d_score, None, None, None, np.zeros(n + 1, np.int32), CUT, COV)
    with pytest.raises(MerizoHipError, match="mincov"):
        ops.cluster_pairs(d_idx, d_score, None, None, None, lengths, CUT, 1.5)
    with pytest.raises(MerizoHipError, match="NaN"):
        ops.cluster_pairs(d_idx, d_score, None, None, None, lengths, float("nan"), COV)
    with pytest.raises(MerizoHipError, match="cap"):
        ops.cluster_pairs(d_idx, d_score, None, None, None, lengths, CUT, COV, cap=-1)
    with pytest.raises(MerizoHipError, match="go together"):
        ops.cluster_pairs(d_idx, None, None, None, None, lengths, CUT, COV)
    with pytest.raises(MerizoHipError, match="keep"):
        ops.cluster_pairs_apply(d_idx, d_score, None, None, None, lengths, CUT, COV, keep.cpu(), ws)
    with pytest.raises(MerizoHipError, match="keep"):
        ops.cluster_pairs_apply(d_idx, d_score, None, None, None, lengths, CUT, COV, keep.to(torch.int32), ws)
    with pytest.raises(MerizoHipError, match="b:"):
        ops.cluster_pairs_find([0, 1], [1], lengths, ws)
    with pytest.raises(MerizoHipError, match="2\\^31"):               # (n k + m >= 2^31: refused before anything of that size exists)
        ops._pairs_workspace("cluster_pairs", 1 << 30, 2, 0, None, ws.device)
    # nothing above touched the lists
    assert np.array_equal(d_idx.cpu().numpy(), idx)
