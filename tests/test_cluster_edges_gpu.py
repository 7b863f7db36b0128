"""ms_cluster_greedy_edges on the GPU against its restatement (cluster_case.cluster_greedy_np on lists widened by the extra
entries): random lists plus random extras with the same garbage mix, m = 0 byte-equal to ms_cluster_greedy, edges only (k = 0) on
the two stars, one set of entries split arbitrarily between lists and extras, and guard zones."""
import numpy as np
import pytest

import cluster_case as cc
import cluster_complete_case as ccc

pytestmark = pytest.mark.gpu
NINF = -np.inf


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu(idx, score, src, dst, esc, lengths, min_score, mincov, **kw):
    from merizo_search_amd import ops
    rep, rep_score, info = ops.cluster_greedy_edges(_dev(idx), _dev(score), _dev(src), _dev(dst), _dev(esc), lengths, min_score, mincov, **kw)
    return rep.cpu().numpy(), rep_score.cpu().numpy(), info


def _same(a, b, rounds=True):
    assert np.array_equal(a[0], b[0]) and np.array_equal(ccc.bits(a[1]), ccc.bits(b[1]))
    keys = ("n_reps", "saturated") + (("rounds",) if rounds else ())
    assert {k: a[2][k] for k in keys} == {k: b[2][k] for k in keys}, (a[2], b[2])


# ------------------------------------------------------------------ random lists plus random extras ----
@pytest.mark.parametrize("n,k", [(1, 1), (65, 5), (257, 20), (1000, 20)])
def test_lists_plus_random_extras_equal_the_restatement(n, k):
    idx, score, lengths = cc.random_lists(n, k, seed=2000 * n + k)
    src, dst, esc = ccc.random_extras(n, 3 * n, idx, score, seed=n + 1)
    assert n < 60 or ((src >= n).any() and (src < 0).any() and (dst >= n).any() and (dst < 0).any() and np.isnan(esc).any() and (src == dst).any())
    for cut, cov in ((float(cc.CUT), 0.7), (NINF, 0.0)):
        want = ccc.cluster_greedy_edges_np(idx, score, src, dst, esc, lengths, cut, cov)
        got = _gpu(idx, score, src, dst, esc, lengths, cut, cov)
        _same(got, want, rounds=False)
        assert 1 <= got[2]["rounds"] <= n
        # the extras matter: without them the answer is another one (on the larger graphs)
        if n >= 257:
            assert not np.array_equal(cc.cluster_greedy_np(idx, score, lengths, cut, cov)[0], want[0])


# ------------------------------------------------------------------ m = 0 ----
@pytest.mark.parametrize("n,k", [(1, 1), (65, 5), (1000, 20)])
def test_no_extras_is_ms_cluster_greedy_byte_for_byte(n, k):
    import torch
    from merizo_search_amd import ops
    idx, score, lengths = cc.random_lists(n, k, seed=31 * n + k)
    a = ops.cluster_greedy(_dev(idx), _dev(score), lengths, float(cc.CUT), 0.7)
    a = (a[0].cpu().numpy(), a[1].cpu().numpy(), a[2])
    _same(_gpu(idx, score, None, None, None, lengths, float(cc.CUT), 0.7), a)
    empty = (torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
             torch.empty(0, dtype=torch.float32, device="cuda"))
    b = ops.cluster_greedy_edges(_dev(idx), _dev(score), *empty, lengths, float(cc.CUT), 0.7)
    _same((b[0].cpu().numpy(), b[1].cpu().numpy(), b[2]), a)
    _same(a, cc.cluster_greedy_np(idx, score, lengths, cc.CUT, 0.7), rounds=False)


# ------------------------------------------------------------------ k = 0: the two stars as extras only ----
LEAVES = 5000


def test_star_given_only_as_extra_entries_in_both_directions():
    from merizo_search_amd import ops
    n, hub = LEAVES + 1, 17
    leaves = np.array([r for r in range(n) if r != hub], np.int64)
    w = (0.5 + 0.0625 * (leaves % 7)).astype(np.float32)
    hubs = np.full(LEAVES, hub, np.int64)
    lengths = np.full(n, 80, np.int32)
    for hub_len in (100, 60):
        lengths[hub] = hub_len
        idx, score = cc.empty_lists(n, 1)                                  # the reference: the leaves' lists, through ms_cluster_greedy
        idx[leaves, 0], score[leaves, 0] = hub, w
        ref = ops.cluster_greedy(_dev(idx), _dev(score), lengths, 0.5, 0.7)
        ref = (ref[0].cpu().numpy(), ref[1].cpu().numpy(), dict(ref[2], saturated=0))
        for src, dst in ((leaves, hubs), (hubs, leaves)):                  # leaf -> hub, and hub -> leaf: 5,000 entries of one row
            got = _gpu(None, None, src, dst, w, lengths, 0.5, 0.7)
            _same(got, ref)
        if hub_len == 100:
            assert got[2]["n_reps"] == 1 and (got[0] == hub).all()
        else:
            assert got[2]["n_reps"] == LEAVES and got[0][hub] == 6 and got[1][hub] == np.float32(0.875)
    # no entry at all: every row its own representative after one round
    got = _gpu(None, None, None, None, None, lengths, 0.5, 0.7)
    assert (got[0] == np.arange(n)).all() and got[2] == {"n_reps": n, "rounds": 1, "saturated": 0}


# ------------------------------------------------------------------ one set of entries, split arbitrarily ----
def test_entries_split_between_lists_and_extras_give_identical_outputs():
    n, k = 1000, 20
    idx, score, lengths = cc.random_lists(n, k, seed=55)
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], (n, k))
    whole = _gpu(idx, score, None, None, None, lengths, float(cc.CUT), 0.7)
    rng = np.random.default_rng(56)
    for share in (0.0, 0.3, 1.0):
        out = rng.random((n, k)) < share                                   # these entries leave the lists and come back as extras
        p_idx, p_score = np.where(out, -1, idx), np.where(out, np.float32(NINF), score).astype(np.float32)
        order = rng.permutation(int(out.sum()))
        src, dst, esc = rows[out][order], idx[out][order], score[out][order]
        got = _gpu(p_idx, p_score, src, dst, esc, lengths, float(cc.CUT), 0.7) if share < 1.0 else _gpu(None, None, src, dst, esc, lengths, float(cc.CUT), 0.7)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(ccc.bits(got[1]), ccc.bits(whole[1]))
        assert got[2]["n_reps"] == whole[2]["n_reps"] and got[2]["rounds"] == whole[2]["rounds"]


# ------------------------------------------------------------------ guard zones ----
@pytest.mark.parametrize("n,k", [(1, 1), (65, 5), (1000, 20)])
def test_guard_zones_around_outputs_and_workspace_stay_untouched(n, k):
    import torch
    from merizo_search_amd import ops
    from merizo_search_amd._lib import MerizoHipError
    idx, score, lengths = cc.random_lists(n, k, seed=77 + n)
    src, dst, esc = ccc.random_extras(n, 3 * n, idx, score, seed=78 + n)
    need = int(ops._lib.load().ms_cluster_workspace_bytes(n))
    G = 256
    rep_buf = torch.full((n + 2 * G,), -77, dtype=torch.int64, device="cuda")
    score_buf = torch.full((n + 2 * G,), -77.0, dtype=torch.float32, device="cuda")
    ws_buf = torch.full((need + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    rep, rep_score, _info = _gpu(idx, score, src, dst, esc, lengths, float(cc.CUT), 0.7, out=(rep_buf[G:G + n], score_buf[G:G + n]),
                                 workspace=ws_buf[G:G + need])
    want = ccc.cluster_greedy_edges_np(idx, score, src, dst, esc, lengths, cc.CUT, 0.7)
    assert np.array_equal(rep, want[0]) and np.array_equal(ccc.bits(rep_score), ccc.bits(want[1]))
    assert np.array_equal(rep_buf[G:G + n].cpu().numpy(), want[0])
    for buf, fill in ((rep_buf, -77), (score_buf, -77.0), (ws_buf, 0x5A)):
        assert bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())
    with pytest.raises(MerizoHipError, match="workspace"):
        _gpu(idx, score, src, dst, esc, lengths, 0.5, 0.7, workspace=ws_buf[:need - 1])
    with pytest.raises(MerizoHipError, match="one length"):
        _gpu(idx, score, src, dst[:-1], esc, lengths, 0.5, 0.7)
    with pytest.raises(MerizoHipError, match="go together"):
        _gpu(idx, None, src, dst, esc, lengths, 0.5, 0.7)
