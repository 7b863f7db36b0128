"""`cluster` on the GPU: ms_cluster_greedy against its sequential numpy restatement -- representatives, assignments, score bits,
counts -- on random graphs full of ties and of entries that are no edges, a dependency chain, the two stars, planted families
over many workgroups; independence of the order inside a list and from run to run; guard zones around outputs and workspace;
and the command end to end on a database of planted families in both layouts."""
import os

import numpy as np
import pytest

import cluster_case as cc

pytestmark = pytest.mark.gpu
NINF = -np.inf


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gpu(idx, score, lengths, min_score, mincov, **kw):
    import torch
    from merizo_search_amd import ops
    rep, rep_score, info = ops.cluster_greedy(torch.from_numpy(idx).cuda(), torch.from_numpy(score).cuda(), lengths, min_score, mincov, **kw)
    return rep.cpu().numpy(), rep_score.cpu().numpy(), info


def _check(idx, score, lengths, min_score, mincov, what=None):
    """The kernel's answer equals the restatement's: out_rep, out_n_reps and out_saturated equal, out_rep_score bit-equal."""
    want_rep, want_score, want = cc.cluster_greedy_np(idx, score, lengths, min_score, mincov)
    rep, rep_score, info = _gpu(idx, score, lengths, min_score, mincov)
    assert rep.dtype == np.int64 and rep_score.dtype == np.float32
    assert np.array_equal(rep, want_rep), what
    assert np.array_equal(_bits(rep_score), _bits(want_score)), what
    assert info["n_reps"] == want["n_reps"] and info["saturated"] == want["saturated"], (what, info, want)
    assert 1 <= info["rounds"] <= idx.shape[0], (what, info)
    return rep, rep_score, info


# ------------------------------------------------------------------ 1. random graphs -------------
@pytest.mark.parametrize("k", [1, 5, 20, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_random_graphs_equal_the_restatement(n, k):
    """Lengths from five values (priority ties), scores from a few (weight ties; the cut and one ulp below it among them), lists
    with padding, self-loops, duplicate rows, rows >= n and NaN scores.  Once with the cut and coverage 0.7 (length 70 against
    100 sits on it), once with neither (then -0.0 and +0.0 are weights that tie)."""
    idx, score, lengths = cc.random_lists(n, k, seed=1000 * n + k)
    assert n * k < 300 or (np.isnan(score).any() and (idx >= n).any() and (idx == -1).any() and (idx == np.arange(n)[:, None]).any())
    _rep, _score, info = _check(idx, score, lengths, float(cc.CUT), 0.7, "cut")
    assert n < 60 or info["saturated"] > 0
    _check(idx, score, lengths, NINF, 0.0, "no cut")


# ------------------------------------------------------------------ 2. a dependency chain --------
def test_a_path_of_strictly_decreasing_lengths_takes_many_rounds():
    """Row i lists i + 1 only and is longer than it: row 2m can become a representative only after 2m - 1 became a member, which
    needs 2m - 2 to be a representative first -- the rounds are a chain, and every one of them still decides a row."""
    n = 300
    idx, score = cc.lists_from_edges(n, 1, [(i, i + 1, 0.9 - 0.001 * i) for i in range(n - 1)])
    lengths = (1000 - np.arange(n)).astype(np.int32)
    rep, _score, info = _check(idx, score, lengths, 0.5, 0.0)
    assert 1 < info["rounds"] <= n
    assert info["n_reps"] == n // 2 and (rep[0::2] == np.arange(0, n, 2)).all()
    # the same path with the edge in the OTHER endpoint's list: the same clusters
    idx2, score2 = cc.lists_from_edges(n, 1, [(i + 1, i, 0.9 - 0.001 * i) for i in range(n - 1)])
    rep2, _s, info2 = _check(idx2, score2, lengths, 0.5, 0.0)
    assert np.array_equal(rep2, rep) and 1 < info2["rounds"] <= n


# ------------------------------------------------------------------ 3. the two stars -------------
LEAVES = 5000


def test_star_whose_edges_are_in_the_leaves_lists():
    """The hub (row 17) is longest and lists nothing: 5,000 leaves find it in their own lists.  And the same lists with the hub
    SHORTEST: 5,000 rows block, cover and assign the one row they all list."""
    n, hub = LEAVES + 1, 17
    leaves = np.array([r for r in range(n) if r != hub])
    idx, score = cc.empty_lists(n, 1)
    idx[leaves, 0] = hub
    score[leaves, 0] = (0.5 + 0.0625 * (leaves % 7)).astype(np.float32)
    lengths = np.full(n, 80, np.int32)
    lengths[hub] = 100
    rep, _score, info = _check(idx, score, lengths, 0.5, 0.7, "hub longest")
    assert info["n_reps"] == 1 and (rep == hub).all() and info["saturated"] == LEAVES
    lengths[hub] = 60
    rep, rep_score, info = _check(idx, score, lengths, 0.5, 0.7, "hub shortest")
    assert info["n_reps"] == LEAVES and rep[hub] == 6 and rep_score[hub] == np.float32(0.875)       # the first leaf with the top score


def test_mirror_star_whose_edges_are_in_the_hubs_list():
    """The hub is shortest and only ITS list has entries, 5,000 of them: the lanes of one row write that row's flags and key;
    every leaf is a representative and the hub goes to the best-scoring leaf, the smaller row on a tie."""
    n, hub = LEAVES + 1, 4000
    leaves = np.array([r for r in range(n) if r != hub])
    idx, score = cc.empty_lists(n, LEAVES)
    rng = np.random.default_rng(5)
    order = rng.permutation(LEAVES)
    idx[hub] = leaves[order]
    score[hub] = (0.5 + 0.0625 * (leaves[order] % 7)).astype(np.float32)
    lengths = np.full(n, 80, np.int32)
    lengths[hub] = 60
    rep, rep_score, info = _check(idx, score, lengths, 0.5, 0.7)
    assert info["n_reps"] == LEAVES and info["saturated"] == 1 and rep[hub] == 6 and rep_score[hub] == np.float32(0.875)
    assert (rep[leaves] == leaves).all()


# ------------------------------------------------------------------ 4. many workgroups -----------
@pytest.fixture(scope="module")
def families():
    """n = 20,000, k = 10: planted families of up to 12 (their lists are cut short by k), and the restatement's answer."""
    idx, score, lengths, family = cc.family_lists(20_000, 10, seed=11)
    return idx, score, lengths, family, cc.cluster_greedy_np(idx, score, lengths, 0.7, 0.7)


def test_planted_families_over_many_workgroups(families):
    idx, score, lengths, family, want = families
    rep, rep_score, info = _gpu(idx, score, lengths, 0.7, 0.7)
    assert np.array_equal(rep, want[0]) and np.array_equal(_bits(rep_score), _bits(want[1]))
    assert info["n_reps"] == want[2]["n_reps"] and info["saturated"] == want[2]["saturated"] > 0
    assert (family[rep] == family).all() and info["n_reps"] >= len(np.unique(family))
    small = np.bincount(family)[family] <= 11                            # families whose lists are complete come back whole
    assert np.array_equal(rep[small], cc.planted_clusters(lengths, family)[small])


# ------------------------------------------------------------------ 5. order independence --------
def test_outputs_do_not_depend_on_the_order_inside_a_list_nor_on_the_run(families):
    import torch
    from merizo_search_amd import ops
    idx, score, lengths, _family, want = families
    rng = np.random.default_rng(6)
    runs = []
    for trial in range(3):
        perm = np.argsort(rng.random(idx.shape), axis=1) if trial else np.broadcast_to(np.arange(idx.shape[1]), idx.shape)
        p_idx, p_score = np.take_along_axis(idx, perm, 1), np.take_along_axis(score, perm, 1)
        runs.append(_gpu(np.ascontiguousarray(p_idx), np.ascontiguousarray(p_score), lengths, 0.7, 0.7))
    runs.append(_gpu(idx, score, lengths, 0.7, 0.7))                       # the first one again
    for rep, rep_score, info in runs:
        assert np.array_equal(rep, want[0]) and np.array_equal(_bits(rep_score), _bits(want[1]))
        assert (info["n_reps"], info["saturated"]) == (want[2]["n_reps"], want[2]["saturated"])
    # a reused workspace that holds another call's state gives the same answer: the call initialises it
    ws = torch.full((int(ops._lib.load().ms_cluster_workspace_bytes(idx.shape[0])),), 0xA5, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        rep, rep_score, _info = _gpu(idx, score, lengths, 0.7, 0.7, workspace=ws)
        assert np.array_equal(rep, want[0]) and np.array_equal(_bits(rep_score), _bits(want[1]))


# ------------------------------------------------------------------ 6. guard zones ---------------
@pytest.mark.parametrize("n,k", [(1, 1), (65, 5), (1000, 20)])
def test_guard_zones_around_outputs_and_workspace_stay_untouched(n, k):
    import torch
    from merizo_search_amd import ops
    from merizo_search_amd._lib import MerizoHipError
    idx, score, lengths = cc.random_lists(n, k, seed=77 + n)
    need = int(ops._lib.load().ms_cluster_workspace_bytes(n))
    G = 256                                                               # guard elements on either side
    rep_buf = torch.full((n + 2 * G,), -77, dtype=torch.int64, device="cuda")
    score_buf = torch.full((n + 2 * G,), -77.0, dtype=torch.float32, device="cuda")
    ws_buf = torch.full((need + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    rep, rep_score, info = ops.cluster_greedy(torch.from_numpy(idx).cuda(), torch.from_numpy(score).cuda(), lengths, float(cc.CUT), 0.7,
                                              out=(rep_buf[G:G + n], score_buf[G:G + n]), workspace=ws_buf[G:G + need])
    assert rep.data_ptr() == rep_buf.data_ptr() + 8 * G
    want = cc.cluster_greedy_np(idx, score, lengths, cc.CUT, 0.7)
    assert np.array_equal(rep.cpu().numpy(), want[0]) and np.array_equal(_bits(rep_score.cpu().numpy()), _bits(want[1]))
    for buf, fill in ((rep_buf, -77), (score_buf, -77.0), (ws_buf, 0x5A)):
        assert bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())
    # and what the op refuses
    with pytest.raises(MerizoHipError, match="workspace"):
        ops.cluster_greedy(torch.from_numpy(idx).cuda(), torch.from_numpy(score).cuda(), lengths, 0.5, 0.7, workspace=ws_buf[:need - 1])
    with pytest.raises(MerizoHipError, match="lengths"):
        ops.cluster_greedy(torch.from_numpy(idx).cuda(), torch.from_numpy(score).cuda(), np.zeros(n + 1, np.int32), 0.5, 0.7)
    with pytest.raises(MerizoHipError):
        ops.cluster_greedy(torch.from_numpy(idx).cuda().int(), torch.from_numpy(score).cuda(), lengths, 0.5, 0.7)
    with pytest.raises(MerizoHipError, match="mincov"):
        ops.cluster_greedy(torch.from_numpy(idx).cuda(), torch.from_numpy(score).cuda(), lengths, 0.5, 1.5)


# ------------------------------------------------------------------ 7. end to end ----------------
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("cluster_gpu"))
    names, lengths, family = cc.write_planted(work)
    return work, names, lengths, family


@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_cli_cluster_returns_the_planted_families(planted, tmp_path, monkeypatch, layout):
    """`cli cluster` on the planted database: the planted clusters, and a TSV that equals the one derived from the restatement
    applied to the neighbour lists the GPU search itself handed to ms_cluster_greedy."""
    from merizo_search_amd import cli
    from merizo_search_amd.foldclass import cluster
    from merizo_search_amd.foldclass.engine import HipEngine
    work, names, lengths, family = planted
    seen = {}
    real = HipEngine.cluster_greedy

    def spy(self, nbr_idx, nbr_score, lens, min_score, mincov=0.0):
        seen.update(idx=nbr_idx.cpu().numpy(), score=nbr_score.cpu().numpy(), lengths=np.asarray(lens), cut=min_score, cov=mincov)
        return real(self, nbr_idx, nbr_score, lens, min_score, mincov)

    monkeypatch.setattr(HipEngine, "cluster_greedy", spy)
    out = str(tmp_path / layout)
    cli.cluster([os.path.join(work, layout), out, str(tmp_path / "t"), "-s", str(cc.PLANTED_MINCOS), "-k", "20", "--query_batchsize", "128",
                 "--output_headers"])
    rows = cc.read_tsv(out + "_cluster.tsv")
    assert rows[0] == ["representative", "member", "emb_score"] and len(rows) == 501
    row_of = {nm: r for r, nm in enumerate(names)}
    want_rep = cc.planted_clusters(lengths, family)
    assert all(want_rep[row_of[member]] == row_of[rep] for rep, member, _ in rows[1:])
    assert sorted(row_of[r[1]] for r in rows[1:]) == list(range(500))
    # the graph the search built: [n,k] lists without the row itself, nothing below the cut, the database's lengths
    assert seen["idx"].shape == (500, 20) and np.array_equal(seen["lengths"], lengths) and seen["cov"] == 0.7
    assert not (seen["idx"] == np.arange(500)[:, None]).any() and (seen["score"][seen["idx"] >= 0] >= np.float32(cc.PLANTED_MINCOS)).all()
    assert ((seen["idx"] >= 0).sum(axis=1) == np.bincount(family)[family] - 1).all()
    rep, rep_score, _info = cc.cluster_greedy_np(seen["idx"], seen["score"], seen["lengths"], seen["cut"], seen["cov"])
    cluster.write_cluster_tsv(out + "_want.tsv", names, rep, rep_score, True)
    assert open(out + "_want.tsv", "rb").read() == open(out + "_cluster.tsv", "rb").read()
