"""CPU checks of tests/merge_case.py: the restatements against brute force, the families against the list contract, the packers
against each other.  What test_merge_gpu.py compares the kernels with has to be right first."""
import numpy as np
import pytest

import merge_case as mc


def _brute_merge(S, I, k, row_offset):
    occ = I != mc.NONE
    sc, rows = S[occ], I[occ].astype(np.int64)
    order = np.lexsort((rows, -(sc.astype(np.float64) + 0.0)))[:k]
    out_s = np.full(k, -np.inf, np.float32)
    out_i = np.full(k, -1, np.int64)
    out_s[:order.size] = sc[order]
    out_i[:order.size] = rows[order] + row_offset
    full = order.size == k
    return out_s.view(np.uint32), out_i, (sc[order[-1]].view(np.uint32) if full else np.uint32(0xFF800000)), (rows[order[-1]] if full else mc.NONE)


def test_merge_ref_equals_a_brute_force_lexsort_on_200_random_cases():
    rng = np.random.default_rng(11)
    for case in range(200):
        P, k = int(rng.integers(1, 40)), int(rng.integers(1, 65))
        S, I = mc.random(P, k, seed=case)
        mc.check_contract(S, I, k)
        off = int(rng.integers(0, 1 << 40))
        s, i, us, ui = mc.merge_ref(S, I, k, off)
        bs, bi, bus, bui = _brute_merge(S, I, k, off)
        assert np.array_equal(s, bs) and np.array_equal(i, bi) and int(us) == int(bus) and int(ui) == int(bui), case


def test_merge_ref_orders_zeros_by_row_and_keeps_their_sign():
    S, I = mc.lists_from_entries(3, 2, [0, 1, 2, 2], [0.0, -0.0, -0.0, 1.0], [7, 3, 5, 9])
    mc.check_contract(S, I, 2)
    s, i, us, ui = mc.merge_ref(S, I, 3, 10)
    assert i.tolist() == [19, 13, 15] and s.tolist() == [0x3F800000, 0x80000000, 0x80000000] and (int(us), int(ui)) == (0x80000000, 5)
    s, i, us, ui = mc.merge_ref(S, I, 5, 0)
    assert i.tolist() == [9, 3, 5, 7, -1] and s[3] == 0 and s[4] == 0xFF800000 and (int(us), int(ui)) == (0xFF800000, mc.NONE)


def test_bound_ref_equals_np_sort():
    rng = np.random.default_rng(5)
    for case in range(200):
        P, k = int(rng.integers(1, 50)), int(rng.integers(1, 65))
        ranks = int(rng.integers(1, k + 1))
        _names, S = mc.bound_batch(P, k, ranks, seed=case)
        for q in range(S.shape[0]):
            v = np.sort(np.concatenate([S[q, :, :ranks].reshape(-1), np.full(k, -np.inf, np.float32)]))[::-1]
            assert mc.bound_ref(S[q], k, ranks) == v[k - 1], (case, q)


@pytest.mark.parametrize("P", [1, 64, 257])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_every_family_obeys_the_list_contract(P, k):
    seen = 0
    for names, S, I in mc.family_batches(P, k, seed=3):          # (family_batches asserts the contract itself)
        assert 3 <= len(names) <= 9 and S.shape == (len(names), P, k) == I.shape
        for q in range(len(names)):
            mc.check_contract(S[q], I[q], k)
        seen += len(names)
    assert seen >= len(mc.FAMILIES)
    for total in (0, k - 1, k, 100, 511, 512, 513, 2000):
        S, I = mc.sparse_total(P, k, 9, total, lens_first=(3, 4, 5) if P >= 3 and total == 100 else ())
        mc.check_contract(S, I, k)
        assert int((I != mc.NONE).sum()) == min(total, P * k)


def test_the_contract_check_rejects_what_it_should():
    S, I = mc.random(5, 4, 0)
    bad = I.copy(); bad[0, :] = mc.NONE; bad[0, 1] = 99
    with pytest.raises(AssertionError):
        mc.check_contract(np.where(bad == mc.NONE, -np.inf, 1.0).astype(np.float32), bad, 4)          # a hole in a list
    S2, I2 = mc.lists_from_entries(2, 2, [0, 0], [1.0, 2.0], [1, 2])
    with pytest.raises(AssertionError):
        mc.check_contract(S2[:, ::-1].copy(), I2[:, ::-1].copy(), 2)                                      # worst first
    S3, I3 = mc.lists_from_entries(2, 2, [0, 1], [1.0, 2.0], [4, 4])
    with pytest.raises(AssertionError):
        mc.check_contract(S3, I3, 2)                                                                      # a row twice


def test_families_reach_the_shapes_they_are_named_for():
    k, P = 17, 256
    for name, want in (("top_heavy", k * (k - 1) + 1), ("top_heavy_256", 256), ("top_heavy_257", 257)):
        S, I = mc.FAMILIES[name](P, k, 1)
        heads = np.sort(S[:, 0])[::-1]
        assert int((S >= heads[k - 1]).sum()) == want, name               # entries at or above the k-th best head (scores are distinct)
    S, I = mc.tied_kth(64, 10, 2)
    s, _i, _us, _ui = mc.merge_ref(S, I, 10)
    assert int((S == s.view(np.float32)[9]).sum()) >= 3 * 10
    S, I = mc.FAMILIES["late_wave_last"](256, 10, 3)
    assert set(np.argsort(-S[:, 0])[:10].tolist()) == set(range(246, 256))
    names, B = mc.bound_batch(256, 10, 4, seed=0)
    v = B[names.index("lane_pops_8"), :, :4].T.reshape(-1)
    assert len({int(i) % 64 for i in np.argsort(-v)[:8]}) == 1


def test_the_packers_invert_each_other():
    _names, S, I = mc.family_batches(7, 5, seed=1)[0]
    ps, pi = mc.pack_rank_major(S, I)
    assert ps.shape == (S.shape[0], 5, 7) and ps[2, 3, 6] == S[2, 6, 3]
    assert all(np.array_equal(a, b) for a, b in zip(mc.unpack_rank_major(ps, pi), (S, I)))
    pad = S.shape[0] + 3
    ss, si = mc.pack_stream_major(S, I, pad)
    assert ss.shape == (7, pad, 5) and si[6, 2, 3] == I[2, 6, 3] and np.all(si[:, S.shape[0]:] == mc.PAD_I)
    assert all(np.array_equal(a, b) for a, b in zip(mc.unpack_stream_major(ss, si, S.shape[0]), (S, I)))
    # one layout re-packed as the other
    a, b = mc.unpack_stream_major(*mc.pack_stream_major(*mc.unpack_rank_major(ps, pi), pad), S.shape[0])
    assert np.array_equal(a.view(np.uint32), S.view(np.uint32)) and np.array_equal(b, I)
