"""The list merges and the sample bound on crafted lists (tests/merge_case.py), through the two test hooks of the library.

Every search answer passes through one of these kernels, and which one depends on the list count P that a search derives from the
card and the batch: here P, k, the layout and the lists themselves are chosen, the launch is the one a search makes for that (P, k)
(ms_debug_merge_lists calls launch_merge unchanged), and every output word -- rows, score BITS, the bound of the next pass, the
canaries around them -- is compared with a plain sort.  No tolerance anywhere."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import merge_case as mc

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROW_OFFSET = (1 << 33) + 5


@pytest.fixture(scope="module")
def gpu():
    import torch
    from merizo_search_amd import _lib
    _lib.require_gpu()
    return torch, _lib.load()


# ---- workgroup merge: P <= 256 ------------------------------------------------------------------------------------------------
WG_PAIRS = [(1, 1), (2, 1), (64, 1), (256, 1),
            (1, 2), (2, 2), (3, 2), (65, 2),
            (2, 3), (4, 3), (127, 3),
            (3, 4), (4, 4), (129, 4),
            (5, 5), (6, 5), (255, 5),
            (9, 10), (10, 10), (11, 10), (63, 10), (64, 10), (65, 10), (128, 10), (256, 10),
            (16, 16), (17, 16), (256, 16),
            (16, 17), (17, 17), (18, 17), (129, 17), (255, 17),
            (20, 20), (127, 20), (256, 20),
            (32, 32), (128, 32),
            (33, 33), (255, 33),
            (63, 63), (64, 63), (255, 63),
            (63, 64), (64, 64), (65, 64), (128, 64), (256, 64)]


def test_the_pairs_cover_both_stagings():
    assert any(P * k % 4 == 0 for P, k in WG_PAIRS) and any(P * k % 4 != 0 for P, k in WG_PAIRS)
    assert {(256, 64), (255, 63), (1, 2), (2, 2), (9, 10), (10, 10), (63, 64), (64, 64)} <= set(WG_PAIRS)
    assert all(P <= 256 for P, _k in WG_PAIRS)


@pytest.mark.parametrize("P,k", WG_PAIRS)
def test_workgroup_merge_on_every_family(gpu, P, k):
    """ms_block_merge_kernel: the threshold merge and, where it declines (P < k, no k-th head, more than 256 survivors), the
    head-advance merge of its first wave; vector staging (k P a multiple of 4), scalar staging, stream-major lists."""
    torch, lib = gpu
    for b, (names, S, I) in enumerate(mc.family_batches(P, k, seed=17 * P + k)):
        mc.check_merge(torch, lib, names, S, I, what=f"P={P} k={k}", layout="rank", row_offset=ROW_OFFSET, with_ub=True)
        mc.check_merge(torch, lib, names, S, I, what=f"P={P} k={k}", layout="stream", row_offset=b, with_ub=b % 2 == 1)


# ---- more than 256 lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,k", [(257, 10), (257, 63), (320, 20), (512, 32), (513, 10), (1024, 1), (1024, 16)])
def test_head_advance_merge_beyond_256_lists(gpu, P, k):
    """ms_head_merge_kernel<8> and <16>, as a search picks them: k P entries within 128 KiB of LDS ((512, 32) and (1024, 16):
    exactly)."""
    torch, lib = gpu
    assert P > 256 and k * P * 8 <= 128 * 1024
    for b, (names, S, I) in enumerate(mc.family_batches(P, k, seed=3 * P + k)):
        mc.check_merge(torch, lib, names, S, I, what=f"P={P} k={k}", row_offset=ROW_OFFSET, with_ub=b != 1)


@pytest.mark.parametrize("P,k", [(257, 64), (600, 40), (1024, 17), (1024, 64)])
def test_pool_merge_beyond_256_lists(gpu, P, k):
    """ms_partial_merge_kernel with up to four list heads per thread, as a search picks it: k P entries beyond 128 KiB."""
    torch, lib = gpu
    assert P > 256 and k * P * 8 > 128 * 1024
    for b, (names, S, I) in enumerate(mc.family_batches(P, k, seed=5 * P + k)):
        mc.check_merge(torch, lib, names, S, I, what=f"P={P} k={k}", row_offset=ROW_OFFSET, with_ub=b != 1)


def _untouched(out):
    _rc, out_s, out_i, ub_s, ub_i = out
    return (np.all(out_s == mc.CANARY_S.view(np.uint32)) and np.all(out_i == mc.CANARY_I) and np.all(ub_s == mc.CANARY_UB_S.view(np.uint32))
            and np.all(ub_i == mc.CANARY_UB_I))


def test_what_the_merge_launch_declines(gpu):
    torch, lib = gpu
    names, S, I = mc.family_batches(1025, 2, seed=1, names=["random", "short", "tied_kth"])[0]
    out = mc.run_merge(torch, lib, S, I)
    assert out[0] == -4 and b"exceed the merge limit" in lib.ms_last_error() and _untouched(out)
    names, S, I = mc.family_batches(257, 10, seed=1, names=["random", "short", "tied_kth"])[0]
    out = mc.run_merge(torch, lib, S, I, layout="stream")
    assert out[0] == -4 and b"need the block merge" in lib.ms_last_error() and _untouched(out)
    out = mc.run_merge(torch, lib, S, I, dp=(3, 257), qmap=[2, 0, 1], launch=(3, 257))
    assert out[0] == -4 and b"needs the block merge" in lib.ms_last_error() and _untouched(out)


# ---- sparse pool --------------------------------------------------------------------------------------------------------------
SPARSE_TOTALS = (0, -1, -2, 100, 511, 512, 513, 2000)           # (-1: k - 1, -2: k)


def _sparse_batch(k, seed):
    P = 256
    cases = []
    for j, t in enumerate(SPARSE_TOTALS):
        total = {-1: k - 1, -2: k}.get(t, t)
        S, I = mc.sparse_total(P, k, seed + j, total, lens_first=(3, 4, 5, k) if total >= 100 else ())
        mc.check_contract(S, I, k)
        assert int((I != mc.NONE).sum()) == total
        cases.append((f"sparse_total_{total}", S, I))
    return [c[0] for c in cases], np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])


@pytest.mark.parametrize("k", [10, 20, 32, 64])
def test_sparse_pool_merge(gpu, k):
    """sparse = 1 on stream-major lists, as the prefiltered search calls it: up to 512 entries rank themselves in the pool, more
    take the general merge -- the same answer either side of the switch.  With ub_s the launch is the general merge."""
    torch, lib = gpu
    names, S, I = _sparse_batch(k, seed=40 + k)
    mc.check_merge(torch, lib, names, S, I, what=f"sparse k={k}", layout="stream", sparse=1, with_ub=False, row_offset=ROW_OFFSET)
    mc.check_merge(torch, lib, names, S, I, what=f"sparse k={k}", layout="rank", sparse=1, with_ub=False)
    mc.check_merge(torch, lib, names, S, I, what=f"sparse k={k} + ub", layout="stream", sparse=1, with_ub=True)
    for b, (names, S, I) in enumerate(mc.family_batches(256, k, seed=k)):          # dense lists: the pool overflows
        mc.check_merge(torch, lib, names, S, I, what=f"sparse k={k}", layout="stream", sparse=1, with_ub=False, row_offset=b)


@pytest.mark.parametrize("k", [10, 64])
def test_sparse_pool_reads_ranks_from_4_only_behind_an_occupied_fourth(gpu, k):
    """A list of exactly 3 entries and one of exactly 4: every thread fetches four ranks at once and walks on only where the fourth
    is occupied.  Stale slots from rank 4 on behind an EMPTY fourth (left here on purpose; a pool that walked on would collect them,
    they outscore everything) are not read; the list of 4 and the longer ones are read to their end."""
    torch, lib = gpu
    P = 256
    S, I = mc.sparse_total(P, k, 77, 100, lens_first=(3, 4, 5, k))
    mc.check_contract(S, I, k)
    assert [(I[l] != mc.NONE).sum() for l in range(4)] == [3, 4, 5, k]
    S3, I3 = np.stack([S] * 3), np.stack([I] * 3)
    want = mc.expected_merge(S3, I3, k, 0, [0, 1, 2], 3, False)
    Sp, Ip = S3.copy(), I3.copy()
    Sp[:, 0, 4:] = mc.FMAX
    Ip[:, 0, 4:] = 424242 + np.arange(k - 4, dtype=np.uint32)
    rc, *got = mc.run_merge(torch, lib, Sp, Ip, layout="stream", sparse=1, with_ub=False)
    assert rc == 0
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- device plan and qmap -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 20])
@pytest.mark.parametrize("dp_nq", [1, 5, 8])
@pytest.mark.parametrize("dp_P", [0, 100, 256])
def test_device_plan_and_qmap(gpu, k, dp_nq, dp_P):
    """The merge behind the exact pass of a prefiltered search: launched for 8 queries of 256 lists, it merges the dp_nq queries of
    dp_P lists (0: k lists) its device plan names, laid out with dp_P, into the output rows qmap names -- and writes no other row."""
    torch, lib = gpu
    dp_P = dp_P or k
    names = ["random", "tied_kth", "top_heavy", "short", "empty", "late_wave_last", "one_list_last", "all_equal_blocked"][:dp_nq]
    S = np.zeros((dp_nq, dp_P, k), np.float32)
    I = np.zeros((dp_nq, dp_P, k), np.uint32)
    for q, name in enumerate(names):
        S[q], I[q] = mc.FAMILIES[name](dp_P, k, 50 + q)
        mc.check_contract(S[q], I[q], k)
    qmap = np.random.default_rng(dp_nq * 1000 + dp_P).permutation(8)[:dp_nq].tolist()
    for with_ub in (True, False):
        mc.check_merge(torch, lib, names, S, I, what=f"dp_nq={dp_nq} dp_P={dp_P} k={k}", dp=(dp_nq, dp_P), qmap=qmap, launch=(8, 256),
                       row_offset=ROW_OFFSET, with_ub=with_ub)
    mc.check_merge(torch, lib, names, S, I, what=f"dp_nq={dp_nq} dp_P={dp_P} k={k} no qmap", dp=(dp_nq, dp_P), launch=(8, 256))


# ---- the other forms at P <= 256: a child process per setting -------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"MS_BLOCK_MERGE": "0"}, {"MS_BLOCK_MERGE": "0", "MS_HEAD_MERGE": "0"}])
def test_head_advance_and_pool_merge_at_small_list_counts(env):
    """MS_BLOCK_MERGE=0: ms_head_merge_kernel<1|2|4> at P in {1, 63, 64, 65, 128, 129, 256}; with MS_HEAD_MERGE=0 as well:
    ms_partial_merge_kernel there.  The switches are read once per process, hence a fresh child (merge_case.py: child_main)."""
    assert {P for P, _k in mc.CHILD_PAIRS} == {1, 63, 64, 65, 128, 129, 256}
    r = subprocess.run([sys.executable, os.path.join(TESTS, "merge_case.py"), "child"], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "merge child ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


# ---- public k-way merges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_lists,k", [(1, 1), (1, 10), (2, 10), (63, 10), (64, 64), (64, 3), (65, 10), (65, 33), (200, 10), (200, 20)])
def test_topk_merge_and_its_strided_form(gpu, S_lists, k):
    """ms_topk_merge / ms_topk_merge_strided on the same families re-packed as [S, nq, k] float32 / int64 lists ((-inf, -1) padding,
    some lists padding from slot 0): the kernel for up to 64 lists and the one beyond."""
    torch, lib = gpu
    from merizo_search_amd._lib import current_stream
    padded_from_slot_0 = False
    for names, S, I in mc.family_batches(S_lists, k, seed=S_lists + k):
        nq = len(names)
        sc = np.ascontiguousarray(S.transpose(1, 0, 2))                                           # [S, nq, k]
        ix = np.ascontiguousarray(np.where(I == mc.NONE, -1, I.astype(np.int64)).transpose(1, 0, 2))
        padded_from_slot_0 |= bool(np.any(ix[:, :, 0] < 0))
        want_s = np.full(nq * k + mc.GUARD, mc.CANARY_S, np.float32).view(np.uint32)
        want_i = np.full(nq * k + mc.GUARD, mc.CANARY_I, np.int64)
        for q in range(nq):
            want_s[q * k:q * k + k], want_i[q * k:q * k + k], _us, _ui = mc.merge_ref(S[q], I[q], k)
        # dense
        outs = []
        d_sc, d_ix = mc._dev(torch, sc), mc._dev(torch, ix)
        d_os = mc._dev(torch, np.full(nq * k + mc.GUARD, mc.CANARY_S, np.float32))
        d_oi = mc._dev(torch, np.full(nq * k + mc.GUARD, mc.CANARY_I, np.int64))
        assert lib.ms_topk_merge(d_sc.data_ptr(), d_ix.data_ptr(), S_lists, nq, k, d_os.data_ptr(), d_oi.data_ptr(), current_stream()) == 0
        torch.cuda.synchronize()
        outs.append(("dense", mc._host(d_os, np.uint32), mc._host(d_oi, np.int64)))
        # strided: one packed block per list, [scores | pad to 8 bytes | rows | 24 spare bytes]
        s_bytes = (nq * k * 4 + 7) // 8 * 8
        block = s_bytes + nq * k * 8 + 24
        buf = np.full(S_lists * block, 0xEE, np.uint8)
        for s in range(S_lists):
            buf[s * block:s * block + nq * k * 4] = sc[s].reshape(-1).view(np.uint8)
            buf[s * block + s_bytes:s * block + s_bytes + nq * k * 8] = ix[s].reshape(-1).view(np.uint8)
        d_buf = mc._dev(torch, buf)
        d_os2 = mc._dev(torch, np.full(nq * k + mc.GUARD, mc.CANARY_S, np.float32))
        d_oi2 = mc._dev(torch, np.full(nq * k + mc.GUARD, mc.CANARY_I, np.int64))
        assert d_buf.data_ptr() % 8 == 0
        assert lib.ms_topk_merge_strided(d_buf.data_ptr(), d_buf.data_ptr() + s_bytes, block, block, S_lists, nq, k, d_os2.data_ptr(),
                                         d_oi2.data_ptr(), current_stream()) == 0
        torch.cuda.synchronize()
        outs.append(("strided", mc._host(d_os2, np.uint32), mc._host(d_oi2, np.int64)))
        for form, got_s, got_i in outs:
            bad = np.flatnonzero((got_s != want_s) | (got_i != want_i))
            assert bad.size == 0, (form, S_lists, k, names[min(int(bad[0]) // k, nq - 1)], int(bad[0]) % k)
    assert padded_from_slot_0


# ---- sample bound -------------------------------------------------------------------------------------------------------------
# (P, ranks, k): ranks * P two or three times at every count either side of a switch of values per lane (4 | 8 | 16 | 32 per lane at
# 256 | 512 | 1024 values) and of a lane's first second value (64), ranks <= k
BOUND_CASES = [(1, 1, 1), (1, 1, 5), (63, 1, 1), (21, 3, 3), (64, 1, 2), (16, 4, 4), (65, 1, 10), (13, 5, 5), (255, 1, 3), (51, 5, 20),
               (256, 1, 10), (128, 2, 2), (64, 4, 64), (257, 1, 4), (257, 1, 2), (511, 1, 5), (73, 7, 10), (256, 2, 10), (128, 4, 20), (513, 1, 64),
               (171, 3, 3), (341, 3, 20), (1023, 1, 1), (256, 4, 5), (512, 2, 64), (205, 5, 10), (1025, 1, 2), (2047, 1, 20),
               (89, 23, 64), (256, 8, 10), (32, 64, 64), (2048, 1, 4),
               # a lane's sixth, seventh and eighth value decide (value set lane_pops_8 with k = 6, 7, 8: the tail of the 8-value network)
               (257, 1, 6), (300, 1, 7), (512, 1, 8), (64, 6, 6), (73, 7, 7), (64, 8, 8), (128, 4, 6), (100, 5, 7),
               # ... and its third and fourth of four (lane_pops_4 with k = 3, 4)
               (200, 1, 3), (256, 1, 4), (40, 4, 4), (85, 3, 3)]


def test_the_bound_cases_sit_on_both_sides_of_every_switch():
    counts = [P * r for P, r, _k in BOUND_CASES]
    for c in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048):
        assert counts.count(c) >= 2, c
    assert {k for _P, _r, k in BOUND_CASES} >= {1, 2, 3, 4, 5, 10, 20, 64} and all(r <= k for _P, r, k in BOUND_CASES)


@pytest.mark.parametrize("P,ranks,k", BOUND_CASES)
def test_sample_bound_on_every_value_set(gpu, P, ranks, k):
    """ms_sample_bound_kernel<4|8|16|32>: lb == the k-th largest with multiplicity (compared with ==: either zero is right), in
    both layouts, with and without the histogram outputs; nothing behind nq or behind `ranks` is touched or read.
    The bucket width hstep is asserted where it is determined: finite and >= 0; 0 without a bound or with best == k-th; > 0 when
    best - k-th >= 1e-3; for k < 4 exactly float32(best - kth) * float32(1 / 12).  For k >= 4 it goes through __logf (the slope of
    the sample's tail) and only steers the speed of the scan behind it, never a result: no value is asserted there."""
    torch, lib = gpu
    names, S = mc.bound_batch(P, k, ranks, seed=P + 7 * ranks + k)
    nq = len(names)
    want = [mc.bound_ref(S[q], k, ranks) for q in range(nq)]
    for layout, with_hist in (("rank", False), ("rank", True), ("stream", True)):
        rc, lb, hist, hstep = mc.run_bound(torch, lib, S, k, ranks, layout=layout, with_hist=with_hist)
        assert rc == 0, lib.ms_last_error()
        for q in range(nq):
            assert lb[q] == want[q], (layout, names[q], float(lb[q]), float(want[q]))
        assert np.all(lb[nq:] == mc.CANARY_LB)
        assert np.all(hist[nq * 16:] == mc.CANARY_HIST) and np.all(hstep[nq:] == mc.CANARY_HSTEP)
        if not with_hist:
            assert np.all(hist == mc.CANARY_HIST) and np.all(hstep == mc.CANARY_HSTEP)
            continue
        assert np.all(hist[:nq * 16] == 0)
        for q in range(nq):
            assert np.isfinite(hstep[q]) and hstep[q] >= 0, (layout, names[q], float(hstep[q]))
            exact = mc.hstep_ref(S[q], k, ranks)
            if exact is not None:
                assert hstep[q] == exact, (layout, names[q], float(hstep[q]), float(exact))
            elif S[q, :, :ranks].max() - want[q] >= 1e-3:
                assert hstep[q] > 0, (layout, names[q])


def _fake(n=1):
    return [ctypes.c_void_p(4096 * (j + 1)) for j in range(n)]


def test_sample_bound_range_answers(gpu):
    _torch, lib = gpu
    a, b = _fake(2)
    for P, ranks, k in ((2049, 1, 1), (683, 3, 3), (10, 11, 10), (10, 0, 10), (10, -1, 10)):
        assert lib.ms_debug_sample_bound(a, P, 3, k, ranks, 0, b, None, None, None) == -4, (P, ranks, k)
        assert b"ms_debug_sample_bound" in lib.ms_last_error()


def test_argument_checks_of_both_hooks(gpu):
    _torch, lib = gpu
    ps, pi, os_, oi, us, ui = _fake(6)

    def merge(part_s=ps, part_i=pi, P=4, nq=3, k=10, out_s=os_, out_i=oi, stride=15, ub_s=None, ub_i=None, qmap=None, scratch=None, dp=(0, 0)):
        return lib.ms_debug_merge_lists(part_s, part_i, P, nq, k, 0, 0, 0, out_s, out_i, stride, 2, ub_s, ub_i, dp[0], dp[1], qmap, scratch, None)

    for bad in (dict(part_s=None), dict(part_i=None), dict(out_s=None), dict(out_i=None), dict(ub_s=us), dict(ub_i=ui), dict(k=0), dict(k=65),
                dict(nq=0), dict(P=0), dict(stride=11), dict(part_s=ctypes.c_void_p(4100)), dict(qmap=us), dict(scratch=us, dp=(4, 4)),
                dict(scratch=us, dp=(3, 5)), dict(scratch=us, dp=(0, 4))):
        assert merge(**bad) == -1, bad
        assert b"ms_debug_merge_lists" in lib.ms_last_error(), bad

    def bound(part_s=ps, P=4, nq=3, k=10, lb=os_, hist=None, hstep=None):
        return lib.ms_debug_sample_bound(part_s, P, nq, k, 1, 0, lb, hist, hstep, None)

    for bad in (dict(part_s=None), dict(lb=None), dict(hist=us), dict(hstep=us), dict(k=0), dict(k=65), dict(nq=0), dict(P=0)):
        assert bound(**bad) == -1, bad
        assert b"ms_debug_sample_bound" in lib.ms_last_error(), bad
