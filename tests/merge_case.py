"""Crafted inputs and plain restatements for the list merges and the sample bound (ms_search.hip, ms_common.h, ms_scan.h).

THE LIST CONTRACT -- what a scan leaves for a merge, and what every family here is asserted against (check_contract):

  * a query has P lists of k slots, 1 <= k <= 64;
  * a list is sorted best first under (score descending, row ascending), where -0.0 == +0.0;
  * empty slots are (-inf, 0xFFFFFFFF) and come only at the end of a list;
  * rows are distinct across all lists of a query (streams are disjoint row ranges) and below 2^31 (larger shards are declined);
  * scores of occupied slots are finite: the scans never emit NaN or +-inf (tests/test_search_gpu.py:
    test_nan_and_inf_rows_are_never_returned), so none are fed here.

A query's lists are a pair (S float32 [P, k], I uint32 [P, k]); a batch stacks them to [nq, P, k].  Two device layouts
(pack_rank_major: [q][rank][list]; pack_stream_major: [list][q][rank] with sm_nq_pad >= nq queries per list).

The operations are exact -- a total order and a k-th largest value -- so the restatements are plain sorts and nothing here has a
tolerance: merge_ref gives score BITS (a -0.0 that wins keeps its sign), bound_ref a value compared with == (either zero is right).

Everything above `# ---- device side` is numpy only.  Below it: thin ctypes wrappers of the two test hooks (ms_debug_merge_lists,
ms_debug_sample_bound) and the runners the GPU tests and their child processes share; `python merge_case.py child` runs CHILD_PAIRS
under whatever MS_BLOCK_MERGE / MS_HEAD_MERGE the parent set (the switches are read once per process) and prints one line.
"""
import heapq
import os
import sys

import numpy as np

NONE = 0xFFFFFFFF
FMAX = np.finfo(np.float32).max
_NEG_INF_BITS = 0xFF800000


# ---- contract ------------------------------------------------------------------------------------------------------------------
def check_contract(S, I, k):
    """Assert the list contract for one query's lists (S, I: [P, k])."""
    assert S.dtype == np.float32 and I.dtype == np.uint32 and S.shape == I.shape and S.ndim == 2 and S.shape[1] == k and 1 <= k <= 64
    occ = I != NONE
    assert np.all(occ[:, :-1] >= occ[:, 1:]), "an occupied slot behind an empty one"
    assert np.all(np.isneginf(S[~occ])), "empty slots carry -inf"
    assert np.all(np.isfinite(S[occ])), "occupied slots carry finite scores"
    rows = I[occ]
    assert rows.size == np.unique(rows).size, "rows repeat"
    assert rows.size == 0 or int(rows.max()) < 2 ** 31
    a_s, b_s, a_i, b_i = S[:, :-1], S[:, 1:], I[:, :-1].astype(np.int64), I[:, 1:].astype(np.int64)
    both = occ[:, 1:]
    assert np.all(~both | (a_s > b_s) | ((a_s == b_s) & (a_i < b_i))), "a list is not sorted best first"


def lists_from_entries(P, k, lid, sc, row):
    """(S, I) [P, k] from loose entries (list, score, row): every list sorted into the contract's order, empty slots behind."""
    lid = np.asarray(lid, np.int64).reshape(-1)
    sc = np.asarray(sc, np.float32).reshape(-1)
    row = np.asarray(row, np.uint32).reshape(-1)
    S = np.full((P, k), -np.inf, np.float32)
    I = np.full((P, k), NONE, np.uint32)
    if lid.size:
        order = np.lexsort((row, -(sc + np.float32(0.0)), lid))
        lid, sc, row = lid[order], sc[order], row[order]
        slot = np.arange(lid.size) - np.searchsorted(lid, lid, side="left")
        assert lid.min() >= 0 and lid.max() < P and slot.max() < k
        S[lid, slot] = sc
        I[lid, slot] = row
    return S, I


# ---- restatements --------------------------------------------------------------------------------------------------------------
def merge_ref(S, I, k, row_offset=0):
    """The merge of one query's lists, restated: all occupied entries sorted by (-(score + 0.0), row), the first k, (-inf, -1)
    behind them, row_offset added to the rows.  -> (score bits uint32 [k], rows int64 [k], ub score bits, ub raw row): ub is entry
    k - 1 without the offset, (-inf, 0xFFFFFFFF) when fewer than k entries exist."""
    occ = I != NONE
    sc, rows = S[occ], I[occ]
    ents = sorted(zip((-(sc + np.float32(0.0))).tolist(), rows.tolist(), sc.view(np.uint32).tolist()))[:k]
    out_s = np.full(k, _NEG_INF_BITS, np.uint32)
    out_i = np.full(k, -1, np.int64)
    for r, (_neg, row, bits) in enumerate(ents):
        out_s[r] = bits
        out_i[r] = row + row_offset
    if len(ents) == k:
        return out_s, out_i, np.uint32(ents[-1][2]), np.uint32(ents[-1][1])
    return out_s, out_i, np.uint32(_NEG_INF_BITS), np.uint32(NONE)


def bound_ref(S, k, ranks):
    """The sample bound of one query, restated: the k-th largest, with multiplicity, of the first `ranks` slots of all lists
    (-inf = an empty slot; -inf when fewer than k values are above it)."""
    top = heapq.nlargest(k, S[:, :ranks].reshape(-1).tolist())
    return np.float32(top[k - 1]) if len(top) >= k else np.float32(-np.inf)


# ---- layouts -------------------------------------------------------------------------------------------------------------------
PAD_S, PAD_I = np.float32(3.0e38), np.uint32(0x00BADBAD)      # what a packer leaves where no query's list lives: a read of it shows


def pack_rank_major(S, I):
    """[nq, P, k] -> [nq, k, P] (entry (rank r, list l) of query q at (q * k + r) * P + l)."""
    return np.ascontiguousarray(S.transpose(0, 2, 1)), np.ascontiguousarray(I.transpose(0, 2, 1))


def unpack_rank_major(ps, pi):
    return np.ascontiguousarray(ps.transpose(0, 2, 1)), np.ascontiguousarray(pi.transpose(0, 2, 1))


def pack_stream_major(S, I, sm_nq_pad):
    """[nq, P, k] -> [P, sm_nq_pad, k] (entry (r, l) of query q at (l * sm_nq_pad + q) * k + r); queries behind nq hold PAD."""
    nq, P, k = S.shape
    assert sm_nq_pad >= nq
    ps = np.full((P, sm_nq_pad, k), PAD_S, np.float32)
    pi = np.full((P, sm_nq_pad, k), PAD_I, np.uint32)
    ps[:, :nq] = S.transpose(1, 0, 2)
    pi[:, :nq] = I.transpose(1, 0, 2)
    return ps, pi


def unpack_stream_major(ps, pi, nq):
    return np.ascontiguousarray(ps[:, :nq].transpose(1, 0, 2)), np.ascontiguousarray(pi[:, :nq].transpose(1, 0, 2))


# ---- families ------------------------------------------------------------------------------------------------------------------
def _rows(rng, n):
    """n distinct rows below 2^31 in random order: small ones (row 0 among them now and then) and large ones."""
    if n == 0:
        return np.zeros(0, np.uint32)
    r = np.unique(np.concatenate([rng.integers(0, 4 * n + 8, size=n), rng.integers(0, 2 ** 31 - 1, size=2 * n + 8)]))
    assert r.size >= n
    return rng.permutation(r)[:n].astype(np.uint32)


def score_pool(rng, k):
    """About 2k scores to draw from WITH replacement (ties are frequent): normal values and their one-ulp neighbours, both zeros,
    +-FLT_MAX, denormals, the smallest normal, negatives."""
    base = rng.standard_normal(max(2, k)).astype(np.float32)
    near = np.nextafter(base[:max(1, k // 2)], np.float32(np.inf))
    special = np.array([0.0, -0.0, FMAX, -FMAX, 1e-45, -1e-45, 1e-40, 1.17549435e-38, -1.0, -2.5, 1.0,
                        np.nextafter(np.float32(1.0), np.float32(2.0))], np.float32)
    return np.concatenate([base, near, special])


def _spread(lens, rng, P, k, total):
    """Add `total` entries to the per-list lengths `lens`, one at a time into a random list that still has room."""
    total = min(total, int(P * k - lens.sum()))
    for _ in range(total):
        free = np.flatnonzero(lens < k)
        lens[free[rng.integers(free.size)]] += 1
    return lens


def _from_lens(rng, P, k, lens, scores=None):
    lid = np.repeat(np.arange(P), lens)
    sc = rng.choice(score_pool(rng, k), lid.size) if scores is None else scores
    return lists_from_entries(P, k, lid, sc, _rows(rng, lid.size))


def random(P, k, seed):
    """Lengths 0..k per list, scores from the pool."""
    rng = np.random.default_rng(seed)
    return _from_lens(rng, P, k, rng.integers(0, k + 1, size=P))


def signed_zeros(P, k, seed):
    """Lengths 0..k per list, every score +0.0 or -0.0: one tie that the rows alone order, whatever the sign bit says."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, k + 1, size=P)
    return _from_lens(rng, P, k, lens, scores=rng.choice(np.array([0.0, -0.0], np.float32), int(lens.sum())))


def one_list(P, k, seed, lstar):
    """Everything in list lstar (P - 1 when there is no such list), all other lists empty."""
    rng = np.random.default_rng(seed)
    lens = np.zeros(P, np.int64)
    lens[min(lstar, P - 1)] = k
    return _from_lens(rng, P, k, lens)


def singletons(P, k, seed, m, place):
    """Exactly m (at most P) non-empty lists of one entry each: the first lists, the last ones, or spread over all."""
    rng = np.random.default_rng(seed)
    m = max(0, min(m, P))
    lens = np.zeros(P, np.int64)
    at = {"first": np.arange(m), "last": np.arange(P - m, P), "spread": (np.arange(m) * P) // max(m, 1)}[place]
    lens[at] = 1
    return _from_lens(rng, P, k, lens)


def short(P, k, seed):
    """k - 1 entries in all (fewer where P * k is less), spread over the lists."""
    rng = np.random.default_rng(seed)
    return _from_lens(rng, P, k, _spread(np.zeros(P, np.int64), rng, P, k, k - 1))


def empty(P, k, seed):
    return lists_from_entries(P, k, [], [], [])


def all_equal_interleaved(P, k, seed):
    """One score everywhere, full lists, list l holds rows l, l + P, ..."""
    lid = np.repeat(np.arange(P), k)
    return lists_from_entries(P, k, lid, np.full(P * k, 0.5, np.float32), np.tile(np.arange(k), P) * P + lid)


def all_equal_blocked(P, k, seed):
    """One score everywhere, full lists, list l holds rows l * k ... l * k + k - 1."""
    return lists_from_entries(P, k, np.repeat(np.arange(P), k), np.full(P * k, -0.0, np.float32), np.arange(P * k))


def top_heavy(P, k, seed, survivors=None):
    """min(P, k) heavy lists whose every entry beats every head of the other (full) lists.  The k-th best head is the threshold of
    the workgroup merge; the entries of a list behind its own head are below that head, so the threshold's list contributes one
    survivor and the most there can be is k (k - 1) + 1 -- more than 256 from k = 17.  survivors: that many entries at or above the
    threshold where the shape allows it (default: the most)."""
    rng = np.random.default_rng(seed)
    m = min(P, k)
    heavy = rng.permutation(P)[:m]
    above = np.full(m, k, np.int64)          # per heavy list: entries above the threshold; the LAST heavy list is the threshold's
    above[-1] = 0
    if survivors is not None and m == k and k - 1 <= survivors - 1 <= k * (k - 1):
        above[:-1] = 1
        for _ in range(survivors - 1 - (k - 1)):
            j = rng.integers(m - 1)
            while above[j] == k:
                j = (j + 1) % (m - 1)
            above[j] += 1
    sc = rng.uniform(0.0, 0.9, size=(P, k)).astype(np.float32)                 # light lists
    for j, l in enumerate(heavy):
        sc[l, :above[j]] = rng.uniform(2.1, 3.0, size=above[j])
        sc[l, above[j]:] = rng.uniform(1.0, 1.9, size=k - above[j])
    sc[heavy[-1], 0] = 2.0                                                     # the k-th best head when m == k
    return lists_from_entries(P, k, np.repeat(np.arange(P), k), sc.reshape(-1), _rows(rng, P * k))


def tied_kth(P, k, seed):
    """The k-th answer ties in score with about 3k further entries in other lists: k - 1 entries above, the rest of the room below;
    the row decides."""
    rng = np.random.default_rng(seed)
    n_hi, n_tie = k - 1, 3 * k + 1
    total = min(P * k, n_hi + n_tie + 2 * k)
    sc = np.concatenate([rng.uniform(1.0, 2.0, n_hi), np.full(n_tie, 0.25), rng.uniform(-1.0, 0.2, 2 * k)]).astype(np.float32)[:total]
    lens = _spread(np.zeros(P, np.int64), rng, P, k, total)
    return lists_from_entries(P, k, rng.permutation(np.repeat(np.arange(P), lens)), sc, _rows(rng, total))


def late_wave(P, k, seed, wave):
    """Full lists; the k best heads (as many as fit) all sit in the lists of one wave of 64 (wave -1: the last one), at its upper
    end: the threshold candidates of that wave fill slots wave * k + rank of the workgroup merge to the top."""
    rng = np.random.default_rng(seed)
    nw = (P + 63) // 64
    w = nw - 1 if wave < 0 else min(wave, nw - 1)
    lo, hi = 64 * w, min(P, 64 * w + 64)
    sc = rng.uniform(-1.0, 1.0, size=(P, k)).astype(np.float32)
    best = np.arange(max(lo, hi - k), hi)
    sc[best, 0] = rng.uniform(10.0, 11.0, size=best.size)
    return lists_from_entries(P, k, np.repeat(np.arange(P), k), sc.reshape(-1), _rows(rng, P * k))


def sparse_total(P, k, seed, total, lens_first=()):
    """`total` entries in all (the prefilter's mostly empty lists); the first lists take the lengths lens_first."""
    rng = np.random.default_rng(seed)
    lens = np.zeros(P, np.int64)
    nf = len(lens_first)
    lens[:nf] = np.minimum(lens_first, k)
    assert lens.sum() <= total and nf <= P
    lens[nf:] = _spread(lens[nf:], rng, P - nf, k, total - int(lens.sum()))
    return _from_lens(rng, P, k, lens)


def _named(fn, **kw):
    return lambda P, k, seed: fn(P, k, seed, **kw)


# name -> (P, k, seed) -> lists.  A case a kernel once got wrong is added here by name.
FAMILIES = {
    "random": random,
    "signed_zeros": signed_zeros,
    "one_list_0": _named(one_list, lstar=0),
    "one_list_63": _named(one_list, lstar=63),
    "one_list_64": _named(one_list, lstar=64),
    "one_list_last": _named(one_list, lstar=1 << 30),
    "short": short,
    "empty": empty,
    "all_equal_interleaved": all_equal_interleaved,
    "all_equal_blocked": all_equal_blocked,
    "top_heavy": top_heavy,
    "top_heavy_256": _named(top_heavy, survivors=256),
    "top_heavy_257": _named(top_heavy, survivors=257),
    "tied_kth": tied_kth,
    "late_wave_last": _named(late_wave, wave=-1),
    "late_wave_0": _named(late_wave, wave=0),
    "late_wave_2": _named(late_wave, wave=2),
}
for _m, _mname in ((-1, "km1"), (0, "k"), (1, "kp1")):
    for _place in ("first", "last", "spread"):
        FAMILIES[f"singletons_{_mname}_{_place}"] = (lambda P, k, seed, _m=_m, _place=_place: singletons(P, k, seed, k + _m, _place))


def family_batches(P, k, seed=0, size=9, names=None):
    """Every family at (P, k), each asserted against the contract, in batches of 3..size queries:
    -> [(names, S [nq, P, k], I [nq, P, k])]."""
    names = list(FAMILIES) if names is None else list(names)
    cases = []
    for j, name in enumerate(names):
        S, I = FAMILIES[name](P, k, seed + 101 * j)
        check_contract(S, I, k)
        cases.append((name, S, I))
    out = []
    for at in range(0, len(cases), size):
        chunk = cases[at:at + size]
        while len(chunk) < 3:                              # (a short tail: more seeds of the random family)
            S, I = random(P, k, seed + 7919 + len(chunk))
            check_contract(S, I, k)
            chunk.append(("random+", S, I))
        out.append(([c[0] for c in chunk], np.stack([c[1] for c in chunk]), np.stack([c[2] for c in chunk])))
    return out


# sample bound: value sets.  The selection looks at values only (no rows, no order inside a list), so a set is a flat array in the
# kernel's own index order, value (rank r, list l) at r * P + l, and may put its values wherever the case needs them.
def _distinct(rng, count):
    return ((rng.permutation(count) - count // 2) / 64.0).astype(np.float32)


def _few_finite(rng, count, m):
    v = np.full(count, -np.inf, np.float32)
    at = rng.permutation(count)[:max(0, min(m, count))]
    v[at] = _distinct(rng, count)[at]
    return v


def _lane_pops(rng, count, n):
    """The n largest values all at indices congruent modulo 64: one lane's head pops n times running."""
    v = _distinct(rng, count) - np.float32(count)
    c = int(rng.integers(0, min(64, count)))
    at = np.array([c + 64 * i for i in range(32) if c + 64 * i < count])
    at = rng.permutation(at)[:n]
    v[at] = (100.0 + rng.permutation(at.size)).astype(np.float32)
    return v


def _zeros_mixed(rng, count, k):
    v = rng.choice(np.array([0.0, -0.0, -1.0], np.float32), count)
    v[rng.permutation(count)[:k // 2]] = 1.0
    return v


BOUND_SETS = {
    "distinct": lambda rng, count, k: _distinct(rng, count),
    "three_values": lambda rng, count, k: rng.choice(np.array([-1.5, 0.25, 2.0], np.float32), count),
    "all_equal": lambda rng, count, k: np.full(count, 0.75, np.float32),
    "finite_km1": lambda rng, count, k: _few_finite(rng, count, k - 1),
    "finite_k": lambda rng, count, k: _few_finite(rng, count, k),
    "finite_kp1": lambda rng, count, k: _few_finite(rng, count, k + 1),
    "all_negative": lambda rng, count, k: -np.abs(_distinct(rng, count)) - np.float32(1.0),
    "zeros_mixed": _zeros_mixed,
    "lane_pops_8": lambda rng, count, k: _lane_pops(rng, count, 8),
    "lane_pops_4": lambda rng, count, k: _lane_pops(rng, count, 4),
}


def bound_batch(P, k, ranks, seed=0):
    """Every value set at (P, k, ranks) as sample lists: -> (names, S [nq, P, k]); slots behind `ranks` hold PAD_S (never read)."""
    names = list(BOUND_SETS)
    S = np.full((len(names), P, k), PAD_S, np.float32)
    for j, name in enumerate(names):
        v = np.asarray(BOUND_SETS[name](np.random.default_rng(seed + 31 * j), ranks * P, k), np.float32)
        assert v.shape == (ranks * P,) and not np.any(np.isnan(v)) and not np.any(np.isposinf(v))
        S[j, :, :ranks] = v.reshape(ranks, P).T
    return names, S


def hstep_ref(S, k, ranks):
    """The bucket width of one query where it is determined: 0 without a bound or a spread, float32(best - kth) * float32(1 / 12)
    for k < 4; None for k >= 4 with a spread (the width then goes through __logf and only steers speed)."""
    v = S[:, :ranks].reshape(-1)
    kth, best = bound_ref(S, k, ranks), np.float32(v.max())
    if np.isneginf(kth) or best == kth:
        return np.float32(0.0)
    if k < 4:
        return np.float32(np.float32(best - kth) * np.float32(1.0 / 12.0))
    return None


# ---- device side ---------------------------------------------------------------------------------------------------------------
CANARY_S, CANARY_I = np.float32(777.25), np.int64(-7777)
CANARY_UB_S, CANARY_UB_I = np.float32(555.5), np.uint32(0xABCDABCD)
CANARY_LB, CANARY_HIST, CANARY_HSTEP = np.float32(-321.5), np.uint32(0x5A5A5A5A), np.float32(-4.0)
GUARD = 16
COL0, EXTRA = 2, 5            # outputs start at column 2 of rows k + 5 wide


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def debug_merge_lists(lib, part_s, part_i, P, nq, k, sm_nq_pad, sparse, row_offset, out_s, out_i, out_stride, col0, ub_s, ub_i, dp_nq, dp_P,
                      qmap, dp_scratch, stream):
    """ctypes call of ms_debug_merge_lists: tensors (or None) for the pointers."""
    p = lambda t: None if t is None else t.data_ptr()
    return lib.ms_debug_merge_lists(p(part_s), p(part_i), P, nq, k, sm_nq_pad, sparse, row_offset, p(out_s), p(out_i), out_stride, col0,
                                    p(ub_s), p(ub_i), dp_nq, dp_P, p(qmap), p(dp_scratch), stream)


def debug_sample_bound(lib, part_s, P, nq, k, ranks, sm_nq_pad, lb, hist, hstep, stream):
    """ctypes call of ms_debug_sample_bound."""
    p = lambda t: None if t is None else t.data_ptr()
    return lib.ms_debug_sample_bound(p(part_s), P, nq, k, ranks, sm_nq_pad, p(lb), p(hist), p(hstep), stream)


def expected_merge(S, I, k, row_offset, out_rows, n_out, with_ub):
    """The four output arrays, guards included, as the merge of S, I must leave them: query q in output row out_rows[q], the
    canary everywhere else."""
    stride = k + EXTRA
    out_s = np.full(n_out * stride + GUARD, CANARY_S, np.float32).view(np.uint32)
    out_i = np.full(n_out * stride + GUARD, CANARY_I, np.int64)
    ub_s = np.full(n_out + GUARD, CANARY_UB_S, np.float32).view(np.uint32)
    ub_i = np.full(n_out + GUARD, CANARY_UB_I, np.uint32)
    for q in range(S.shape[0]):
        s, i, us, ui = merge_ref(S[q], I[q], k, row_offset)
        o = out_rows[q] * stride + COL0
        out_s[o:o + k] = s
        out_i[o:o + k] = i
        if with_ub:
            ub_s[out_rows[q]], ub_i[out_rows[q]] = us, ui
    return out_s, out_i, ub_s, ub_i


def run_merge(torch, lib, S, I, layout="rank", sparse=0, row_offset=0, with_ub=True, dp=None, qmap=None, launch=None, stream=None):
    """One call of the hook on the batch S, I [nq, P, k] -> (rc, out_s bits, out_i, ub_s bits, ub_i), guards included.
    layout "stream": stream-major with sm_nq_pad = nq + 3.  dp = (dp_nq, dp_P): S, I are the dp_nq queries' dp_P lists, laid out
    rank-major with dp_P at the front of a buffer for launch = (nq, P); qmap: int array [dp_nq] or None."""
    nq, P, k = S.shape
    sm_nq_pad = nq + 3 if layout == "stream" else 0
    ps, pi = pack_stream_major(S, I, sm_nq_pad) if sm_nq_pad else pack_rank_major(S, I)
    l_nq, l_P = (nq, P) if launch is None else launch
    if dp is not None:
        assert sm_nq_pad == 0 and dp == (nq, P) and l_nq >= nq and l_P >= P
        room = l_nq * k * l_P
        ps = np.concatenate([ps.reshape(-1), np.full(room - ps.size, PAD_S, np.float32)])
        pi = np.concatenate([pi.reshape(-1), np.full(room - pi.size, PAD_I, np.uint32)])
    stride = k + EXTRA
    d_ps, d_pi = _dev(torch, ps), _dev(torch, pi)
    d_os = _dev(torch, np.full(l_nq * stride + GUARD, CANARY_S, np.float32))
    d_oi = _dev(torch, np.full(l_nq * stride + GUARD, CANARY_I, np.int64))
    d_us = _dev(torch, np.full(l_nq + GUARD, CANARY_UB_S, np.float32))
    d_ui = _dev(torch, np.full(l_nq + GUARD, CANARY_UB_I, np.uint32))
    d_qmap = None if qmap is None else _dev(torch, np.asarray(qmap, np.int32))
    d_dp = None if dp is None else torch.full((16,), -1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = debug_merge_lists(lib, d_ps, d_pi, l_P, l_nq, k, sm_nq_pad, sparse, row_offset, d_os, d_oi, stride, COL0,
                           d_us if with_ub else None, d_ui if with_ub else None, 0 if dp is None else dp[0], 0 if dp is None else dp[1],
                           d_qmap, d_dp, st)
    torch.cuda.synchronize()
    return rc, _host(d_os, np.uint32), _host(d_oi, np.int64), _host(d_us, np.uint32), _host(d_ui, np.uint32)


def check_merge(torch, lib, names, S, I, what="", **kw):
    """run_merge and compare every output word with the restatement; raises AssertionError naming the first query that differs."""
    nq, _P, k = S.shape
    rc, *got = run_merge(torch, lib, S, I, **kw)
    assert rc == 0, (what, rc, lib.ms_last_error())
    n_out = nq if kw.get("launch") is None else kw["launch"][0]
    out_rows = list(range(nq)) if kw.get("qmap") is None else list(kw["qmap"])
    want = expected_merge(S, I, k, kw.get("row_offset", 0), out_rows, n_out, kw.get("with_ub", True))
    stride = k + EXTRA
    for label, g, w, per in zip(("out_s", "out_i", "ub_s", "ub_i"), got, want, (stride, stride, 1, 1)):
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            row = at // per
            who = names[out_rows.index(row)] if row in out_rows else "no query (canary or guard)"
            raise AssertionError(f"{what} {kw}: {label} differs first at word {at} (output row {row}, column {at % per}): {who}; "
                                 f"got {int(g[at]):#x} want {int(w[at]):#x}")


def run_bound(torch, lib, S, k, ranks, layout="rank", with_hist=True, stream=None):
    """One call of the bound hook on S [nq, P, k] -> (rc, lb, hist, hstep), guards included."""
    nq, P, _k = S.shape
    sm_nq_pad = nq + 3 if layout == "stream" else 0
    ps = pack_stream_major(S, np.zeros(S.shape, np.uint32), sm_nq_pad)[0] if sm_nq_pad else pack_rank_major(S, np.zeros(S.shape, np.uint32))[0]
    d_ps = _dev(torch, ps)
    d_lb = _dev(torch, np.full(nq + GUARD, CANARY_LB, np.float32))
    d_hist = _dev(torch, np.full((nq + GUARD) * 16, CANARY_HIST, np.uint32))
    d_hstep = _dev(torch, np.full(nq + GUARD, CANARY_HSTEP, np.float32))
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = debug_sample_bound(lib, d_ps, P, nq, k, ranks, sm_nq_pad, d_lb, d_hist if with_hist else None, d_hstep if with_hist else None, st)
    torch.cuda.synchronize()
    return rc, _host(d_lb, np.float32), _host(d_hist, np.uint32), _host(d_hstep, np.float32)


# The forms a search only takes with MS_BLOCK_MERGE=0 (the head-advance merge with 1, 2 and 4 lists per lane) and with MS_HEAD_MERGE=0
# as well (the pool merge) at P <= 256: run in a child process, rank-major (stream-major lists always take the workgroup merge).
CHILD_PAIRS = [(1, 1), (1, 10), (63, 10), (64, 64), (64, 3), (65, 10), (128, 20), (129, 5), (256, 10), (256, 64)]


def child_main():
    import torch
    from merizo_search_amd import _lib
    _lib.require_gpu()
    lib = _lib.load()
    n = 0
    for P, k in CHILD_PAIRS:
        for b, (names, S, I) in enumerate(family_batches(P, k, seed=1000 + P + k)):
            check_merge(torch, lib, names, S, I, what=f"child P={P} k={k}", row_offset=(1 << 33) + 5, with_ub=b % 2 == 0)
            n += len(names)
    print(f"merge child ok {n} queries, MS_BLOCK_MERGE={os.environ.get('MS_BLOCK_MERGE', '')} MS_HEAD_MERGE={os.environ.get('MS_HEAD_MERGE', '')}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["child"]:
        child_main()
