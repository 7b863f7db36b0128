"""ip_topk_large without a GPU: the routing predicate at its edges, the constants against the header, and the rounds of the
driver (gather, second round, fallback, scatter) against a stub entry that returns chosen statuses."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_and_symbols_match_the_header():
    from merizo_search_amd import _lib
    header = open(os.path.join(REPO, "include", "merizo_search_amd.h")).read()
    assert int(re.search(r"#define MS_LARGE_K_MAX\s+(\d+)", header).group(1)) == _lib.LARGE_K_MAX
    assert int(re.search(r"#define MS_LARGE_K_CAND\s+(\d+)", header).group(1)) == _lib.LARGE_K_CAND
    assert _lib.LARGE_K_MAX % 64 == 0 and _lib.LARGE_K_CAND * 8 == 64 * 1024       # one 64 KB sort of 8-byte keys
    assert len(_lib.SIGNATURES["ms_ip_topk_large"][1]) == 20 and len(_lib.SIGNATURES["ms_ip_topk_large_workspace_bytes"][1]) == 3


def test_large_k_serves_at_its_edges(monkeypatch):
    from merizo_search_amd import _lib, ops
    assert ops.LARGE_K_MIN_ROWS == int(os.environ.get("MS_LARGE_K_MIN_ROWS", "200000")) and ops.LARGE_K_TWO_SCAN_MIN_NQ == 8
    monkeypatch.setattr(ops, "LARGE_K_MIN_ROWS", 0)
    assert not ops.large_k_serves(10 ** 6, 8, 64) and ops.large_k_serves(10 ** 6, 8, 65)
    assert ops.large_k_serves(10 ** 6, 8, _lib.LARGE_K_MAX) and not ops.large_k_serves(10 ** 6, 8, _lib.LARGE_K_MAX + 1)
    assert ops.large_k_serves(256, 8, 128) and not ops.large_k_serves(255, 8, 128)          # G = 2: 128 rows per group
    assert ops.large_k_serves(384, 1, 129) and not ops.large_k_serves(383, 1, 129)          # G = 3
    assert not ops.large_k_serves(10 ** 6, 7, 128) and ops.large_k_serves(10 ** 6, 1, 129)  # two scans pay from 8 queries on
    assert not ops.large_k_serves(0, 8, 100) and not ops.large_k_serves(10 ** 6, 0, 200)
    monkeypatch.setattr(ops, "LARGE_K_TWO_SCAN_MIN_NQ", 1)
    assert ops.large_k_serves(256, 1, 128) and ops.large_k_serves(10 ** 6, 1, 65)
    monkeypatch.setattr(ops, "LARGE_K_MIN_ROWS", 5000)
    assert ops.large_k_serves(5000, 1, 100) and not ops.large_k_serves(4999, 1, 100)
    monkeypatch.setattr(ops, "LARGE_K_MIN_ROWS", 1 << 62)
    assert not ops.large_k_serves(2 ** 31 - 2, 4096, 1000)


class _Stub:
    """A stand-in for the entry and for ip_topk on CPU tensors.  Query j (identified by q[j, 0]) has the answer row
    (scores j + r / 1000, rows 1000 j + r); first[j] / second[j] is the status the entry gives it in each round."""

    def __init__(self, k, first, second):
        self.k, self.first, self.second, self.calls, self.fell = k, first, second, [], []

    def answer(self, ids):
        import torch
        r = torch.arange(self.k)
        return ids[:, None].float() + r[None, :].float() / 1000, (1000 * ids[:, None] + r[None, :]).long()

    def call(self, q, qlen, lb_in):
        import torch
        ids = q[:, 0].long()
        table = self.first if lb_in is None else self.second
        status = torch.tensor([table[int(j)] for j in ids], dtype=torch.int32)
        if lb_in is not None:                                      # the second round is handed the first round's out_lb, gathered
            assert torch.equal(lb_in, ids.float() + 0.5) and all(self.first[int(j)] == 1 for j in ids)
        if qlen is not None:
            assert torch.equal(qlen, ids.float() * 2)
        self.calls.append((ids.tolist(), lb_in is not None))
        s, i = self.answer(ids)
        s[status != 0] = float("-inf")
        i[status != 0] = -1
        st = torch.tensor([int((status == v).sum()) for v in (0, 1, 2)] + [10 * len(ids)])
        return s, i, status, ids.float() + 0.5, st

    def fallback(self, q, qlen):
        ids = q[:, 0].long()
        if qlen is not None:
            import torch
            assert torch.equal(qlen, ids.float() * 2)
        self.fell.append(ids.tolist())
        return self.answer(ids)


@pytest.mark.parametrize("with_qlen", [False, True])
def test_rounds_gather_relaunch_fall_back_and_scatter(with_qlen):
    import torch
    from merizo_search_amd import ops
    nq, k = 9, 5
    first = {0: 0, 1: 1, 2: 2, 3: 1, 4: 0, 5: 1, 6: 2, 7: 0, 8: 1}
    second = {1: 0, 3: 1, 5: 2, 8: 0}
    stub = _Stub(k, first, second)
    q = torch.zeros(nq, 128)
    q[:, 0] = torch.arange(nq).float()
    qlen = torch.arange(nq).float() * 2 if with_qlen else None
    stats = {}
    s, i = ops._large_k_rounds(stub.call, stub.fallback, q, qlen, stats)
    want_s, want_i = stub.answer(torch.arange(nq))
    assert torch.equal(s, want_s) and torch.equal(i, want_i)
    assert stub.calls == [(list(range(nq)), False), ([1, 3, 5, 8], True)] and stub.fell == [[2, 3, 5, 6]]
    assert stats == {"first_round": 3, "second_round": 2, "fallback": 4, "rescored": 90 + 40, "forwarded": False}


def test_rounds_stop_as_soon_as_every_query_is_final(caplog):
    import logging
    import torch
    from merizo_search_amd import ops
    q = torch.zeros(4, 128)
    q[:, 0] = torch.arange(4).float()
    stub = _Stub(3, {j: 0 for j in range(4)}, {})
    stats = {}
    s, i = ops._large_k_rounds(stub.call, stub.fallback, q, None, stats)
    assert len(stub.calls) == 1 and stub.fell == [] and stats["first_round"] == 4 and stats["fallback"] == 0
    assert torch.equal(i, stub.answer(torch.arange(4))[1])
    # only status 2: no second round, the fallback alone; and more than a tenth on the fallback is worth one INFO line
    stub = _Stub(3, {0: 0, 1: 2, 2: 0, 3: 2}, {})
    with caplog.at_level(logging.INFO):
        s, i = ops._large_k_rounds(stub.call, stub.fallback, q, None, stats)
    assert len(stub.calls) == 1 and stub.fell == [[1, 3]] and stats["fallback"] == 2 and stats["second_round"] == 0
    assert torch.equal(s, stub.answer(torch.arange(4))[0])
    notes = [r for r in caplog.records if "ordered by family" in r.getMessage()]
    assert len(notes) == 1 and notes[0].levelno == logging.INFO


def test_a_forwarded_call_is_reported(monkeypatch):
    import torch
    from merizo_search_amd import ops
    stub = _Stub(3, {0: 0, 1: 0}, {})
    real = stub.call

    def forwarded(q, qlen, lb_in):
        s, i, status, lb, st = real(q, qlen, lb_in)
        st[3] = -1
        return s, i, status, lb, st

    q = torch.zeros(2, 128)
    q[:, 0] = torch.arange(2).float()
    stats = {}
    ops._large_k_rounds(forwarded, stub.fallback, q, None, stats)
    assert stats == {"first_round": 2, "second_round": 0, "fallback": 0, "rescored": 0, "forwarded": True}
