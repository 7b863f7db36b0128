"""Every entry point keeps to its caller's stream (include/merizo_search_amd.h: "asynchronous on `stream`, never allocate, never
synchronise ... a WORKSPACE serves one stream at a time ... entry points may be called from any host thread").

1. The ordering test, one case per entry point and plan form (stream_case.TABLE): the op runs on a side stream behind a delay, with
   other inputs copied in on that stream in front of it and the primed ones copied back behind it.  A launch on any other stream reads
   the wrong set and shows in the bits; a call that waits for the device shows in `gate.query()`.
2. The first use of a fresh workspace on a side stream (the library zeroes its per-workspace block on first need).
3. Two searches in flight on two streams with a workspace each, from one thread and from two.
4. One encoder used from two streams.
One process, the default stream and at most two more, at most two host threads; nothing is captured into a graph."""
import threading
import time

import numpy as np
import pytest

import stream_case as sc

pytestmark = pytest.mark.gpu
MIN_DELAY_MS = 20.0
MAX_DELAY_MS = 1000.0
DELAY_FACTOR = 10.0


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    from merizo_search_amd import _lib
    _lib.require_gpu()
    return torch


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault(torch_gpu):
    """A test that leaves the device in an error state ends the session: nothing more is started on a GPU that has faulted."""
    yield
    try:
        torch_gpu.cuda.synchronize()
    except Exception as exc:          # noqa: BLE001 -- whatever the runtime raises for a sticky error
        pytest.exit("the GPU reported an error after this test, stopping: %s" % exc, returncode=3)


@pytest.fixture(scope="module")
def sleep_cycles_per_ms(torch_gpu):
    """torch.cuda._sleep counts a clock that is not specified: measured once per session with events (the longer of two runs' rates,
    so that a delay is never shorter than asked for)."""
    torch = torch_gpu
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    rates = []
    for cycles in (5_000_000, 20_000_000):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        torch.cuda.synchronize()
        rates.append(cycles / max(a.elapsed_time(b), 1e-3))
    return max(rates)


def _canon(built, outs):
    if built.canon is not None:
        return [np.array(a, copy=True) for a in built.canon(outs)]
    return [o.cpu().numpy() if hasattr(o, "cpu") else np.array(o, copy=True) for o in outs]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _fill(bufs, payload):
    for buf, src in zip(bufs, payload):
        buf.copy_(src, non_blocking=True)


# ------------------------------------------------------------------ 1. the ordering test ----
@pytest.mark.parametrize("cid", list(sc.CASES))
def test_the_call_runs_on_the_callers_stream_and_nowhere_else(cid, torch_gpu, sleep_cycles_per_ms):
    torch = torch_gpu
    case = sc.CASES[cid]
    built = case.build()
    for a, b in zip(built.A, built.B):
        assert a.shape == b.shape and a.dtype == b.dtype
        if a.dtype in (torch.int32, torch.int64):
            assert torch.equal(a, b), "integer inputs are identical in both sets"
    # prime: the op on A into the buffers, workspace and outputs the side stream will use
    bufs = [a.clone() for a in built.A]
    state = built.fresh()
    primed = _canon(built, built.run(bufs, state, "A"))
    _fill(bufs, built.A)              # (a call that edits its inputs in place: they hold A again)
    torch.cuda.synchronize()
    # expect: the op on B on the default stream with fresh buffers, twice (the second run timed warm, host plus device)
    fresh_bufs = [b.clone() for b in built.B]
    built.run(fresh_bufs, built.fresh(), "B")
    torch.cuda.synchronize()
    _fill(fresh_bufs, built.B)
    torch.cuda.synchronize()
    fresh_state = built.fresh()
    t0 = time.perf_counter()
    outs = built.run(fresh_bufs, fresh_state, "B")
    torch.cuda.synchronize()
    warm_ms = (time.perf_counter() - t0) * 1e3
    want = _canon(built, outs)
    assert len(want) == len(primed)
    for j, (w, p) in enumerate(zip(want, primed)):
        assert (j in built.same) or not _same_bits(w, p), f"{cid}: output {j} is the same for A and B: the case cannot tell them apart"
    if built.check is not None:
        built.check(want, torch)
    delay_ms = max(MIN_DELAY_MS, DELAY_FACTOR * warm_ms)
    assert delay_ms <= MAX_DELAY_MS, f"{cid}: a warm call of {warm_ms:.1f} ms needs a delay of {delay_ms:.0f} ms: the case is mis-sized"
    # the side stream: its allocator pool is warmed with one more run on A (the state stays A's), then the real thing
    S = torch.cuda.Stream()
    S.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(S):
        built.run(bufs, state, "A")
        _fill(bufs, built.A)
    S.synchronize()
    torch.cuda.synchronize()
    begin = torch.cuda.Event(enable_timing=True)
    gate = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(S):
        begin.record()
        torch.cuda._sleep(int(1.25 * delay_ms * sleep_cycles_per_ms))
        gate.record()
        _fill(bufs, built.B)
        t0 = time.perf_counter()
        outs = built.run(bufs, state, "B")
        returned_early = not gate.query()
        host_ms = (time.perf_counter() - t0) * 1e3
        _fill(bufs, built.A)
    S.synchronize()
    got = _canon(built, outs)
    slept_ms = begin.elapsed_time(gate)
    torch.cuda.synchronize()
    note = f"{cid}: delay {slept_ms:.1f} ms (asked {delay_ms:.1f}), warm default-stream call {warm_ms:.2f} ms, the call took {host_ms:.2f} ms of host time"
    assert slept_ms >= delay_ms, "the delay ran short of what the rule asks for: " + note
    if case.asynchronous:
        assert returned_early, "the call returned only after the work in front of it on its stream had finished: " + note
    else:
        assert case.sync_why
    for j, (g, w) in enumerate(zip(got, want)):
        assert _same_bits(g, w), f"output {j} on the side stream differs from the default-stream result ({int((g != w).sum()) if g.shape == w.shape else 'shape'}" \
                                 f" elements; equals the primed A result: {_same_bits(g, primed[j])}): " + note
    for buf, a in zip(bufs, built.A):
        assert torch.equal(buf.view(torch.uint8), a.view(torch.uint8)), "the input buffers hold A again"


# ------------------------------------------------------------------ shared by 2. and 3. ----
def _oracle(db, q, k, row_offset=0):
    from oracle import oracle as orc
    return orc.ip_topk(db, q, k, row_offset=row_offset, order=1)


def _equals(torch, got, ref):
    s, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    return np.array_equal(i, ref[1]) and _same_bits(s.view(np.uint32), np.ascontiguousarray(ref[0]).view(np.uint32))


def _search_forms(torch, form):
    """-> (n, nq, k, search(q, ws) on the current stream, new workspace(), host rows): the forms of sections 2 and 3."""
    from merizo_search_amd import _lib, ops
    lib = _lib.load()
    if form == "few":
        n, nq, k = 5000, 3, 10
    elif form == "large":
        n, nq, k = 3000, 37, 200
    else:
        n, nq, k = 70_000, 100, (5 if form == "prefiltered" else 10)
    rows = sc._unit_rows(n, 700)
    d = sc._t(rows)
    if form == "prefiltered":
        image = ops.pf_build_image(d, fmt=ops.PF_F16X1, row_norm_bound=sc.BOUND)
        need = int(lib.ms_ip_topk_prefiltered_workspace_bytes(n, nq, k))
        search = lambda q, ws: ops.ip_topk_prefiltered(d, q, k, sc.BOUND, workspace=ws, image=image)
    elif form == "large":
        need = int(lib.ms_ip_topk_large_workspace_bytes(n, nq, k))
        search = lambda q, ws: ops.ip_topk_large(d, q, k, sc.BOUND, workspace=ws)
    else:
        need = int(lib.ms_ip_topk_workspace_bytes(n, nq, k))
        search = lambda q, ws: ops.ip_topk(d, q, k, workspace=ws)
    return n, nq, k, search, (lambda: torch.empty(need, dtype=torch.uint8, device="cuda")), rows


# ------------------------------------------------------------------ 2. a fresh workspace, first used on a side stream ----
@pytest.mark.parametrize("form", ["few", "prefiltered"])
def test_first_use_of_a_fresh_workspace_on_a_side_stream(form, torch_gpu):
    """The library keeps a block of counters per workspace and zeroes it on first need (ms_wsstate::alloc_zeroed) from the calling host
    thread, not on the caller's stream: the first search must see it zeroed all the same.  Ten brand-new workspaces (all kept alive, so
    that none gets another's address), no priming run, no delay; the in-launch merge of the few-query form counts arrivals in that
    block, the prefiltered search keeps its gate and tickets there."""
    torch = torch_gpu
    from merizo_search_amd.foldclass import synthetic as syn
    n, nq, k, search, new_ws, rows = _search_forms(torch, form)
    S = torch.cuda.Stream()
    spaces = []
    for j in range(10):
        q = syn.normalized_database(nq, 900 + j)
        dq = sc._t(q)
        ws = new_ws()
        spaces.append(ws)
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            got = search(dq, ws)
        S.synchronize()
        assert _equals(torch, got, _oracle(rows, q, k)), f"workspace {j}"


# ------------------------------------------------------------------ 3. two searches in flight ----
FORMS_IN_FLIGHT = ["ordinary", "few", "prefiltered", "large"]


@pytest.mark.parametrize("form", FORMS_IN_FLIGHT)
def test_two_searches_in_flight_with_a_workspace_each(form, torch_gpu):
    """bench.py's pipelined_rate with assertions: two streams, two workspaces, the database (and image) shared, another query batch
    per slot, 20 steps taken in turns.  Every result equals the serial default-stream result of its batch bit for bit."""
    torch = torch_gpu
    from merizo_search_amd.foldclass import synthetic as syn
    n, nq, k, search, new_ws, rows = _search_forms(torch, form)
    qs = [sc._t(syn.normalized_database(nq, 950 + j)) for j in range(2)]
    serial = [tuple(t.clone() for t in search(q, new_ws())) for q in qs]
    torch.cuda.synchronize()
    ref = [_oracle(rows, q.cpu().numpy(), k) for q in qs]
    assert all(_equals(torch, s, r) for s, r in zip(serial, ref))
    streams = [torch.cuda.Stream() for _ in range(2)]
    spaces = [new_ws() for _ in range(2)]
    torch.cuda.synchronize()
    results = []
    for step in range(20):
        slot = step % 2
        with torch.cuda.stream(streams[slot]):
            results.append((slot, tuple(t.clone() for t in search(qs[slot], spaces[slot]))))
    torch.cuda.synchronize()
    for step, (slot, got) in enumerate(results):
        assert torch.equal(got[1], serial[slot][1]) and torch.equal(got[0].view(torch.int32), serial[slot][0].view(torch.int32)), (form, step)


def test_two_host_threads_search_on_a_stream_each(torch_gpu):
    """The same from two Python threads (ctypes releases the GIL for the call), each with its own stream, workspace and query batch.
    Thread 0 also makes a refused call between its searches: ms_last_error is the CALLING thread's, thread 1 never sees it."""
    torch = torch_gpu
    from merizo_search_amd import _lib, ops
    from merizo_search_amd.foldclass import synthetic as syn
    lib = _lib.load()
    n, nq, k, search, new_ws, rows = _search_forms(torch, "ordinary")
    qs = [sc._t(syn.normalized_database(nq, 970 + j)) for j in range(2)]
    serial = [tuple(t.clone() for t in search(q, new_ws())) for q in qs]
    streams = [torch.cuda.Stream() for _ in range(2)]
    spaces = [new_ws() for _ in range(2)]
    torch.cuda.synchronize()
    start = threading.Barrier(2)
    results, errors, failures = [[], []], [[], []], []

    def work(slot):
        try:
            start.wait(timeout=30)
            with torch.cuda.stream(streams[slot]):
                for _ in range(10):
                    results[slot].append(tuple(t.clone() for t in search(qs[slot], spaces[slot])))
                    if slot == 0:
                        with pytest.raises(_lib.MerizoHipError):
                            ops.ip_topk(qs[0], qs[0], 0, workspace=spaces[0])                 # k = 0: refused, nothing launched
                    errors[slot].append(lib.ms_last_error() or b"")
            streams[slot].synchronize()
        except BaseException as exc:          # noqa: BLE001 -- reported by the main thread
            failures.append((slot, repr(exc)))

    threads = [threading.Thread(target=work, args=(slot,)) for slot in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not failures, failures
    assert all(e != b"" for e in errors[0]) and all(e == b"" for e in errors[1]), errors
    for slot in range(2):
        assert len(results[slot]) == 10
        for got in results[slot]:
            assert torch.equal(got[1], serial[slot][1]) and torch.equal(got[0].view(torch.int32), serial[slot][0].view(torch.int32)), slot


# ------------------------------------------------------------------ 4. one encoder, two streams ----
def test_one_encoder_serves_two_streams_one_after_the_other(torch_gpu, sleep_cycles_per_ms):
    """ops.EgnnEncoder keeps ONE staging buffer and ONE workspace.  embed records an event behind its last launch and the next call's
    stream waits on it before it touches either, so a call on a second stream queues behind the kernels of the first instead of
    overwriting what they still read.  The first call sits behind a delay on S1, the second is issued at once on S2; both batches have
    the same lengths (a race could corrupt values only, never an offset) and other coordinates; both results equal their default-stream
    results bit for bit."""
    torch = torch_gpu
    from merizo_search_amd import ops
    from merizo_search_amd.foldclass import weights as W
    weights, pe = W.pack_state_dict(W.synthetic_state_dict(0))
    enc = ops.EgnnEncoder(weights, pe, "cuda:0")
    batches = [sc._egnn_coords("A"), sc._egnn_coords("B")]
    want = [enc.embed(b).clone() for b in batches]
    torch.cuda.synchronize()
    assert not torch.equal(want[0], want[1])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s, b in ((s1, batches[0]), (s2, batches[1])):          # (warms each stream's allocator pool)
        with torch.cuda.stream(s):
            enc.embed(b)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        torch.cuda._sleep(int(1.25 * MIN_DELAY_MS * sleep_cycles_per_ms))
        first = enc.embed(batches[0])
    with torch.cuda.stream(s2):
        second = enc.embed(batches[1])
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), want[0].view(torch.int32)), "the call on S1 was disturbed by the call on S2"
    assert torch.equal(second.view(torch.int32), want[1].view(torch.int32)), "the call on S2"
