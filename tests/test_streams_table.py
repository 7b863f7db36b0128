"""The stream case table stays complete (no GPU): every entry point that takes a stream has a case in stream_case.TABLE or a reason
in stream_case.EXCLUDED, so a new entry point fails here until it gets a stream case."""
import stream_case as sc


def test_the_header_and_the_binding_name_the_same_streamed_entry_points():
    from merizo_search_amd import _lib
    streamed = sc.streamed_entry_points()
    assert len(streamed) >= 30 and "ms_ip_topk" in streamed and "ms_tmalign_batch" in streamed and "ms_version" not in streamed
    missing = [name for name in streamed if name not in _lib.SIGNATURES]
    assert not missing, f"declared in the header, not bound: {missing}"
    for name in streamed:                  # the stream is the last argument of the binding too: a pointer
        assert _lib.SIGNATURES[name][1][-1] is _lib._vp, name


def test_every_streamed_entry_point_has_a_case_or_a_reason():
    streamed = set(sc.streamed_entry_points())
    covered = set(sc.TABLE) | set(sc.EXCLUDED)
    assert not streamed - covered, f"entry points that take a stream and have no stream case: {sorted(streamed - covered)}"
    assert not covered - streamed, f"the table names entry points that take no stream: {sorted(covered - streamed)}"
    assert not set(sc.TABLE) & set(sc.EXCLUDED)
    assert all(isinstance(why, str) and len(why) > 20 for why in sc.EXCLUDED.values())


def test_every_case_is_listed_and_says_whether_it_may_block():
    listed = {cid for ids in sc.TABLE.values() for cid in ids}
    assert listed == set(sc.CASES) and len(sc.CASES) == len(sc._CASES), "duplicate or unlisted case ids"
    for case in sc.CASES.values():
        assert case.entries and callable(case.build)
        assert case.asynchronous or len(case.sync_why) > 20, f"{case.id}: a case that may block names the line that says so"
    # the entry points the header calls asynchronous have at least one case that checks it; the cluster calls document their wait
    blocking = {"ms_cluster_greedy", "ms_cluster_greedy_edges", "ms_cluster_components", "ms_cluster_tree"}
    for name, ids in sc.TABLE.items():
        if name not in blocking:
            assert any(sc.CASES[cid].asynchronous for cid in ids), f"{name}: no case checks that the call returns at once"
