"""dbrecords.Records, the one host-side reader of a database's rows, on a 12-row database written in both on-disk layouts from
the same inputs, once with metadata and once without: every accessor, as a range and as a row list, against the written input;
the per-row conveniences against the accessors; lengths, the chain table, the dict's cached object; dbutil.Blob on a zero-byte
data file."""
import os

import numpy as np
import pytest

from merizo_search_amd.foldclass import dbsearch as ds
from merizo_search_amd.foldclass import dbutil, synthetic as syn
from merizo_search_amd.foldclass.dbrecords import Records

# adjacent rows of one chain, a chain id that comes back (A), and one name of exactly NAME_WIDTH characters
CHAINS = ["A", "A", "A", "B", "C", "C", "A", "W" * (dbutil.NAME_WIDTH - 6), "D", "D", "E", "B"]
NAMES = ["%s_TED%02d" % (c, i + 1) for i, c in enumerate(CHAINS)]
N = len(NAMES)
LENGTHS = [7, 31, 12, 6, 40, 9, 23, 18, 6, 11, 35, 8]
SEQS = ["".join("ACDEFGHIKL"[(r + i) % 10] for i in range(l)) for r, l in enumerate(LENGTHS)]
COORDS = [syn.random_walk(l, 100 + r) for r, l in enumerate(LENGTHS)]
METADATA = ['{ "row": %d }' % r for r in range(N)]
METADATA[4] = ""                                                          # one empty metadata string
FORMS = [(0, N), (5, 6), (2, 9), (3, 3), ([],), ([7, 2, 7, 0],)]        # ranges, the empty range, the empty list, descending + duplicate


def _expected(values, form):
    return values[form[0]:form[1]] if len(form) == 2 else [values[r] for r in form[0]]


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("dbrecords"))
    rng = np.random.default_rng(3)
    raw = rng.standard_normal((N, 128)).astype(np.float32)
    norm = raw / np.linalg.norm(raw, axis=1, keepdims=True)
    for tag, metadata in (("md", METADATA), ("plain", None)):
        dbutil.write_faiss_db(os.path.join(work, "fa_" + tag), norm, NAMES, SEQS, COORDS, metadata)
        dbutil.write_pt_db(os.path.join(work, "pt_" + tag), raw, ["dir/" + n + ".pdb" for n in NAMES], COORDS, SEQS, metadata)
    return work


def test_the_case_is_the_one_asked_for():
    assert N == 12 and len(NAMES[7]) == dbutil.NAME_WIDTH and max(len(n) for n in NAMES) == dbutil.NAME_WIDTH
    assert CHAINS[0] == CHAINS[1] == CHAINS[2] == CHAINS[6] != CHAINS[5] and "" in METADATA


@pytest.mark.parametrize("tag", ["md", "plain"])
@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_every_accessor_returns_the_written_input(written, layout, tag):
    rec = Records(os.path.join(written, layout + "_" + tag))
    assert rec.faiss == (layout == "fa") and rec.n == N
    stored = NAMES if layout == "fa" else ["dir/" + n + ".pdb" for n in NAMES]
    metadata = METADATA if tag == "md" else ["{ }"] * N
    for form in FORMS:
        assert rec.stored_names(*form) == _expected(stored, form), form
        assert rec.names(*form) == _expected(NAMES, form), form
        assert rec.seqs(*form) == _expected(SEQS, form), form
        assert rec.metadata(*form) == _expected(metadata, form), form
        got, want = rec.coords(*form), _expected(COORDS, form)
        assert len(got) == len(want) and all(g.dtype == np.float32 and np.array_equal(g, w) for g, w in zip(got, want)), form
    assert rec.names(np.asarray([7, 2, 7, 0], dtype=np.int64)) == [NAMES[r] for r in (7, 2, 7, 0)]       # (an int array as the row list)
    entries = [rec.entry(r) for r in range(N)]
    assert rec.names(0, N) == [e[0] for e in entries] == [rec.entry_name(r) for r in range(N)]
    for r, e in enumerate(entries):
        assert rec.name_meta(r) == (e[0], e[4]) and e[3] == r and rec.name(r) == stored[r]
        assert np.array_equal(e[1], COORDS[r]) and e[2] == SEQS[r] and e[4] == metadata[r]
    lengths = rec.lengths()
    assert lengths.dtype == np.int32 and lengths.tolist() == [len(s) for s in SEQS]
    starts = rec.chain_starts()
    assert starts.tolist() == [r for r in range(N) if r == 0 or CHAINS[r] != CHAINS[r - 1]] + [N] and rec.chain_starts() is starts
    rec.close()
    rec.close()                                                           # (a second close is harmless)


@pytest.mark.parametrize("layout", ["fa", "pt"])
def test_the_dict_keeps_one_records_object(written, layout):
    d = ds.read_database(os.path.join(written, layout + "_md"))
    rec = Records.of(d)
    assert Records.of(d) is rec and rec.n == N and rec.metadata([4, 1]) == ["", METADATA[1]]
    if layout == "pt":
        assert rec.index is d["index"]
    plain = Records.of(ds.read_database(os.path.join(written, layout + "_plain")))
    assert plain is not rec and plain.metadata(0, 2) == ["{ }", "{ }"]
    for r in (rec, plain):
        r.close()
        r.close()


def test_blob_serves_a_zero_byte_data_file(tmp_path):
    index, data = str(tmp_path / "empty.index"), str(tmp_path / "empty.db")
    np.asarray([[0, 0]], dtype=np.int64).tofile(index)
    open(data, "wb").close()
    blob = dbutil.Blob(index, data)
    assert blob.fetch([0], dbutil.ascii_conv) == [""] and blob.fetch(slice(0, 1), dbutil.ascii_conv) == [""]
    assert blob.offsets([0, 0]).tolist() == [[0, 0], [0, 0]] and blob.offsets([]).shape == (0, 2)
    blob.close()
    blob.close()
