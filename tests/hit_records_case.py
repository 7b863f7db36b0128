"""The hit-record case (TEST INFRASTRUCTURE): one db-search of dbquery_case's 120-row database against itself per layout, and a
`search` of three of its rows, on the oracle engine with md_case's stand-in aligner -- the runs whose files and result dicts
tests/golden/hit_records/ holds as the code before the one hit-record path (dbsearch.hit_records) wrote them.

    python tests/hit_records_case.py DIR      records the files into DIR (how the golden ones were made)

Every branch of the hit-record step is populated: hits at or above mintm, hits below it (the faiss layout keys them by ONE
counter over the run), `.pt` hits dropped by the coverage rule, ranks below mincos, lists that the exclusion left short."""
import json
import os
import sys

import numpy as np

LAYOUTS = ("fa", "pt")
SUFFIXES = ("_search.tsv", "_search_insignificant.tsv", "_search.tsv.hit_metadata.json", "_search_insignificant.tsv.hit_metadata.json")
QUERY_ROWS = (12, 31, 57)             # the rows `search` is run with
REFUSED_LEN = 44                      # the stub GPU aligner refuses every pair whose target has this many residues


def write_database(work):
    import dbquery_case as dq
    return dq.write_case(work, n=120, seed=5)


def db_search(work, layout, out, batch=64, skip=False, backend="auto"):
    """The case's db-search of `layout` against itself -> {suffix: the bytes of <out><suffix>}."""
    import dbquery_case as dq
    from merizo_search_amd.foldclass import dbsearch as ds
    Engine = dq.install_oracle_drop()
    p = os.path.join(work, layout)
    ds.run_dbsearch_db(p, p, out, os.path.join(work, "tmp"), "cuda", engine=Engine(), topk=4, mincos=0.05, mintm=0.5, mincov=0.7,
                       query_rows="10:60", exclude_same_chain=True, report_insignificant_hits=True, header=True,
                       metadata_json=True, query_batchsize=batch, skip_tmalign=skip, tmalign_backend=backend)
    return {suffix: open(out + suffix, "rb").read() for suffix in SUFFIXES}


def stand_in_output(n_query: int, n_target: int) -> dict:
    """What extract_tmalign_values makes of md_case.fake_tmalign's output for chains of these lengths."""
    tm = 0.9 if n_query == n_target else 0.2
    return {"len_ali": min(n_query, n_target), "rmsd": 1.0, "seq_id": 0.5, "qtm": tm, "ttm": tm}


def align_many_stub(items, fast=False, device="cuda"):
    """tmalign.align_many's stand-in: the stand-in binary's rule per (coords, seq, coords, seq); None for a target of REFUSED_LEN."""
    return [None if len(ts) == REFUSED_LEN else stand_in_output(len(qc), len(tc)) for qc, _qs, tc, ts in items]


def search_queries(work):
    """Three rows of the case as the query dicts of `search` (inputs_are_ca)."""
    from merizo_search_amd.foldclass.dbrecords import Records
    rec = Records(os.path.join(work, "pt"))
    rows = list(QUERY_ROWS)
    out = [{"coords": np.asarray(c, np.float32), "seq": s, "name": "/q/%s.pdb" % n}
           for c, s, n in zip(rec.coords(rows), rec.seqs(rows), rec.names(rows))]
    rec.close()
    return out


def search(work, layout):
    """run_dbsearch of search_queries against `layout` with the stand-in binary -> (results, all_results)."""
    from oracle_engine import oracle_network
    from merizo_search_amd.foldclass import dbsearch as ds
    return ds.run_dbsearch(search_queries(work), os.path.join(work, layout), os.path.join(work, "tmp"), "cpu", topk=6, fastmode=False,
                           threads=-1, mincos=0.0, mintm=0.5, mincov=0.7, inputs_are_ca=True, network=oracle_network(0))


def as_json(results) -> str:
    """One side of run_dbsearch's result as text, one line per query: its [key, hit] pairs in dict order, the score as %.6f."""
    def plain(v):
        return v.item() if isinstance(v, np.generic) else v
    return "".join(json.dumps([[plain(key), {f: ("%.6f" % hit[f] if f == "score" else plain(hit[f])) for f in hit}]
                               for key, hit in per_query.items()], sort_keys=True) + "\n" for per_query in results)


def record(golden):
    """Write the golden files: <layout>[_skip]<suffix> of db_search, <layout>_search[_all].json of search."""
    import tempfile

    import md_case
    work = tempfile.mkdtemp()
    write_database(work)
    os.environ["MERIZO_TMALIGN"] = md_case.fake_tmalign(work)
    os.makedirs(golden, exist_ok=True)
    for layout in LAYOUTS:
        for tag, skip in (("", False), ("_skip", True)):
            for suffix, data in db_search(work, layout, os.path.join(work, "rec_" + layout + tag), skip=skip).items():
                with open(os.path.join(golden, layout + tag + suffix), "wb") as handle:
                    handle.write(data)
        for name, side in zip(("_search.json", "_search_all.json"), search(work, layout)):
            with open(os.path.join(golden, layout + name), "w") as handle:
                handle.write(as_json(side))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[1])
