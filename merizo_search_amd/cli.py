"""Command line: `search`, `easy-search`, `createdb` with the reference's arguments, `db-search`, `chain-search` and `cluster`.

Mirror of merizo_search/merizo.py for the Foldclass path (search :126-226, easy_search :229-407,
createdb :102-123).  `segment` (the Merizo IPA network) is out of scope: easy-search takes the
chopping as an input (--chopping / --segment_tsv) instead of predicting it.

    python -m merizo_search_amd.cli search  <pdb...> <db_name> <output> <tmp> [-d cuda] [-k 10] ...
    python -m merizo_search_amd.cli createdb <input_dir> <out_db> [-d cuda] [--layout pt|faiss|both]
    python -m merizo_search_amd.cli easy-search <pdb...> <db_name> <output> <tmp> --chopping "71-189,190-290"
    python -m merizo_search_amd.cli db-search <query_db> <target_db> <output> <tmp> [-k 10] [--exclude_self] ...
    python -m merizo_search_amd.cli chain-search <query_db> <target_db> <output> <tmp> [-s 0.5] [--exclude_same_chain] ...
    python -m merizo_search_amd.cli cluster <db_name> <output> <tmp> -s 0.8 [-k 20] [-c 0.7] [--complete] [--cluster_mode connected [--tree] [--levels 0.85,0.9]] [-m 0.5 [-f]] ...

`--multi_domain_search` (search, easy-search, db-search) also writes `<output>_search_multi_dom.tsv`: the target chains that match
every domain of a query chain.  `--multi_domain_mode exhaustive_tmalign` (the reference's; search and easy-search) aligns every
query domain with every domain of every hit chain and needs a TM-align binary or `--tmalign_backend hip`;
`exhaustive_cosine` (the only mode of db-search, where the query chains are the runs of adjacent query rows with one chain id)
scores those pairs with the search's own embedding score on the GPU and needs neither (foldclass/multidomain.py).
`database_cosine` (search and easy-search) gives exhaustive_cosine's answer for the WHOLE database -- every target chain, not only
the chains the top-k lists name -- from one more pass over the rows on the GPU: it needs no aligner and does not depend on -k.

`--multi_domain_report best` (all four commands; the two embedding-score modes) writes per (query chain, hit chain) pair the best
any-order mapping with its score and, when that one breaks the domain order, the best order-preserving one -- solved on the GPU
(ms_md_best_mappings), pairs ranked per query chain, no pair skipped for having too many mappings; the default `all` lists every mapping.

`db-search` has no counterpart in the reference: it searches the stored embeddings of one database against another (or
against itself), in batches of thousands of queries, without parsing or embedding a structure (foldclass/dbquery.py).
`chain-search` is `database_cosine` with a whole database as the query side: for every multi-domain chain of query_db (the runs of
adjacent rows with one chain id) every chain of target_db that matches all its domains, whatever -k would have been -- the file
`db-search --multi_domain_search` writes when -k covers the whole target -- with thousands of query domains per pass over the
target's rows on the 16-bit matrix pipe (foldclass/chainsearch.py).
`cluster` has none either: it makes a database non-redundant from the neighbour lists of that self-search (foldclass/cluster.py).

Several GPUs of one node: start one process per GPU with torchrun,

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m merizo_search_amd.cli search ...

Every rank then uses GPU LOCAL_RANK (whatever -d says), holds and scans 1/N of the database rows, the
per-shard top-k lists are exchanged with one RCCL all-gather, and rank 0 writes the output files
(foldclass/sharded.py; replaces the reference's index_cpu_to_all_gpus, dbsearch.py:228-230).
"""
from __future__ import annotations

import argparse
import logging
import os
import shutil
import sys
import time
import uuid

from .foldclass import chopping as chop
from .foldclass import sharded
from .foldclass.dbsearch import run_dbsearch
from .foldclass.makedb import run_createdb
from .foldclass.results import (EASY_SEARCH_FIELDS, SEARCH_FIELDS, check_for_database, embedding_only_format, parse_output_format,
                                write_search_results, write_segment_results)

logging.basicConfig(level=logging.INFO, format="%(asctime)s | %(levelname)s | %(message)s")


def munge_tmp_with_uuid(tmp: str) -> str:
    return os.path.join(tmp, str(uuid.uuid4()))


def _add_report_flag(p: argparse.ArgumentParser) -> None:
    p.add_argument("--multi_domain_report", type=str, default="all", choices=["all", "best"],
                   help="What <output>_search_multi_dom.tsv holds. 'all': every one-to-one mapping of a (query chain, hit chain) pair "
                        "(pairs with more than a million candidate mappings are skipped). 'best': per pair the best any-order mapping "
                        "with its score and, when that one breaks the domain order, the best order-preserving one -- solved on the GPU, "
                        "no pair is skipped; needs one of the embedding-score modes (exhaustive_cosine, database_cosine).")


def _check_report(args) -> None:
    """A report the multi-domain mode cannot serve is refused here, before any work (no database is opened, no GPU call made)."""
    if args.multi_domain_search:
        from .foldclass.multidomain import check_report
        try:
            check_report(args.multi_domain_report, args.multi_domain_mode)
        except ValueError as exc:
            logging.error(str(exc))
            sys.exit(1)


def _add_search_flags(p: argparse.ArgumentParser, default_format: str) -> None:
    p.add_argument("-d", "--device", type=str, default="cuda", help="'cuda' / 'cuda:N' = the MI355X. 'cpu' is refused by this build.")
    p.add_argument("-k", "--topk", type=int, default=1, help="Max number of domain matches to return per query domain.")
    p.add_argument("-t", "--threads", type=int, default=-1, help="Accepted for compatibility; unused.")
    p.add_argument("-s", "--mincos", type=float, default=0.5, help="Minimum cosine similarity of reported hits.")
    p.add_argument("-m", "--mintm", type=float, default=0.5, help="Minimum TM-align score of reported hits.")
    p.add_argument("-c", "--mincov", type=float, default=0.7, help="Minimum coverage of database matches.")
    p.add_argument("-f", "--fastmode", action="store_true", help="TM-align -fast.")
    p.add_argument("--format", type=str, default=default_format, help="Comma-separated output columns.")
    p.add_argument("--output_headers", action="store_true", default=False)
    p.add_argument("--pdb_chain", type=str, dest="pdb_chain", default="A")
    p.add_argument("--search_batchsize", type=int, default=262144)
    p.add_argument("--search_metric", type=str, default="IP")
    p.add_argument("--report_insignificant_hits", action="store_true", default=False)
    p.add_argument("--metadata_json", action="store_true", default=False)
    p.add_argument("--multi_domain_search", action="store_true", default=False,
                   help="Search DB for entries that match all query domains (all query structures are treated as single "
                        "domains coming from one chain).  'exhaustive_tmalign' needs a TM-align binary ($MERIZO_TMALIGN) or "
                        "--tmalign_backend hip.")
    p.add_argument("--multi_domain_mode", type=str, default="exhaustive_tmalign",
                   choices=["exhaustive_tmalign", "exhaustive_cosine", "database_cosine"],
                   help="If --multi_domain_search is used, specifies the multi-domain search mode. 'exhaustive_tmalign': TM-align "
                        "every query domain with every domain of every hit chain. 'exhaustive_cosine': score those pairs with "
                        "the search's own embedding score on the GPU instead (entries below --mincos count as no match); needs "
                        "no TM-align binary. 'database_cosine': exhaustive_cosine's scores and output for EVERY chain of the database, "
                        "found by one pass over all its rows on the GPU; needs no aligner and does not depend on -k.")
    _add_report_flag(p)
    p.add_argument("--skip_tmalign", action="store_true", default=False,
                   help="Embedding-only search (automatic when no TM-align binary is found and --tmalign_backend is auto).")
    p.add_argument("--tmalign_backend", type=str, default="auto", choices=["auto", "hip"],
                   help="'auto': the TM-align binary ($MERIZO_TMALIGN) if one is found, else an embedding-only search. "
                        "'hip': TM-align every hit on the GPU in one batch (needs a cuda device). --skip_tmalign wins over both.")
    p.add_argument("--weights", type=str, default=None, help="Path to FINAL_foldclass_model.pt.")


# The reference's easy-search also takes the Merizo segmenter's options (merizo.py:262-286).  The segmenter is out of scope
# here (the chopping is an input), but a reference command line must still parse: every one of them is accepted with the
# reference's type and default, and reported as ignored when the user set it.
_SEGMENTER_FLAGS = (
    ("--merizo_output", dict(type=str, default=os.environ.get("PWD", "."))),
    ("--save_pdf", dict(action="store_true", default=False)),
    ("--save_pdb", dict(action="store_true", default=False)),
    ("--save_domains", dict(action="store_true", default=False)),
    ("--save_fasta", dict(action="store_true", default=False)),
    ("--conf_filter", dict(type=float, default=None)),
    ("--plddt_filter", dict(type=float, default=None)),
    ("--iterate", dict(action="store_true", default=False)),
    ("--length_conditional_iterate", dict(action="store_true", default=False)),
    ("--max_iterations", dict(type=int, default=3)),
    ("--shuffle_indices", dict(action="store_true", default=False)),
    ("--return_indices", dict(action="store_true", default=False)),
    ("--min_domain_size", dict(type=int, default=50)),
    ("--min_fragment_size", dict(type=int, default=10)),
    ("--domain_ave_size", dict(type=int, default=200)),
    ("--conf_threshold", dict(type=float, default=0.5)),
)


def _add_segmenter_flags(p: argparse.ArgumentParser) -> None:
    g = p.add_argument_group("Merizo segmenter options (accepted for command-line compatibility with the reference, ignored: "
                             "the chopping is an input of this build)")
    for flag, kw in _SEGMENTER_FLAGS:
        g.add_argument(flag, help="Ignored.", **kw)


def _warn_ignored_segmenter_flags(args) -> None:
    given = [flag for flag, kw in _SEGMENTER_FLAGS if getattr(args, flag[2:]) != kw["default"]]
    if given:
        logging.warning("Ignoring the Merizo segmenter option(s) %s: the segmenter is not part of this build, domains come "
                        "from --chopping / --segment_tsv." % ", ".join(given))


def _join_process_group(args) -> None:
    """Under torchrun (WORLD_SIZE > 1): join the process group before the first GPU call and pin this
    rank to its GPU; ranks other than 0 log warnings only."""
    rank, world, device = sharded.init_distributed()
    if world > 1:
        args.device = device
        if rank != 0:
            logging.getLogger().setLevel(logging.WARNING)
        logging.info(f"{world} ranks, one GPU each: database rows are sharded, rank 0 writes the results.")


def _log_command(mode: str) -> None:
    logging.info("Starting %s with command: \n\n%s\n" % (mode, " ".join(f'"{a}"' if " " in a else a for a in sys.argv)))


def _embedding_only_format(fields, skip):
    return embedding_only_format(fields, skip)


def _search_and_write(args, inputs, inputs_are_ca, pdb_chain, fields, tmp):
    from .foldclass import tmalign as tm
    if args.tmalign_backend == "hip" and not str(args.device).startswith("cuda"):
        logging.error("--tmalign_backend hip runs TM-align on the GPU: it needs a cuda device, got -d %s." % args.device)
        sys.exit(1)
    hip = args.tmalign_backend == "hip"
    skip = args.skip_tmalign or (not hip and tm.find_tmalign() is None)
    search_output = args.output + "_search.tsv"
    all_output = args.output + "_search_insignificant.tsv"
    for path in (search_output, all_output):
        if os.path.exists(path):
            logging.warning(f"Search output file '{path}' already exists. Results will be overwritten!")
    multi_output = args.output + "_search_multi_dom.tsv"
    cosine_md = args.multi_domain_search and args.multi_domain_mode in ("exhaustive_cosine", "database_cosine")
    database_md = args.multi_domain_search and args.multi_domain_mode == "database_cosine"
    if args.multi_domain_search:
        if not cosine_md and not hip and tm.find_tmalign() is None:
            logging.error("--multi_domain_search aligns every query domain with every candidate target domain and needs a "
                          "TM-align binary (set $MERIZO_TMALIGN).")
            sys.exit(1)
        if os.path.exists(multi_output):
            logging.warning(f"Multi-domain search output file '{multi_output}' already exists. Results will be overwritten!")
    network = None
    if cosine_md:       # the multi-domain step re-embeds the query domains with the encoder the search runs with
        from .foldclass import dbsearch as _ds
        network, _device = _ds.network_setup(threads=args.threads, device=args.device, weights_path=args.weights)
    target_db = None
    if database_md:     # ONE open (and one upload) of the database for the search and for the multi-domain step's scan of all rows
        target_db = _ds.read_database(db_name=args.db_name, device=args.device, engine=network.engine)
    results, all_results = run_dbsearch(
        target_db=target_db, network=network, inputs=inputs, db_name=args.db_name, tmp=tmp, device=args.device, topk=args.topk, fastmode=args.fastmode,
        threads=args.threads, mincos=args.mincos, mintm=args.mintm, mincov=args.mincov, inputs_are_ca=inputs_are_ca,
        pdb_chain=pdb_chain, search_batchsize=args.search_batchsize, search_type=args.search_metric,
        skip_tmalign=skip, weights_path=args.weights, tmalign_backend=args.tmalign_backend)
    md_kwargs = dict(queries=inputs, db_name=args.db_name, tmp_root=tmp, device=args.device, fastmode=args.fastmode, threads=args.threads,
                     mintm=args.mintm, inputs_from_easy_search=inputs_are_ca, mode=args.multi_domain_mode, pdb_chain=pdb_chain,
                     tmalign_backend=args.tmalign_backend, mincos=args.mincos, mincov=args.mincov, network=network,
                     report=args.multi_domain_report)
    mda = None
    if database_md:     # every rank scans its shard of the database and takes part in the gather; the mode reads no search_results
        from .foldclass.multidomain import multi_domain_search
        mda = multi_domain_search(search_results=None, target_db=target_db, search_batchsize=args.search_batchsize, **md_kwargs)
    if sharded.rank_world()[0] != 0:
        return                                            # every rank searched its shard; rank 0 reports
    fields = _embedding_only_format(fields, skip)
    write_search_results(results=results, output_file=search_output, format_list=fields, header=args.output_headers,
                         metadata_json=args.metadata_json)
    if args.report_insignificant_hits:
        write_search_results(results=all_results, output_file=all_output, format_list=fields, header=args.output_headers,
                             metadata_json=args.metadata_json)
    if args.multi_domain_search:
        # merizo.py:207-222 / :396-411.  `search`: the inputs are single-domain files of ONE chain (the reference
        # passes inputs_from_easy_search=True here, which fails on file names; its stated intent is one chain 'A').
        from .foldclass.multidomain import multi_domain_search
        from .foldclass.results import multi_dom_writer
        if not database_md:
            mda = multi_domain_search(search_results=results, **md_kwargs)
        multi_dom_writer(args.multi_domain_report)(mda, multi_output, args.output_headers)


def search(argv) -> None:
    p = argparse.ArgumentParser(prog="search", description="Search query PDBs against a Foldclass database on the GPU.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("input", type=str, nargs="+")
    p.add_argument("db_name", type=str)
    p.add_argument("output", type=str)
    p.add_argument("tmp", type=str)
    _add_search_flags(p, SEARCH_FIELDS)
    args = p.parse_args(argv)
    _check_report(args)
    _join_process_group(args)
    tmp = munge_tmp_with_uuid(args.tmp)
    _log_command("search")
    check_for_database(args.db_name)
    fields = parse_output_format(args.format, SEARCH_FIELDS)
    t0 = time.time()
    os.makedirs(tmp, exist_ok=True)
    _search_and_write(args, args.input, False, args.pdb_chain, fields, tmp)
    logging.info(f"Finished search in {time.time() - t0} seconds.")
    shutil.rmtree(tmp, ignore_errors=True)


def easy_search(argv) -> None:
    p = argparse.ArgumentParser(prog="easy-search", description="Chop each input chain into domains (chopping supplied) "
                                "and search every domain.", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("input", type=str, nargs="+")
    p.add_argument("db_name", type=str)
    p.add_argument("output", type=str)
    p.add_argument("tmp", type=str)
    _add_search_flags(p, EASY_SEARCH_FIELDS)
    p.add_argument("--chopping", type=str, action="append", default=None,
                   help="Domain chopping of the corresponding input, reference syntax e.g. '71-189,190-290,291-453' "
                        "(repeat the flag once per input).")
    p.add_argument("--segment_tsv", type=str, default=None, help="A reference `_segment.tsv` to take the choppings from.")
    _add_segmenter_flags(p)
    args = p.parse_args(argv)
    _check_report(args)
    _warn_ignored_segmenter_flags(args)
    _join_process_group(args)
    tmp = munge_tmp_with_uuid(args.tmp)
    _log_command("easy-search")
    check_for_database(args.db_name)
    fields = parse_output_format(args.format, EASY_SEARCH_FIELDS)
    chains = args.pdb_chain.rstrip(",").split(",")
    if len(chains) != len(args.input):
        if len(chains) == 1:
            chains = chains * len(args.input)
        else:
            logging.error("Number of specified chain IDs not equal to number of input PDB files.")
            sys.exit(1)
    if args.segment_tsv:
        table = chop.read_segment_tsv(args.segment_tsv)
        choppings = [table.get(os.path.basename(pth).replace(".pdb", "")) for pth in args.input]
    else:
        choppings = args.chopping or []
    if len(choppings) != len(args.input) or any(c is None for c in choppings):
        logging.error("easy-search needs one chopping per input (--chopping ... or --segment_tsv): the Merizo segmenter "
                      "is not part of this build.")
        sys.exit(1)
    t0 = time.time()
    os.makedirs(tmp, exist_ok=True)
    domains, seg_rows = [], []
    for pth, chain, chopping in zip(args.input, chains, choppings):
        t1 = time.time()
        doms = chop.domains_from_chopping(pth, chopping, chain)
        domains.extend(doms)
        seg_rows.append(chop.segment_row(pth, chopping, chain, runtime=time.time() - t1))
    if sharded.rank_world()[0] == 0:
        write_segment_results(results=seg_rows, output_file=args.output + "_segment.tsv", header=args.output_headers)
    if not domains:
        logging.info("easy-search finished after segmentation: no domains to search.")
        return
    _search_and_write(args, domains, True, None, fields, tmp)
    logging.info(f"Finished easy-search in {time.time() - t0:.3f} seconds.")
    shutil.rmtree(tmp, ignore_errors=True)


def db_search(argv) -> None:
    p = argparse.ArgumentParser(prog="db-search", description="Search the entries of one Foldclass database against another "
                                "database (or against itself) on the GPU: the stored embeddings are the queries.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("query_db", type=str, help="Database prefix whose rows are the queries (either layout).")
    p.add_argument("target_db", type=str, help="Database prefix to search (either layout; may be query_db itself).")
    p.add_argument("output", type=str)
    p.add_argument("tmp", type=str)
    p.add_argument("-d", "--device", type=str, default="cuda", help="'cuda' / 'cuda:N' = the MI355X. 'cpu' is refused by this build.")
    p.add_argument("-k", "--topk", type=int, default=1, help="Max number of domain matches to return per query domain.")
    p.add_argument("-s", "--mincos", type=float, default=0.5, help="Minimum cosine similarity of reported hits.")
    p.add_argument("-m", "--mintm", type=float, default=0.5, help="Minimum TM-align score of reported hits.")
    p.add_argument("-c", "--mincov", type=float, default=0.7, help="Minimum coverage of database matches.")
    p.add_argument("-f", "--fastmode", action="store_true", help="TM-align -fast.")
    p.add_argument("--format", type=str, default=SEARCH_FIELDS, help="Comma-separated output columns.")
    p.add_argument("--output_headers", action="store_true", default=False)
    p.add_argument("--search_batchsize", type=int, default=262144, help="Target rows per block when the target is streamed.")
    p.add_argument("--report_insignificant_hits", action="store_true", default=False)
    p.add_argument("--metadata_json", action="store_true", default=False)
    p.add_argument("--skip_tmalign", action="store_true", default=False,
                   help="Embedding-only search (automatic when no TM-align binary is found and --tmalign_backend is auto).")
    p.add_argument("--tmalign_backend", type=str, default="auto", choices=["auto", "hip"],
                   help="'auto': the TM-align binary ($MERIZO_TMALIGN) if one is found, else an embedding-only search. "
                        "'hip': TM-align every hit of a query batch on the GPU in one launch. --skip_tmalign wins over both.")
    p.add_argument("--query_batchsize", type=int, default=4096, help="Queries per scan call.")
    p.add_argument("--query_rows", type=str, default=None, metavar="LO:HI", help="Rows of query_db to search (default: all).")
    p.add_argument("--exclude_self", action="store_true", default=False,
                   help="query_db and target_db are the same database: never report a query as its own hit.")
    p.add_argument("--exclude_same_chain", action="store_true", default=False,
                   help="query_db and target_db are the same database: report no domain of the query's own chain "
                        "(implies --exclude_self).")
    p.add_argument("--multi_domain_search", action="store_true", default=False,
                   help="Also search for target chains that match ALL domains of a query chain (the runs of adjacent query rows "
                        "with one chain id) and write <output>_search_multi_dom.tsv.")
    p.add_argument("--multi_domain_mode", type=str, default="exhaustive_cosine", choices=["exhaustive_cosine"],
                   help="The multi-domain search mode: every query domain against every domain of every hit chain, scored with "
                        "the search's own embedding score on the GPU (entries below --mincos count as no match).")
    _add_report_flag(p)
    args = p.parse_args(argv)
    _join_process_group(args)
    tmp = munge_tmp_with_uuid(args.tmp)
    _log_command("db-search")
    from .foldclass.dbsearch import run_dbsearch_db
    fields = parse_output_format(args.format, SEARCH_FIELDS)
    t0 = time.time()
    n = run_dbsearch_db(query_db=args.query_db, db_name=args.target_db, output=args.output, tmp=tmp, device=args.device,
                        topk=args.topk, fastmode=args.fastmode, mincos=args.mincos, mintm=args.mintm, mincov=args.mincov,
                        search_batchsize=args.search_batchsize, skip_tmalign=args.skip_tmalign, tmalign_backend=args.tmalign_backend,
                        query_batchsize=args.query_batchsize, query_rows=args.query_rows, exclude_self=args.exclude_self,
                        exclude_same_chain=args.exclude_same_chain, format_list=fields,
                        header=args.output_headers, metadata_json=args.metadata_json,
                        report_insignificant_hits=args.report_insignificant_hits, multi_domain_search=args.multi_domain_search,
                        multi_domain_mode=args.multi_domain_mode, multi_domain_report=args.multi_domain_report)
    logging.info(f"Finished db-search of {n} queries in {time.time() - t0:.3f} seconds.")
    shutil.rmtree(tmp, ignore_errors=True)


def chain_search_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="chain-search", description="Every multi-domain match between two Foldclass databases: for each "
                                "chain of query_db with 2-64 domains (adjacent rows with one chain id), every chain of target_db that "
                                "matches ALL its domains at or above --mincos, from passes over all target rows on the GPU.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("query_db", type=str, help="Database prefix whose chains are the queries (either layout).")
    p.add_argument("target_db", type=str, help="Database prefix to search (either layout; may be query_db itself).")
    p.add_argument("output", type=str, help="Writes <output>_search_multi_dom.tsv.")
    p.add_argument("tmp", type=str)
    p.add_argument("-d", "--device", type=str, default="cuda", help="'cuda' / 'cuda:N' = the MI355X. 'cpu' is refused by this build.")
    p.add_argument("-s", "--mincos", type=float, default=0.5, help="Minimum cosine similarity of a matching domain pair.")
    p.add_argument("-c", "--mincov", type=float, default=0.7, help="Minimum coverage of database matches (the `.pt` layout's mask).")
    p.add_argument("--query_batchsize", type=int, default=4096, help="Query rows (whole query chains) per pass over the target.")
    p.add_argument("--search_batchsize", type=int, default=262144, help="Target rows per block when the target is streamed.")
    p.add_argument("--query_rows", type=str, default=None, metavar="LO:HI", help="Rows of query_db to take the query chains from.")
    p.add_argument("--exclude_same_chain", action="store_true", default=False,
                   help="query_db and target_db are the same database: a query chain is never its own match.")
    p.add_argument("--output_headers", action="store_true", default=False)
    _add_report_flag(p)
    return p


def chain_search(argv) -> None:
    args = chain_search_parser().parse_args(argv)
    _join_process_group(args)
    tmp = munge_tmp_with_uuid(args.tmp)
    _log_command("chain-search")
    from .foldclass.chainsearch import run_chain_search
    t0 = time.time()
    n = run_chain_search(query_db=args.query_db, db_name=args.target_db, output=args.output, tmp=tmp, device=args.device,
                         mincos=args.mincos, mincov=args.mincov, query_batchsize=args.query_batchsize,
                         search_batchsize=args.search_batchsize, query_rows=args.query_rows,
                         exclude_same_chain=args.exclude_same_chain, output_headers=args.output_headers,
                         report=args.multi_domain_report)
    logging.info(f"Finished chain-search of {n} query chains in {time.time() - t0:.3f} seconds.")
    shutil.rmtree(tmp, ignore_errors=True)


def cluster(argv) -> None:
    p = argparse.ArgumentParser(prog="cluster", description="Make a Foldclass database non-redundant on the GPU: search it against "
                                "itself, pick representatives greedily (the longer domain first) and assign every other domain "
                                "to its best-scoring representative.", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("db_name", type=str, help="Database prefix to cluster (either layout).")
    p.add_argument("output", type=str)
    p.add_argument("tmp", type=str)
    p.add_argument("-d", "--device", type=str, default="cuda", help="'cuda' / 'cuda:N' = the MI355X. 'cpu' is refused by this build.")
    p.add_argument("-k", "--topk", type=int, default=20, help="Neighbours kept per domain.")
    p.add_argument("-s", "--mincos", type=float, required=True,
                   help="Minimum cosine similarity of two domains of one cluster (no default: choose it for your database).")
    p.add_argument("-c", "--mincov", type=float, default=0.7, help="Minimum length of the shorter domain relative to the longer.")
    p.add_argument("--query_batchsize", type=int, default=4096, help="Rows per scan call.")
    p.add_argument("--search_batchsize", type=int, default=262144, help="Target rows per block when the database is streamed.")
    p.add_argument("--output_headers", action="store_true", default=False)
    p.add_argument("--complete", action="store_true", default=False,
                   help="Cluster the full threshold graph, whatever -k: domains whose -k neighbours all reach --mincos get ALL their "
                        "neighbours from one more pass over the database.")
    p.add_argument("--cluster_mode", type=str, default="greedy", choices=("greedy", "connected"),
                   help="greedy: representatives picked greedily, every other domain with its best adjacent representative. connected: "
                        "the connected components of the same neighbour graph (single linkage), the longest domain of each as its "
                        "representative; with --complete the true components, whatever -k.")
    p.add_argument("--max_edges", type=int, default=2 ** 27,
                   help="--complete: directed neighbour entries that pass may hold (20 bytes of device memory each); beyond it the run is refused.")
    p.add_argument("-m", "--mintm", type=float, default=None,
                   help="Verify every edge with TM-align on the GPU: two domains are neighbours only if max(q_tm, t_tm) reaches this "
                        "value, in (0, 1]. Off when not given: the embedding cosine alone decides.")
    p.add_argument("-f", "--fastmode", action="store_true", default=False, help="--mintm: run TM-align in its fast mode (-fast).")
    p.add_argument("--tree", action="store_true", default=False,
                   help="--cluster_mode connected: also write <output>_cluster_tree.tsv, the single-linkage tree of the neighbour graph "
                        "(its maximum spanning forest): cut at any cosine >= --mincos it gives the components at that cosine.")
    p.add_argument("--levels", type=str, default=None, metavar="T1,T2,...",
                   help="--cluster_mode connected: cut the tree at these cosines (each >= --mincos) and write "
                        "<output>_cluster_<T>.tsv per level: the file a run at --mincos T writes, from one search. Implies --tree.")
    args = p.parse_args(argv)
    _join_process_group(args)
    tmp = munge_tmp_with_uuid(args.tmp)
    _log_command("cluster")
    from .foldclass.cluster import run_cluster
    t0 = time.time()
    run_cluster(db_name=args.db_name, output=args.output, tmp=tmp, device=args.device, topk=args.topk, mincos=args.mincos,
                mincov=args.mincov, query_batchsize=args.query_batchsize, search_batchsize=args.search_batchsize,
                header=args.output_headers, complete=args.complete, max_edges=args.max_edges, mode=args.cluster_mode,
                mintm=args.mintm, fastmode=args.fastmode, tree=args.tree,
                levels=None if args.levels is None else args.levels.split(","))
    logging.info(f"Finished cluster in {time.time() - t0:.3f} seconds.")
    shutil.rmtree(tmp, ignore_errors=True)


def createdb(argv) -> None:
    p = argparse.ArgumentParser(prog="createdb", description="Embed a directory of PDB files into a Foldclass database.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("input_dir", type=str)
    p.add_argument("out_db", type=str)
    p.add_argument("-d", "--device", type=str, default="cuda")
    p.add_argument("--layout", type=str, default="pt", choices=["pt", "faiss", "both"])
    p.add_argument("--weights", type=str, default=None)
    args = p.parse_args(argv)
    _join_process_group(args)
    _log_command("createdb")
    t0 = time.time()
    run_createdb(pdb_files=args.input_dir, out_db=args.out_db, device=args.device, layout=args.layout, weights_path=args.weights)
    logging.info(f"Finished createdb in {time.time() - t0} seconds.")


def main(argv=None) -> None:
    argv = sys.argv[1:] if argv is None else argv
    modes = {"search": search, "easy-search": easy_search, "createdb": createdb, "db-search": db_search, "chain-search": chain_search,
             "cluster": cluster}
    if not argv or argv[0] not in modes:
        print("usage: python -m merizo_search_amd.cli {search,easy-search,createdb,db-search,chain-search,cluster} ...  "
              "(segment: out of scope, use the reference)", file=sys.stderr)
        sys.exit(2)
    modes[argv[0]](argv[1:])
    sharded.finalize_distributed()        # (a rank that fails exits on its own; torchrun then ends the others)


if __name__ == "__main__":
    main()
