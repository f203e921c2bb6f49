"""Python CLI, same contract as ./final (stdin -> "#i: score: S, n: N, k: K" lines), over torch.distributed:

    python -m mpi_openmp_cuda_amd < input.txt
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m mpi_openmp_cuda_amd \
        --input input.txt

Only rank 0 reads the input and writes the output (PDF p.5).
"""
from __future__ import annotations

import argparse
import json
import sys

from .models.problem import Problem
from .models.scoring import Semantics
from .parallel import dist as D
from .parallel.search import DistributedSearch
from .utils.io import (format_hits, format_report, format_summary, format_targets, format_targets_hits,
                       format_targets_rank, format_targets_summary, format_targets_topk, format_topk,
                       write_results)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="mpi_openmp_cuda_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input", default="-", help="input file (default: stdin)")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "cpu"])
    ap.add_argument("--transport", default="auto", choices=["auto", "shm", "bcast"],
                    help="shm: node-shared window (one node); bcast: every record broadcast (--partition=offsets "
                         "only). Record slices between nodes: ./final --transport=rccl (the retired p2p transport "
                         "of this driver moved into ./final's device batch)")
    ap.add_argument("--partition", default="auto", choices=["auto", "records", "offsets"],
                    help="records: cost-balanced record ranges (one node); offsets: context parallel (split every "
                         "record; the only partition across nodes here). auto: records on one node, else offsets")
    ap.add_argument("--dist-backend", default="auto", choices=["auto", "nccl", "gloo"])
    ap.add_argument("--semantics", default="reference", choices=["reference", "spec"])
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--strict-limits", action="store_true")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--top", type=int, default=1, metavar="K",
                    help="print every record's K best offsets (1..64): rank 1 as always, ranks j >= 2 as "
                         "'#i.j: score: S, n: N, k: K'. Record slices on one node only (--partition records)")
    ap.add_argument("--show-alignment", action="store_true",
                    help="after every result line print the alignment it stands for: the sign counts, the piece of "
                         "Seq1, the marker line and the record with its hyphen. With --top K or without; record "
                         "slices on one node only (--partition records)")
    hits = ap.add_mutually_exclusive_group()
    hits.add_argument("--min-score", type=int, default=None, metavar="T",
                      help="after every result line print that record's threshold hits, every offset whose best "
                           "candidate scores at least T, as '  hit: score: S, n: N, k: K' in ascending n. Not with "
                           "--top K > 1 or --show-alignment; record slices on one node only (--partition records)")
    hits.add_argument("--within", type=int, default=None, metavar="D",
                      help="the same for every offset within D >= 0 of the record's own best score")
    ap.add_argument("--distinct", type=int, default=None, metavar="R",
                    help="with --top K or --min-score / --within: distinct placements only — an offset is printed "
                         "only when no offset within R of it (0..2048) scores higher, or the same at a smaller n, so "
                         "the one-column shadow of a placement and the rest of its slope drop out. Same line "
                         "formats, fewer lines; R = 0 prints what no flag prints")
    ap.add_argument("--summary", action="store_true",
                    help="after every result line print '  summary: offsets: C, min: A, max: B, mean: M, sd: S, z: Z': "
                         "the record's candidate offsets, the extremes, mean and standard deviation of their scores, "
                         "and how many standard deviations of the other offsets the best one lies above them (nan when "
                         "undefined). Not with --top K > 1, --show-alignment, --min-score or --within; record slices "
                         "on one node only (--partition records)")
    ap.add_argument("--hist", default=None, metavar="LO:WIDTH:BINS",
                    help="with --summary: one more line '  hist: c0 c1 ...', the counts of the record's scores in BINS "
                         "(1..256) bins of WIDTH (>= 1) from LO up; scores outside land in the first and last bin (a "
                         "negative LO takes the = form, --hist=-50:10:16)")
    ap.add_argument("--targets", default=None, metavar="FILE",
                    help="multi-target search: FILE holds one more target sequence per line (letters, as Seq1). The "
                         "target set is the input's own Seq1 as target 1, then the file's lines; under every "
                         "result line print one line per target, '  target t: score: S, n: N, k: K' with n relative "
                         "to that target, or '  target t: none' where the record is longer than the target, and a "
                         "final '  best: t'. No placement straddles two targets. Not with --top K > 1, "
                         "--show-alignment, --min-score, --within, --distinct, --summary or --hist; record slices on "
                         "one node only (--partition records)")
    ap.add_argument("--target-summary", action="store_true",
                    help="with --targets: under each '  target t: ...' line print '    summary: offsets: C, min: A, "
                         "max: B, mean: M, sd: S, z: Z', the --summary line of the record against that target alone, "
                         "and after '  best: t' a line '  best by z: t' (or 'none'): the target whose best score lies "
                         "the most standard deviations above the rest of its own profile")
    ap.add_argument("--target-hist", default=None, metavar="LO:WIDTH:BINS",
                    help="with --target-summary: one more line '    hist: c0 c1 ...' per target, the bins of --hist")
    ap.add_argument("--target-top", type=int, default=None, metavar="K",
                    help="with --targets: the K (1..64) best placements of the record inside every target; under each "
                         "'  target t: ...' line (rank 1) print '    top j: score: S, n: N, k: K' for the ranks j >= 2 "
                         "that exist. Not with --target-summary, --target-min-score or --target-within")
    ap.add_argument("--target-min-score", type=int, default=None, metavar="T",
                    help="with --targets: under each '  target t: ...' line print '    hit: score: S, n: N, k: K' for "
                         "every placement inside that target that scores at least T (an int32; a negative T takes the "
                         "= form), by ascending n. Not with --target-summary, --target-top or --target-within")
    ap.add_argument("--target-within", type=int, default=None, metavar="D",
                    help="with --targets: as --target-min-score with every (record, target) pair's own threshold, that "
                         "target's best score minus D (D >= 0). Not with --target-summary, --target-top or "
                         "--target-min-score")
    ap.add_argument("--target-distinct", type=int, default=None, metavar="R",
                    help="with --targets and --target-top K (K > 1) or --target-min-score / --target-within: distinct "
                         "placements inside every target only — a placement is printed only when no placement of the "
                         "same target within R of it (0..2048) scores higher, or the same at a smaller n; the windows "
                         "end at the target's own first and last placement. Same line formats, fewer lines; R = 0 "
                         "prints what no flag prints")
    ap.add_argument("--target-best", type=int, default=None, metavar="M",
                    help="with --targets: only each record's M (1..64) best targets; under the record's line print "
                         "'  best j: target t: score: S, n: N, k: K' for j = 1 .. min(M, targets the record fits), "
                         "the higher score first, then the smaller t, or '  best: none' when no target fits — and none "
                         "of the per-target lines. Not with --target-top, --target-min-score, --target-within, "
                         "--target-summary, --target-hist or --target-distinct")
    a = ap.parse_args(argv)
    if not 1 <= a.top <= 64:
        ap.error("--top K: K must be in 1..64")
    want_hits = a.min_score is not None or a.within is not None
    if want_hits and (a.top > 1 or a.show_alignment):
        ap.error("--min-score / --within do not combine with --top K > 1 or --show-alignment")
    if a.within is not None and a.within < 0:
        ap.error("--within D: D must be >= 0")
    if a.distinct is not None:
        if not 0 <= a.distinct <= 2048:
            ap.error("--distinct R: R must be in 0..2048")
        if not want_hits and a.top <= 1:
            ap.error("--distinct R filters the lines of --top K (K > 1) or --min-score / --within: give one of them")
    radius = a.distinct or 0
    hist_args = (0, 0, 1)
    if a.hist is not None:
        if not a.summary:
            ap.error("--hist LO:WIDTH:BINS needs --summary")
        try:
            h_lo, h_width, h_bins = (int(x) for x in a.hist.split(":"))
        except ValueError:
            ap.error("--hist LO:WIDTH:BINS: three integers separated by colons")
        if not (-2 ** 31 <= h_lo < 2 ** 31 and 1 <= h_width < 2 ** 31 and 1 <= h_bins <= 256):
            ap.error("--hist LO:WIDTH:BINS: LO an int32, WIDTH an int32 >= 1, BINS in 1..256")
        hist_args = (h_bins, h_lo, h_width)
    if a.target_summary and a.targets is None:
        ap.error("--target-summary needs --targets FILE")
    target_hist_args = (0, 0, 1)
    if a.target_hist is not None:
        if not a.target_summary:
            ap.error("--target-hist LO:WIDTH:BINS needs --target-summary")
        try:
            h_lo, h_width, h_bins = (int(x) for x in a.target_hist.split(":"))
        except ValueError:
            ap.error("--target-hist LO:WIDTH:BINS: three integers separated by colons")
        if not (-2 ** 31 <= h_lo < 2 ** 31 and 1 <= h_width < 2 ** 31 and 1 <= h_bins <= 256):
            ap.error("--target-hist LO:WIDTH:BINS: LO an int32, WIDTH an int32 >= 1, BINS in 1..256")
        target_hist_args = (h_bins, h_lo, h_width)
    if a.summary and (a.top > 1 or a.show_alignment or want_hits):
        ap.error("--summary does not combine with --top K > 1, --show-alignment, --min-score or --within")
    if a.min_score is not None and not -2 ** 31 <= a.min_score < 2 ** 31:
        ap.error("--min-score T: T must be an int32")
    target_rows_flags = [f for f, v in (("--target-top", a.target_top), ("--target-min-score", a.target_min_score),
                                        ("--target-within", a.target_within)) if v is not None]
    if target_rows_flags:
        if a.targets is None:
            ap.error(f"{target_rows_flags[0]} needs --targets FILE")
        if len(target_rows_flags) > 1 or a.target_summary:
            ap.error("--target-top, --target-min-score, --target-within and --target-summary exclude each other")
        if a.target_top is not None and not 1 <= a.target_top <= 64:
            ap.error("--target-top K: K must be in 1..64")
        if a.target_min_score is not None and not -2 ** 31 <= a.target_min_score < 2 ** 31:
            ap.error("--target-min-score T: T must be an int32")
        if a.target_within is not None and a.target_within < 0:
            ap.error("--target-within D: D must be >= 0")
    if a.target_distinct is not None:
        if not 0 <= a.target_distinct <= 2048:
            ap.error("--target-distinct R: R must be in 0..2048")
        if a.targets is None or not (a.target_min_score is not None or a.target_within is not None or
                                     (a.target_top or 0) > 1):
            ap.error("--target-distinct R filters the lines of --targets FILE with --target-top K (K > 1) or "
                     "--target-min-score / --target-within: give one of them")
    target_radius = a.target_distinct or 0
    if a.target_best is not None:
        if a.targets is None:
            ap.error("--target-best needs --targets FILE")
        if target_rows_flags or a.target_summary or a.target_hist is not None or a.target_distinct is not None:
            ap.error("--target-best does not combine with --target-top, --target-min-score, --target-within, "
                     "--target-summary, --target-hist or --target-distinct")
        if not 1 <= a.target_best <= 64:
            ap.error("--target-best M: M must be in 1..64")
    if a.targets is not None:
        if a.top > 1 or a.show_alignment or want_hits or a.distinct is not None or a.summary or a.hist is not None:
            ap.error("--targets does not combine with --top K > 1, --show-alignment, --min-score, --within, "
                     "--distinct, --summary or --hist")
        if a.partition == "offsets":
            ap.error("--targets needs record slices (--partition records, one node); --partition offsets combines "
                     "one packed key per record")

    from .ops.align import device_count

    use_gpu = a.backend == "hip" or (a.backend == "auto" and device_count() > 0)
    ctx = D.init(a.dist_backend, use_gpu=use_gpu and a.dist_backend != "gloo")
    rc = 0
    problem = None
    own_problem = None  # --target-best: the input as it came, for the records' own lines
    target_set = None
    err = ""
    if ctx.is_root:
        try:
            data = sys.stdin.buffer.read() if a.input == "-" else open(a.input, "rb").read()
            problem = Problem.parse(data, a.strict_limits)
            if a.targets is not None:
                from .ops.align import TargetSet

                with open(a.targets, "r", encoding="ascii") as f:
                    lines = [ln.strip() for ln in f.read().splitlines()]
                lines = [ln for ln in lines if ln]
                if a.strict_limits and any(len(ln) > 3000 for ln in lines):
                    raise ValueError("--targets: a target sequence is longer than 3000 letters")
                target_set = TargetSet.from_sequences([problem.seq1] + [TargetSet.from_strings([ln]).seq1 for ln in lines])
                own_problem = problem
                problem = Problem(problem.weights, target_set.seq1, problem.codes, problem.offsets)
        except Exception as e:  # report, then make every rank exit consistently
            err = str(e)
    import numpy as np

    status = D.bcast_array(ctx, np.array([1 if err else 0], np.int64) if ctx.is_root else None, 1, np.int64)
    if int(status[0]):
        if ctx.is_root:
            print(f"input error: {err}", file=sys.stderr)
        D.finalize(ctx)
        return 1
    search = DistributedSearch(ctx, backend="hip" if use_gpu else "cpu", transport=a.transport, threads=a.threads,
                               partition=a.partition)
    if a.top > 1 and search.partition != "records":
        if ctx.is_root:
            print("--top K > 1 needs record slices (--partition records, one node); --partition offsets combines "
                  "one candidate per record", file=sys.stderr)
        D.finalize(ctx)
        return 2
    if a.show_alignment and search.partition != "records":
        if ctx.is_root:
            print("--show-alignment needs record slices (--partition records, one node); --partition offsets "
                  "combines one packed key per record", file=sys.stderr)
        D.finalize(ctx)
        return 2
    if want_hits and search.partition != "records":
        if ctx.is_root:
            print("--min-score / --within need record slices (--partition records, one node); --partition offsets "
                  "combines one packed key per record", file=sys.stderr)
        D.finalize(ctx)
        return 2
    if a.summary and search.partition != "records":
        if ctx.is_root:
            print("--summary needs record slices (--partition records, one node); --partition offsets combines one "
                  "packed key per record", file=sys.stderr)
        D.finalize(ctx)
        return 2
    if a.targets is not None and search.partition != "records":
        if ctx.is_root:
            print("--targets needs record slices (--partition records, one node); --partition offsets combines one "
                  "packed key per record", file=sys.stderr)
        D.finalize(ctx)
        return 2
    hit_rows = None
    summary = None
    target_rows = None
    target_summary = None
    target_topk = None
    target_hits = None
    target_rank = None
    if a.targets is not None:
        try:
            if a.target_best is not None:
                target_rank = search.run_targets_rank(problem, target_set, a.target_best, Semantics.parse(a.semantics))
            elif a.target_top is not None:
                target_topk = search.run_targets_topk(problem, target_set, a.target_top, Semantics.parse(a.semantics),
                                                      target_radius)
            elif a.target_min_score is not None or a.target_within is not None:
                target_hits = search.run_targets_hits(problem, target_set, a.target_min_score, a.target_within,
                                                      Semantics.parse(a.semantics), target_radius)
            elif a.target_summary:
                target_summary = search.run_targets_summary(problem, target_set, *target_hist_args,
                                                            semantics=Semantics.parse(a.semantics))
            else:
                target_rows = search.run_targets(problem, target_set, Semantics.parse(a.semantics))
        except ValueError as e:  # an invalid target set (more than 4096 targets) or the exactness bound: every rank raises it
            if ctx.is_root:
                print(f"input error: {e}", file=sys.stderr)
            D.finalize(ctx)
            return 1
        # the records' own lines are the search against the input's Seq1 alone (target 1), which a ranking may not list
        results = search.run(own_problem, Semantics.parse(a.semantics)) if a.target_best is not None else None
    elif a.summary:
        try:
            summary = search.run_summary(problem, *hist_args, semantics=Semantics.parse(a.semantics))
        except ValueError as e:  # the exactness bound: every rank raises it
            if ctx.is_root:
                print(f"input error: {e}", file=sys.stderr)
            D.finalize(ctx)
            return 1
        results = None
    elif want_hits:
        got = search.run_hits(problem, a.min_score, a.within, Semantics.parse(a.semantics), radius)
        results, hit_rows = (got[0], got[1:]) if ctx.is_root else (None, None)
    elif a.top > 1:
        results = search.run_topk(problem, a.top, Semantics.parse(a.semantics), radius)
    else:
        results = search.run(problem, Semantics.parse(a.semantics))
    if ctx.is_root:
        if a.show_alignment:
            from .ops.align import as_triples

            rows = results if a.top > 1 else as_triples(results)
            counts, marks = search.report(problem, rows)
            sys.stdout.write(format_report(problem, rows, counts, marks))
            sys.stdout.flush()
        elif a.top > 1:
            sys.stdout.write(format_topk(results))
            sys.stdout.flush()
        elif want_hits:
            sys.stdout.write(format_hits(results, *hit_rows))
            sys.stdout.flush()
        elif a.summary:
            sys.stdout.write(format_summary(*summary))
            sys.stdout.flush()
        elif a.target_summary:
            sys.stdout.write(format_targets_summary(*target_summary))
            sys.stdout.flush()
        elif target_rank is not None:
            sys.stdout.write(format_targets_rank(results, target_rank))
            sys.stdout.flush()
        elif target_topk is not None:
            sys.stdout.write(format_targets_topk(target_topk[:, 0, 0], target_topk))
            sys.stdout.flush()
        elif target_hits is not None:
            sys.stdout.write(format_targets_hits(target_hits[0][:, 0], *target_hits))
            sys.stdout.flush()
        elif a.targets is not None:
            sys.stdout.write(format_targets(target_rows[:, 0], target_rows))
            sys.stdout.flush()
        else:
            write_results(results)
        if a.timing:
            print(json.dumps({"timing": json.loads(search.timer.json()), "ranks": ctx.world,
                              "backend": search.backend, "transport": search.transport}), file=sys.stderr)
    D.barrier(ctx)
    D.finalize(ctx)
    return rc


if __name__ == "__main__":
    sys.exit(main())
