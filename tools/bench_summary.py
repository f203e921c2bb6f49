"""Cost of the profile summary next to the calls it builds on, on device-resident batches (no PCIe in the loop).
Every device figure is the median over --reps (>= 10) repetitions, after --warmup, of the device time between the
events the engine records around its launches (HipSearchEngine.device_kernel_ms: the host's per-call planning is
outside the bracket). All calls of a shape run in one process on one engine, interleaved per repetition.

Per shape:
  (p) solve_profile_device: the sweep with one 8-byte store per offset and no reduction (unchunked);
  (s) solve_summary_device at bins = 0 and bins = 64: device time and the share of the summary (+ histogram)
      launches in it (MOC_PROFILE_TIMING=1 event pairs around those launches), and the bytes that come out;
  (h) solve_hits_device with cap = 0 (counts only), the nearest existing reduction, at the 0.5 quantile;
  (u) the use case without the feature: solve_profile (host form, the whole profile over PCIe) plus the numpy
      reduction to the same five numbers per record, wall clock, next to solve_summary (host form), wall clock.

  python tools/bench_summary.py [--reps 10] [--warmup 2] [--markdown] [--profile-only] [shape[:records] ...]

--profile-only times (p) alone: the one row a library without the summary can give (the parent commit's build through
MOC_LIB_PATH), to show that the sweep itself did not move.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

from mpi_openmp_cuda_amd import HipSearchEngine, make_synthetic  # noqa: E402

CASES = {"input3": 1 << 13, "input4": 1 << 13, "input6": 1 << 20}
BINS = 64


def numpy_reduction(prof, po):
    """count, sum, sumsq, min, max per record from the flat profile, vectorised (records without offsets skipped)."""
    s = prof["score"].astype(np.int64)
    has = np.diff(po) > 0
    at = po[:-1][has]
    return (np.diff(po), np.add.reduceat(s, at), np.add.reduceat(s * s, at), np.minimum.reduceat(s, at),
            np.maximum.reduceat(s, at))


def run(shape, n, reps, warmup, profile_only=False):
    prob = make_synthetic(shape, n, seed=7)
    L2 = prob.lengths.astype(np.int64)
    dev = torch.device("cuda:0")
    codes_t = torch.from_numpy(prob.codes).to(dev)
    offs_t = torch.from_numpy(prob.offsets).to(dev)
    os.environ["MOC_PROFILE_TIMING"] = "1"  # read when the engine starts
    eng = HipSearchEngine(device=0)
    eng.set_problem(prob.weights, prob.seq1)
    poffsets = eng.profile_offsets(prob.offsets)
    entries = int(poffsets[-1])
    row = {"shape": shape, "records": prob.n, "L1": prob.L1, "mean_L2": float(L2.mean()), "profile_entries": entries,
           "profile_bytes": 8 * entries}
    prof_t = torch.empty((entries, 2), dtype=torch.int32, device=dev)
    eng.solve_profile_device(codes_t, offs_t, prob.offsets, prof_t)
    torch.cuda.synchronize()
    scores = prof_t[:, 0].sort().values
    lo, hi, T = int(scores[0]), int(scores[-1]), int(scores[entries // 2])
    del scores
    width = max((hi - lo + BINS) // BINS, 1)
    s_t = torch.empty((prob.n, 7), dtype=torch.int64, device=dev)
    hist_t = torch.empty((prob.n, BINS), dtype=torch.int32, device=dev)
    h_t = torch.empty(prob.n + 1, dtype=torch.int64, device=dev)
    calls = {
        "p_profile": lambda: eng.solve_profile_device(codes_t, offs_t, prob.offsets, prof_t),
        "s_summary_0": lambda: eng.solve_summary_device(codes_t, offs_t, prob.offsets, 0, 0, 1, s_t),
        f"s_summary_{BINS}": lambda: eng.solve_summary_device(codes_t, offs_t, prob.offsets, BINS, lo, width, s_t,
                                                              hist_t),
        "h_hits_count": lambda: eng.solve_hits_device(codes_t, offs_t, prob.offsets, min_score=T, cap=0,
                                                      hoffsets_t=h_t),
    }
    if profile_only:
        calls = {"p_profile": calls["p_profile"]}
    ms = {k: [] for k in calls}
    sel = {k: [] for k in calls}
    for it in range(warmup + reps):
        for k, call in calls.items():
            call()
            t = eng.device_kernel_ms()
            if it >= warmup:
                ms[k].append(t)
                sel[k].append(eng.summary_ms() if k != "p_profile" else 0.0)
    for k in calls:
        row[k + "_ms"] = statistics.median(ms[k])
        if k != "p_profile":
            row[k + "_select_ms"] = statistics.median(sel[k])
            row[k + "_select_share"] = row[k + "_select_ms"] / row[k + "_ms"]
            row[k + "_over_profile"] = row[k + "_ms"] / row["p_profile_ms"]
    if profile_only:
        eng.close()
        return row
    row["summary_out_bytes"] = 56 * prob.n
    row["hist_out_bytes"] = 4 * BINS * prob.n
    row["hist_lo"], row["hist_width"] = lo, width
    row["chunks"] = int(eng.stats()["chunks"])
    # the use case end to end from host memory, wall clock: the whole profile to the host and numpy, or the summary
    wall = {"u_profile_numpy": [], "u_summary_host": []}
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        prof, po = eng.solve_profile(prob.codes, prob.offsets)
        numpy_reduction(prof, po)
        t1 = time.perf_counter()
        eng.solve_summary(prob.codes, prob.offsets)
        t2 = time.perf_counter()
        if it >= warmup:
            wall["u_profile_numpy"].append(1e3 * (t1 - t0))
            wall["u_summary_host"].append(1e3 * (t2 - t1))
    for k, v in wall.items():
        row[k + "_wall_ms"] = statistics.median(v)
    eng.close()
    return row


def markdown(rows):
    out = ["| shape | records | profile entries | (p) profile ms | (s) bins = 0: ms (summary share) | "
           f"(s) bins = {BINS}: ms (summary share) | (h) hits cap = 0: ms (share) | (u) profile + numpy wall ms | "
           "(u) solve_summary wall ms |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        c = " | ".join(f"{r[k + '_ms']:.3f} ({100 * r[k + '_select_share']:.0f} %)"
                       for k in ("s_summary_0", f"s_summary_{BINS}", "h_hits_count"))
        out.append(f"| {r['shape']} | {r['records']} | {r['profile_entries']} | {r['p_profile_ms']:.3f} | {c} | "
                   f"{r['u_profile_numpy_wall_ms']:.1f} | {r['u_summary_host_wall_ms']:.1f} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shapes", nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--markdown", action="store_true", help="print the table after the JSON lines")
    ap.add_argument("--profile-only", action="store_true", help="time solve_profile_device alone")
    a = ap.parse_args()
    rows = []
    for s in a.shapes:
        shape, _, n = s.partition(":")
        rows.append(run(shape, int(n) if n else CASES[shape], max(a.reps, 10), a.warmup, a.profile_only))
        print(json.dumps(rows[-1]), flush=True)
    if a.markdown and not a.profile_only:
        print(markdown(rows))


if __name__ == "__main__":
    main()
