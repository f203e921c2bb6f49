"""Cost of threshold hits next to the calls they build on, on device-resident batches (no PCIe in the loop).
Every figure is the median over --reps (>= 10) repetitions, after --warmup, of the device time between the events
the engine records around its launches (HipSearchEngine.device_kernel_ms: the host's per-call planning is outside
the bracket). All calls of a shape run in one process on one engine, interleaved per repetition.

Per shape:
  (p) solve_profile_device: the sweep with one 8-byte store per offset and no selection (unchunked);
  (h) solve_hits_device at a batch-wide threshold that roughly 1 % and roughly 50 % of the profile's entries reach
      (the 0.99 and 0.5 quantiles of its scores), cap = the exact total: device time, the share of count + scan +
      compact in it (MOC_PROFILE_TIMING=1 event pairs around those launches), hits and row bytes written;
  (t) solve_topk_device at K = 1 and K = 64.

  python tools/bench_hits.py [--reps 10] [--warmup 2] [--markdown] [shape[:records] ...]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

from mpi_openmp_cuda_amd import HipSearchEngine, make_synthetic  # noqa: E402

CASES = {"input3": 1 << 13, "input4": 1 << 13, "input6": 1 << 20}
FRACTIONS = (0.01, 0.5)


def run(shape, n, reps, warmup):
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
    calls = {"p_profile": lambda: eng.solve_profile_device(codes_t, offs_t, prob.offsets, prof_t)}
    hits_of = {}
    for f in FRACTIONS:
        T = int(scores[min(entries - 1, int(round((1 - f) * entries)))])
        _, h_t = eng.solve_hits_device(codes_t, offs_t, prob.offsets, min_score=T, cap=0)
        torch.cuda.synchronize()
        total = int(h_t[-1])
        rows_t = torch.empty((max(total, 1), 3), dtype=torch.int32, device=dev)
        name = f"h_hits_{int(100 * f)}pct"
        hits_of[name] = (T, total)
        calls[name] = lambda T=T, total=total, rows_t=rows_t, h_t=h_t: eng.solve_hits_device(
            codes_t, offs_t, prob.offsets, min_score=T, cap=total, rows_t=rows_t, hoffsets_t=h_t)
    del scores
    for K in (1, 64):
        top_t = torch.empty((prob.n, K, 3), dtype=torch.int32, device=dev)
        calls[f"t_top{K}"] = lambda K=K, top_t=top_t: eng.solve_topk_device(codes_t, offs_t, prob.offsets, K, top_t)
    ms = {k: [] for k in calls}
    sel = {k: [] for k in calls}
    for it in range(warmup + reps):
        for k, call in calls.items():
            call()
            t = eng.device_kernel_ms()
            if it >= warmup:
                ms[k].append(t)
                sel[k].append(eng.hits_select_ms() if k != "p_profile" else 0.0)
    for k in calls:
        row[k + "_ms"] = statistics.median(ms[k])
        if k != "p_profile":
            row[k + "_select_ms"] = statistics.median(sel[k])
            row[k + "_select_share"] = row[k + "_select_ms"] / row[k + "_ms"]
        if k in hits_of:
            row[k + "_threshold"], row[k + "_hits"] = hits_of[k]
            row[k + "_fraction"] = hits_of[k][1] / max(entries, 1)
            row[k + "_row_bytes"] = 12 * hits_of[k][1]
            row[k + "_over_profile"] = row[k + "_ms"] / row["p_profile_ms"]
    row["chunks"] = int(eng.stats()["chunks"])
    eng.close()
    return row


def markdown(rows):
    out = ["| shape | records | profile entries | (p) profile ms | (h) 1 % ms (select share; rows MB) | "
           "(h) 50 % ms (select share; rows MB) | (t) K=1 ms (select) | (t) K=64 ms (select) |",
           "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        h = " | ".join(f"{r[k + '_ms']:.3f} ({100 * r[k + '_select_share']:.0f} %; {r[k + '_row_bytes'] / 1e6:.1f})"
                       for k in ("h_hits_1pct", "h_hits_50pct"))
        t = " | ".join(f"{r[k + '_ms']:.3f} ({100 * r[k + '_select_share']:.0f} %)" for k in ("t_top1", "t_top64"))
        out.append(f"| {r['shape']} | {r['records']} | {r['profile_entries']} | {r['p_profile_ms']:.3f} | {h} | {t} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shapes", nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--markdown", action="store_true", help="print the table after the JSON lines")
    a = ap.parse_args()
    rows = []
    for s in a.shapes:
        shape, _, n = s.partition(":")
        rows.append(run(shape, int(n) if n else CASES[shape], max(a.reps, 10), a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if a.markdown:
        print(markdown(rows))


if __name__ == "__main__":
    main()
