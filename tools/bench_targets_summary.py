"""Cost of the per-target profile summary next to the only route without it, T rounds of set_problem(target_t) +
solve_summary, and next to solve_targets on the same batch. All calls of a case run in one process, interleaved per
repetition; every figure is the median over --reps (>= 10) repetitions after --warmup, with the smallest and largest
repetition beside it.

Per shape (input3-, input4- and input6-shaped records) and per catalog (8 and 256 random targets of equal length,
the same total length for both, every target at least as long as the shape's own Seq1 — the catalogs of
tools/bench_targets.py):
  (s) solve_targets_summary, host form, bins = 0: one upload, one pass over the catalog profile, 56 n T bytes back;
      wall clock;
  (r) the T-round route, host forms: per target set_problem + solve_summary, wall clock; its stacked rows are also
      the correctness cross-check of (s) — the run stops if they differ;
  (g) solve_targets_summary_device on the device-resident batch with the lane-group size forced to 4, 16 and 64
      (MOC_TARGETS_GROUP, read when an engine starts) and with the host's own choice: device time between the engine's
      events, and the time and share of the summary launches in it (MOC_PROFILE_TIMING=1 event pairs around those
      launches); with the host's choice also at bins = 64 (summary + histogram launches), and solve_targets_device on
      the same engine: what the moments and the histogram cost over the select kernel. read_gbs: the slice entries'
      8 bytes each over the summary launches' time at bins = 0.

  python tools/bench_targets_summary.py [--reps 10] [--warmup 2] [--markdown] [--target-counts 8,256] [shape[:records] ...]

--target-counts: other divisors of 256 cut the same catalog into other target lengths — the sweep over slice lengths
against which the two cut-over constants of bounds::targets_group are checked for this kernel.
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

from mpi_openmp_cuda_amd import HipSearchEngine, TargetSet, make_synthetic  # noqa: E402

CASES = {"input3": 64, "input4": 512, "input6": 1 << 16}
TARGET_COUNTS = (8, 256)
GROUPS = (0, 4, 16, 64)  # 0: the host's own choice
HIST = (64, -200, 10)    # bins, lo, width of the histogram case


def engine_with(env):
    """An engine started under extra environment switches (they are read when the engine starts)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return HipSearchEngine(device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(shape, n, T, reps, warmup):
    prob = make_synthetic(shape, n, seed=7)
    L2 = prob.lengths.astype(np.int64)
    per = max(prob.L1, int(L2.max()) + 1)  # letters per target at the largest T: every record fits every target
    total = per * max(TARGET_COUNTS)
    rng = np.random.default_rng(11)
    ts = TargetSet.from_sequences(np.split(rng.integers(1, 27, total).astype(np.uint8), T))
    slice_entries = int((total // T - L2).clip(min=0).sum()) * T
    row = {"shape": shape, "records": prob.n, "T": T, "catalog": total, "target_len": total // T,
           "mean_L2": float(L2.mean()), "pairs": prob.n * T, "slice_entries": slice_entries}
    eng = engine_with({"MOC_PROFILE_TIMING": "1"})
    round_eng = HipSearchEngine(device=0)
    wall = {"s_summary": [], "r_rounds": []}
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        eng.set_problem(prob.weights, ts.seq1)
        summary, _ = eng.solve_targets_summary(prob.codes, prob.offsets, ts)
        t1 = time.perf_counter()
        per_target = []
        for t in range(T):
            round_eng.set_problem(prob.weights, ts.target(t))
            per_target.append(round_eng.solve_summary(prob.codes, prob.offsets)[0])
        t2 = time.perf_counter()
        if it == 0 and not np.array_equal(summary, np.stack(per_target, axis=1)):
            raise SystemExit(f"{shape} T={T}: solve_targets_summary differs from the T-round route")
        if it >= warmup:
            wall["s_summary"].append(1e3 * (t1 - t0))
            wall["r_rounds"].append(1e3 * (t2 - t1))
    for k, v in wall.items():
        row[k + "_wall_ms"] = spread(v)
    row["rounds_over_summary"] = row["r_rounds_wall_ms"]["median"] / row["s_summary_wall_ms"]["median"]
    row["chunks"] = int(eng.stats()["chunks"])
    round_eng.close()
    eng.close()
    # (g) the kernels per lane-group size, device-resident
    dev = torch.device("cuda:0")
    codes_t = torch.from_numpy(prob.codes).to(dev)
    offs_t = torch.from_numpy(prob.offsets).to(dev)
    rows_t = torch.empty((prob.n, T, 3), dtype=torch.int32, device=dev)
    sum_t = torch.empty((prob.n, T, 7), dtype=torch.int64, device=dev)
    hist_t = torch.empty((prob.n, T, HIST[0]), dtype=torch.int32, device=dev)
    engines = {g: engine_with({"MOC_PROFILE_TIMING": "1", **({"MOC_TARGETS_GROUP": str(g)} if g else {})}) for g in GROUPS}
    ms = {g: [] for g in GROUPS}
    part = {g: [] for g in GROUPS}
    extra = {"hist_device": [], "hist_kernels": [], "targets_device": [], "targets_select": []}
    for g, e in engines.items():
        e.set_problem(prob.weights, ts.seq1)
    for it in range(warmup + reps):
        for g, e in engines.items():
            e.solve_targets_summary_device(codes_t, offs_t, prob.offsets, ts, summary_t=sum_t)
            t = e.device_kernel_ms()
            if it >= warmup:
                ms[g].append(t)
                part[g].append(e.targets_summary_ms())
        e = engines[0]
        e.solve_targets_summary_device(codes_t, offs_t, prob.offsets, ts, *HIST, summary_t=sum_t, hist_t=hist_t)
        th, tk = e.device_kernel_ms(), e.targets_summary_ms()
        e.solve_targets_device(codes_t, offs_t, prob.offsets, ts, rows_t)
        tt, tsel = e.device_kernel_ms(), e.targets_ms()
        if it >= warmup:
            extra["hist_device"].append(th)
            extra["hist_kernels"].append(tk)
            extra["targets_device"].append(tt)
            extra["targets_select"].append(tsel)
    for g, e in engines.items():
        name = f"g{g}" if g else "g_auto"
        row[name + "_device_ms"] = spread(ms[g])
        row[name + "_summary_ms"] = spread(part[g])
        row[name + "_summary_share"] = row[name + "_summary_ms"]["median"] / row[name + "_device_ms"]["median"]
        e.close()
    for k, v in extra.items():
        row[k + "_ms"] = spread(v)
    row["read_gbs"] = 8 * slice_entries / (row["g_auto_summary_ms"]["median"] * 1e-3) / 1e9 if slice_entries else 0.0
    return row


def markdown(rows):
    out = ["| shape | records | T | (s) summary wall ms (min .. max) | (r) T rounds wall ms (min .. max) | (r) / (s) | "
           "summary ms at G = 4 / 16 / 64 / auto | share (auto) | read GB/s | select ms | + hist 64 ms |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        s, rr = r["s_summary_wall_ms"], r["r_rounds_wall_ms"]
        g = " / ".join(f"{r[k + '_summary_ms']['median']:.3f}" for k in ("g4", "g16", "g64", "g_auto"))
        out.append(f"| {r['shape']} | {r['records']} | {r['T']} | {s['median']:.2f} ({s['min']:.2f} .. {s['max']:.2f}) | "
                   f"{rr['median']:.2f} ({rr['min']:.2f} .. {rr['max']:.2f}) | {r['rounds_over_summary']:.2f} | {g} | "
                   f"{100 * r['g_auto_summary_share']:.0f} % | {r['read_gbs']:.0f} | "
                   f"{r['targets_select_ms']['median']:.3f} | {r['hist_kernels_ms']['median']:.3f} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shapes", nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--markdown", action="store_true", help="print the table after the JSON lines")
    ap.add_argument("--target-counts", default=",".join(str(t) for t in TARGET_COUNTS),
                    help="comma list of target counts, each a divisor of 256 (the catalog's length does not change)")
    a = ap.parse_args()
    rows = []
    counts = [int(t) for t in a.target_counts.split(",")]
    if any(t < 1 or max(TARGET_COUNTS) % t for t in counts):
        ap.error("--target-counts: divisors of 256")
    for s in a.shapes:
        shape, _, n = s.partition(":")
        for T in counts:
            rows.append(run(shape, int(n) if n else CASES[shape], T, max(a.reps, 10), a.warmup))
            print(json.dumps(rows[-1]), flush=True)
    if a.markdown:
        print(markdown(rows))


if __name__ == "__main__":
    main()
