"""Cost of the per-target distinct placements (radius > 0 on solve_targets_topk / solve_targets_hits) on input6-shaped
records: next to radius = 0 of the same call, next to the only route without it — T rounds of set_problem(target_t) +
solve_topk(radius) —, and per forced segment width of the peak pass. All calls of a case run in one process,
interleaved per repetition; every figure is the median over --reps (>= 10) repetitions after --warmup, with the
smallest and largest repetition beside it.

Per catalog (8 and 256 random targets of equal length, the same total length for both, every target at least as long as
the shape's own Seq1 — the catalogs of tools/bench_targets_rows.py: at T = 256 every pair profile has at most 64
entries and takes a lane segment, at T = 8 every one is long and takes a workgroup per tile):
  (g) solve_targets_topk_device(K = 4) and solve_targets_hits_device (thresholds = solve_targets_device's scores - 20,
      built on the device) on the device-resident batch at radius 0, 1, 20 and 2048 with the host's own segment width:
      device time between the engine's events, and the time of the launches behind the profile kernel in it
      (MOC_PROFILE_TIMING=1: peak pass + masked consumers, or the unmasked consumers at radius 0);
  (w) the same at radius 1 with the segment width forced to 4, 8, 16, 32 and 64 (MOC_TARGETS_PEAKS_SEG, read when an engine
      starts): a profile longer than a forced width goes to the tile kernel;
  (s) solve_targets_topk(K = 4, radius = 1), host form, wall clock;
  (r) the T-round route, host forms: per target set_problem + solve_topk(K = 4, radius = 1); wall clock. Its stacked
      rows are also the correctness cross-check of (s) — the run stops if they differ.

  python tools/bench_targets_peaks.py [--reps 10] [--warmup 2] [--markdown] [--target-counts 8,256] [--no-rounds] [shape[:records] ...]
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

CASES = {"input6": 1 << 16}
TARGET_COUNTS = (8, 256)
RADII = (0, 1, 20, 2048)
SEGS = (4, 8, 16, 32, 64)
K, WITHIN = 4, 20
I32 = np.iinfo(np.int32)


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


def run(shape, n, T, reps, warmup, rounds):
    prob = make_synthetic(shape, n, seed=7)
    L2 = prob.lengths.astype(np.int64)
    per = max(prob.L1, int(L2.max()) + 1)  # letters per target at the largest T: every record fits every target
    total = per * max(TARGET_COUNTS)
    rng = np.random.default_rng(11)
    ts = TargetSet.from_sequences(np.split(rng.integers(1, 27, total).astype(np.uint8), T))
    row = {"shape": shape, "records": prob.n, "T": T, "catalog": total, "target_len": total // T,
           "mean_L2": float(L2.mean()), "pairs": prob.n * T, "K": K, "within": WITHIN,
           "pair_profile_entries": [int(total // T - L2.max()), int(total // T - L2.min())]}
    if rounds:
        eng = HipSearchEngine(device=0)
        round_eng = HipSearchEngine(device=0)
        wall = {"s_topk": [], "r_topk": []}
        for it in range(warmup + reps):
            t0 = time.perf_counter()
            eng.set_problem(prob.weights, ts.seq1)
            topk = eng.solve_targets_topk(prob.codes, prob.offsets, ts, K, radius=1)
            t1 = time.perf_counter()
            per_target = []
            for t in range(T):
                round_eng.set_problem(prob.weights, ts.target(t))
                per_target.append(round_eng.solve_topk(prob.codes, prob.offsets, K, radius=1))
            t2 = time.perf_counter()
            if it == 0 and not np.array_equal(topk, np.stack(per_target, axis=1)):
                raise SystemExit(f"{shape} T={T}: solve_targets_topk(radius=1) differs from the T-round route")
            if it >= warmup:
                wall["s_topk"].append(1e3 * (t1 - t0))
                wall["r_topk"].append(1e3 * (t2 - t1))
        for k, v in wall.items():
            row[k + "_wall_ms"] = spread(v)
        row["rounds_over_topk"] = row["r_topk_wall_ms"]["median"] / row["s_topk_wall_ms"]["median"]
        row["chunks"] = int(eng.stats()["chunks"])
        round_eng.close()
        eng.close()
    dev = torch.device("cuda:0")
    codes_t = torch.from_numpy(prob.codes).to(dev)
    offs_t = torch.from_numpy(prob.offsets).to(dev)
    rows_t = torch.empty((prob.n, T, 3), dtype=torch.int32, device=dev)
    topk_t = torch.empty((prob.n, T, K, 3), dtype=torch.int32, device=dev)
    toff_t = torch.empty(prob.n * T + 1, dtype=torch.int64, device=dev)
    engines = {s: engine_with({"MOC_PROFILE_TIMING": "1", **({"MOC_TARGETS_PEAKS_SEG": str(s)} if s else {})})
               for s in (0,) + SEGS}
    for e in engines.values():
        e.set_problem(prob.weights, ts.seq1)
    engines[0].solve_targets_device(codes_t, offs_t, prob.offsets, ts, rows_t)
    torch.cuda.synchronize()  # torch's default stream is not ordered with the engine's compute stream: wait both ways
    thr_t = (rows_t[:, :, 0].to(torch.int64) - WITHIN).clamp(I32.min, I32.max).to(torch.int32).contiguous()
    torch.cuda.synchronize()
    _, toff_t = engines[0].solve_targets_hits_device(codes_t, offs_t, prob.offsets, ts, thresholds_t=thr_t, cap=0,
                                                     toffsets_t=toff_t)
    torch.cuda.synchronize()
    cap = max(int(toff_t[-1].item()), 1)  # radius 0 lists the most rows
    hits_t = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    configs = [(0, R) for R in RADII] + [(s, 1) for s in SEGS]
    ms = {(w, c): [] for w in ("topk", "hits") for c in configs}
    part = {(w, c): [] for w in ("topk", "hits") for c in configs}
    for it in range(warmup + reps):
        for c in configs:
            e, R = engines[c[0]], c[1]
            e.solve_targets_topk_device(codes_t, offs_t, prob.offsets, ts, K, topk_t, radius=R)
            t, p = e.device_kernel_ms(), e.targets_ms()
            e.solve_targets_hits_device(codes_t, offs_t, prob.offsets, ts, thresholds_t=thr_t, cap=cap, rows_t=hits_t,
                                        toffsets_t=toff_t, radius=R)
            th, ph = e.device_kernel_ms(), e.targets_ms()
            if it == 0:
                row.setdefault("hits_rows", {})[f"R{R}"] = int(toff_t[-1].item())
            if it >= warmup:
                ms["topk", c].append(t)
                part["topk", c].append(p)
                ms["hits", c].append(th)
                part["hits", c].append(ph)
    for c in configs:
        name = f"R{c[1]}" if not c[0] else f"seg{c[0]}_R{c[1]}"
        for w in ("topk", "hits"):
            row[f"{name}_{w}_device_ms"] = spread(ms[w, c])
            row[f"{name}_{w}_behind_profile_ms"] = spread(part[w, c])
    for e in engines.values():
        e.close()
    return row


def markdown(rows):
    out = ["| shape | records | T | pair profile entries | call | device ms at R = 0 / 1 / 20 / 2048 | behind the profile kernel, "
           "ms at R = 0 / 1 / 20 / 2048 | the same at R = 1, segment width 4 / 8 / 16 / 32 / 64 | (s) top-4 R = 1 wall ms | (r) T rounds "
           "wall ms | (r) / (s) |", "|---|---|---|---|---|---|---|---|---|---|---|"]

    def w(r, k):
        if k not in r:
            return "-"
        s = r[k]
        return f"{s['median']:.2f} ({s['min']:.2f} .. {s['max']:.2f})"

    for r in rows:
        for call in ("topk", "hits"):
            d = " / ".join(f"{r[f'R{R}_{call}_device_ms']['median']:.3f}" for R in RADII)
            b = " / ".join(f"{r[f'R{R}_{call}_behind_profile_ms']['median']:.3f}" for R in RADII)
            s = " / ".join(f"{r[f'seg{g}_R1_{call}_behind_profile_ms']['median']:.3f}" for g in SEGS)
            wall = (w(r, "s_topk_wall_ms"), w(r, "r_topk_wall_ms"), f"{r['rounds_over_topk']:.2f}") \
                if call == "topk" and "rounds_over_topk" in r else ("-", "-", "-")
            e = r["pair_profile_entries"]
            out.append(f"| {r['shape']} | {r['records']} | {r['T']} | {e[0]} .. {e[1]} | {call} | {d} | {b} | {s} | "
                       f"{wall[0]} | {wall[1]} | {wall[2]} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shapes", nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--markdown", action="store_true", help="print the table after the JSON lines")
    ap.add_argument("--no-rounds", action="store_true", help="skip (s) and (r): the device-resident kernels only")
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
            rows.append(run(shape, int(n) if n else CASES.get(shape, 1 << 12), T, max(a.reps, 10), a.warmup, not a.no_rounds))
            print(json.dumps(rows[-1]), flush=True)
    if a.markdown:
        print(markdown(rows))


if __name__ == "__main__":
    main()
