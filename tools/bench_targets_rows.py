"""Cost of per-target top-K and threshold hits next to the only route without them, T rounds of set_problem(target_t)
+ solve_topk / solve_hits, and next to solve_targets on the same batch. All calls of a case run in one process,
interleaved per repetition; every figure is the median over --reps (>= 10) repetitions after --warmup, with the
smallest and largest repetition beside it.

Per shape (input3-, input4- and input6-shaped records) and per catalog (8 and 256 random targets of equal length, the
same total length for both, every target at least as long as the shape's own Seq1 — the catalogs of
tools/bench_targets.py):
  (s) solve_targets_topk(K = 4) and solve_targets_hits(within = 20), host forms: one upload, one pass over the catalog
      profile (hits: solve_targets first for the thresholds); wall clock;
  (r) the T-round route, host forms: per target set_problem + solve_topk(K = 4), and per target set_problem +
      solve_hits(within = 20); wall clock. Their stacked rows are also the correctness cross-check of (s) — the run
      stops if they differ;
  (g) solve_targets_topk_device and solve_targets_hits_device (thresholds = solve_targets_device's scores - 20, built
      on the device) on the device-resident batch with the lane-group size forced to 4, 16 and 64 (MOC_TARGETS_GROUP,
      read when an engine starts) and with the host's own choice: device time between the engine's events, and the time
      and share of the new launches in it (MOC_PROFILE_TIMING=1 event pairs around those launches); with the host's
      choice also solve_targets_device on the same engine.

  python tools/bench_targets_rows.py [--reps 10] [--warmup 2] [--markdown] [--target-counts 8,256] [--no-rounds] [shape[:records] ...]

--target-counts: other divisors of 256 cut the same catalog into other target lengths — the sweep over slice lengths
against which the two cut-over constants of bounds::targets_group are checked for the top-K kernel (--no-rounds skips
(r) there).
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


def stacked_hits(per_target, n, T):
    """The T-round route's (rows, hoffsets) per target as pair-major (rows, toffsets)."""
    counts = np.stack([np.diff(h) for _, h in per_target], axis=1)  # [n, T]
    toffsets = np.zeros(n * T + 1, np.int64)
    np.cumsum(counts.reshape(-1), out=toffsets[1:])
    rows = np.zeros((int(toffsets[-1]), 3), np.int32)
    first = toffsets[:-1].reshape(n, T)
    for t, (r, h) in enumerate(per_target):
        dest = np.repeat(first[:, t] - h[:-1], counts[:, t]) + np.arange(r.shape[0])
        rows[dest] = r
    return rows, toffsets


def run(shape, n, T, reps, warmup, rounds):
    prob = make_synthetic(shape, n, seed=7)
    L2 = prob.lengths.astype(np.int64)
    per = max(prob.L1, int(L2.max()) + 1)  # letters per target at the largest T: every record fits every target
    total = per * max(TARGET_COUNTS)
    rng = np.random.default_rng(11)
    ts = TargetSet.from_sequences(np.split(rng.integers(1, 27, total).astype(np.uint8), T))
    slice_entries = int((total // T - L2).clip(min=0).sum()) * T
    row = {"shape": shape, "records": prob.n, "T": T, "catalog": total, "target_len": total // T,
           "mean_L2": float(L2.mean()), "pairs": prob.n * T, "slice_entries": slice_entries, "K": K, "within": WITHIN}
    if rounds:
        eng = HipSearchEngine(device=0)
        round_eng = HipSearchEngine(device=0)
        wall = {"s_topk": [], "r_topk": [], "s_hits": [], "r_hits": []}
        for it in range(warmup + reps):
            t0 = time.perf_counter()
            eng.set_problem(prob.weights, ts.seq1)
            topk = eng.solve_targets_topk(prob.codes, prob.offsets, ts, K)
            t1 = time.perf_counter()
            per_target = []
            for t in range(T):
                round_eng.set_problem(prob.weights, ts.target(t))
                per_target.append(round_eng.solve_topk(prob.codes, prob.offsets, K))
            t2 = time.perf_counter()
            if it == 0 and not np.array_equal(topk, np.stack(per_target, axis=1)):
                raise SystemExit(f"{shape} T={T}: solve_targets_topk differs from the T-round route")
            t3 = time.perf_counter()
            eng.set_problem(prob.weights, ts.seq1)
            hits, toffsets = eng.solve_targets_hits(prob.codes, prob.offsets, ts, within=WITHIN)
            passes = eng.hits_passes()
            t4 = time.perf_counter()
            per_target = []
            for t in range(T):
                round_eng.set_problem(prob.weights, ts.target(t))
                per_target.append(round_eng.solve_hits(prob.codes, prob.offsets, within=WITHIN))
            t5 = time.perf_counter()
            if it == 0:
                want, woff = stacked_hits(per_target, prob.n, T)
                if not (np.array_equal(toffsets, woff) and np.array_equal(hits, want)):
                    raise SystemExit(f"{shape} T={T}: solve_targets_hits differs from the T-round route")
                row["hits"], row["hits_passes"] = int(toffsets[-1]), passes
            if it >= warmup:
                for k, v in (("s_topk", t1 - t0), ("r_topk", t2 - t1), ("s_hits", t4 - t3), ("r_hits", t5 - t4)):
                    wall[k].append(1e3 * v)
        for k, v in wall.items():
            row[k + "_wall_ms"] = spread(v)
        row["rounds_over_topk"] = row["r_topk_wall_ms"]["median"] / row["s_topk_wall_ms"]["median"]
        row["rounds_over_hits"] = row["r_hits_wall_ms"]["median"] / row["s_hits_wall_ms"]["median"]
        row["chunks"] = int(eng.stats()["chunks"])
        round_eng.close()
        eng.close()
    # (g) the kernels per lane-group size, device-resident
    dev = torch.device("cuda:0")
    codes_t = torch.from_numpy(prob.codes).to(dev)
    offs_t = torch.from_numpy(prob.offsets).to(dev)
    rows_t = torch.empty((prob.n, T, 3), dtype=torch.int32, device=dev)
    topk_t = torch.empty((prob.n, T, K, 3), dtype=torch.int32, device=dev)
    toff_t = torch.empty(prob.n * T + 1, dtype=torch.int64, device=dev)
    engines = {g: engine_with({"MOC_PROFILE_TIMING": "1", **({"MOC_TARGETS_GROUP": str(g)} if g else {})}) for g in GROUPS}
    for e in engines.values():
        e.set_problem(prob.weights, ts.seq1)
    engines[0].solve_targets_device(codes_t, offs_t, prob.offsets, ts, rows_t)
    torch.cuda.synchronize()  # torch's default stream is not ordered with the engine's compute stream: wait both ways
    thr_t = (rows_t[:, :, 0].to(torch.int64) - WITHIN).clamp(I32.min, I32.max).to(torch.int32).contiguous()
    torch.cuda.synchronize()
    _, toff_t = engines[0].solve_targets_hits_device(codes_t, offs_t, prob.offsets, ts, thresholds_t=thr_t, cap=0,
                                                     toffsets_t=toff_t)
    torch.cuda.synchronize()
    cap = max(int(toff_t[-1].item()), 1)
    hits_t = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    ms = {(w, g): [] for w in ("topk", "hits") for g in GROUPS}
    part = {(w, g): [] for w in ("topk", "hits") for g in GROUPS}
    extra = {"targets_device": [], "targets_select": []}
    for it in range(warmup + reps):
        for g, e in engines.items():
            e.solve_targets_topk_device(codes_t, offs_t, prob.offsets, ts, K, topk_t)
            t, p = e.device_kernel_ms(), e.targets_ms()
            e.solve_targets_hits_device(codes_t, offs_t, prob.offsets, ts, thresholds_t=thr_t, cap=cap, rows_t=hits_t,
                                        toffsets_t=toff_t)
            th, ph = e.device_kernel_ms(), e.targets_ms()
            if it >= warmup:
                ms["topk", g].append(t)
                part["topk", g].append(p)
                ms["hits", g].append(th)
                part["hits", g].append(ph)
        e = engines[0]
        e.solve_targets_device(codes_t, offs_t, prob.offsets, ts, rows_t)
        tt, tsel = e.device_kernel_ms(), e.targets_ms()
        if it >= warmup:
            extra["targets_device"].append(tt)
            extra["targets_select"].append(tsel)
    for g, e in engines.items():
        name = f"g{g}" if g else "g_auto"
        for w in ("topk", "hits"):
            row[f"{name}_{w}_device_ms"] = spread(ms[w, g])
            row[f"{name}_{w}_kernels_ms"] = spread(part[w, g])
            row[f"{name}_{w}_share"] = row[f"{name}_{w}_kernels_ms"]["median"] / row[f"{name}_{w}_device_ms"]["median"]
        e.close()
    for k, v in extra.items():
        row[k + "_ms"] = spread(v)
    row["device_hits"] = cap
    if "hits" in row and row["hits"] != cap:
        raise SystemExit(f"{shape} T={T}: the device form counts {cap} hits, the host form {row['hits']}")
    return row


def markdown(rows):
    out = ["| shape | records | T | (s) top-4 wall ms | (r) T rounds wall ms | (r) / (s) | (s) within-20 wall ms | (r) T rounds "
           "wall ms | (r) / (s) | top-K kernel ms at G = 4 / 16 / 64 / auto | share (auto) | hits kernels ms at G = 4 / 16 / "
           "64 / auto | share (auto) | top-K / hits / solve_targets device ms |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]

    def w(r, k):
        if k not in r:
            return "-"
        s = r[k]
        return f"{s['median']:.2f} ({s['min']:.2f} .. {s['max']:.2f})"

    for r in rows:
        gk = " / ".join(f"{r[k + '_topk_kernels_ms']['median']:.3f}" for k in ("g4", "g16", "g64", "g_auto"))
        gh = " / ".join(f"{r[k + '_hits_kernels_ms']['median']:.3f}" for k in ("g4", "g16", "g64", "g_auto"))
        ro = (f"{r['rounds_over_topk']:.2f}", f"{r['rounds_over_hits']:.2f}") if "rounds_over_topk" in r else ("-", "-")
        out.append(f"| {r['shape']} | {r['records']} | {r['T']} | {w(r, 's_topk_wall_ms')} | {w(r, 'r_topk_wall_ms')} | {ro[0]} | "
                   f"{w(r, 's_hits_wall_ms')} | {w(r, 'r_hits_wall_ms')} | {ro[1]} | {gk} | {100 * r['g_auto_topk_share']:.0f} % | "
                   f"{gh} | {100 * r['g_auto_hits_share']:.0f} % | {r['g_auto_topk_device_ms']['median']:.2f} / "
                   f"{r['g_auto_hits_device_ms']['median']:.2f} / {r['targets_device_ms']['median']:.2f} |")
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
            rows.append(run(shape, int(n) if n else CASES[shape], T, max(a.reps, 10), a.warmup, not a.no_rounds))
            print(json.dumps(rows[-1]), flush=True)
    if a.markdown:
        print(markdown(rows))


if __name__ == "__main__":
    main()
