"""Cost of the target ranking next to the route users had without it: the n x T pair rows of solve_targets reduced
afterwards. All calls of a case run in one process, interleaved per repetition; every time is the median over --reps
(>= 10) repetitions after --warmup, with the smallest and largest repetition beside it.

Per case (input6-shaped records against T in {16, 256, 4096} random targets of equal length, every target at least as
long as the longest record, M in {1, 8}; batches both routes can hold):
  (a) rank, host form: solve_targets_rank end to end; wall clock, the bytes it copies back (stats()["d2h_bytes"]);
  (b) rows, host form: solve_targets, then targets_best (M = 1) or a numpy stable sort of the scores cut at M; wall
      clock and bytes copied back. Its result is the cross-check of (a): the run stops if they differ;
  (c) rank, device form on a device-resident batch with MOC_PROFILE_TIMING=1: a host clock around the call and a
      device synchronise, the device time between the engine's events, and the time of the select + rank launches;
  (d) rows, device form: solve_targets_device into an [n, T, 3] tensor, then a stable torch sort of the scores cut at
      M and a gather; the same host clock, and the engine's device time of solve_targets_device alone.
Peak device bytes of a route: the device memory in use (torch.cuda.mem_get_info, device-wide) after the route has run
on an engine of its own, less what was in use before that engine existed — the engine's pooled buffers are grown and
never shrunk, so what is in use afterwards is the most the route needed, torch's tensors included. Other processes on
the device move that figure; the n * T * 12 and n * M * 16 bytes of the two results are printed beside it.

  python tools/bench_targets_rank.py [--reps 10] [--warmup 2] [--markdown] [--targets 16,256,4096] [--ms 1,8] [--records N]
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

from mpi_openmp_cuda_amd import HipSearchEngine, TargetSet, make_synthetic, targets_best  # noqa: E402

RECORDS = {16: 1 << 16, 256: 1 << 15, 4096: 1 << 12}  # n * T * 12 bytes: 12 MB, 100 MB, 200 MB of pair rows
I32 = np.iinfo(np.int32)
DEV = torch.device("cuda:0")


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


def in_use():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info(DEV)
    return total - free


def rank_of_rows_numpy(rows, M):
    """Route (b)'s reduction: [n, T, 3] -> [n, M, 4]."""
    n, T, _ = rows.shape
    if M == 1:
        t, row = targets_best(rows)
        return np.concatenate([t[:, None], row], axis=1)[:, None, :]
    order = np.argsort(-rows[:, :, 0].astype(np.int64), axis=1, kind="stable")[:, :M]
    picked = np.take_along_axis(rows, order[:, :, None], axis=1)
    out = np.concatenate([order[:, :, None].astype(np.int32), picked], axis=2)
    out[picked[:, :, 0] == I32.min] = (-1, I32.min, 0, 0)
    if M > T:
        pad = np.empty((n, M - T, 4), np.int32)
        pad[:] = (-1, I32.min, 0, 0)
        out = np.concatenate([out, pad], axis=1)
    return out


def rank_of_rows_torch(rows_t, M):
    """Route (d)'s reduction on the device: a stable sort of the scores, cut at M, and a gather."""
    score = rows_t[:, :, 0]
    order = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :M]
    picked = rows_t.gather(1, order.unsqueeze(2).expand(-1, -1, 3))
    out = torch.cat([order.unsqueeze(2).to(torch.int32), picked], dim=2)
    pad = torch.tensor([-1, I32.min, 0, 0], dtype=torch.int32, device=rows_t.device)
    return torch.where((picked[:, :, 0] == I32.min).unsqueeze(2), pad.expand_as(out), out)


def run(n, T, M, reps, warmup):
    prob = make_synthetic("input6", n, seed=7)
    L2 = prob.lengths.astype(np.int64)
    per = int(L2.max()) + 8  # letters per target: every record fits every target, slices of 8 entries and more
    rng = np.random.default_rng(11)
    ts = TargetSet.from_sequences(np.split(rng.integers(1, 27, per * T).astype(np.uint8), T))
    row = {"records": prob.n, "T": T, "M": M, "target_len": per, "catalog": per * T, "mean_L2": float(L2.mean()),
           "rows_bytes": prob.n * T * 12, "rank_bytes": prob.n * M * 16}
    # ---- host forms, an engine per route
    base = in_use()
    rank_eng = HipSearchEngine(device=0)
    rank_eng.set_problem(prob.weights, ts.seq1)
    rank_eng.solve_targets_rank(prob.codes, prob.offsets, ts, M)
    row["a_peak_device_bytes"] = in_use() - base
    base = in_use()
    rows_eng = HipSearchEngine(device=0)
    rows_eng.set_problem(prob.weights, ts.seq1)
    rows_eng.solve_targets(prob.codes, prob.offsets, ts)
    row["b_peak_device_bytes"] = in_use() - base
    wall = {"a": [], "b": [], "b_solve": []}
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        rank = rank_eng.solve_targets_rank(prob.codes, prob.offsets, ts, M)
        t1 = time.perf_counter()
        rows = rows_eng.solve_targets(prob.codes, prob.offsets, ts)
        t2 = time.perf_counter()
        today = rank_of_rows_numpy(rows, M)
        t3 = time.perf_counter()
        if it == 0:
            if not np.array_equal(rank, today):
                raise SystemExit(f"T={T} M={M}: solve_targets_rank differs from the sorted rows of solve_targets")
            row["a_d2h_bytes"] = int(rank_eng.stats()["d2h_bytes"])
            row["b_d2h_bytes"] = int(rows_eng.stats()["d2h_bytes"])
            row["a_chunks"], row["b_chunks"] = int(rank_eng.stats()["chunks"]), int(rows_eng.stats()["chunks"])
        if it >= warmup:
            wall["a"].append(1e3 * (t1 - t0))
            wall["b"].append(1e3 * (t3 - t1))
            wall["b_solve"].append(1e3 * (t2 - t1))
    for k, v in wall.items():
        row[k + "_wall_ms"] = spread(v)
    row["b_over_a_wall"] = row["b_wall_ms"]["median"] / row["a_wall_ms"]["median"]
    rank_eng.close()
    rows_eng.close()
    del rank, rows, today
    # ---- device forms, an engine per route. Everything is queued on one side stream: the engine's calls and torch's
    # sort are then ordered by the stream alone (torch's default stream is not ordered with the engine's own).
    codes_t = torch.from_numpy(prob.codes).to(DEV)
    offs_t = torch.from_numpy(prob.offsets).to(DEV)
    side = torch.cuda.Stream(device=DEV)
    ms = {"c_wall": [], "c_device": [], "c_select_rank": [], "d_wall": [], "d_device_solve": []}
    with torch.cuda.stream(side):
        base = in_use()
        rank_eng = engine_with({"MOC_PROFILE_TIMING": "1"})
        rank_eng.set_problem(prob.weights, ts.seq1)
        rank_t = torch.empty((prob.n, M, 4), dtype=torch.int32, device=DEV)
        rank_eng.solve_targets_rank_device(codes_t, offs_t, prob.offsets, ts, M, rank_t, stream=side)
        row["c_peak_device_bytes"] = in_use() - base
        base = in_use()
        rows_eng = engine_with({"MOC_PROFILE_TIMING": "1"})
        rows_eng.set_problem(prob.weights, ts.seq1)
        rows_t = torch.empty((prob.n, T, 3), dtype=torch.int32, device=DEV)
        rows_eng.solve_targets_device(codes_t, offs_t, prob.offsets, ts, rows_t, stream=side)
        today_t = rank_of_rows_torch(rows_t, M)
        row["d_peak_device_bytes"] = in_use() - base  # torch's cached sort buffers stay counted: they were needed
        row["d_torch_peak_allocated"] = int(torch.cuda.max_memory_allocated(DEV))
        if not torch.equal(today_t[:, :min(M, T)], rank_t[:, :min(M, T)]):
            raise SystemExit(f"T={T} M={M}: the device forms differ")
        for it in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rank_eng.solve_targets_rank_device(codes_t, offs_t, prob.offsets, ts, M, rank_t, stream=side)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            cd, cs = rank_eng.device_kernel_ms(), rank_eng.targets_ms()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            rows_eng.solve_targets_device(codes_t, offs_t, prob.offsets, ts, rows_t, stream=side)
            today_t = rank_of_rows_torch(rows_t, M)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            dd = rows_eng.device_kernel_ms()
            if it >= warmup:
                for k, v in (("c_wall", 1e3 * (t1 - t0)), ("c_device", cd), ("c_select_rank", cs),
                             ("d_wall", 1e3 * (t3 - t2)), ("d_device_solve", dd)):
                    ms[k].append(v)
    for k, v in ms.items():
        row[k + "_ms"] = spread(v)
    row["d_over_c_wall"] = row["d_wall_ms"]["median"] / row["c_wall_ms"]["median"]
    rank_eng.close()
    rows_eng.close()
    return row


def markdown(rows):
    out = ["| T | M | records | (a) rank host ms | (b) rows + reduce host ms | (b) / (a) | D2H (a) / (b) MB | (c) rank device ms "
           "(engine events; select + rank) | (d) rows + torch sort device ms (solve_targets events) | (d) / (c) | peak device "
           "MB a / b / c / d |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]

    def w(s):
        return f"{s['median']:.2f} ({s['min']:.2f} .. {s['max']:.2f})"

    for r in rows:
        out.append(f"| {r['T']} | {r['M']} | {r['records']} | {w(r['a_wall_ms'])} | {w(r['b_wall_ms'])} | {r['b_over_a_wall']:.2f} | "
                   f"{r['a_d2h_bytes'] / 1e6:.2f} / {r['b_d2h_bytes'] / 1e6:.2f} | {w(r['c_wall_ms'])} "
                   f"({r['c_device_ms']['median']:.2f}; {r['c_select_rank_ms']['median']:.2f}) | {w(r['d_wall_ms'])} "
                   f"({r['d_device_solve_ms']['median']:.2f}) | {r['d_over_c_wall']:.2f} | "
                   + " / ".join(f"{r[k + '_peak_device_bytes'] / 1e6:.0f}" for k in "abcd") + " |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--markdown", action="store_true", help="print the table after the JSON lines")
    ap.add_argument("--targets", default="16,256,4096", help="comma list of target counts (1..4096)")
    ap.add_argument("--ms", default="1,8", help="comma list of M (1..64)")
    ap.add_argument("--records", type=int, default=0, help="records per case (default: 65536 / 32768 / 4096 by T)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_targets_rank needs a GPU")
    rows = []
    run(256, 16, 2, 10, 1)  # unmeasured: loads every code object and torch's sort once, before any memory figure
    for T in (int(t) for t in a.targets.split(",")):
        for M in (int(m) for m in a.ms.split(",")):
            n = a.records or RECORDS.get(T, max(1 << 12, (1 << 24) // (12 * T)))
            rows.append(run(n, T, M, max(a.reps, 10), a.warmup))
            print(json.dumps(rows[-1]), flush=True)
    if a.markdown:
        print(markdown(rows))


if __name__ == "__main__":
    main()
