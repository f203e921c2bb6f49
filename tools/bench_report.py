"""Cost of the alignment report next to the search it annotates, on device-resident batches (no PCIe in the loop).
Every figure is the median over --reps (>= 20) repetitions, after --warmup, of the time between two torch events
recorded around the call on the current stream — the host's per-call planning is inside the bracket for the search
and the report alike — with the engine's own device time (events around the launches only) beside it.

Per shape:
  (a) solve_device;
  (b) report_device, counts only, K = 1, over (a)'s rows;
  (c) (b) with marker bytes;
  (d) report_device, counts only, over the K = 8 rows of solve_topk_device.
Beside each report the effective rate: bytes = letters + 8 (n + 1) + 12 n K + 16 n K [+ K letters of marker bytes]
over the time, and the device-to-device copy rate of moc_transfer_probe(5, ...) measured in the same run.

  python tools/bench_report.py [--reps 20] [--warmup 3] [--markdown] [--out FILE] [shape[:records] ...]
"""
import argparse
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

from mpi_openmp_cuda_amd import HipSearchEngine, _lib, make_synthetic  # noqa: E402

CASES = {"input6": 1 << 22, "input1": 1 << 18, "input3": 1 << 12}


def timed(eng, call, reps, warmup):
    """(median ms between torch events around the call, median ms of the engine's own device events)."""
    ev, dv = [], []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            ev.append(e0.elapsed_time(e1))
            dv.append(eng.device_kernel_ms())
    return statistics.median(ev), statistics.median(dv)


def run(shape, n, reps, warmup):
    # a stream of our own: the default stream's handle is 0, which the engine reads as "its own compute stream",
    # and events recorded on the default stream would then bracket nothing
    with torch.cuda.stream(torch.cuda.Stream(torch.device("cuda:0"))):
        return run_on_stream(shape, n, reps, warmup)


def run_on_stream(shape, n, reps, warmup):
    prob = make_synthetic(shape, n, seed=7)
    letters = int(prob.total_chars)
    dev = torch.device("cuda:0")
    codes_t = torch.from_numpy(prob.codes).to(dev)
    offs_t = torch.from_numpy(prob.offsets).to(dev)
    rows_t = torch.empty((prob.n, 3), dtype=torch.int32, device=dev)
    eng = HipSearchEngine(device=0)
    eng.set_problem(prob.weights, prob.seq1)
    d2d = float(_lib.lib().moc_transfer_probe(5, 256 << 20, 10))  # GB/s
    row = {"shape": shape, "records": prob.n, "L1": prob.L1, "letters": letters, "d2d_gb_s": d2d}

    def put(tag, ms, dms, K, marks):
        nbytes = letters + 8 * (prob.n + 1) + 28 * prob.n * K + (K * letters if marks else 0)
        row[f"{tag}_ms"], row[f"{tag}_device_ms"], row[f"{tag}_bytes"] = ms, dms, nbytes
        row[f"{tag}_gb_s"] = nbytes / (ms * 1e-3) / 1e9
        row[f"{tag}_of_d2d"] = row[f"{tag}_gb_s"] / d2d

    ms, dms = timed(eng, lambda: eng.solve_device(codes_t, offs_t, prob.offsets, rows_t), reps, warmup)
    row["a_search_ms"], row["a_search_device_ms"], row["a_kernels"] = ms, dms, eng.stats()["kernels"]
    counts_t = torch.empty((prob.n, 4), dtype=torch.int32, device=dev)
    put("b_report", *timed(eng, lambda: eng.report_device(codes_t, offs_t, prob.offsets, rows_t, counts_t), reps, warmup),
        1, False)
    row["b_launches"] = int(eng.stats()["chunks"])
    marks_t = torch.empty(max(letters, 1), dtype=torch.uint8, device=dev)
    put("c_marks", *timed(eng, lambda: eng.report_device(codes_t, offs_t, prob.offsets, rows_t, counts_t, marks_t), reps,
                          warmup), 1, True)
    del marks_t, counts_t
    K = 8
    top_t = torch.empty((prob.n, K, 3), dtype=torch.int32, device=dev)
    eng.solve_topk_device(codes_t, offs_t, prob.offsets, K, top_t)
    counts_t = torch.empty((prob.n, K, 4), dtype=torch.int32, device=dev)
    put("d_top8", *timed(eng, lambda: eng.report_device(codes_t, offs_t, prob.offsets, top_t, counts_t), reps, warmup),
        K, False)
    row["b_over_a"] = row["b_report_ms"] / row["a_search_ms"]
    eng.close()
    return row


def markdown(rows):
    out = ["| shape | records | (a) search ms (device) | (b) report ms (device), GB/s, of D2D | (c) + markers | "
           "(d) K = 8 | (b)/(a) | D2D GB/s |", "|---|---|---|---|---|---|---|---|"]

    def cell(r, tag):
        return (f"{r[tag + '_ms']:.3f} ({r[tag + '_device_ms']:.3f}), {r[tag + '_gb_s']:.0f}, "
                f"{100 * r[tag + '_of_d2d']:.0f} %")

    for r in rows:
        out.append(f"| {r['shape']} | {r['records']} | {r['a_search_ms']:.3f} ({r['a_search_device_ms']:.3f}) "
                   f"{'+'.join(r['a_kernels'])} | {cell(r, 'b_report')} | {cell(r, 'c_marks')} | {cell(r, 'd_top8')} | "
                   f"{r['b_over_a']:.2f} | {r['d2d_gb_s']:.0f} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shapes", nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--markdown", action="store_true", help="print the table after the JSON lines")
    ap.add_argument("--out", help="also write the JSON lines to this file")
    a = ap.parse_args()
    rows = []
    for s in a.shapes:
        shape, _, n = s.partition(":")
        rows.append(run(shape, int(n) if n else CASES[shape], max(a.reps, 20), a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
    if a.markdown:
        print(markdown(rows))


if __name__ == "__main__":
    main()
