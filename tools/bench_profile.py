"""Throughput of the per-offset profile and top-K kernels next to the search they extend, on device-resident
batches (no PCIe in the loop). Every figure is the median over --reps (>= 10) repetitions, after --warmup, of
the device time between the events the engine records around its launches (HipSearchEngine.device_kernel_ms:
the host's per-call planning is outside the bracket), reported as cells/s with cells = sum (L1 - L2 + 1) * L2.

Per shape:
  (a) solve_device as shipped (the engine's own kernel choice);
  (b) long-record shapes: solve_device with MOC_TILE16=0 — the LUT tile kernel, the same sweep as the profile
      kernel without the per-offset store: the like-for-like baseline;
  (c) solve_profile_device;
  (d) solve_topk_device at K = 1, 8, 64, with the select kernel's share of the time (MOC_PROFILE_TIMING=1
      event pairs around the select launches).

  python tools/bench_profile.py [--reps 10] [--warmup 2] [--markdown] [shape[:records] ...]
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

# shape -> (records, long-record shape: measure (b))
CASES = {"input3": (1 << 13, True), "input4": (1 << 13, True), "limits": (1 << 10, True), "input6": (1 << 20, False)}


def median_ms(eng, call, reps, warmup, extra=None):
    ms, ex = [], []
    for it in range(warmup + reps):
        call()
        t = eng.device_kernel_ms()
        if it >= warmup:
            ms.append(t)
            if extra:
                ex.append(extra())
    return statistics.median(ms), (statistics.median(ex) if extra else None)


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


def run(shape, n, long_shape, reps, warmup):
    prob = make_synthetic(shape, n, seed=7)
    L2 = prob.lengths.astype(np.int64)
    cells = int(((prob.L1 - L2 + 1) * L2)[L2 <= prob.L1].sum())
    dev = torch.device("cuda:0")
    codes_t = torch.from_numpy(prob.codes).to(dev)
    offs_t = torch.from_numpy(prob.offsets).to(dev)
    out_t = torch.empty((prob.n, 3), dtype=torch.int32, device=dev)
    row = {"shape": shape, "records": prob.n, "L1": prob.L1, "cells": cells}

    def rate(ms):
        return cells / (ms * 1e-3)

    eng = engine_with({"MOC_PROFILE_TIMING": "1"})
    eng.set_problem(prob.weights, prob.seq1)
    ms, _ = median_ms(eng, lambda: eng.solve_device(codes_t, offs_t, prob.offsets, out_t), reps, warmup)
    row["a_search_ms"], row["a_search_cells_s"], row["a_kernels"] = ms, rate(ms), eng.stats()["kernels"]
    if long_shape:
        lut = engine_with({"MOC_TILE16": "0"})
        lut.set_problem(prob.weights, prob.seq1)
        ms, _ = median_ms(lut, lambda: lut.solve_device(codes_t, offs_t, prob.offsets, out_t), reps, warmup)
        row["b_lut_ms"], row["b_lut_cells_s"], row["b_kernels"] = ms, rate(ms), lut.stats()["kernels"]
        lut.close()
    poffsets = eng.profile_offsets(prob.offsets)
    row["profile_entries"] = int(poffsets[-1])
    prof_t = torch.empty((int(poffsets[-1]), 2), dtype=torch.int32, device=dev)
    ms, _ = median_ms(eng, lambda: eng.solve_profile_device(codes_t, offs_t, prob.offsets, prof_t), reps, warmup)
    row["c_profile_ms"], row["c_profile_cells_s"] = ms, rate(ms)
    if long_shape:
        row["c_over_b"] = row["c_profile_cells_s"] / row["b_lut_cells_s"]
    del prof_t
    for K in (1, 8, 64):
        top_t = torch.empty((prob.n, K, 3), dtype=torch.int32, device=dev)
        ms, sel = median_ms(eng, lambda: eng.solve_topk_device(codes_t, offs_t, prob.offsets, K, top_t), reps, warmup,
                            extra=eng.topk_select_ms)
        row[f"d_top{K}_ms"], row[f"d_top{K}_cells_s"], row[f"d_top{K}_select_share"] = ms, rate(ms), sel / ms
        row["topk_chunks"] = int(eng.stats()["chunks"])
        del top_t
    eng.close()
    return row


def markdown(rows):
    def t(v):
        return f"{v / 1e12:.2f}"

    out = ["| shape | records | (a) search, kernels | (b) LUT tile | (c) profile | (c)/(b) | (d) K=1 (select) | "
           "(d) K=8 (select) | (d) K=64 (select) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        b = t(r["b_lut_cells_s"]) if "b_lut_cells_s" in r else "-"
        cb = f"{r['c_over_b']:.2f}" if "c_over_b" in r else "-"
        d = " | ".join(f"{t(r[f'd_top{K}_cells_s'])} ({100 * r[f'd_top{K}_select_share']:.0f} %)" for K in (1, 8, 64))
        out.append(f"| {r['shape']} | {r['records']} | {t(r['a_search_cells_s'])} {'+'.join(r['a_kernels'])} | {b} | "
                   f"{t(r['c_profile_cells_s'])} | {cb} | {d} |")
    return "\n".join(out) + "\n\nT cells/s; (select): the select kernel's share of the top-K device time.\n"


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
        rows.append(run(shape, int(n) if n else CASES[shape][0], CASES[shape][1], max(a.reps, 10), a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if a.markdown:
        print(markdown(rows))


if __name__ == "__main__":
    main()
