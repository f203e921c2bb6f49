"""Cost of distinct placements (the `radius` keyword of top-K and hits) on device-resident batches, on the shapes of
tools/bench_hits.py. Every figure is the median over --reps (>= 10) repetitions, after --warmup, of the device time
between the events the engine records around a call's launches (HipSearchEngine.device_kernel_ms: the host's per-call
planning is outside the bracket); all calls of a shape are interleaved per repetition in one process.

Per shape, for radius in 0, 1, 64, 2048:
  (h) solve_hits_device at the batch-wide threshold that roughly 1 % of the profile's entries reach, cap = the exact
      total of that radius;
  (t) solve_topk_device at K = 4;
and with each: the device time of everything behind the chunk's profile kernel (peak kernels + select or count / scan /
compact; MOC_PROFILE_TIMING=1 event pairs), and `peaks_ms` = that bracket minus the same bracket at radius 0 — the peak
kernels plus what the masked forms cost over the plain ones (a difference of two medians, not a kernel trace).

With --base-lib PATH (a libmoc.so built from the parent commit) the radius-0 calls also run on that library: child
processes, one library each, alternate --rounds times (base, this, base, this, ...), and the run-to-run spread of each
is the range of its per-round medians. radius=0 calls the same native entry points as no keyword, so the old library
serves them.

  python tools/bench_peaks.py [--reps 10] [--warmup 3] [--rounds 3] [--base-lib PATH] [--markdown] [shape[:records] ...]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys


sys.path.insert(0, ".")

CASES = {"input3": 1 << 13, "input4": 1 << 13, "input6": 1 << 20}
RADII = (0, 1, 64, 2048)
K = 4


def child(shape, n, reps, warmup, radii):
    import torch

    from mpi_openmp_cuda_amd import HipSearchEngine, make_synthetic

    prob = make_synthetic(shape, n, seed=7)
    dev = torch.device("cuda:0")
    codes_t = torch.from_numpy(prob.codes).to(dev)
    offs_t = torch.from_numpy(prob.offsets).to(dev)
    os.environ["MOC_PROFILE_TIMING"] = "1"  # read when the engine starts
    eng = HipSearchEngine(device=0)
    eng.set_problem(prob.weights, prob.seq1)
    entries = int(eng.profile_offsets(prob.offsets)[-1])
    row = {"shape": shape, "records": prob.n, "L1": prob.L1, "profile_entries": entries}
    prof_t = torch.empty((entries, 2), dtype=torch.int32, device=dev)
    eng.solve_profile_device(codes_t, offs_t, prob.offsets, prof_t)
    torch.cuda.synchronize()
    T = int(prof_t[:, 0].sort().values[min(entries - 1, int(round(0.99 * entries)))])
    del prof_t
    row["threshold"] = T
    kw = (lambda R: {"radius": R}) if any(radii) else (lambda R: {})  # an old library: no keyword at all
    calls = {}
    for R in radii:
        _, h_t = eng.solve_hits_device(codes_t, offs_t, prob.offsets, min_score=T, cap=0, **kw(R))
        torch.cuda.synchronize()
        total = int(h_t[-1])
        row[f"hits_r{R}_rows"] = total
        rows_t = torch.empty((max(total, 1), 3), dtype=torch.int32, device=dev)
        calls[f"hits_r{R}"] = lambda R=R, total=total, rows_t=rows_t, h_t=h_t: eng.solve_hits_device(
            codes_t, offs_t, prob.offsets, min_score=T, cap=total, rows_t=rows_t, hoffsets_t=h_t, **kw(R))
        top_t = torch.empty((prob.n, K, 3), dtype=torch.int32, device=dev)
        calls[f"top{K}_r{R}"] = lambda R=R, top_t=top_t: eng.solve_topk_device(codes_t, offs_t, prob.offsets, K, top_t,
                                                                              **kw(R))
    ms = {k: [] for k in calls}
    sel = {k: [] for k in calls}
    for it in range(warmup + reps):
        for k, call in calls.items():
            call()
            t = eng.device_kernel_ms()
            if it >= warmup:
                ms[k].append(t)
                sel[k].append(eng.hits_select_ms())
    for k in calls:
        row[k + "_ms"] = statistics.median(ms[k])
        row[k + "_min_ms"], row[k + "_max_ms"] = min(ms[k]), max(ms[k])
        row[k + "_behind_profile_ms"] = statistics.median(sel[k])
    row["chunks"] = int(eng.stats()["chunks"])
    eng.close()
    print(json.dumps(row), flush=True)


def spawn(lib, shape, n, a, radii):
    env = dict(os.environ)
    if lib:
        env["MOC_LIB_PATH"] = lib
    cmd = [sys.executable, __file__, "--child", f"{shape}:{n}", "--reps", str(a.reps), "--warmup", str(a.warmup),
           "--radii", ",".join(str(r) for r in radii)]
    r = subprocess.run(cmd, env=env, capture_output=True, timeout=1200)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({lib or 'this build'}):\n{r.stderr.decode()[-3000:]}")
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def summarise(shape, n, base_rounds, this_rounds):
    """Per call: the median of the rounds' medians and their range (the run-to-run spread)."""
    out = {"shape": shape, "records": n, "rounds": len(this_rounds)}
    for key in ("profile_entries", "threshold", "chunks"):
        out[key] = this_rounds[0][key]
    for label, rounds in (("base", base_rounds), ("this", this_rounds)):
        if not rounds:
            continue
        for k in [k for k in rounds[0] if k.endswith("_ms") and "_min_" not in k and "_max_" not in k]:
            v = [r[k] for r in rounds]
            out[f"{label}_{k}"] = statistics.median(v)
            out[f"{label}_{k}_range"] = [min(v), max(v)]
    for k in [k for k in this_rounds[0] if k.endswith("_rows")]:
        out[k] = this_rounds[0][k]
    for call in ("hits", f"top{K}"):
        for R in RADII[1:]:
            d = out[f"this_{call}_r{R}_behind_profile_ms"] - out[f"this_{call}_r0_behind_profile_ms"]
            out[f"{call}_r{R}_peaks_ms"] = d
            out[f"{call}_r{R}_peaks_share"] = d / out[f"this_{call}_r{R}_ms"]
    return out


def markdown(rows, have_base):
    out = ["| shape | call | " + ("parent ms (range) | " if have_base else "") + "radius 0 ms (range) | " +
           " | ".join(f"radius {R} ms (peaks share)" for R in RADII[1:]) + " |",
           "|---|---|" + ("---|" if have_base else "") + "---|" + "---|" * (len(RADII) - 1)]
    for r in rows:
        for call in ("hits", f"top{K}"):
            def cell(label, R):
                lo, hi = r[f"{label}_{call}_r{R}_ms_range"]
                return f"{r[f'{label}_{call}_r{R}_ms']:.3f} ({lo:.3f}..{hi:.3f})"
            cells = ([cell("base", 0)] if have_base else []) + [cell("this", 0)]
            cells += [f"{r[f'this_{call}_r{R}_ms']:.3f} ({100 * r[f'{call}_r{R}_peaks_share']:.0f} %)" for R in RADII[1:]]
            out.append(f"| {r['shape']} ({r['records']}) | {call} | " + " | ".join(cells) + " |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shapes", nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--base-lib", default=None, help="libmoc.so of the parent commit: its radius-0 calls are timed too")
    ap.add_argument("--markdown", action="store_true", help="print the table after the JSON lines")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--radii", default=",".join(str(r) for r in RADII), help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.reps = max(a.reps, 10)
    if a.child:
        shape, _, n = a.child.partition(":")
        child(shape, int(n), a.reps, a.warmup, [int(r) for r in a.radii.split(",")])
        return
    rows = []
    for s in a.shapes:
        shape, _, n = s.partition(":")
        n = int(n) if n else CASES[shape]
        base_rounds, this_rounds = [], []
        for _ in range(max(a.rounds, 1)):  # alternate the two builds
            if a.base_lib:
                base_rounds.append(spawn(os.path.abspath(a.base_lib), shape, n, a, [0]))
            this_rounds.append(spawn(None, shape, n, a, RADII))
        rows.append(summarise(shape, n, base_rounds, this_rounds))
        print(json.dumps(rows[-1]), flush=True)
    if a.markdown:
        print(markdown(rows, bool(a.base_lib)))


if __name__ == "__main__":
    main()
