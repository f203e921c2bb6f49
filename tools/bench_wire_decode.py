"""Top-K from a wire batch next to top-K from its bytes, and the decode kernels alone, on one MI355X.
Every figure is the median over --reps (>= 10) repetitions after --warmup rounds; all calls of a shape run in one
process on one engine, interleaved per repetition, from page-locked host arrays (hipHostMalloc).

Per shape (make_synthetic, seed 7), the records encoded by WireSlice in its narrowest forms — P33 letters, and
base-6 lengths + one offset per 64 records where the length range allows (input6), else dense offsets:
  (a) solve_topk_wire, K = 1: wall time of the synchronous host call (decode on the GPU from the packed arrays read
      in place, sweep, select, D2H of the rows), the engine's device time of sweep + select, and stats().h2d_bytes;
  (b) solve_topk, K = 1, on the same records as one byte per letter + dense int64 offsets — what a caller had to
      unpack to on the host before the wire forms existed (that host unpacking is not in the figure);
  (c) the decode kernels alone: device time between the events the engine records around the decode's launches
      (device_kernel_ms after decode_wire_into on a side stream; the host's expansion of the offsets is outside
      them), from the page-locked host arrays (zero-copy over PCIe) and from device-resident copies of them.

  python tools/bench_wire_decode.py [--reps 10] [--warmup 2] [--markdown] [shape[:records] ...]
"""
import argparse
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402

from mpi_openmp_cuda_amd import HipSearchEngine, WireSlice, _lib, make_synthetic, wire_batch_of  # noqa: E402

CASES = {"input6": 1 << 20, "input4": 1 << 13, "input3": 1 << 13}
_buffers = []


def host_alloc(name, dtype, count):
    """WireSlice allocator: every array in page-locked host memory of its own."""
    dtype = np.dtype(dtype)
    buf = _lib.HostBuffer(max(int(count) * dtype.itemsize, 1))
    _buffers.append(buf)
    return buf.array(dtype, int(count))


def run(shape, n, reps, warmup):
    prob = make_synthetic(shape, n, seed=7)
    dev = torch.device("cuda:0")
    ws = WireSlice.from_csr(prob.codes, prob.offsets, letter_format="p33", alloc=host_alloc)
    shift = 6 if ws.lengths is not None else 0
    ws.wire_offsets(shift)
    codes = host_alloc("bytes", np.uint8, prob.codes.shape[0])
    codes[:] = prob.codes
    offsets = host_alloc("dense", np.int64, prob.offsets.shape[0])
    offsets[:] = prob.offsets
    eng = HipSearchEngine(device=0)
    eng.set_problem(prob.weights, prob.seq1)
    row = {"shape": shape, "records": prob.n, "L1": prob.L1, "letters": int(ws.total), "len_bits": int(ws.len_bits),
           "off_shift": shift}
    # (c): destinations, device-resident sources and their host description
    codes_t = torch.empty(ws.total, dtype=torch.uint8, device=dev)
    dense_t = torch.empty(ws.n + 1, dtype=torch.int64, device=dev)
    host_b, keep = wire_batch_of(ws, shift)
    d_letters = torch.from_numpy(np.ascontiguousarray(ws.codes)).to(dev)
    d_offsets = torch.from_numpy(np.ascontiguousarray(ws.wire_offsets(shift))).to(dev)
    d_lengths = None if ws.lengths is None else torch.from_numpy(np.ascontiguousarray(ws.lengths)).to(dev)
    dev_b = _lib.WireBatch(letters=d_letters.data_ptr(), offsets=d_offsets.data_ptr(),
                           lengths=None if d_lengths is None else d_lengths.data_ptr(), n=ws.n,
                           len_base=int(ws.len_base), packed=3, off_shift=shift, len_bits=int(ws.len_bits or 8), device=1)
    stream = torch.cuda.Stream(device=dev)

    def decode_ms(b, meta):
        eng.decode_wire_into(b, codes_t, dense_t, host_meta=meta, stream=stream)
        return eng.device_kernel_ms()  # the engine's events around the decode's launches; waits for them

    def topk_wire():
        eng.solve_topk_wire(ws, 1, shift)
        st = eng.stats()
        return st["total_ms"], st["kernel_ms"], int(st["h2d_bytes"])

    def topk_bytes():
        eng.solve_topk(codes, offsets, 1)
        st = eng.stats()
        return st["total_ms"], st["kernel_ms"], int(st["h2d_bytes"])

    a, b, c_host, c_dev = [], [], [], []
    for it in range(warmup + reps):
        ra, rb = topk_wire(), topk_bytes()
        rc, rd = decode_ms(host_b, None), decode_ms(dev_b, host_b)
        if it >= warmup:
            a.append(ra)
            b.append(rb)
            c_host.append(rc)
            c_dev.append(rd)
    assert np.array_equal(eng.solve_topk_wire(ws, 1, shift), eng.solve_topk(codes, offsets, 1))
    med = statistics.median
    row.update(a_wire_ms=med(x[0] for x in a), a_wire_kernel_ms=med(x[1] for x in a), a_h2d_bytes=a[0][2],
               b_bytes_ms=med(x[0] for x in b), b_bytes_kernel_ms=med(x[1] for x in b), b_h2d_bytes=b[0][2],
               c_decode_host_ms=med(c_host), c_decode_device_ms=med(c_dev))
    row["a_over_b"] = row["a_wire_ms"] / row["b_bytes_ms"]
    row["a_ms_min_max"] = [min(x[0] for x in a), max(x[0] for x in a)]
    row["b_ms_min_max"] = [min(x[0] for x in b), max(x[0] for x in b)]
    del keep
    eng.close()
    return row


def markdown(rows):
    out = ["| shape | records | letters | lengths / offsets | (a) wire ms (sweep + select) | (b) bytes ms (sweep + select) | "
           "(a)/(b) | (c) decode ms: host arrays / device arrays | h2d bytes (a) / (b) |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        form = f"{'base-6' if r['len_bits'] == 6 else str(r['len_bits']) + '-bit' if r['len_bits'] else 'none'} / " \
               f"{'1 per ' + str(1 << r['off_shift']) if r['off_shift'] else 'dense'}"
        out.append(f"| {r['shape']} | {r['records']} | {r['letters']} | {form} | {r['a_wire_ms']:.3f} "
                   f"({r['a_wire_kernel_ms']:.3f}) | {r['b_bytes_ms']:.3f} ({r['b_bytes_kernel_ms']:.3f}) | "
                   f"{r['a_over_b']:.2f} | {r['c_decode_host_ms']:.3f} / {r['c_decode_device_ms']:.3f} | "
                   f"{r['a_h2d_bytes']} / {r['b_h2d_bytes']} |")
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
