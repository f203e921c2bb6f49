/* Flat C ABI of libmoc.so — consumed by the Python package through ctypes (no pybind/torch build
 * dependency, so the same shared object serves the CLI, the tests and the torch-facing ops).
 * Every function returns 0 on success or -1 on error (message: moc_last_error()). */
#ifndef MOC_CAPI_H_
#define MOC_CAPI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct moc_result {
  int32_t score, n, k;
} moc_result;

const char* moc_last_error(void);
int moc_abi_version(void);
int moc_set_log_level(const char* level);

/* ---- problem / io ---- */
void* moc_parse(const char* data, size_t len, int strict_limits);
void moc_problem_free(void* p);
int moc_problem_info(void* p, int32_t* weights4, int64_t* L1, int64_t* n, int64_t* total_chars);
const uint8_t* moc_problem_seq1(void* p);
const uint8_t* moc_problem_codes(void* p);
const int64_t* moc_problem_offsets(void* p);
/* Formats rows into buf (cap bytes); returns bytes written or -1 (needs ~96 B per row). */
int64_t moc_format_results(const moc_result* r, int64_t n, int64_t first_index, char* buf, int64_t cap);

/* ---- 5-bit packed letter codes (moc/problem.hpp) ---- */
int64_t moc_packed5_bytes(int64_t n_chars);
int moc_pack5(const uint8_t* codes, int64_t n, uint8_t* out);
int moc_unpack5(const uint8_t* packed, int64_t begin, int64_t n, uint8_t* out);
// 33-bit fields: 7 letters per field, 56 letters per 33 bytes (moc::pack33, 4.714 bits per letter)
int64_t moc_packed33_bytes(int64_t n_chars);
int moc_pack33(const uint8_t* codes, int64_t n, uint8_t* out);
int moc_unpack33(const uint8_t* packed, int64_t begin, int64_t n, uint8_t* out);
// narrow record lengths from CSR offsets (moc::pack_lengths): bits 3 / 4 / 8, or 6 = base-6 octets
int moc_pack_lengths(const int64_t* offsets, int64_t n, int bits, int64_t base, uint8_t* out);

/* ---- score table ---- */
int moc_score_table(const int32_t* weights4, int32_t* lut1024, uint8_t* cls1024);

/* ---- exactness bounds of the kernels' narrow-integer forms (moc/kernel_bounds.hpp); no GPU needed ----
 * out6: [0] swipe key form (moc::bounds::kFormSwipeKBits / kFormSwipeRK, 0 = the swipe kernel's integer
 * bounds refuse the batch), [1] 1 if the short kernel's packed int16 form is exact, [2] the int32 hot-key
 * shift of the short / tile kernels (0 = 64-bit keys), [3] 1 if the tile16 profile holds the table, [4] the
 * index bits of tile16's 32-bit selection keys (0 = 64-bit keys), [5] 1 if the int16 tile16 profile holds the
 * table. */
int moc_kernel_bounds(const int32_t* weights4, int64_t L1, int64_t min_l2, int64_t max_l2, int32_t* out6);
/* ---- the staged pipeline's cut (moc/tile_plan.hpp plan::staged_chunks); no GPU needed ----
 * The chunks an engine made with these sizes cuts a batch into (0 for a size: the engine's default): their bounds
 * 0 = b0 < b1 < ... = n into bounds_out (room for n + 1 entries). Returns the number of chunks, -1 on error. */
int64_t moc_staged_chunks(const int64_t* offsets, int64_t n, int64_t chunk_records, int64_t chunk_bytes,
                          int64_t* bounds_out);
/* "src=<source hash> defs=<-D flags of the kernel objects>" (empty defs: the product build) */
const char* moc_build_info(void);

/* ---- CPU engine (OpenMP) ---- */
int moc_cpu_solve(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                  const int64_t* offsets, int64_t n, int semantics, int threads, moc_result* out);
int moc_brute_force(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                    const int64_t* offsets, int64_t n, int semantics, moc_result* out);

/* ---- context-parallel partial searches (packed 64-bit keys; 0 = no candidate) ---- */
int moc_cpu_solve_keys(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                       const int64_t* offsets, int64_t n, int semantics, int part, int parts, int threads,
                       uint64_t* keys);
/* MAX-combined pass-1 keys -> results: k resolved on each record's winning diagonal (needs the batch). */
int moc_resolve_keys(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                     const int64_t* offsets, int64_t n, const uint64_t* keys, moc_result* out);

/* ---- per-offset score profile and top-K alignments (moc/cpu_engine.hpp) ----
 * A record's profile has C = moc_candidate_offsets(L1, L2, semantics) entries {int32 score, int32 k}: entry o is
 * the best candidate at offset o. poffsets (n + 1, filled by the call) indexes the batch's flat profile; prof may
 * be NULL to get poffsets alone. Top-K: out is int32 [n, K, 3] rows (score, n, k) in better() order, padded with
 * (INT32_MIN, 0, 0); K outside 1..64 is an error. */
typedef struct moc_profile_entry {
  int32_t score, k;
} moc_profile_entry;
int64_t moc_candidate_offsets(int64_t L1, int64_t L2, int semantics);
int moc_cpu_profile(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                    const int64_t* offsets, int64_t n, int semantics, int threads, int64_t* poffsets,
                    moc_profile_entry* prof);
int moc_cpu_topk(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                 const int64_t* offsets, int64_t n, int semantics, int threads, int K, moc_result* out);

/* ---- threshold hits (moc/cpu_engine.hpp hits_batch_cpu) ----
 * Every offset o of record i whose profile score is >= its threshold (thresholds[i], or min_score for all records
 * when thresholds is NULL; INT32_MIN selects the whole profile), as rows (score, n = o, k) in ascending o.
 * hoffsets: int64 [n + 1], filled completely whatever cap is: hoffsets[0] = 0, record i's rows are
 * rows[hoffsets[i] .. hoffsets[i + 1]), hoffsets[n] is the total. A row is written iff its flat index is < cap;
 * nothing at or past rows + cap is touched; cap = 0 with rows = NULL counts only. */
int moc_cpu_hits(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes, const int64_t* offsets,
                 int64_t n, int semantics, int threads, int32_t min_score, const int32_t* thresholds, int64_t* hoffsets,
                 moc_result* rows, int64_t cap);
/* out2: records per scan block and block sums per pass of the single scanning block of the GPU's prefix sum
 * (moc/kernel_bounds.hpp); no GPU needed */
int moc_hits_geometry(int32_t* out2);

/* ---- alignment report (moc/cpu_engine.hpp report_batch_cpu) ----
 * rows: [n, K] result rows, K in 1..64. counts: int32 [n, K, 4] sign counts ($ % # space) of each row — 0 for an
 * empty row (score INT32_MIN), -1 for a row whose n / k do not place the record inside Seq1. marks (NULL = none):
 * K * letters bytes, row j of record i at K * (offsets[i] - offsets[0]) + j * L2_i, one of '$' '%' '#' ' ' per
 * letter (0 for empty and invalid rows). The row's score is not checked against the counts. */
int moc_cpu_report(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                   const int64_t* offsets, int64_t n, int threads, int K, const moc_result* rows, int32_t* counts,
                   uint8_t* marks);

/* ---- partition ---- */
int moc_partition(const int64_t* lengths, int64_t n, int64_t L1, int parts, double cell_w, double byte_w,
                  double record_w, int64_t* bounds_out /* parts+1 */);

/* ---- HIP engine ---- */
int moc_device_count(void);
/* Page-locks [p, p+bytes) for direct DMA (hipHostRegister on the enclosing page range). */
int moc_host_register(void* p, size_t bytes);
// Page-locked host allocation known to the streaming paths (nullptr on failure; moc_last_error).
void* moc_host_alloc(size_t bytes);
int moc_host_free(void* p);
/* Binds CPUs + future host allocations of this process to the device's NUMA node; returns node or -1. */
int moc_bind_numa(int device);
int moc_device_numa_node(int device);
/* Runs the DPP/shuffle self-test kernel; fills 192 ints (layout: align_kernels.hip dpp_probe_kernel). */
int moc_dpp_probe(int32_t* out192);
/* i8 MFMA layout self-test: c = a * b for row-major 32x32 int8 a, b (tile_mfma_kernels.hip). */
int moc_mfma_i8_probe(const int8_t* a32x32, const int8_t* b32x32, int32_t* c32x32);
/* Transfer calibration: GB/s for kind 0 H2D, 1 D2H, 2 both, 3 zero-copy read, 4 zero-copy write, 5 D2D. */
double moc_transfer_probe(int kind, size_t bytes, int iters);
/* out6: type, hostPointer, devicePointer, hipHostGetDevicePointer, hipMemGetAddressRange base, size */
int moc_pointer_info(const void* p, size_t bytes, uint64_t* out6);
/* 1 when every byte of [p, p+bytes) is page-locked through this library's registry */
int moc_pinned_covers(const void* p, size_t bytes);
int moc_host_unregister(void* p);
int moc_device_info_json(int device, char* buf, int64_t cap);
void* moc_engine_create(int device, int64_t chunk_records, int64_t chunk_bytes, int allow_direct);
void moc_engine_destroy(void* e);
int moc_engine_set_problem(void* e, const int32_t* weights4, const uint8_t* seq1, int64_t L1, int semantics);
int moc_engine_solve(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, moc_result* out);
/* fmt: 0 = R12 (moc_result), 1 = R8 {i32,u16,u16}, 2 = R4 {i16,u8,u8}, 3 = R2 (u16 mixed-radix code,
 * moc_engine_r2_params); lengths (len_bits 8, or 4 = two per byte, value + len_base) / min_l2 / max_l2
 * optional (NULL / -1). Pinned host buffers + short records -> zero-copy streaming kernel. */
int moc_engine_solve_ex(void* e, const uint8_t* codes, const int64_t* offsets, const uint8_t* lengths, int len_bits,
                        int len_base, int64_t n, void* out, int fmt, int64_t min_l2, int64_t max_l2,
                        int packed);  // packed: 0 byte letters, 1 5-bit packed, 3 P33 fields
int moc_engine_auto_format(void* e, int64_t max_l2, int64_t min_l2);
/* R2 parameters {smin, kw, j} for records with lengths in [min_l2, max_l2] */
int moc_engine_r2_params(void* e, int64_t min_l2, int64_t max_l2, int32_t* out3);
int moc_engine_pin(void* e, const void* p, size_t bytes);

// Device-resident batch in the wire formats (every pointer device memory of the engine's GPU; packed 3 =
// P33 letters, 0 = bytes; dense offsets; narrow lengths as in moc_engine_solve_ex): the swipe kernel reads
// them in place (the rccl transport's path, csrc/src/device_batch.cpp). Synchronous; stats give the
// kernel time.
int moc_engine_solve_wire_device(void* e, const uint8_t* d_letters, const int64_t* d_offsets, const uint8_t* d_lengths,
                                 int len_bits, int len_base, int64_t n, void* d_out, int fmt, int64_t min_l2,
                                 int64_t max_l2, int packed);
// The same with sparse offsets (the rccl transport's batches): d_offsets holds one entry per 2^off_shift
// records and the batch end (moc::sparse_count entries; off_shift 0: dense); narrow lengths are then required.
int moc_engine_solve_wire_device_sparse(void* e, const uint8_t* d_letters, const int64_t* d_offsets, int off_shift,
                                        const uint8_t* d_lengths, int len_bits, int len_base, int64_t n, void* d_out,
                                        int fmt, int64_t min_l2, int64_t max_l2, int packed);
// device time (ms) of the last moc_engine_solve_device's kernels; waits for them
int moc_engine_device_kernel_ms(void* e, double* ms);
int moc_engine_solve_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                            int64_t n, moc_result* d_out, void* stream);
int moc_engine_search_keys(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int part, int parts,
                           uint64_t* keys);
int moc_engine_search_keys_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                  int64_t n, int part, int parts, uint64_t* d_keys, void* stream);
int moc_engine_finalize_keys_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, const uint64_t* d_keys, void* d_out,
                                    int fmt, void* stream);
/* Profile / top-K on the GPU (byte letters, dense offsets; moc/hip_engine.hpp). Host forms are synchronous
 * (poffsets: n + 1 entries, filled; prof: poffsets[n] entries, NULL = poffsets alone); device forms queue on
 * `stream` without a sync (d_prof: the flat profile in the host-computed poffsets order; d_out: [n, K, 3]). */
int moc_engine_solve_profile(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int64_t* poffsets,
                             moc_profile_entry* prof);
int moc_engine_solve_topk(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int K, moc_result* out);
int moc_engine_solve_profile_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, moc_profile_entry* d_prof, void* stream);
int moc_engine_solve_topk_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                 int64_t n, int K, moc_result* d_out, void* stream);
/* bound (bytes) of the top-K profile scratch; a record larger than it still runs, alone in its chunk */
int moc_engine_set_profile_scratch(void* e, int64_t bytes);
/* device time (ms) of the last top-K call's select launches (engines started with MOC_PROFILE_TIMING=1; else 0) */
int moc_engine_topk_select_ms(void* e, double* ms);
/* Alignment report on the GPU (byte letters, dense offsets): as moc_cpu_report. The host form is synchronous; the
 * device form queues on `stream` without a sync (d_counts 16-byte aligned; d_marks NULL or K * letters bytes). */
int moc_engine_report(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int K, const moc_result* rows,
                      int32_t* counts, uint8_t* marks);
int moc_engine_report_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                             int64_t n, int K, const moc_result* d_rows, int32_t* d_counts, uint8_t* d_marks,
                             void* stream);
/* Threshold hits on the GPU (byte letters, dense offsets; moc/hip_engine.hpp), as moc_cpu_hits. The device form
 * queues on `stream` without a sync (d_thresholds: device int32 [n] or NULL; d_hoffsets: device int64 [n + 1];
 * d_rows: cap rows, NULL with cap = 0). The host form is synchronous and optimistic: it runs with room for
 * max(max_rows_hint, 1) rows (hint < 0: 4 n) and once more with the exact total when that was too few
 * (moc_engine_hits_passes); it fills hoffsets, keeps the rows for this thread's next moc_engine_hits_rows and
 * copies the first min(total, cap) of them to rows (NULL with cap = 0: none). */
int moc_engine_solve_hits(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int32_t min_score,
                          const int32_t* thresholds, int64_t max_rows_hint, int64_t* hoffsets, moc_result* rows,
                          int64_t cap);
/* the first min(total, cap) rows of this thread's last moc_engine_solve_hits; releases them */
int moc_engine_hits_rows(moc_result* rows, int64_t cap);
int moc_engine_hits_passes(void* e);
int moc_engine_solve_hits_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                 int64_t n, int32_t min_score, const int32_t* d_thresholds, int64_t* d_hoffsets,
                                 moc_result* d_rows, int64_t cap, void* stream);
/* device time (ms) of the last hits call's count + scan + compact launches (MOC_PROFILE_TIMING=1; else 0) */
int moc_engine_hits_select_ms(void* e, double* ms);
/* ---- wire-format batches (moc/wire.hpp) ----
 * One batch in the wire formats: letters as P33 fields (packed 3), 5-bit packed (1) or bytes (0), record i at letter
 * offsets[i]; offsets dense (off_shift 0, n + 1 entries) or sparse (one per 2^off_shift records and the batch end;
 * lengths required); lengths NULL or narrow (len_bits 8 / 4 / 3, or 6 = base-6 octets, value + len_base). device 1:
 * every pointer is device memory of the engine's GPU. */
typedef struct moc_wire_batch {
  const uint8_t* letters;
  const int64_t* offsets;
  const uint8_t* lengths;
  int64_t n;
  int64_t len_base;
  int32_t packed;
  int32_t off_shift;
  int32_t len_bits;
  int32_t device;
} moc_wire_batch;
/* Host reference decode (moc::decode_wire_cpu): sizes2 = {bytes of codes_out, bytes of offsets_out}; with
 * codes_out and offsets_out NULL only the sizes are computed. codes_out: one byte per letter of
 * [offsets[0], end); offsets_out: n + 1 absolute dense offsets. An inconsistent batch is an error. */
int moc_cpu_decode_wire(const moc_wire_batch* b, uint8_t* codes_out, int64_t* offsets_out, int64_t* sizes2);
/* The decode on the GPU (moc::HipEngine::decode_wire_device), queued on `stream` without a sync into buffers of the
 * engine that stay valid until its next decode. host_meta: for a device-resident batch, the same batch with host
 * copies of its offsets and lengths (letters unused); NULL for a host batch. out3: the device addresses of the
 * letters' base (record i at base + offsets[i]) and of the n + 1 dense offsets, and the letter count.
 * h_offsets_out: n + 1 entries, the host copy of the dense offsets. d_codes_dst / d_offsets_dst: NULL, or device
 * buffers of the caller (letter count bytes / n + 1 entries) that receive the decode instead of the engine's. */
int moc_engine_decode_wire_device(void* e, const moc_wire_batch* b, const moc_wire_batch* host_meta, void* stream,
                                  uint64_t* out3, int64_t* h_offsets_out, uint8_t* d_codes_dst, int64_t* d_offsets_dst);
/* The search of a host wire batch (moc::HipEngine::solve_wire, what ./final's GPU ranks call): results in `fmt`
 * (moc_engine_solve_ex) into out; min_l2 / max_l2: the batch's length range (-1: unknown; required with sparse
 * offsets). Zero-copy when every array is page-locked and the streaming kernel takes the batch, else the staged
 * pipeline (P33 letters unpacked and sparse offsets expanded on the host first). Synchronous. */
int moc_engine_solve_wire(void* e, const moc_wire_batch* b, void* out, int fmt, int64_t min_l2, int64_t max_l2);
/* Profile, top-K, hits and report of a host wire batch: the decode above, then moc_engine_solve_profile /
 * _solve_topk / _solve_hits / _report on the decoded buffers, with their arguments and contracts. Synchronous. */
int moc_engine_solve_profile_wire(void* e, const moc_wire_batch* b, int64_t* poffsets, moc_profile_entry* prof);
int moc_engine_solve_topk_wire(void* e, const moc_wire_batch* b, int K, moc_result* out);
int moc_engine_solve_hits_wire(void* e, const moc_wire_batch* b, int32_t min_score, const int32_t* thresholds,
                               int64_t max_rows_hint, int64_t* hoffsets, moc_result* rows, int64_t cap);
int moc_engine_report_wire(void* e, const moc_wire_batch* b, int K, const moc_result* rows, int32_t* counts,
                           uint8_t* marks);
/* ---- distinct placements (moc/cpu_engine.hpp peaks_filter) ----
 * Top-K and hits over the peaks of radius `radius` only: entry o of a record's profile is a peak iff no entry o' with
 * 0 < |o - o'| <= radius inside the profile has a higher score, or an equal score and a smaller offset. Arguments,
 * shapes and contracts are those of the calls they are named after (top-K pads with (INT32_MIN, 0, 0) past the
 * record's peaks; the hits index is exact and the capacity contract unchanged); radius = 0 gives their results,
 * a radius outside 0 .. moc_peaks_max_radius() is an error. */
int moc_peaks_max_radius(void);
/* out3: the largest radius, the most profile entries of a record the GPU's wave-per-record peak kernel takes, and the
 * entries per tile of its tile kernel (moc/kernel_bounds.hpp); no GPU needed */
int moc_peaks_geometry(int32_t* out3);
int moc_cpu_topk_distinct(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                          const int64_t* offsets, int64_t n, int semantics, int threads, int K, int64_t radius,
                          moc_result* out);
int moc_cpu_hits_distinct(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                          const int64_t* offsets, int64_t n, int semantics, int threads, int32_t min_score,
                          const int32_t* thresholds, int64_t radius, int64_t* hoffsets, moc_result* rows, int64_t cap);
int moc_engine_solve_topk_distinct(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int K,
                                   int64_t radius, moc_result* out);
int moc_engine_solve_topk_device_distinct(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                          const int64_t* h_offsets, int64_t n, int K, int64_t radius, moc_result* d_out,
                                          void* stream);
int moc_engine_solve_topk_wire_distinct(void* e, const moc_wire_batch* b, int K, int64_t radius, moc_result* out);
/* rows: as moc_engine_solve_hits (kept for this thread's next moc_engine_hits_rows; moc_engine_hits_passes tells) */
int moc_engine_solve_hits_distinct(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int32_t min_score,
                                   const int32_t* thresholds, int64_t radius, int64_t max_rows_hint, int64_t* hoffsets,
                                   moc_result* rows, int64_t cap);
int moc_engine_solve_hits_device_distinct(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                          const int64_t* h_offsets, int64_t n, int32_t min_score,
                                          const int32_t* d_thresholds, int64_t radius, int64_t* d_hoffsets,
                                          moc_result* d_rows, int64_t cap, void* stream);
int moc_engine_solve_hits_wire_distinct(void* e, const moc_wire_batch* b, int32_t min_score, const int32_t* thresholds,
                                        int64_t radius, int64_t max_rows_hint, int64_t* hoffsets, moc_result* rows,
                                        int64_t cap);
/* ---- profile summary (moc/cpu_engine.hpp summary_batch_cpu) ----
 * Per record the moments and extremes of its whole per-offset profile and, optionally, a histogram of its scores.
 * summary: int64 [n, 7], columns (count, sum, sumsq, min, max, n, k): count = the record's candidate offsets C, sum and
 * sumsq of the scores (exact), min and max over them, (max, n, k) the search's result; C = 0 gives
 * (0, 0, 0, INT32_MAX, INT32_MIN, 0, 0). hist: int32 [n, bins], bins in 0 .. 256 (0: none, hist may be NULL and is
 * not touched): a score s counts in bin clamp(floor((s - lo) / width), 0, bins - 1), computed in 64 bits; width >= 1;
 * every row sums to count. Errors, all reported before any work and with a message that starts with "summary:": bins
 * or width out of range, and the exactness bound — with M = min(2^31, max |W| * the call's longest record), a record
 * of more than moc_summary_bound(max |W|, longest record) = floor((2^63 - 1) / M^2) candidate offsets could overflow
 * sumsq. The engine forms are as moc_engine_solve_hits*: the host and wire forms synchronous, the device form queued
 * on `stream` without a sync (d_summary: device int64 [n, 7]; d_hist: device int32 [n, bins] or NULL). */
int moc_cpu_summary(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                    const int64_t* offsets, int64_t n, int semantics, int threads, int32_t bins, int32_t lo,
                    int32_t width, int64_t* summary, int32_t* hist);
/* out3: records per workgroup of the GPU's summary kernels (one wave each), threads per workgroup, and the largest
 * bins (moc/kernel_bounds.hpp); no GPU needed */
int moc_summary_geometry(int32_t* out3);
int64_t moc_summary_bound(int32_t max_abs_weight, int64_t max_l2);
int moc_engine_solve_summary(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int32_t bins, int32_t lo,
                             int32_t width, int64_t* summary, int32_t* hist);
int moc_engine_solve_summary_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, int32_t bins, int32_t lo, int32_t width, int64_t* d_summary,
                                    int32_t* d_hist, void* stream);
int moc_engine_solve_summary_wire(void* e, const moc_wire_batch* b, int32_t bins, int32_t lo, int32_t width,
                                  int64_t* summary, int32_t* hist);
/* device time (ms) of the last summary call's summary + histogram launches (MOC_PROFILE_TIMING=1; else 0) */
int moc_engine_summary_ms(void* e, double* ms);
/* ---- multi-target search (moc/cpu_engine.hpp targets_batch_cpu) ----
 * Seq1 is a catalog: T target sequences concatenated without separators, delimited by starts (int64 [T + 1], strictly
 * rising from 0 to L1; 1 <= T <= 4096). rows: moc_result [n * T], record-major: rows[i * T + t] is what the search
 * returns for record i against target t alone, n relative to the target's start ((INT32_MIN, 0, 0) where the record
 * is longer than the target). Errors in T or starts are reported before any work, with a message that starts with
 * "targets:". The engine forms are as moc_engine_solve_summary*: the host and wire forms synchronous, the device
 * form queued on `stream` without a sync (d_rows: device moc_result [n * T]; d_starts: a device copy of h_starts, or
 * NULL — then the engine uploads h_starts with its plan). */
int moc_cpu_targets(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                    const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics, int threads,
                    moc_result* rows);
/* 0 when starts / T describe a target set over a catalog of L1 letters, else the "targets:" error; no GPU needed */
int moc_check_targets(const int64_t* starts, int64_t T, int64_t L1);
/* out4: the largest T, threads per workgroup of the GPU's targets kernel, and the longest slices a 4-lane and a
 * 16-lane group take (moc/kernel_bounds.hpp); no GPU needed */
int moc_targets_geometry(int32_t* out4);
int moc_engine_solve_targets(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts,
                             int64_t T, moc_result* rows);
int moc_engine_solve_targets_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, const int64_t* d_starts, const int64_t* h_starts, int64_t T,
                                    moc_result* d_rows, void* stream);
int moc_engine_solve_targets_wire(void* e, const moc_wire_batch* b, const int64_t* starts, int64_t T, moc_result* rows);
/* device time (ms) of the last targets call's select launches (MOC_PROFILE_TIMING=1; else 0) */
int moc_engine_targets_ms(void* e, double* ms);
/* ---- target ranking (moc/cpu_engine.hpp targets_rank_batch_cpu) ----
 * Seq1 is a catalog delimited by starts as above. rows: moc_rank_row [n * M], record-major, 1 <= M <= 64: record i's
 * min(M, F_i) best targets among the F_i that fit it (record length <= target length), higher score first, then
 * smaller target index, each (target, score, n, k) with (score, n, k) exactly moc_cpu_targets' row [i, target]; then
 * (-1, INT32_MIN, 0, 0) rows. The n * T pair rows never exist as a whole. Errors, all reported before any work: the
 * target set's ("targets:"), then M ("rank:"). The engine forms are as moc_engine_solve_targets* (d_rows: device
 * moc_rank_row [n * M]); moc_engine_targets_ms gives the device time of the select and rank launches. */
typedef struct moc_rank_row {
  int32_t target, score, n, k;
} moc_rank_row;
int moc_cpu_targets_rank(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                         const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics, int threads,
                         int M, moc_rank_row* rows);
/* out3: the bytes of profile scratch a chunk of the engine's rank call needs per (record, target) pair, and the most
 * targets a 4-lane and a 16-lane group of the rank kernel take (moc/kernel_bounds.hpp); no GPU needed */
int moc_targets_rank_geometry(int32_t* out3);
/* The chunks an engine's rank call cuts a batch into under `scratch_bytes` of profile scratch (moc/tile_plan.hpp
 * plan::plan_profile with record_bytes = 12 T; T = 0: no per-record bytes, the cut of top-K and hits); no GPU needed.
 * Their bounds 0 = b0 < b1 < ... = n go into bounds_out (room for n + 1 entries). Returns the number of chunks, -1 on
 * error. */
int64_t moc_targets_rank_chunks(int64_t L1, const int64_t* offsets, int64_t n, int64_t T, int64_t scratch_bytes,
                                int semantics, int64_t* bounds_out);
int moc_engine_solve_targets_rank(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts,
                                  int64_t T, int M, moc_rank_row* rows);
int moc_engine_solve_targets_rank_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                         const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                         const int64_t* h_starts, int64_t T, int M, moc_rank_row* d_rows, void* stream);
int moc_engine_solve_targets_rank_wire(void* e, const moc_wire_batch* b, const int64_t* starts, int64_t T, int M,
                                       moc_rank_row* rows);
/* ---- per-target profile summary (moc/cpu_engine.hpp targets_summary_batch_cpu) ----
 * Seq1 is a catalog delimited by starts as above. summary: int64 [n * T * 7], record-major: row (i * T + t) holds
 * (count, sum, sumsq, min, max, n, k) of record i's profile against target t alone, n relative to the target's start;
 * (0, 0, 0, INT32_MAX, INT32_MIN, 0, 0) where the record is longer than the target. hist: int32 [n * T * bins], the
 * bins, lo and width of moc_cpu_summary (bins = 0: none, hist may be NULL and is not touched). Errors, all reported
 * before any work: the target set's ("targets:"), then bins, width and the exactness bound over the largest target
 * profile of the call ("summary:"). The engine forms are as moc_engine_solve_targets*. */
int moc_cpu_targets_summary(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                            const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics,
                            int threads, int32_t bins, int32_t lo, int32_t width, int64_t* summary, int32_t* hist);
/* out4: threads per workgroup of the GPU's per-target summary kernels, the largest bins, the most bins a 4-lane group
 * takes in the histogram kernel (above it a 4-lane choice becomes 16 lanes), and the LDS bytes a workgroup's
 * counters stay within (moc/kernel_bounds.hpp); no GPU needed */
int moc_targets_summary_geometry(int32_t* out4);
int moc_engine_solve_targets_summary(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n,
                                     const int64_t* starts, int64_t T, int32_t bins, int32_t lo, int32_t width,
                                     int64_t* summary, int32_t* hist);
int moc_engine_solve_targets_summary_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                            const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                            const int64_t* h_starts, int64_t T, int32_t bins, int32_t lo, int32_t width,
                                            int64_t* d_summary, int32_t* d_hist, void* stream);
int moc_engine_solve_targets_summary_wire(void* e, const moc_wire_batch* b, const int64_t* starts, int64_t T,
                                          int32_t bins, int32_t lo, int32_t width, int64_t* summary, int32_t* hist);
/* device time (ms) of the last per-target summary call's summary + histogram launches (MOC_PROFILE_TIMING=1; else 0) */
int moc_engine_targets_summary_ms(void* e, double* ms);
/* ---- per-target top-K and threshold hits (moc/cpu_engine.hpp targets_topk_batch_cpu / targets_hits_batch_cpu) ----
 * Seq1 is a catalog delimited by starts as above; pair p = i * T + t is record i against target t alone, every n
 * relative to the target's start.
 * Top-K, 1 <= K <= 64: rows [n * T * K], pair-major: the pair's min(K, entries) best placements in better() order,
 * then (INT32_MIN, 0, 0) rows. K = 1 is moc_cpu_targets.
 * Hits: thresholds NULL (min_score for every pair) or int32 [n * T], pair-major. toffsets: int64 [n * T + 1], always
 * complete and exact; pair p's hits, ascending in n, are rows[toffsets[p] .. toffsets[p + 1]); a row is written iff its
 * flat index is < cap, nothing at or past rows + cap is touched, cap = 0 (rows may be NULL) counts only — the
 * contract of moc_cpu_hits. The engine's host forms are optimistic as moc_engine_solve_hits is (max_rows_hint < 0:
 * n * T; moc_engine_hits_passes, moc_engine_hits_rows); the device forms queue on `stream` with no sync
 * (d_thresholds: device int32 [n * T] or NULL; d_starts / h_starts as moc_engine_solve_targets_device).
 * Errors, all reported before any work: the target set's ("targets:"), then K ("top-K:") or the buffers ("hits:").
 * moc_engine_targets_ms gives the device time of the new launches. */
int moc_cpu_targets_topk(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                         const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics, int threads,
                         int K, moc_result* rows);
int moc_cpu_targets_hits(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                         const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics, int threads,
                         int32_t min_score, const int32_t* thresholds, int64_t* toffsets, moc_result* rows, int64_t cap);
int moc_engine_solve_targets_topk(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts,
                                  int64_t T, int K, moc_result* rows);
int moc_engine_solve_targets_topk_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                         const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                         const int64_t* h_starts, int64_t T, int K, moc_result* d_rows, void* stream);
int moc_engine_solve_targets_topk_wire(void* e, const moc_wire_batch* b, const int64_t* starts, int64_t T, int K,
                                       moc_result* rows);
int moc_engine_solve_targets_hits(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts,
                                  int64_t T, int32_t min_score, const int32_t* thresholds, int64_t max_rows_hint,
                                  int64_t* toffsets, moc_result* rows, int64_t cap);
int moc_engine_solve_targets_hits_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                         const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                         const int64_t* h_starts, int64_t T, int32_t min_score,
                                         const int32_t* d_thresholds, int64_t* d_toffsets, moc_result* d_rows, int64_t cap,
                                         void* stream);
int moc_engine_solve_targets_hits_wire(void* e, const moc_wire_batch* b, const int64_t* starts, int64_t T,
                                       int32_t min_score, const int32_t* thresholds, int64_t max_rows_hint,
                                       int64_t* toffsets, moc_result* rows, int64_t cap);
/* The distinct forms of the eight calls above: `radius` (0 .. 2048, as moc_cpu_topk_distinct's) keeps only the peaks of
 * every pair's OWN profile — local entry o is a peak iff it is the best of the local offsets [o - radius, o + radius]
 * clipped to the pair's entries, the boundary entry among them — so pair (i, t)'s rows are those of the single-target
 * distinct calls on target t alone. radius = 0 is the call above. Errors: as above, then the radius ("distinct:"). */
int moc_cpu_targets_topk_distinct(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                                  const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics,
                                  int threads, int K, int64_t radius, moc_result* rows);
int moc_cpu_targets_hits_distinct(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                                  const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics,
                                  int threads, int32_t min_score, const int32_t* thresholds, int64_t radius,
                                  int64_t* toffsets, moc_result* rows, int64_t cap);
int moc_engine_solve_targets_topk_distinct(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n,
                                           const int64_t* starts, int64_t T, int K, int64_t radius, moc_result* rows);
int moc_engine_solve_targets_topk_device_distinct(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                                  const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                                  const int64_t* h_starts, int64_t T, int K, int64_t radius,
                                                  moc_result* d_rows, void* stream);
int moc_engine_solve_targets_topk_wire_distinct(void* e, const moc_wire_batch* b, const int64_t* starts, int64_t T, int K,
                                                int64_t radius, moc_result* rows);
int moc_engine_solve_targets_hits_distinct(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n,
                                           const int64_t* starts, int64_t T, int32_t min_score, const int32_t* thresholds,
                                           int64_t max_rows_hint, int64_t radius, int64_t* toffsets, moc_result* rows,
                                           int64_t cap);
int moc_engine_solve_targets_hits_device_distinct(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                                  const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                                  const int64_t* h_starts, int64_t T, int32_t min_score,
                                                  const int32_t* d_thresholds, int64_t radius, int64_t* d_toffsets,
                                                  moc_result* d_rows, int64_t cap, void* stream);
int moc_engine_solve_targets_hits_wire_distinct(void* e, const moc_wire_batch* b, const int64_t* starts, int64_t T,
                                                int32_t min_score, const int32_t* thresholds, int64_t max_rows_hint,
                                                int64_t radius, int64_t* toffsets, moc_result* rows, int64_t cap);
/* stats: kernel_ms, total_ms, h2d_bytes, d2h_bytes, chunks, cells, records, direct, format, kernels,
 * r2 smin, r2 kw, r2 j, forms (moc::bounds::FormBits of the last solve) */
int moc_engine_stats(void* e, double* out14);

#ifdef __cplusplus
}
#endif

#endif
