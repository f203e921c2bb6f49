// C ABI implementation (see moc/capi.h).
#include "moc/capi.h"

#include <cstring>
#include <exception>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "moc/cpu_engine.hpp"
#include "moc/device.hpp"
#include "moc/hip_engine.hpp"
#include "moc/io.hpp"
#include "moc/partition.hpp"
#include "moc/problem.hpp"
#include "moc/runtime/device.hpp"
#include "moc/runtime/hip_check.hpp"
#include "moc/runtime/log.hpp"
#include "moc/runtime/pinned.hpp"
#include "moc/score_table.hpp"
#include "moc/tile_plan.hpp"

static_assert(sizeof(moc_result) == sizeof(moc::Result), "ABI result layout");
static_assert(sizeof(moc_rank_row) == sizeof(moc::RankRow), "ABI rank row layout");
static_assert(sizeof(moc_profile_entry) == sizeof(moc::ProfileEntry), "ABI profile entry layout");

namespace {
thread_local std::string g_err;

template <class F>
int guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
  } catch (...) {
    g_err = "unknown error";
  }
  return -1;
}

moc::Weights weights_of(const int32_t* w4) {
  moc::Weights w;
  for (int i = 0; i < 4; ++i) w.w[i] = w4[i];
  return w;
}

// moc_host_register calls -> the registrations each made (released together by moc_host_unregister)
std::mutex g_host_regs_mu;
std::map<void*, std::vector<void*>> g_host_regs;

moc::RecordBatch view_batch(const uint8_t* codes, const int64_t* offsets, int64_t n) {
  moc::RecordBatch b;
  const int64_t base = offsets[0];
  b.codes.assign(codes + base, codes + offsets[n]);
  b.offsets.resize(static_cast<size_t>(n) + 1);
  for (int64_t i = 0; i <= n; ++i) b.offsets[i] = offsets[i] - base;
  return b;
}
}  // namespace

extern "C" {

const char* moc_last_error(void) { return g_err.c_str(); }
int moc_abi_version(void) { return 1; }
int moc_set_log_level(const char* level) {
  return guard([&] { moc::log_set_level(std::string(level)); });
}

void* moc_parse(const char* data, size_t len, int strict_limits) {
  moc::Problem* p = nullptr;
  int rc = guard([&] {
    moc::ParseOptions opt;
    opt.strict_limits = strict_limits != 0;
    p = new moc::Problem(moc::parse_problem(data, len, opt));
  });
  return rc == 0 ? p : nullptr;
}

void moc_problem_free(void* p) { delete static_cast<moc::Problem*>(p); }

int moc_problem_info(void* p, int32_t* weights4, int64_t* L1, int64_t* n, int64_t* total_chars) {
  return guard([&] {
    auto* pr = static_cast<moc::Problem*>(p);
    for (int i = 0; i < 4; ++i) weights4[i] = pr->weights.w[i];
    *L1 = pr->L1();
    *n = pr->seq2.size();
    *total_chars = pr->seq2.total_chars();
  });
}
const uint8_t* moc_problem_seq1(void* p) { return static_cast<moc::Problem*>(p)->seq1.data(); }
const uint8_t* moc_problem_codes(void* p) { return static_cast<moc::Problem*>(p)->seq2.codes.data(); }
const int64_t* moc_problem_offsets(void* p) { return static_cast<moc::Problem*>(p)->seq2.offsets.data(); }

int64_t moc_format_results(const moc_result* r, int64_t n, int64_t first_index, char* buf, int64_t cap) {
  int64_t written = -1;
  guard([&] {
    std::string s = moc::format_results(reinterpret_cast<const moc::Result*>(r), n, first_index);
    if (static_cast<int64_t>(s.size()) > cap) throw moc::Error("format buffer too small");
    std::memcpy(buf, s.data(), s.size());
    written = static_cast<int64_t>(s.size());
  });
  return written;
}

int64_t moc_packed5_bytes(int64_t n_chars) { return moc::packed5_bytes(n_chars); }
int moc_pack5(const uint8_t* codes, int64_t n, uint8_t* out) {
  return guard([&] { moc::pack5(codes, n, out); });
}
int moc_unpack5(const uint8_t* packed, int64_t begin, int64_t n, uint8_t* out) {
  return guard([&] { moc::unpack5(packed, begin, n, out); });
}
int64_t moc_packed33_bytes(int64_t n_chars) { return moc::packed33_bytes(n_chars); }
int moc_pack33(const uint8_t* codes, int64_t n, uint8_t* out) {
  return guard([&] { moc::pack33(codes, n, out); });
}
int moc_unpack33(const uint8_t* packed, int64_t begin, int64_t n, uint8_t* out) {
  return guard([&] { moc::unpack33(packed, begin, n, out); });
}
int moc_pack_lengths(const int64_t* offsets, int64_t n, int bits, int64_t base, uint8_t* out) {
  return guard([&] { moc::pack_lengths(offsets, n, bits, base, out); });
}

int moc_score_table(const int32_t* weights4, int32_t* lut1024, uint8_t* cls1024) {
  return guard([&] {
    moc::ScoreTable t = moc::ScoreTable::build(weights_of(weights4));
    if (lut1024) std::memcpy(lut1024, t.lut.data(), sizeof(int32_t) * t.lut.size());
    if (cls1024) std::memcpy(cls1024, t.cls.data(), t.cls.size());
  });
}

int moc_kernel_bounds(const int32_t* weights4, int64_t L1, int64_t min_l2, int64_t max_l2, int32_t* out6) {
  return guard([&] {
    const moc::ScoreTable t = moc::ScoreTable::build(weights_of(weights4));
    const int32_t w = t.max_abs();
    const int64_t searched = std::max<int64_t>(1, std::min(max_l2, L1 + 1));  // longer records are not searched
    out6[0] = moc::dev::swipe_form(L1, min_l2, max_l2, w);
    out6[1] = moc::bounds::short_pk_exact(w, searched) ? 1 : 0;
    out6[2] = moc::bounds::key_shift(w, searched);
    out6[3] = moc::profile16_fits(t) ? 1 : 0;
    out6[4] = moc::bounds::tile16_key32_bits(L1, w, searched);
    out6[5] = moc::profile16_i16_fits(t) ? 1 : 0;
  });
}

int64_t moc_staged_chunks(const int64_t* offsets, int64_t n, int64_t chunk_records, int64_t chunk_bytes,
                          int64_t* bounds_out) {
  int64_t chunks = -1;
  guard([&] {
    if (n < 0 || chunk_records < 0 || chunk_bytes < 0) throw moc::Error("staged_chunks: negative size");
    for (int64_t i = 0; i < n; ++i)
      if (offsets[i + 1] < offsets[i]) throw moc::Error("staged_chunks: offsets must not decrease");
    const moc::EngineOptions defaults;
    chunks = moc::plan::staged_chunks(offsets, n, chunk_records > 0 ? chunk_records : defaults.chunk_records,
                                      chunk_bytes > 0 ? chunk_bytes : defaults.chunk_bytes, bounds_out);
  });
  return chunks;
}

int moc_cpu_solve(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                  const int64_t* offsets, int64_t n, int semantics, int threads, moc_result* out) {
  return guard([&] {
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::solve_batch_cpu(t, seq1, L1, b, reinterpret_cast<moc::Result*>(out), static_cast<moc::Semantics>(semantics),
                         threads);
  });
}

int moc_cpu_solve_keys(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                       const int64_t* offsets, int64_t n, int semantics, int part, int parts, int threads,
                       uint64_t* keys) {
  return guard([&] {
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::solve_keys_cpu(t, seq1, L1, b, part, parts, keys, static_cast<moc::Semantics>(semantics), threads);
  });
}

int moc_resolve_keys(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                     const int64_t* offsets, int64_t n, const uint64_t* keys, moc_result* out) {
  return guard([&] {
    const moc::ScoreTable t = moc::ScoreTable::build(weights_of(weights4));
    for (int64_t i = 0; i < n; ++i) {
      const moc::Result r = moc::resolve_key(t, seq1, L1, codes + offsets[i], offsets[i + 1] - offsets[i], keys[i]);
      std::memcpy(out + i, &r, sizeof r);
    }
  });
}

int moc_brute_force(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                    const int64_t* offsets, int64_t n, int semantics, moc_result* out) {
  return guard([&] {
    moc::ScoreTable t = moc::ScoreTable::build(weights_of(weights4));
    for (int64_t i = 0; i < n; ++i) {
      moc::Result r = moc::brute_force_record(t, seq1, L1, codes + offsets[i], offsets[i + 1] - offsets[i],
                                              static_cast<moc::Semantics>(semantics));
      std::memcpy(out + i, &r, sizeof r);
    }
  });
}

int64_t moc_candidate_offsets(int64_t L1, int64_t L2, int semantics) {
  return moc::candidate_offsets(L1, L2, static_cast<moc::Semantics>(semantics));
}

int moc_cpu_profile(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                    const int64_t* offsets, int64_t n, int semantics, int threads, int64_t* poffsets,
                    moc_profile_entry* prof) {
  return guard([&] {
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    const auto sem = static_cast<moc::Semantics>(semantics);
    moc::profile_offsets(L1, b, sem, poffsets);
    if (!prof) return;
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::profile_batch_cpu(t, seq1, L1, b, poffsets, reinterpret_cast<moc::ProfileEntry*>(prof), sem, threads);
  });
}

int moc_cpu_topk(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                 const int64_t* offsets, int64_t n, int semantics, int threads, int K, moc_result* out) {
  return guard([&] {
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::topk_batch_cpu(t, seq1, L1, b, K, reinterpret_cast<moc::Result*>(out), static_cast<moc::Semantics>(semantics),
                        threads);
  });
}

int moc_cpu_hits(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes, const int64_t* offsets,
                 int64_t n, int semantics, int threads, int32_t min_score, const int32_t* thresholds, int64_t* hoffsets,
                 moc_result* rows, int64_t cap) {
  return guard([&] {
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::hits_batch_cpu(t, seq1, L1, b, min_score, thresholds, hoffsets, reinterpret_cast<moc::Result*>(rows), cap,
                        static_cast<moc::Semantics>(semantics), threads);
  });
}

int moc_hits_geometry(int32_t* out2) {
  out2[0] = moc::bounds::kHitsScanBlockRecords;
  out2[1] = moc::bounds::kHitsScanSumsPerPass;
  return 0;
}

int moc_cpu_report(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                   const int64_t* offsets, int64_t n, int threads, int K, const moc_result* rows, int32_t* counts,
                   uint8_t* marks) {
  return guard([&] {
    const moc::ScoreTable t = moc::ScoreTable::build(weights_of(weights4));
    const moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::report_batch_cpu(t, seq1, L1, b, reinterpret_cast<const moc::Result*>(rows), K, counts, marks, threads);
  });
}

int moc_partition(const int64_t* lengths, int64_t n, int64_t L1, int parts, double cell_w, double byte_w,
                  double record_w, int64_t* bounds_out) {
  return guard([&] {
    moc::CostModel m{cell_w, byte_w, record_w};
    auto b = moc::partition_by_cost(lengths, n, L1, parts, m);
    std::memcpy(bounds_out, b.data(), sizeof(int64_t) * b.size());
  });
}

int moc_device_count(void) { return moc::device_count(); }

int moc_dpp_probe(int32_t* out192) {
  return guard([&] {
    int* d = nullptr;
    MOC_HIP_CHECK(hipMalloc(&d, 192 * sizeof(int)));
    moc::dev::launch_dpp_probe(d, nullptr);
    MOC_HIP_CHECK(hipGetLastError());
    MOC_HIP_CHECK(hipMemcpy(out192, d, 192 * sizeof(int), hipMemcpyDeviceToHost));
    MOC_HIP_CHECK(hipFree(d));
  });
}

int moc_mfma_i8_probe(const int8_t* a32x32, const int8_t* b32x32, int32_t* c32x32) {
  return guard([&] {
    char* d = nullptr;
    MOC_HIP_CHECK(hipMalloc(&d, 2 * 1024 + 4 * 1024));
    MOC_HIP_CHECK(hipMemcpy(d, a32x32, 1024, hipMemcpyHostToDevice));
    MOC_HIP_CHECK(hipMemcpy(d + 1024, b32x32, 1024, hipMemcpyHostToDevice));
    moc::dev::launch_mfma_i8_probe(reinterpret_cast<const int8_t*>(d), reinterpret_cast<const int8_t*>(d + 1024),
                                   reinterpret_cast<int*>(d + 2048), nullptr);
    MOC_HIP_CHECK(hipGetLastError());
    MOC_HIP_CHECK(hipMemcpy(c32x32, d + 2048, 4 * 1024, hipMemcpyDeviceToHost));
    MOC_HIP_CHECK(hipFree(d));
  });
}

double moc_transfer_probe(int kind, size_t bytes, int iters) {
  double gbs = -1;
  guard([&] { gbs = moc::dev::transfer_probe(kind, bytes, iters); });
  return gbs;
}

int moc_bind_numa(int device) { return moc::bind_numa_to_device(device); }
int moc_device_numa_node(int device) { return moc::device_numa_node(device); }

void* moc_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (guard([&] { p = moc::pinned::alloc_host(bytes); }) != 0) return nullptr;
  return p;
}

int moc_host_free(void* p) {
  return guard([&] { moc::pinned::free_host(p); });
}

int moc_host_register(void* p, size_t bytes) {
  return guard([&] {
    std::vector<void*> made = moc::pinned::register_range(p, bytes);
    std::lock_guard<std::mutex> lock(g_host_regs_mu);
    auto& v = g_host_regs[p];
    v.insert(v.end(), made.begin(), made.end());
  });
}

/* Diagnostics: device address of a pinned host range (0 when the range is not page-locked as one
 * registration), and the runtime's view of the pointer (type, host and device pointers). */
int moc_pointer_info(const void* p, size_t bytes, uint64_t* out4) {
  return guard([&] {
    out4[0] = out4[1] = out4[2] = out4[3] = out4[4] = out4[5] = 0;
    {
      hipDeviceptr_t base = nullptr;
      size_t size = 0;
      if (hipMemGetAddressRange(&base, &size, reinterpret_cast<hipDeviceptr_t>(const_cast<void*>(p))) == hipSuccess) {
        out4[4] = reinterpret_cast<uint64_t>(base);
        out4[5] = size;
      } else {
        (void)hipGetLastError();
      }
    }
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    out4[0] = static_cast<uint64_t>(a.type);
    out4[1] = reinterpret_cast<uint64_t>(a.hostPointer);
    out4[2] = reinterpret_cast<uint64_t>(a.devicePointer);
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) == hipSuccess) out4[3] = reinterpret_cast<uint64_t>(d);
    else (void)hipGetLastError();
    (void)bytes;
  });
}

int moc_pinned_covers(const void* p, size_t bytes) { return moc::pinned::covers(p, bytes) ? 1 : 0; }

int moc_host_unregister(void* p) {
  return guard([&] {
    std::vector<void*> bases;
    {
      std::lock_guard<std::mutex> lock(g_host_regs_mu);
      auto it = g_host_regs.find(p);
      if (it == g_host_regs.end()) return;
      bases = std::move(it->second);
      g_host_regs.erase(it);
    }
    moc::pinned::unregister(bases);
  });
}

int moc_device_info_json(int device, char* buf, int64_t cap) {
  return guard([&] {
    std::string s = moc::device_info(device).json();
    if (static_cast<int64_t>(s.size()) + 1 > cap) throw moc::Error("buffer too small");
    std::memcpy(buf, s.c_str(), s.size() + 1);
  });
}

void* moc_engine_create(int device, int64_t chunk_records, int64_t chunk_bytes, int allow_direct) {
  moc::HipEngine* e = nullptr;
  int rc = guard([&] {
    moc::EngineOptions o;
    o.device = device;
    if (chunk_records > 0) o.chunk_records = chunk_records;
    if (chunk_bytes > 0) o.chunk_bytes = chunk_bytes;
    o.allow_direct = allow_direct != 0;
    e = new moc::HipEngine(o);
  });
  return rc == 0 ? e : nullptr;
}

void moc_engine_destroy(void* e) { delete static_cast<moc::HipEngine*>(e); }

int moc_engine_set_problem(void* e, const int32_t* weights4, const uint8_t* seq1, int64_t L1, int semantics) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->set_problem(weights_of(weights4), seq1, L1, static_cast<moc::Semantics>(semantics));
  });
}

int moc_engine_solve(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, moc_result* out) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve(codes, offsets, n, reinterpret_cast<moc::Result*>(out));
  });
}

int moc_engine_solve_ex(void* e, const uint8_t* codes, const int64_t* offsets, const uint8_t* lengths, int len_bits,
                        int len_base, int64_t n, void* out, int fmt, int64_t min_l2, int64_t max_l2, int packed) {
  return guard([&] {
    moc::BatchHints h;
    h.min_l2 = min_l2;
    h.max_l2 = max_l2;
    static_cast<moc::HipEngine*>(e)->solve_ex(codes, offsets, lengths, n, out, static_cast<moc::ResultFormat>(fmt), h,
                                              packed, len_bits, len_base);
  });
}

int moc_engine_solve_wire_device(void* e, const uint8_t* d_letters, const int64_t* d_offsets, const uint8_t* d_lengths,
                                 int len_bits, int len_base, int64_t n, void* d_out, int fmt, int64_t min_l2,
                                 int64_t max_l2, int packed) {
  return moc_engine_solve_wire_device_sparse(e, d_letters, d_offsets, 0, d_lengths, len_bits, len_base, n, d_out, fmt,
                                             min_l2, max_l2, packed);
}

int moc_engine_solve_wire_device_sparse(void* e, const uint8_t* d_letters, const int64_t* d_offsets, int off_shift,
                                        const uint8_t* d_lengths, int len_bits, int len_base, int64_t n, void* d_out,
                                        int fmt, int64_t min_l2, int64_t max_l2, int packed) {
  return guard([&] {
    if (packed != 0 && packed != 3) throw moc::Error("device-resident letters: 0 bytes or 3 P33 fields");
    if (off_shift < 0 || off_shift > 6) throw moc::Error("sparse offsets: one per 2^shift records, shift 0..6");
    moc::WireBatch b;
    b.letters = d_letters;
    b.packed33 = packed == 3;
    b.offsets = d_offsets;
    b.off_shift = off_shift;
    b.lengths = d_lengths;
    b.len_bits = len_bits;
    b.len_base = len_base;
    b.n = n;
    b.min_l2 = min_l2;
    b.max_l2 = max_l2;
    b.device = true;
    static_cast<moc::HipEngine*>(e)->solve_wire(b, d_out, static_cast<moc::ResultFormat>(fmt));
  });
}

int moc_engine_auto_format(void* e, int64_t max_l2, int64_t min_l2) {
  return static_cast<int>(static_cast<moc::HipEngine*>(e)->auto_format(max_l2, min_l2));
}

int moc_engine_r2_params(void* e, int64_t min_l2, int64_t max_l2, int32_t* out3) {
  return guard([&] {
    const moc::R2Params p = static_cast<moc::HipEngine*>(e)->r2_params_for(min_l2, max_l2);
    out3[0] = p.smin;
    out3[1] = p.kw;
    out3[2] = p.j;
  });
}

int moc_engine_pin(void* e, const void* p, size_t bytes) {
  return guard([&] { static_cast<moc::HipEngine*>(e)->pin(p, bytes); });
}

int moc_engine_device_kernel_ms(void* e, double* ms) {
  return guard([&] { *ms = static_cast<moc::HipEngine*>(e)->device_kernel_ms(); });
}

int moc_engine_solve_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                            int64_t n, moc_result* d_out, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_device(d_codes, d_offsets, h_offsets, n,
                                                  reinterpret_cast<moc::Result*>(d_out),
                                                  static_cast<hipStream_t>(stream));
  });
}

int moc_engine_search_keys(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int part, int parts,
                           uint64_t* keys) {
  return guard([&] { static_cast<moc::HipEngine*>(e)->search_keys(codes, offsets, n, part, parts, keys); });
}

int moc_engine_search_keys_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                  int64_t n, int part, int parts, uint64_t* d_keys, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->search_keys_device(d_codes, d_offsets, h_offsets, n, part, parts,
                                                        reinterpret_cast<unsigned long long*>(d_keys),
                                                        static_cast<hipStream_t>(stream));
  });
}

int moc_engine_finalize_keys_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, const uint64_t* d_keys, void* d_out,
                                    int fmt, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->finalize_keys_device(d_codes, d_offsets, h_offsets, n,
                                                          reinterpret_cast<const unsigned long long*>(d_keys), d_out,
                                                          static_cast<moc::ResultFormat>(fmt),
                                                          static_cast<hipStream_t>(stream));
  });
}

int moc_engine_solve_profile(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int64_t* poffsets,
                             moc_profile_entry* prof) {
  return guard([&] {
    auto* eng = static_cast<moc::HipEngine*>(e);
    if (!prof)
      eng->profile_offsets(offsets, n, poffsets);
    else
      eng->solve_profile(codes, offsets, n, reinterpret_cast<moc::ProfileEntry*>(prof), poffsets);
  });
}

int moc_engine_solve_topk(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int K, moc_result* out) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_topk(codes, offsets, n, K, reinterpret_cast<moc::Result*>(out));
  });
}

int moc_engine_solve_profile_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, moc_profile_entry* d_prof, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_profile_device(d_codes, d_offsets, h_offsets, n,
                                                          reinterpret_cast<moc::ProfileEntry*>(d_prof),
                                                          static_cast<hipStream_t>(stream));
  });
}

int moc_engine_solve_topk_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                 int64_t n, int K, moc_result* d_out, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_topk_device(d_codes, d_offsets, h_offsets, n, K,
                                                       reinterpret_cast<moc::Result*>(d_out),
                                                       static_cast<hipStream_t>(stream));
  });
}

int moc_engine_set_profile_scratch(void* e, int64_t bytes) {
  return guard([&] { static_cast<moc::HipEngine*>(e)->set_profile_scratch(bytes); });
}

int moc_engine_topk_select_ms(void* e, double* ms) {
  return guard([&] { *ms = static_cast<moc::HipEngine*>(e)->topk_select_ms(); });
}

namespace {
thread_local std::vector<moc::Result> g_hits_rows;  // moc_engine_solve_hits -> moc_engine_hits_rows
}

int moc_engine_solve_hits(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int32_t min_score,
                          const int32_t* thresholds, int64_t max_rows_hint, int64_t* hoffsets, moc_result* rows,
                          int64_t cap) {
  return guard([&] {
    if (cap < 0 || (cap > 0 && !rows)) throw moc::Error("hits: cap rows need a rows buffer");
    static_cast<moc::HipEngine*>(e)->solve_hits(codes, offsets, n, min_score, thresholds, hoffsets, g_hits_rows,
                                                max_rows_hint);
    const size_t m = std::min(g_hits_rows.size(), static_cast<size_t>(cap));
    if (m) std::memcpy(rows, g_hits_rows.data(), sizeof(moc::Result) * m);
  });
}

int moc_engine_hits_rows(moc_result* rows, int64_t cap) {
  return guard([&] {
    if (cap < 0 || (cap > 0 && !rows)) throw moc::Error("hits: cap rows need a rows buffer");
    const size_t m = std::min(g_hits_rows.size(), static_cast<size_t>(cap));
    if (m) std::memcpy(rows, g_hits_rows.data(), sizeof(moc::Result) * m);
    std::vector<moc::Result>().swap(g_hits_rows);
  });
}

int moc_engine_hits_passes(void* e) { return static_cast<moc::HipEngine*>(e)->hits_passes(); }

int moc_engine_solve_hits_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                 int64_t n, int32_t min_score, const int32_t* d_thresholds, int64_t* d_hoffsets,
                                 moc_result* d_rows, int64_t cap, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_hits_device(d_codes, d_offsets, h_offsets, n, min_score, d_thresholds,
                                                       d_hoffsets, reinterpret_cast<moc::Result*>(d_rows), cap,
                                                       static_cast<hipStream_t>(stream));
  });
}

int moc_engine_hits_select_ms(void* e, double* ms) {
  return guard([&] { *ms = static_cast<moc::HipEngine*>(e)->hits_select_ms(); });
}

int moc_engine_report(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int K, const moc_result* rows,
                      int32_t* counts, uint8_t* marks) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->report(codes, offsets, n, K, reinterpret_cast<const moc::Result*>(rows), counts,
                                            marks);
  });
}

int moc_engine_report_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                             int64_t n, int K, const moc_result* d_rows, int32_t* d_counts, uint8_t* d_marks,
                             void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->report_device(d_codes, d_offsets, h_offsets, n, K,
                                                   reinterpret_cast<const moc::Result*>(d_rows), d_counts, d_marks,
                                                   static_cast<hipStream_t>(stream));
  });
}

namespace {
moc::WireBatch wire_batch(const moc_wire_batch* w) {
  if (!w) throw moc::Error("wire batch: null");
  if (w->packed != 0 && w->packed != 1 && w->packed != 3) throw moc::Error("letters: 0 bytes, 1 5-bit packed or 3 P33 fields");
  moc::WireBatch b;
  b.letters = w->letters;
  b.packed5 = w->packed == 1;
  b.packed33 = w->packed == 3;
  b.offsets = w->offsets;
  b.off_shift = w->off_shift;
  b.lengths = w->lengths;
  b.len_bits = w->len_bits;
  b.len_base = w->len_base;
  b.n = w->n;
  b.device = w->device != 0;
  return b;
}
}  // namespace

int moc_cpu_decode_wire(const moc_wire_batch* w, uint8_t* codes_out, int64_t* offsets_out, int64_t* sizes2) {
  return guard([&] {
    const moc::WireBatch b = wire_batch(w);
    if (b.device) throw moc::Error("decode_wire_cpu: host pointers only");
    const moc::WireDecodedBytes sz = moc::wire_decoded_bytes(b);
    if (sizes2) {
      sizes2[0] = sz.codes;
      sizes2[1] = sz.offsets;
    }
    if (offsets_out) moc::decode_wire_cpu(b, codes_out, offsets_out);
  });
}

int moc_engine_decode_wire_device(void* e, const moc_wire_batch* w, const moc_wire_batch* host_meta, void* stream,
                                  uint64_t* out3, int64_t* h_offsets_out, uint8_t* d_codes_dst, int64_t* d_offsets_dst) {
  return guard([&] {
    const moc::WireBatch b = wire_batch(w);
    moc::WireBatch m;
    if (host_meta) m = wire_batch(host_meta);
    const moc::HipEngine::DecodedWire dw = static_cast<moc::HipEngine*>(e)->decode_wire_device(
        b, host_meta ? &m : nullptr, static_cast<hipStream_t>(stream), d_codes_dst, d_offsets_dst);
    out3[0] = reinterpret_cast<uint64_t>(dw.d_codes);
    out3[1] = reinterpret_cast<uint64_t>(dw.d_offsets);
    out3[2] = static_cast<uint64_t>(dw.h_offsets[dw.n] - dw.h_offsets[0]);
    if (h_offsets_out) std::memcpy(h_offsets_out, dw.h_offsets, sizeof(int64_t) * static_cast<size_t>(dw.n + 1));
  });
}

int moc_engine_solve_profile_wire(void* e, const moc_wire_batch* w, int64_t* poffsets, moc_profile_entry* prof) {
  return guard([&] {
    auto* eng = static_cast<moc::HipEngine*>(e);
    const moc::WireBatch b = wire_batch(w);
    if (!prof)
      eng->wire_profile_offsets(b, poffsets);
    else
      eng->solve_profile_wire(b, reinterpret_cast<moc::ProfileEntry*>(prof), poffsets);
  });
}

int moc_engine_solve_wire(void* e, const moc_wire_batch* w, void* out, int fmt, int64_t min_l2, int64_t max_l2) {
  return guard([&] {
    moc::WireBatch b = wire_batch(w);
    if (b.device) throw moc::Error("solve_wire: host pointers only (moc_engine_solve_wire_device)");
    b.min_l2 = min_l2;
    b.max_l2 = max_l2;
    static_cast<moc::HipEngine*>(e)->solve_wire(b, out, static_cast<moc::ResultFormat>(fmt));
  });
}

int moc_engine_solve_topk_wire(void* e, const moc_wire_batch* w, int K, moc_result* out) {
  return guard([&] { static_cast<moc::HipEngine*>(e)->solve_topk_wire(wire_batch(w), K, reinterpret_cast<moc::Result*>(out)); });
}

int moc_engine_solve_hits_wire(void* e, const moc_wire_batch* w, int32_t min_score, const int32_t* thresholds,
                               int64_t max_rows_hint, int64_t* hoffsets, moc_result* rows, int64_t cap) {
  return guard([&] {
    if (cap < 0 || (cap > 0 && !rows)) throw moc::Error("hits: cap rows need a rows buffer");
    static_cast<moc::HipEngine*>(e)->solve_hits_wire(wire_batch(w), min_score, thresholds, hoffsets, g_hits_rows,
                                                     max_rows_hint);
    const size_t m = std::min(g_hits_rows.size(), static_cast<size_t>(cap));
    if (m) std::memcpy(rows, g_hits_rows.data(), sizeof(moc::Result) * m);
  });
}

int moc_engine_report_wire(void* e, const moc_wire_batch* w, int K, const moc_result* rows, int32_t* counts,
                           uint8_t* marks) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->report_wire(wire_batch(w), K, reinterpret_cast<const moc::Result*>(rows), counts, marks);
  });
}

// ---- distinct placements: the calls above over the peaks of a radius
int moc_peaks_max_radius(void) { return moc::bounds::kPeaksMaxRadius; }

int moc_peaks_geometry(int32_t* out3) {
  out3[0] = moc::bounds::kPeaksMaxRadius;
  out3[1] = moc::bounds::kPeaksWaveEntries;
  out3[2] = moc::bounds::kPeaksTile;
  return 0;
}

int moc_cpu_topk_distinct(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                          const int64_t* offsets, int64_t n, int semantics, int threads, int K, int64_t radius,
                          moc_result* out) {
  return guard([&] {
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::topk_batch_cpu(t, seq1, L1, b, K, reinterpret_cast<moc::Result*>(out), static_cast<moc::Semantics>(semantics),
                        threads, radius);
  });
}

int moc_cpu_hits_distinct(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                          const int64_t* offsets, int64_t n, int semantics, int threads, int32_t min_score,
                          const int32_t* thresholds, int64_t radius, int64_t* hoffsets, moc_result* rows, int64_t cap) {
  return guard([&] {
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::hits_batch_cpu(t, seq1, L1, b, min_score, thresholds, hoffsets, reinterpret_cast<moc::Result*>(rows), cap,
                        static_cast<moc::Semantics>(semantics), threads, radius);
  });
}

int moc_engine_solve_topk_distinct(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int K,
                                   int64_t radius, moc_result* out) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_topk(codes, offsets, n, K, reinterpret_cast<moc::Result*>(out), radius);
  });
}

int moc_engine_solve_topk_device_distinct(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                          const int64_t* h_offsets, int64_t n, int K, int64_t radius, moc_result* d_out,
                                          void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_topk_device(d_codes, d_offsets, h_offsets, n, K,
                                                       reinterpret_cast<moc::Result*>(d_out),
                                                       static_cast<hipStream_t>(stream), radius);
  });
}

int moc_engine_solve_topk_wire_distinct(void* e, const moc_wire_batch* w, int K, int64_t radius, moc_result* out) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_topk_wire(wire_batch(w), K, reinterpret_cast<moc::Result*>(out), radius);
  });
}

int moc_engine_solve_hits_distinct(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int32_t min_score,
                                   const int32_t* thresholds, int64_t radius, int64_t max_rows_hint, int64_t* hoffsets,
                                   moc_result* rows, int64_t cap) {
  return guard([&] {
    if (cap < 0 || (cap > 0 && !rows)) throw moc::Error("hits: cap rows need a rows buffer");
    static_cast<moc::HipEngine*>(e)->solve_hits(codes, offsets, n, min_score, thresholds, hoffsets, g_hits_rows,
                                                max_rows_hint, radius);
    const size_t m = std::min(g_hits_rows.size(), static_cast<size_t>(cap));
    if (m) std::memcpy(rows, g_hits_rows.data(), sizeof(moc::Result) * m);
  });
}

int moc_engine_solve_hits_device_distinct(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                          const int64_t* h_offsets, int64_t n, int32_t min_score,
                                          const int32_t* d_thresholds, int64_t radius, int64_t* d_hoffsets,
                                          moc_result* d_rows, int64_t cap, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_hits_device(d_codes, d_offsets, h_offsets, n, min_score, d_thresholds,
                                                       d_hoffsets, reinterpret_cast<moc::Result*>(d_rows), cap,
                                                       static_cast<hipStream_t>(stream), radius);
  });
}

int moc_engine_solve_hits_wire_distinct(void* e, const moc_wire_batch* w, int32_t min_score, const int32_t* thresholds,
                                        int64_t radius, int64_t max_rows_hint, int64_t* hoffsets, moc_result* rows,
                                        int64_t cap) {
  return guard([&] {
    if (cap < 0 || (cap > 0 && !rows)) throw moc::Error("hits: cap rows need a rows buffer");
    static_cast<moc::HipEngine*>(e)->solve_hits_wire(wire_batch(w), min_score, thresholds, hoffsets, g_hits_rows,
                                                     max_rows_hint, radius);
    const size_t m = std::min(g_hits_rows.size(), static_cast<size_t>(cap));
    if (m) std::memcpy(rows, g_hits_rows.data(), sizeof(moc::Result) * m);
  });
}

// ---- profile summary
int moc_summary_geometry(int32_t* out3) {
  out3[0] = moc::bounds::kSummaryRecordsPerBlock;
  out3[1] = moc::bounds::kSummaryThreads;
  out3[2] = moc::bounds::kSummaryMaxBins;
  return 0;
}

int64_t moc_summary_bound(int32_t max_abs_weight, int64_t max_l2) {
  return moc::bounds::summary_max_count(max_abs_weight, max_l2);
}

int moc_cpu_summary(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                    const int64_t* offsets, int64_t n, int semantics, int threads, int32_t bins, int32_t lo,
                    int32_t width, int64_t* summary, int32_t* hist) {
  return guard([&] {
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::summary_batch_cpu(t, seq1, L1, b, summary, hist, bins, lo, width, static_cast<moc::Semantics>(semantics),
                           threads);
  });
}

int moc_engine_solve_summary(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, int32_t bins, int32_t lo,
                             int32_t width, int64_t* summary, int32_t* hist) {
  return guard([&] { static_cast<moc::HipEngine*>(e)->solve_summary(codes, offsets, n, summary, hist, bins, lo, width); });
}

int moc_engine_solve_summary_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, int32_t bins, int32_t lo, int32_t width, int64_t* d_summary,
                                    int32_t* d_hist, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_summary_device(d_codes, d_offsets, h_offsets, n, d_summary, d_hist, bins, lo,
                                                          width, static_cast<hipStream_t>(stream));
  });
}

int moc_engine_solve_summary_wire(void* e, const moc_wire_batch* w, int32_t bins, int32_t lo, int32_t width,
                                  int64_t* summary, int32_t* hist) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_summary_wire(wire_batch(w), summary, hist, bins, lo, width);
  });
}

int moc_engine_summary_ms(void* e, double* ms) {
  return guard([&] { *ms = static_cast<moc::HipEngine*>(e)->summary_ms(); });
}

// ---- multi-target search
int moc_targets_geometry(int32_t* out4) {
  out4[0] = moc::bounds::kTargetsMax;
  out4[1] = moc::bounds::kTargetsThreads;
  out4[2] = static_cast<int32_t>(moc::bounds::kTargetsGroup4MaxSlice);
  out4[3] = static_cast<int32_t>(moc::bounds::kTargetsGroup16MaxSlice);
  return 0;
}

int moc_check_targets(const int64_t* starts, int64_t T, int64_t L1) {
  return guard([&] { moc::check_targets(starts, T, L1); });
}

int moc_cpu_targets(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                    const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics, int threads,
                    moc_result* rows) {
  return guard([&] {
    moc::check_targets(starts, T, L1);
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::targets_batch_cpu(t, seq1, L1, b, starts, T, reinterpret_cast<moc::Result*>(rows),
                           static_cast<moc::Semantics>(semantics), threads);
  });
}

int moc_engine_solve_targets(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts,
                             int64_t T, moc_result* rows) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets(codes, offsets, n, starts, T, reinterpret_cast<moc::Result*>(rows));
  });
}

int moc_engine_solve_targets_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets,
                                    int64_t n, const int64_t* d_starts, const int64_t* h_starts, int64_t T,
                                    moc_result* d_rows, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_device(d_codes, d_offsets, h_offsets, n, d_starts, h_starts, T,
                                                          reinterpret_cast<moc::Result*>(d_rows),
                                                          static_cast<hipStream_t>(stream));
  });
}

int moc_engine_solve_targets_wire(void* e, const moc_wire_batch* w, const int64_t* starts, int64_t T, moc_result* rows) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_wire(wire_batch(w), starts, T, reinterpret_cast<moc::Result*>(rows));
  });
}

int moc_engine_targets_ms(void* e, double* ms) {
  return guard([&] { *ms = static_cast<moc::HipEngine*>(e)->targets_ms(); });
}

// ---- target ranking
int moc_targets_rank_geometry(int32_t* out3) {
  out3[0] = static_cast<int32_t>(moc::bounds::kTargetsRankRecordBytes);
  out3[1] = static_cast<int32_t>(moc::bounds::kTargetsRankGroup4MaxT);
  out3[2] = static_cast<int32_t>(moc::bounds::kTargetsRankGroup16MaxT);
  return 0;
}

int moc_cpu_targets_rank(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                         const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics, int threads,
                         int M, moc_rank_row* rows) {
  return guard([&] {
    moc::check_targets(starts, T, L1);
    moc::check_targets_rank(M);
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::targets_rank_batch_cpu(t, seq1, L1, b, starts, T, M, reinterpret_cast<moc::RankRow*>(rows),
                                static_cast<moc::Semantics>(semantics), threads);
  });
}

int64_t moc_targets_rank_chunks(int64_t L1, const int64_t* offsets, int64_t n, int64_t T, int64_t scratch_bytes,
                                int semantics, int64_t* bounds_out) {
  int64_t chunks = -1;
  guard([&] {
    if (n < 0 || L1 < 1) throw moc::Error("rank chunks: negative size");
    if (T < 0 || T > moc::bounds::kTargetsMax)
      throw moc::Error("rank chunks: T must be in 0.." + std::to_string(moc::bounds::kTargetsMax));
    if (scratch_bytes < static_cast<int64_t>(sizeof(moc::ProfileEntry)))
      throw moc::Error("profile scratch: at least one entry (8 bytes)");
    for (int64_t i = 0; i < n; ++i)
      if (offsets[i + 1] < offsets[i]) throw moc::Error("rank chunks: offsets must not decrease");
    bounds_out[0] = 0;
    chunks = 0;
    if (n == 0) return;
    moc::plan::Config c;  // the cut reads L1 alone; the runs' geometry (CUs, tuning) does not move it
    c.L1 = L1;
    const moc::plan::ProfilePlan pp =
        moc::plan::plan_profile(c, static_cast<moc::Semantics>(semantics), offsets, n, true, sizeof(moc::ProfileEntry),
                                scratch_bytes, 0, nullptr, 0, false, 0, moc::bounds::kTargetsRankRecordBytes * T);
    for (const moc::plan::ProfileChunk& k : pp.chunks) bounds_out[++chunks] = k.r1;
  });
  return chunks;
}

int moc_engine_solve_targets_rank(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts,
                                  int64_t T, int M, moc_rank_row* rows) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_rank(codes, offsets, n, starts, T, M,
                                                        reinterpret_cast<moc::RankRow*>(rows));
  });
}

int moc_engine_solve_targets_rank_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                         const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                         const int64_t* h_starts, int64_t T, int M, moc_rank_row* d_rows, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_rank_device(d_codes, d_offsets, h_offsets, n, d_starts, h_starts, T, M,
                                                               reinterpret_cast<moc::RankRow*>(d_rows),
                                                               static_cast<hipStream_t>(stream));
  });
}

int moc_engine_solve_targets_rank_wire(void* e, const moc_wire_batch* w, const int64_t* starts, int64_t T, int M,
                                       moc_rank_row* rows) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_rank_wire(wire_batch(w), starts, T, M,
                                                             reinterpret_cast<moc::RankRow*>(rows));
  });
}

// ---- per-target profile summary
int moc_targets_summary_geometry(int32_t* out4) {
  out4[0] = moc::bounds::kTargetsThreads;
  out4[1] = moc::bounds::kSummaryMaxBins;
  out4[2] = moc::bounds::kTargetsHistGroup4MaxBins;
  out4[3] = moc::bounds::kTargetsHistLdsBytes;
  return 0;
}

int moc_cpu_targets_summary(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                            const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics,
                            int threads, int32_t bins, int32_t lo, int32_t width, int64_t* summary, int32_t* hist) {
  return guard([&] {
    moc::check_targets(starts, T, L1);
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::targets_summary_batch_cpu(t, seq1, L1, b, starts, T, summary, hist, bins, lo, width,
                                   static_cast<moc::Semantics>(semantics), threads);
  });
}

int moc_engine_solve_targets_summary(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n,
                                     const int64_t* starts, int64_t T, int32_t bins, int32_t lo, int32_t width,
                                     int64_t* summary, int32_t* hist) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_summary(codes, offsets, n, starts, T, summary, hist, bins, lo, width);
  });
}

int moc_engine_solve_targets_summary_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                            const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                            const int64_t* h_starts, int64_t T, int32_t bins, int32_t lo, int32_t width,
                                            int64_t* d_summary, int32_t* d_hist, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_summary_device(d_codes, d_offsets, h_offsets, n, d_starts, h_starts, T,
                                                                  d_summary, d_hist, bins, lo, width,
                                                                  static_cast<hipStream_t>(stream));
  });
}

int moc_engine_solve_targets_summary_wire(void* e, const moc_wire_batch* w, const int64_t* starts, int64_t T,
                                          int32_t bins, int32_t lo, int32_t width, int64_t* summary, int32_t* hist) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_summary_wire(wire_batch(w), starts, T, summary, hist, bins, lo, width);
  });
}

int moc_engine_targets_summary_ms(void* e, double* ms) {
  return guard([&] { *ms = static_cast<moc::HipEngine*>(e)->targets_summary_ms(); });
}

// ---- per-target top-K and threshold hits; the *_distinct forms carry the peaks radius, the frozen ones are radius 0
int moc_cpu_targets_topk_distinct(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                                  const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics,
                                  int threads, int K, int64_t radius, moc_result* rows) {
  return guard([&] {
    moc::check_targets(starts, T, L1);
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::targets_topk_batch_cpu(t, seq1, L1, b, starts, T, K, reinterpret_cast<moc::Result*>(rows),
                                static_cast<moc::Semantics>(semantics), threads, radius);
  });
}

int moc_cpu_targets_topk(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                         const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics, int threads,
                         int K, moc_result* rows) {
  return moc_cpu_targets_topk_distinct(weights4, seq1, L1, codes, offsets, n, starts, T, semantics, threads, K, 0, rows);
}

int moc_cpu_targets_hits_distinct(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                                  const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics,
                                  int threads, int32_t min_score, const int32_t* thresholds, int64_t radius,
                                  int64_t* toffsets, moc_result* rows, int64_t cap) {
  return guard([&] {
    moc::check_targets(starts, T, L1);
    moc::Weights w = weights_of(weights4);
    moc::RecordBatch b = view_batch(codes, offsets, n);
    moc::validate_score_range(w, std::max<int64_t>(b.max_length(), 1));
    moc::ScoreTable t = moc::ScoreTable::build(w);
    moc::targets_hits_batch_cpu(t, seq1, L1, b, starts, T, min_score, thresholds, toffsets,
                                reinterpret_cast<moc::Result*>(rows), cap, static_cast<moc::Semantics>(semantics), threads,
                                radius);
  });
}

int moc_cpu_targets_hits(const int32_t* weights4, const uint8_t* seq1, int64_t L1, const uint8_t* codes,
                         const int64_t* offsets, int64_t n, const int64_t* starts, int64_t T, int semantics, int threads,
                         int32_t min_score, const int32_t* thresholds, int64_t* toffsets, moc_result* rows, int64_t cap) {
  return moc_cpu_targets_hits_distinct(weights4, seq1, L1, codes, offsets, n, starts, T, semantics, threads, min_score,
                                       thresholds, 0, toffsets, rows, cap);
}

int moc_engine_solve_targets_topk_distinct(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n,
                                           const int64_t* starts, int64_t T, int K, int64_t radius, moc_result* rows) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_topk(codes, offsets, n, starts, T, K, reinterpret_cast<moc::Result*>(rows),
                                                        radius);
  });
}

int moc_engine_solve_targets_topk(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts,
                                  int64_t T, int K, moc_result* rows) {
  return moc_engine_solve_targets_topk_distinct(e, codes, offsets, n, starts, T, K, 0, rows);
}

int moc_engine_solve_targets_topk_device_distinct(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                                  const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                                  const int64_t* h_starts, int64_t T, int K, int64_t radius,
                                                  moc_result* d_rows, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_topk_device(d_codes, d_offsets, h_offsets, n, d_starts, h_starts, T, K,
                                                               reinterpret_cast<moc::Result*>(d_rows),
                                                               static_cast<hipStream_t>(stream), radius);
  });
}

int moc_engine_solve_targets_topk_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                         const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                         const int64_t* h_starts, int64_t T, int K, moc_result* d_rows, void* stream) {
  return moc_engine_solve_targets_topk_device_distinct(e, d_codes, d_offsets, h_offsets, n, d_starts, h_starts, T, K, 0,
                                                       d_rows, stream);
}

int moc_engine_solve_targets_topk_wire_distinct(void* e, const moc_wire_batch* w, const int64_t* starts, int64_t T, int K,
                                                int64_t radius, moc_result* rows) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_topk_wire(wire_batch(w), starts, T, K, reinterpret_cast<moc::Result*>(rows),
                                                             radius);
  });
}

int moc_engine_solve_targets_topk_wire(void* e, const moc_wire_batch* w, const int64_t* starts, int64_t T, int K,
                                       moc_result* rows) {
  return moc_engine_solve_targets_topk_wire_distinct(e, w, starts, T, K, 0, rows);
}

int moc_engine_solve_targets_hits_distinct(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n,
                                           const int64_t* starts, int64_t T, int32_t min_score, const int32_t* thresholds,
                                           int64_t max_rows_hint, int64_t radius, int64_t* toffsets, moc_result* rows,
                                           int64_t cap) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->check_targets_call(starts, T);  // the target set's errors come first
    if (cap < 0 || (cap > 0 && !rows)) throw moc::Error("hits: cap rows need a rows buffer");
    static_cast<moc::HipEngine*>(e)->solve_targets_hits(codes, offsets, n, starts, T, min_score, thresholds, toffsets,
                                                        g_hits_rows, max_rows_hint, radius);
    const size_t m = std::min(g_hits_rows.size(), static_cast<size_t>(cap));
    if (m) std::memcpy(rows, g_hits_rows.data(), sizeof(moc::Result) * m);
  });
}

int moc_engine_solve_targets_hits(void* e, const uint8_t* codes, const int64_t* offsets, int64_t n, const int64_t* starts,
                                  int64_t T, int32_t min_score, const int32_t* thresholds, int64_t max_rows_hint,
                                  int64_t* toffsets, moc_result* rows, int64_t cap) {
  return moc_engine_solve_targets_hits_distinct(e, codes, offsets, n, starts, T, min_score, thresholds, max_rows_hint, 0,
                                                toffsets, rows, cap);
}

int moc_engine_solve_targets_hits_device_distinct(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                                  const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                                  const int64_t* h_starts, int64_t T, int32_t min_score,
                                                  const int32_t* d_thresholds, int64_t radius, int64_t* d_toffsets,
                                                  moc_result* d_rows, int64_t cap, void* stream) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->solve_targets_hits_device(d_codes, d_offsets, h_offsets, n, d_starts, h_starts, T,
                                                               min_score, d_thresholds, d_toffsets,
                                                               reinterpret_cast<moc::Result*>(d_rows), cap,
                                                               static_cast<hipStream_t>(stream), radius);
  });
}

int moc_engine_solve_targets_hits_device(void* e, const uint8_t* d_codes, const int64_t* d_offsets,
                                         const int64_t* h_offsets, int64_t n, const int64_t* d_starts,
                                         const int64_t* h_starts, int64_t T, int32_t min_score,
                                         const int32_t* d_thresholds, int64_t* d_toffsets, moc_result* d_rows, int64_t cap,
                                         void* stream) {
  return moc_engine_solve_targets_hits_device_distinct(e, d_codes, d_offsets, h_offsets, n, d_starts, h_starts, T, min_score,
                                                       d_thresholds, 0, d_toffsets, d_rows, cap, stream);
}

int moc_engine_solve_targets_hits_wire_distinct(void* e, const moc_wire_batch* w, const int64_t* starts, int64_t T,
                                                int32_t min_score, const int32_t* thresholds, int64_t max_rows_hint,
                                                int64_t radius, int64_t* toffsets, moc_result* rows, int64_t cap) {
  return guard([&] {
    static_cast<moc::HipEngine*>(e)->check_targets_call(starts, T);  // the target set's errors come first
    if (cap < 0 || (cap > 0 && !rows)) throw moc::Error("hits: cap rows need a rows buffer");
    static_cast<moc::HipEngine*>(e)->solve_targets_hits_wire(wire_batch(w), starts, T, min_score, thresholds, toffsets,
                                                             g_hits_rows, max_rows_hint, radius);
    const size_t m = std::min(g_hits_rows.size(), static_cast<size_t>(cap));
    if (m) std::memcpy(rows, g_hits_rows.data(), sizeof(moc::Result) * m);
  });
}

int moc_engine_solve_targets_hits_wire(void* e, const moc_wire_batch* w, const int64_t* starts, int64_t T,
                                       int32_t min_score, const int32_t* thresholds, int64_t max_rows_hint,
                                       int64_t* toffsets, moc_result* rows, int64_t cap) {
  return moc_engine_solve_targets_hits_wire_distinct(e, w, starts, T, min_score, thresholds, max_rows_hint, 0, toffsets,
                                                     rows, cap);
}

int moc_engine_stats(void* e, double* out14) {
  return guard([&] {
    double* out13 = out14;
    double* out10 = out14;
    out14[13] = static_cast<double>(static_cast<moc::HipEngine*>(e)->stats().forms);
    const auto& s = static_cast<moc::HipEngine*>(e)->stats();
    out13[10] = s.r2.smin;
    out13[11] = s.r2.kw;
    out13[12] = s.r2.j;
    out10[0] = s.kernel_ms;
    out10[1] = s.total_ms;
    out10[2] = static_cast<double>(s.h2d_bytes);
    out10[3] = static_cast<double>(s.d2h_bytes);
    out10[4] = static_cast<double>(s.chunks);
    out10[5] = static_cast<double>(s.cells);
    out10[6] = static_cast<double>(s.records);
    out10[7] = static_cast<double>(s.direct);
    out10[8] = static_cast<double>(s.format);
    out10[9] = static_cast<double>(s.kernels);
  });
}

int moc_expand_results(const void* in, int fmt, int64_t n, const int32_t* r2_3, moc_result* out) {
  return guard([&] {
    moc::R2Params p;
    if (r2_3) {
      p.smin = r2_3[0];
      p.kw = r2_3[1];
      p.j = r2_3[2];
    }
    moc::expand_results(in, static_cast<moc::ResultFormat>(fmt), n, reinterpret_cast<moc::Result*>(out),
                        r2_3 ? &p : nullptr);
  });
}

}  // extern "C"
