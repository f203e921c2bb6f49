// Alignment report (gfx950, wave64): the four sign counts ($ % # space) and, optionally, the marker bytes under
// the letter pairs of caller-supplied result rows {score, n, k}. Definitions: moc/cpu_engine.hpp
// (report_batch_cpu is the oracle; the outputs here are equal to its, byte for byte).
//
// Every row is bounds-checked before its n or k forms an address (row_valid, 64-bit): rows come from the caller
// and a device buffer may hold anything. An invalid row gets counts -1 and marker bytes 0, an empty row
// (score == INT32_MIN, top-K padding) counts 0 and marker bytes 0; neither reads Seq1.
//
// The kernel is bound by bytes, not arithmetic (~45 B per input6-shaped record), so there are two regimes,
// split on the host (plan::plan_report) at bounds::kReportShortMaxL2 letters:
//   * alignment_report_kernel — one LANE per row. A wave takes up to 64 / K consecutive short records (whole
//     records: the K rows of a record share its letters, loaded from memory once). Its records' letters are one
//     contiguous span of the batch, staged into a wave-private LDS region with 16-byte loads of the aligned
//     interior and byte loads of the unaligned head and tail (never a byte outside the span). Each lane then
//     walks its own letters out of LDS against Seq1 (LDS when it fits, device memory beyond) and the 32x32
//     class table (LDS, expanded once per block from the 256-byte kernel argument). The four counters are the
//     bytes of one register (counts <= L2 <= 64: bounds::kReportPackedCountMax) and leave as one 16-byte store
//     per row. Marker bytes are written to a second wave-private LDS region laid out like their destination —
//     the wave's rows are one contiguous range of the marker buffer — and stored with the same head / 16-byte
//     interior / tail scheme. Persistent blocks stride over groups of four wave items.
//   * alignment_report_long_kernel — one WAVE per row. Lanes stride the letters 64 at a time (coalesced byte
//     loads of the record and of Seq1, coalesced marker stores), keep int32 counters and reduce them across the
//     wave once at the end. No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernel_common.hpp"
#include "moc/runtime/hip_check.hpp"

namespace moc {
namespace dev {

using namespace kc;

namespace {
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kShortMax = static_cast<int>(bounds::kReportShortMaxL2);
constexpr int kSpanMax = kWave * kShortMax;  // letters (and marker bytes) of one wave item
constexpr int kSpanCap = kSpanMax + 32;      // + the alignment head (< 16) and the last chunk's slack
constexpr int kClsBytes = kLutStride * kLutStride;
// Seq1 staged in LDS up to this size: with the class table and eight span regions the block stays < 64 KiB
constexpr int kMaxSeq1Lds = 24 * 1024;
static_assert(kSpanCap % 16 == 0, "wave regions keep the 16-byte LDS alignment");
static_assert(kClsBytes + 2 * kWavesPerBlock * kSpanCap + kMaxSeq1Lds + 4 <= 64 * 1024, "dynamic LDS below 64 KiB");
constexpr uint32_t kClassChars = 0x20232524u;  // '$' '%' '#' ' ' by PairClass, low byte first
}  // namespace

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ void expand_classes(uint8_t* cls, const ReportClassBits& cb) {
  for (int e = threadIdx.x; e < kClsBytes; e += blockDim.x)
    cls[e] = static_cast<uint8_t>((cb.w[e >> 4] >> (2 * (e & 15))) & 3u);
}

// moc::report_row_valid: 64-bit, so n + L2 cannot wrap
__device__ __forceinline__ bool row_valid(int L1, int L2, int n, int k) {
  return L2 >= 1 && L2 <= L1 && k >= 0 && k <= L2 - 1 && n >= 0 &&
         static_cast<int64_t>(n) + L2 + (k > 0 ? 1 : 0) <= static_cast<int64_t>(L1);
}

// `len` bytes between global memory `g` and the LDS region `l`, where LDS byte (g & 15) + q stands for g[q]:
// whole 16-byte chunks move as one aligned vector access on both sides, the partial first and last chunk byte
// by byte. One wave; lane c takes chunks c, c + 64, ...
template <bool ToLds>
__device__ __forceinline__ void span_copy(uint8_t* g, uint8_t* l, int len, int lane) {
  const int head = static_cast<int>(reinterpret_cast<uintptr_t>(g) & 15);
  const int nch = len > 0 ? (head + len + 15) >> 4 : 0;
  MOC_DCHECK(16 * nch <= kSpanCap);
  for (int c = lane; c < nch; c += kWave) {
    const int b0 = 16 * c - head;  // the chunk's first byte, relative to g
    if (b0 >= 0 && b0 + 16 <= len) {
      if (ToLds)
        *reinterpret_cast<uint4*>(l + 16 * c) = *reinterpret_cast<const uint4*>(g + b0);
      else
        *reinterpret_cast<uint4*>(g + b0) = *reinterpret_cast<const uint4*>(l + 16 * c);
    } else {
      const int qe = min(b0 + 16, len);
      for (int q = max(b0, 0); q < qe; ++q) {
        if (ToLds)
          l[head + q] = g[q];
        else
          g[q] = l[head + q];
      }
    }
  }
}

template <bool Seq1Lds, bool Marks>
__global__ __launch_bounds__(kBlock) void alignment_report_kernel(ProblemView pv, BatchView bv, ReportClassBits cb,
                                                                  ReportArgs ra) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  uint8_t* cls = smem;
  uint8_t* let = smem + kClsBytes + wave * kSpanCap;
  uint8_t* mk = smem + kClsBytes + (kWavesPerBlock + wave) * kSpanCap;  // Marks only
  uint8_t* s1l = smem + kClsBytes + (Marks ? 2 : 1) * kWavesPerBlock * kSpanCap;
  const int L1 = pv.L1;
  expand_classes(cls, cb);
  if (Seq1Lds) stage_bytes(s1l, pv.seq1, L1 + kSeq1Pad);
  const uint8_t* s1 = Seq1Lds ? s1l : pv.seq1;  // the loop's first barrier orders the staging above, too

  const int K = ra.K, rpw = kWave / K;
  const int li = lane / K, j = lane - li * K;
  const int64_t base = bv.offsets[0];
  const int64_t n_groups = (ra.n_items + kWavesPerBlock - 1) / kWavesPerBlock;
  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {  // block-uniform: every wave meets every barrier
    const int64_t w = g * kWavesPerBlock + wave;
    int64_t r0 = 0;
    int cnt = 0;
    if (w < ra.n_items) {
      if (ra.items) {
        const ReportItem it = ra.items[w];
        r0 = it.r0;
        cnt = it.cnt;
      } else {
        r0 = w * rpw;
        cnt = bv.n - r0 < rpw ? static_cast<int>(bv.n - r0) : rpw;
      }
    }
    cnt = __builtin_amdgcn_readfirstlane(cnt);
    MOC_DCHECK(cnt >= 0 && cnt * K <= kWave && r0 >= 0 && r0 + cnt <= bv.n);
    // ---- the item's letters: one contiguous span of the batch -> LDS
    int64_t a = 0;
    int len = 0;
    if (cnt > 0) {
      a = bv.offsets[r0] - base;
      len = static_cast<int>(bv.offsets[r0 + cnt] - bv.offsets[r0]);
    }
    MOC_DCHECK(len >= 0 && len <= kSpanMax && a >= 0);
    len = min(max(len, 0), kSpanMax);  // device offsets that disagree with the plan cannot leave the region
    uint8_t* src = const_cast<uint8_t*>(bv.codes) + a;
    const int head = static_cast<int>(reinterpret_cast<uintptr_t>(src) & 15);
    span_copy<true>(src, let, len, lane);
    uint8_t* mdst = nullptr;
    int mhead = 0;
    if (Marks) {
      mdst = ra.marks + static_cast<int64_t>(K) * a;  // rows of consecutive records are consecutive marker bytes
      mhead = static_cast<int>(reinterpret_cast<uintptr_t>(mdst) & 15);
      MOC_DCHECK(static_cast<int64_t>(K) * (a + len) <= ra.marks_bytes);
    }
    __syncthreads();
    // ---- one lane per row
    if (li < cnt) {
      const int64_t r = r0 + li;
      const int64_t o0 = bv.offsets[r], o1 = bv.offsets[r + 1];
      const int lo = static_cast<int>(o0 - base - a);
      const int L2 = static_cast<int>(o1 - o0);
      MOC_DCHECK(lo >= 0 && L2 >= 0 && L2 <= kShortMax && lo + L2 <= len);
      const int64_t q = r * K + j;
      const Result row = ra.rows[q];
      const bool empty = row.score == INT32_MIN;
      const bool valid = !empty && L2 <= kShortMax && lo >= 0 && lo + L2 <= len && row_valid(L1, L2, row.n, row.k);
      uint8_t* mrow = mk + mhead + K * lo + j * L2;
      int4 out = empty ? make_int4(0, 0, 0, 0) : make_int4(-1, -1, -1, -1);
      if (valid) {
        const uint8_t* my = let + head + lo;
        const int n = row.n, k = row.k;
        uint32_t packed = 0;  // four byte counters, PairClass order from the low byte
        for (int i = 0; i < L2; ++i) {
          const int at = n + i + ((k > 0 && i >= k) ? 1 : 0);
          MOC_DCHECK(at >= 0 && at < L1);
          const uint32_t cl = cls[((my[i] & 31) << 5) | (s1[at] & 31)];
          packed += 1u << (8 * cl);
          if (Marks) {
            MOC_DCHECK(mhead + K * lo + j * L2 + i < kSpanCap);
            mrow[i] = static_cast<uint8_t>(kClassChars >> (8 * cl));
          }
        }
        out = make_int4(packed & 255u, (packed >> 8) & 255u, (packed >> 16) & 255u, packed >> 24);
      } else if (Marks && lo >= 0 && L2 <= kShortMax && lo + L2 <= len) {
        for (int i = 0; i < L2; ++i) mrow[i] = 0;
      }
      MOC_DCHECK(q >= 0 && q < bv.n * K);
      *reinterpret_cast<int4*>(ra.counts + 4 * q) = out;
    }
    if (Marks) {
      __syncthreads();
      span_copy<false>(mdst, mk, min(K * len, kSpanMax), lane);
    }
  }
}

template <bool Marks>
__global__ __launch_bounds__(kBlock) void alignment_report_long_kernel(ProblemView pv, BatchView bv, ReportClassBits cb,
                                                                       ReportArgs ra) {
  __shared__ uint8_t cls[kClsBytes];
  expand_classes(cls, cb);
  __syncthreads();
  const int K = ra.K;
  const int64_t w = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= ra.n_long * K) return;  // wave-uniform; no barrier follows
  const int lane = threadIdx.x & 63;
  const int64_t li = w / K;
  const int j = static_cast<int>(w - li * K);
  const int64_t r = ra.long_recs[li];
  MOC_DCHECK(r >= 0 && r < bv.n);
  const int64_t base = bv.offsets[0], o0 = bv.offsets[r], o1 = bv.offsets[r + 1];
  const int L1 = pv.L1;
  const int L2 = __builtin_amdgcn_readfirstlane(static_cast<int>(o1 - o0));
  const uint8_t* rec = bv.codes + (o0 - base);
  const int64_t q = r * K + j;
  MOC_DCHECK(q >= 0 && q < bv.n * K);
  const Result row = ra.rows[q];
  const int score = __builtin_amdgcn_readfirstlane(row.score);
  const int n = __builtin_amdgcn_readfirstlane(row.n), k = __builtin_amdgcn_readfirstlane(row.k);
  const bool empty = score == INT32_MIN;
  const bool valid = !empty && row_valid(L1, L2, n, k);
  uint8_t* m = Marks ? ra.marks + static_cast<int64_t>(K) * (o0 - base) + static_cast<int64_t>(j) * L2 : nullptr;
  MOC_DCHECK(!Marks || static_cast<int64_t>(K) * (o0 - base) + static_cast<int64_t>(j + 1) * L2 <= ra.marks_bytes);
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  if (valid) {
    for (int i = lane; i < L2; i += kWave) {
      const int at = n + i + ((k > 0 && i >= k) ? 1 : 0);
      MOC_DCHECK(at >= 0 && at < L1);
      const int cl = cls[((rec[i] & 31) << 5) | (pv.seq1[at] & 31)];
      c0 += cl == 0;
      c1 += cl == 1;
      c2 += cl == 2;
      c3 += cl == 3;
      if (Marks) m[i] = static_cast<uint8_t>(kClassChars >> (8 * cl));
    }
    c0 = wave_sum_i32(c0);
    c1 = wave_sum_i32(c1);
    c2 = wave_sum_i32(c2);
    c3 = wave_sum_i32(c3);
  } else {
    c0 = c1 = c2 = c3 = empty ? 0 : -1;
    if (Marks)
      for (int i = lane; i < L2; i += kWave) m[i] = 0;
  }
  if (lane == 0) *reinterpret_cast<int4*>(ra.counts + 4 * q) = make_int4(c0, c1, c2, c3);
}

void preload_report_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&alignment_report_long_kernel<false>));
}

namespace {
template <bool Seq1Lds, bool Marks>
void launch_short(const ProblemView& pv, const BatchView& bv, const ReportClassBits& cb, const ReportArgs& ra,
                  hipStream_t stream) {
  const size_t lds = kClsBytes + static_cast<size_t>(Marks ? 2 : 1) * kWavesPerBlock * kSpanCap +
                     (Seq1Lds ? (static_cast<size_t>(pv.L1 + kSeq1Pad + 3) & ~size_t{3}) : 0);
  const int64_t groups = (ra.n_items + kWavesPerBlock - 1) / kWavesPerBlock;
  const int64_t blocks = std::min<int64_t>(groups, static_cast<int64_t>(ra.num_cus) * 8);
  hipLaunchKernelGGL((alignment_report_kernel<Seq1Lds, Marks>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), lds,
                     stream, pv, bv, cb, ra);
}
}  // namespace

void launch_alignment_report(const ProblemView& pv, const BatchView& bv, const ReportClassBits& cb, const ReportArgs& ra,
                             hipStream_t stream) {
  const bool marks = ra.marks != nullptr;
  if (ra.n_items > 0) {
    const bool s1lds = pv.L1 + kSeq1Pad <= kMaxSeq1Lds;
    if (s1lds)
      marks ? launch_short<true, true>(pv, bv, cb, ra, stream) : launch_short<true, false>(pv, bv, cb, ra, stream);
    else
      marks ? launch_short<false, true>(pv, bv, cb, ra, stream) : launch_short<false, false>(pv, bv, cb, ra, stream);
  }
  if (ra.n_long > 0) {
    const int64_t waves = ra.n_long * ra.K;
    const int64_t blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    if (marks)
      hipLaunchKernelGGL(alignment_report_long_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream,
                         pv, bv, cb, ra);
    else
      hipLaunchKernelGGL(alignment_report_long_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream,
                         pv, bv, cb, ra);
  }
}

}  // namespace dev
}  // namespace moc
