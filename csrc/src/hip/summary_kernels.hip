// Profile summary: per-record moments, extremes and a fixed-bin histogram of the per-offset score profile
// (gfx950, wave64). Definitions: moc/cpu_engine.hpp summary_batch_cpu; exactness bound: moc/kernel_bounds.hpp.
//
// The kernels read a chunk's profile where hits_count_kernel reads it (prof[poffsets[r] - base + o], written by
// offset_profile_kernel just before on the same stream) and reduce it to a few dozen bytes per record. No atomics
// on global memory, no kernel waits on another block; ordering is launch order:
//   profile_summary_kernel  one wave per record, 64 entries per pass: a lane keeps an int64 sum and sum of squares,
//                           an int32 minimum and the largest order-free key (topk_select_kernel's final_key, so the
//                           better() tie-break is top-K's); shuffle reductions; lane 0 stores the seven int64 values.
//   summary_hist_kernel     (bins > 0) one wave per record: the wave owns `bins` int32 counters in LDS, zeroes them,
//                           counts every entry with an LDS add and stores its row hist[r * bins ..). The two
//                           barriers are reached by every wave of the block, with or without a record.
#include <hip/hip_runtime.h>

#include "kernel_common.hpp"
#include "moc/kernel_bounds.hpp"
#include "moc/runtime/hip_check.hpp"

namespace moc {
namespace dev {

using namespace kc;

namespace {
constexpr int kBlock = bounds::kSummaryThreads;
constexpr int kWavesPerBlock = bounds::kSummaryRecordsPerBlock;
constexpr int kCols = 7;  // kSummaryCols: count, sum, sumsq, min, max, n, k
static_assert(kBlock == 64 * kWavesPerBlock, "summary: one wave per record");

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
}  // namespace

__global__ __launch_bounds__(256) void profile_summary_kernel(SummaryArgs sa) {
  const int64_t li = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (li >= sa.view.n_rec) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int64_t r = sa.view.rec0 + li;
  const int64_t pb = chunk_first(sa.view, r);
  const int C = __builtin_amdgcn_readfirstlane(chunk_count(sa.view, r));  // C < 2^30
  long long sum = 0, sumsq = 0;
  int mn = INT32_MAX;
  unsigned long long key = 0ull;  // 0: no entry (a real key is never 0: o < 2^31)
  for (int o = lane; o < C; o += 64) {
    const long long s = sa.view.prof[pb + o].score;
    sum += s;
    sumsq += s * s;
    mn = min(mn, static_cast<int>(s));
    key = max_u64(key, final_key(static_cast<int>(s), static_cast<uint32_t>(o)));
  }
  // every lane reaches the shuffles (the loop above is the only divergent part)
  sum = wave_sum_i64(sum);
  sumsq = wave_sum_i64(sumsq);
  mn = wave_min_i32(mn);
  key = wave_max_u64(key);
  if (lane == 0) {
    long long mx = INT32_MIN, bn = 0, bk = 0;
    if (key != 0ull) {
      const int o = static_cast<int>(0xffffffffu - static_cast<uint32_t>(key));
      MOC_DCHECK(o >= 0 && o < C);
      const ProfileEntry e = sa.view.prof[pb + o];
      mx = e.score;
      bn = o;
      bk = e.k;
    }
    long long* row = reinterpret_cast<long long*>(sa.summary) + r * kCols;
    row[0] = C;
    row[1] = sum;
    row[2] = sumsq;
    row[3] = mn;
    row[4] = mx;
    row[5] = bn;
    row[6] = bk;
  }
}

__global__ __launch_bounds__(256) void summary_hist_kernel(SummaryArgs sa) {
  __shared__ int cnt[kWavesPerBlock][bounds::kSummaryMaxBins];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int64_t li = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + w;
  const bool active = li < sa.view.n_rec;  // wave-uniform; an idle wave still reaches both barriers
  const int bins = sa.bins;
  MOC_DCHECK(bins >= 1 && bins <= bounds::kSummaryMaxBins);
  for (int b = lane; b < bins; b += 64) cnt[w][b] = 0;
  __syncthreads();
  const int64_t r = sa.view.rec0 + li;
  if (active) {
    const int64_t pb = chunk_first(sa.view, r);
    const int C = chunk_count(sa.view, r);
    for (int o = lane; o < C; o += 64) {
      const int b = summary_bin_dev(sa.view.prof[pb + o].score, sa.lo, sa.width, bins);
      MOC_DCHECK(b >= 0 && b < bins);
      atomicAdd(&cnt[w][b], 1);  // LDS add: 64 lanes on one bin serialise and stay exact
    }
  }
  __syncthreads();
  if (active) {
    int32_t* row = sa.hist + r * bins;
    for (int b = lane; b < bins; b += 64) row[b] = cnt[w][b];
  }
}

void preload_summary_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&profile_summary_kernel));
}

void launch_summary(const SummaryArgs& sa, hipStream_t stream) {
  if (sa.view.n_rec <= 0) return;
  const unsigned wave_blocks = static_cast<unsigned>((sa.view.n_rec + kWavesPerBlock - 1) / kWavesPerBlock);
  hipLaunchKernelGGL(profile_summary_kernel, dim3(wave_blocks), dim3(kBlock), 0, stream, sa);
  if (sa.bins > 0 && sa.hist) hipLaunchKernelGGL(summary_hist_kernel, dim3(wave_blocks), dim3(kBlock), 0, stream, sa);
}

}  // namespace dev
}  // namespace moc
