// Threshold hits: every offset of a record whose profile score is at least the record's threshold, as compact
// Result rows in ascending offset order (gfx950, wave64). Definitions: moc/cpu_engine.hpp hits_batch_cpu.
//
// The kernels read a chunk's profile where topk_select_kernel reads it (prof[poffsets[r] - base + o], written by
// offset_profile_kernel just before on the same stream) and turn it into variable-length output by stream
// compaction in separate launches — no kernel waits on another block, no atomics; ordering is launch order:
//   hits_count_kernel    one wave per record, 64 entries per pass: ballot + popcount -> hoffsets[r + 1]
//   hits_block_sums / hits_scan_sums / hits_rescan_kernel
//                        int64 prefix sum over the chunk's counts on top of hoffsets[rec0] (reduce, scan of the
//                        block sums by ONE block, rescan; geometry: moc/kernel_bounds.hpp). A chunk of at most
//                        kHitsScanBlockRecords records is the rescan alone.
//   hits_compact_kernel  one wave per record: ballot, the lane's rank among the set bits (v_mbcnt), a running
//                        wave-uniform base; a hit goes to rows[hoffsets[r] + base + rank] when that is < cap.
#include <hip/hip_runtime.h>

#include "kernel_common.hpp"
#include "moc/kernel_bounds.hpp"
#include "moc/runtime/hip_check.hpp"

namespace moc {
namespace dev {

using namespace kc;

namespace {
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
static_assert(bounds::kHitsScanThreads == kBlock, "hits scan: one thread geometry");
constexpr int kPerThread = bounds::kHitsScanBlockRecords / kBlock;  // 4 consecutive counts
constexpr int kSumsPerThread = bounds::kHitsScanSumsPerPass / kBlock;  // 2 consecutive sums

// Exclusive prefix of v over the block's 256 threads (thread order); total = the block's sum. ws: kWavesPerBlock
// int64 of LDS, reusable right after the call (the leading barrier ends the previous use).
__device__ __forceinline__ long long block_exclusive_sum(long long v, long long* ws, long long& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  __syncthreads();
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  long long before = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kWavesPerBlock; ++i) {
    const long long s = ws[i];
    before += i < w ? s : 0;
    total += s;
  }
  return before + inc - v;
}
}  // namespace

__global__ __launch_bounds__(256) void hits_count_kernel(HitsArgs ha) {
  const int64_t li = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (li >= ha.view.n_rec) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int64_t r = ha.view.rec0 + li;
  const int64_t pb = chunk_first(ha.view, r);
  const int C = __builtin_amdgcn_readfirstlane(chunk_count(ha.view, r));
  const int t = ha.thresholds ? ha.thresholds[r] : ha.min_score;
  int count = 0;  // C < 2^30
  for (int o0 = 0; o0 < C; o0 += 64) {  // wave-uniform: every lane reaches the ballot
    const int o = o0 + lane;
    bool hit = false;
    if (o < C) {
      hit = ha.view.prof[pb + o].score >= t;
    }
    count += __popcll(__builtin_amdgcn_ballot_w64(hit));
  }
  if (lane == 0) {
    ha.hoffsets[r + 1] = count;
    if (r == 0) ha.hoffsets[0] = 0;
  }
}

// sums[b] = the counts of records [b * kHitsScanBlockRecords, ...) of the chunk
__global__ __launch_bounds__(256) void hits_block_sums_kernel(HitsArgs ha) {
  __shared__ long long ws[kWavesPerBlock];
  const int64_t li0 = static_cast<int64_t>(blockIdx.x) * bounds::kHitsScanBlockRecords + threadIdx.x * kPerThread;
  const int64_t* cnt = ha.hoffsets + ha.view.rec0 + 1;
  long long v = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) v += li0 + q < ha.view.n_rec ? cnt[li0 + q] : 0;
  long long total;
  (void)block_exclusive_sum(v, ws, total);
  if (threadIdx.x == 0) ha.sums[blockIdx.x] = total;
}

// One block: sums[b] <- hoffsets[rec0] + sums[0] + ... + sums[b - 1], kHitsScanSumsPerPass sums per pass
__global__ __launch_bounds__(256) void hits_scan_sums_kernel(HitsArgs ha, int64_t n_sums) {
  __shared__ long long ws[kWavesPerBlock];
  long long carry = ha.hoffsets[ha.view.rec0];
  for (int64_t p0 = 0; p0 < n_sums; p0 += bounds::kHitsScanSumsPerPass) {  // block-uniform
    const int64_t i0 = p0 + threadIdx.x * kSumsPerThread;
    long long v[kSumsPerThread], mine = 0;
#pragma unroll
    for (int q = 0; q < kSumsPerThread; ++q) mine += v[q] = i0 + q < n_sums ? ha.sums[i0 + q] : 0;
    long long total;
    long long run = carry + block_exclusive_sum(mine, ws, total);
#pragma unroll
    for (int q = 0; q < kSumsPerThread; ++q) {
      if (i0 + q < n_sums) ha.sums[i0 + q] = run;
      run += v[q];
    }
    carry += total;
  }
}

// hoffsets[r + 1] <- the running total through record r, from the block's base (sums[b]; without sums the chunk
// is one block and its base is hoffsets[rec0])
__global__ __launch_bounds__(256) void hits_rescan_kernel(HitsArgs ha, int use_sums) {
  __shared__ long long ws[kWavesPerBlock];
  const int64_t li0 = static_cast<int64_t>(blockIdx.x) * bounds::kHitsScanBlockRecords + threadIdx.x * kPerThread;
  int64_t* cnt = ha.hoffsets + ha.view.rec0 + 1;
  const long long base = use_sums ? ha.sums[blockIdx.x] : ha.hoffsets[ha.view.rec0];
  long long v[kPerThread], mine = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) mine += v[q] = li0 + q < ha.view.n_rec ? cnt[li0 + q] : 0;
  long long total;
  // a thread stores only over the counts it read itself; hoffsets[rec0] is never stored here
  long long run = base + block_exclusive_sum(mine, ws, total);
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    run += v[q];
    if (li0 + q < ha.view.n_rec) cnt[li0 + q] = run;
  }
}

__global__ __launch_bounds__(256) void hits_compact_kernel(HitsArgs ha) {
  const int64_t li = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (li >= ha.view.n_rec) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int64_t r = ha.view.rec0 + li;
  const int64_t out0 = ha.hoffsets[r], out1 = ha.hoffsets[r + 1];
  if (out0 >= ha.cap || out1 == out0) return;  // wave-uniform: nothing of this record lands below cap
  const int64_t pb = chunk_first(ha.view, r);
  const int C = __builtin_amdgcn_readfirstlane(chunk_count(ha.view, r));
  const int t = ha.thresholds ? ha.thresholds[r] : ha.min_score;
  int base = 0;  // hits of the passes before this one (wave-uniform)
  for (int o0 = 0; o0 < C; o0 += 64) {  // wave-uniform: every lane reaches the ballot
    const int o = o0 + lane;
    ProfileEntry e{0, 0};
    bool hit = false;
    if (o < C) {
      e = ha.view.prof[pb + o];
      hit = e.score >= t;
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
    // set bits below this lane
    const int rank = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                                __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u)));
    if (hit) {
      const int64_t at = out0 + base + rank;
      MOC_DCHECK(at >= out0 && at < out1);
      if (at < ha.cap) ha.rows[at] = Result{e.score, o, e.k};
    }
    base += __popcll(m);
  }
  MOC_DCHECK(out0 + base == out1);
}

void preload_hits_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&hits_count_kernel));
}

void launch_hits_scan(const HitsArgs& ha, hipStream_t stream) {
  if (ha.view.n_rec <= 0) return;
  const int64_t n_sums = (ha.view.n_rec + bounds::kHitsScanBlockRecords - 1) / bounds::kHitsScanBlockRecords;
  if (n_sums > 1) {
    hipLaunchKernelGGL(hits_block_sums_kernel, dim3(static_cast<unsigned>(n_sums)), dim3(kBlock), 0, stream, ha);
    hipLaunchKernelGGL(hits_scan_sums_kernel, dim3(1), dim3(kBlock), 0, stream, ha, n_sums);
  }
  hipLaunchKernelGGL(hits_rescan_kernel, dim3(static_cast<unsigned>(n_sums)), dim3(kBlock), 0, stream, ha,
                     n_sums > 1 ? 1 : 0);
}

void launch_hits(const HitsArgs& ha, hipStream_t stream) {
  if (ha.view.n_rec <= 0) return;
  const unsigned wave_blocks = static_cast<unsigned>((ha.view.n_rec + kWavesPerBlock - 1) / kWavesPerBlock);
  hipLaunchKernelGGL(hits_count_kernel, dim3(wave_blocks), dim3(kBlock), 0, stream, ha);
  launch_hits_scan(ha, stream);
  if (ha.cap > 0 && ha.rows)
    hipLaunchKernelGGL(hits_compact_kernel, dim3(wave_blocks), dim3(kBlock), 0, stream, ha);
}

}  // namespace dev
}  // namespace moc
