// Per-target profile summary: the summary row and histogram of every (record, target) pair's target profile (gfx950,
// wave64). Definitions: moc/cpu_engine.hpp targets_summary_batch_cpu; group sizes, cut-overs and the histogram's LDS
// rule: moc/kernel_bounds.hpp.
//
// The kernels read a chunk's catalog profile where targets_select_kernel reads it (prof[poffsets[r] - base + o],
// written by offset_profile_kernel just before on the same stream) and reduce, per pair, the target's slice of it
// plus at most one un-mutated boundary entry summed from the letters. No atomics on global memory, no kernel waits on
// another block; ordering is launch order:
//   targets_summary_kernel<G>  targets_select_kernel's ownership: a group of G consecutive lanes (4, 16 or 64; aligned
//                              to G, so __shfl_xor steps below G stay inside it) owns pair p = li * T + t of the chunk
//                              (64-bit). A lane strides the slice's len_t - L2 entries keeping an int64 sum and sum of
//                              squares, an int32 minimum and the largest final_key(score, local o); where the
//                              boundary entry takes part the group strides the record's letters for its sum;
//                              xor-shuffle reductions (the int64 ones over both halves); the group's first lane folds
//                              the boundary entry into all five (it has the largest offset: it wins max only with a
//                              strictly higher score), looks up the winner's k and stores the seven values. Every lane
//                              of a wave reaches every shuffle: groups without a pair, with a pair that does not fit
//                              or with an empty slice carry the neutral values. No LDS.
//   targets_hist_kernel<G>     (bins > 0) the same ownership: a group owns `bins` int32 counters in LDS, zeroes them,
//                              counts its slice entries with LDS adds, adds the boundary entry's bin after the group
//                              sum and stores its row. The barriers are reached by every wave of the block, with or
//                              without a pair. A block's counters take at most bounds::kTargetsHistLdsBytes.
#include <hip/hip_runtime.h>

#include "kernel_common.hpp"
#include "moc/kernel_bounds.hpp"
#include "moc/runtime/hip_check.hpp"

namespace moc {
namespace dev {

using namespace kc;

namespace {
constexpr int kBlock = bounds::kTargetsThreads;
constexpr int kCols = 7;  // kSummaryCols: count, sum, sumsq, min, max, n, k
constexpr int64_t kMaxBlocksPerLaunch = int64_t{1} << 30;  // below the 2^31 - 1 grid limit

template <int G>
__device__ __forceinline__ unsigned long long group_max_u64(unsigned long long v) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) {
    const int lo = __shfl_xor(static_cast<int>(v), d, 64);
    const int hi = __shfl_xor(static_cast<int>(v >> 32), d, 64);
    v = max_u64(v, (static_cast<unsigned long long>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo));
  }
  return v;
}

template <int G>
__device__ __forceinline__ long long group_sum_i64(long long v) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) {
    const int lo = __shfl_xor(static_cast<int>(v), d, 64);
    const int hi = __shfl_xor(static_cast<int>(v >> 32), d, 64);
    v += static_cast<long long>((static_cast<unsigned long long>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo));
  }
  return v;
}

template <int G>
__device__ __forceinline__ int group_sum_i32(int v) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <int G>
__device__ __forceinline__ int group_min_i32(int v) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}

// summary_kernels.hip's summary_bin_dev: clamp(floor((score - lo) / width), 0, bins - 1) with the difference formed
// in 64 bits; a negative one clamps to bin 0, a non-negative one is below 2^32 and divides as an unsigned 32-bit one.
__device__ __forceinline__ int targets_bin_dev(int score, int lo, int width, int bins) {
  const long long d = static_cast<long long>(score) - static_cast<long long>(lo);
  if (d < 0) return 0;
  MOC_DCHECK(d <= 0xffffffffll && width >= 1);
  const uint32_t q = static_cast<uint32_t>(d) / static_cast<uint32_t>(width);
  return q < static_cast<uint32_t>(bins) ? static_cast<int>(q) : bins - 1;
}

// What a group knows about its pair: both kernels start from it.
struct Pair {
  int64_t r = 0, pb = 0, b = 0;  // batch-wide record, its profile's first entry in `prof`, the target's start
  int t = 0, L2 = 0;
  int slice = 0;          // entries of the pair's slice; local offset of its boundary entry
  bool active = false;    // the group has a pair (uniform over the group)
  bool fits = false;
  bool boundary = false;  // the boundary entry takes part
  const uint8_t* rec = nullptr;
};

__device__ __forceinline__ Pair pair_of(const TargetsArgs& ta, const ProblemView& pv, const BatchView& bv, int64_t pair,
                                        int64_t n_pairs) {
  Pair p;
  p.active = pair < n_pairs;
  int len = 0;
  if (p.active) {
    const int64_t li = pair / ta.T;
    p.t = static_cast<int>(pair - li * ta.T);
    p.r = ta.view.rec0 + li;
    MOC_DCHECK(li >= 0 && li < ta.view.n_rec && p.r >= 0 && p.r < bv.n && p.t >= 0 && p.t < ta.T);
    p.rec = bv.codes + (bv.offsets[p.r] - bv.offsets[0]);
    p.L2 = static_cast<int>(bv.offsets[p.r + 1] - bv.offsets[p.r]);
    p.b = ta.starts[p.t];
    len = static_cast<int>(ta.starts[p.t + 1] - p.b);
    p.pb = chunk_first(ta.view, p.r);
    MOC_DCHECK(p.b >= 0 && len >= 1 && p.b + len <= pv.L1);
  }
  p.fits = p.active && p.L2 >= 1 && p.L2 <= len && p.L2 <= pv.L1;
  p.slice = p.fits ? len - p.L2 : 0;
  p.boundary = p.fits && (pv.semantics == static_cast<int>(Semantics::Spec) || p.slice == 0);
  return p;
}

// this lane's share of the boundary entry's score (0 where the entry does not take part)
template <int G>
__device__ __forceinline__ int boundary_part(const Pair& p, const ProblemView& pv, int sub) {
  int bsum = 0;
  if (p.boundary) {
    const int64_t a0 = p.b + p.slice;  // the entry's first Seq1 letter; its last is b + len - 1 < L1
    for (int l = sub; l < p.L2; l += G) {
      const int c = p.rec[l];
      MOC_DCHECK(c >= 0 && c < kLutStride);
      MOC_DCHECK(a0 + l >= 0 && a0 + l < pv.L1);
      bsum += pv.lut[(c << 5) + pv.seq1[a0 + l]];
    }
  }
  return bsum;
}
}  // namespace

// pairs [pair0, pair0 + gridDim.x * (kBlock / G)) of the chunk's n_pairs = n_rec * T
template <int G>
__global__ __launch_bounds__(256) void targets_summary_kernel(TargetsSummaryArgs sa, ProblemView pv, BatchView bv,
                                                              int64_t pair0, int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets summary: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  const TargetsArgs& ta = sa.ta;
  const int sub = threadIdx.x & (G - 1);
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G), n_pairs);
  long long sum = 0, sumsq = 0;
  int mn = INT32_MAX;
  unsigned long long key = 0ull;  // 0: no entry (a real key is never 0: o < 2^31)
  for (int o = sub; o < p.slice; o += G) {
    const int64_t at = p.pb + p.b + o;
    MOC_DCHECK(p.b + o < chunk_count(ta.view, p.r));  // the slice lies inside the record's entries
    const int sc = ta.view.prof[at].score;
    const long long s = sc;
    sum += s;
    sumsq += s * s;
    mn = min(mn, sc);
    key = max_u64(key, final_key(sc, static_cast<uint32_t>(o)));
  }
  int bsum = boundary_part<G>(p, pv, sub);
  // every lane of the wave reaches the shuffles (the two loops above are the only divergent parts)
  sum = group_sum_i64<G>(sum);
  sumsq = group_sum_i64<G>(sumsq);
  mn = group_min_i32<G>(mn);
  key = group_max_u64<G>(key);
  bsum = group_sum_i32<G>(bsum);
  if (p.active && sub == 0) {
    long long count = p.slice, mx = INT32_MIN, bn = 0, bk = 0;
    if (key != 0ull) {
      const int o = static_cast<int>(0xffffffffu - static_cast<uint32_t>(key));
      MOC_DCHECK(o >= 0 && o < p.slice);
      const int64_t at = p.pb + p.b + o;
      const ProfileEntry e = ta.view.prof[at];
      mx = e.score;
      bn = o;
      bk = e.k;
    }
    if (p.boundary) {
      const long long s = bsum;
      ++count;
      sum += s;
      sumsq += s * s;
      mn = min(mn, bsum);
      if (key == 0ull || s > mx) {
        mx = s;
        bn = p.slice;
        bk = 0;
      }
    }
    long long* row = reinterpret_cast<long long*>(sa.summary) + (p.r * ta.T + p.t) * kCols;
    row[0] = count;
    row[1] = sum;
    row[2] = sumsq;
    row[3] = mn;
    row[4] = mx;
    row[5] = bn;
    row[6] = bk;
  }
}

// MAXB: the most bins a group of G lanes takes (bounds::targets_hist_group keeps bins within it)
template <int G, int MAXB>
__global__ __launch_bounds__(256) void targets_hist_kernel(TargetsSummaryArgs sa, ProblemView pv, BatchView bv,
                                                           int64_t pair0, int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets summary: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  static_assert(kGroupsPerBlock * MAXB * 4 <= bounds::kTargetsHistLdsBytes, "targets summary: a block's counters within 16 KiB");
  __shared__ int cnt[kGroupsPerBlock * MAXB];
  const TargetsArgs& ta = sa.ta;
  const int sub = threadIdx.x & (G - 1);
  const int g = threadIdx.x / G;
  const int bins = sa.bins;
  MOC_DCHECK(bins >= 1 && bins <= MAXB);
  int* mine = cnt + g * MAXB;
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + g, n_pairs);
  for (int b = sub; b < bins; b += G) mine[b] = 0;
  __syncthreads();
  for (int o = sub; o < p.slice; o += G) {
    const int64_t at = p.pb + p.b + o;
    MOC_DCHECK(p.b + o < chunk_count(ta.view, p.r));  // the slice lies inside the record's entries
    const int b = targets_bin_dev(ta.view.prof[at].score, sa.lo, sa.width, bins);
    MOC_DCHECK(b >= 0 && b < bins);
    atomicAdd(&mine[b], 1);  // LDS add: lanes on one bin serialise and stay exact
  }
  // every lane of the wave reaches the shuffles
  const int bsum = group_sum_i32<G>(boundary_part<G>(p, pv, sub));
  if (p.boundary && sub == 0) {
    const int b = targets_bin_dev(bsum, sa.lo, sa.width, bins);
    MOC_DCHECK(b >= 0 && b < bins);
    atomicAdd(&mine[b], 1);
  }
  __syncthreads();
  if (p.active) {
    int32_t* row = sa.hist + (p.r * ta.T + p.t) * bins;
    for (int b = sub; b < bins; b += G) row[b] = mine[b];
  }
}

void preload_targets_summary_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&targets_summary_kernel<4>));
}

namespace {
template <int G>
void launch_summary_g(const TargetsSummaryArgs& sa, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  constexpr int64_t kGroupsPerBlock = kBlock / G;
  const int64_t n_pairs = sa.ta.view.n_rec * sa.ta.T;
  for (int64_t pair0 = 0; pair0 < n_pairs;) {
    const int64_t blocks = std::min<int64_t>((n_pairs - pair0 + kGroupsPerBlock - 1) / kGroupsPerBlock, kMaxBlocksPerLaunch);
    hipLaunchKernelGGL((targets_summary_kernel<G>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, sa, pv,
                       bv, pair0, n_pairs);
    pair0 += blocks * kGroupsPerBlock;
  }
}

template <int G, int MAXB>
void launch_hist_g(const TargetsSummaryArgs& sa, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  constexpr int64_t kGroupsPerBlock = kBlock / G;
  const int64_t n_pairs = sa.ta.view.n_rec * sa.ta.T;
  for (int64_t pair0 = 0; pair0 < n_pairs;) {
    const int64_t blocks = std::min<int64_t>((n_pairs - pair0 + kGroupsPerBlock - 1) / kGroupsPerBlock, kMaxBlocksPerLaunch);
    hipLaunchKernelGGL((targets_hist_kernel<G, MAXB>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, sa,
                       pv, bv, pair0, n_pairs);
    pair0 += blocks * kGroupsPerBlock;
  }
}
}  // namespace

void launch_targets_summary(const TargetsSummaryArgs& sa, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  if (sa.ta.view.n_rec <= 0 || sa.ta.T <= 0) return;
  switch (sa.ta.group) {
    case 4: launch_summary_g<4>(sa, pv, bv, stream); break;
    case 16: launch_summary_g<16>(sa, pv, bv, stream); break;
    default: launch_summary_g<64>(sa, pv, bv, stream); break;
  }
  if (sa.bins <= 0 || !sa.hist) return;
  switch (bounds::targets_hist_group(sa.ta.group == 4 || sa.ta.group == 16 ? sa.ta.group : 64, sa.bins)) {
    case 4: launch_hist_g<4, bounds::kTargetsHistGroup4MaxBins>(sa, pv, bv, stream); break;
    case 16: launch_hist_g<16, bounds::kSummaryMaxBins>(sa, pv, bv, stream); break;
    default: launch_hist_g<64, bounds::kSummaryMaxBins>(sa, pv, bv, stream); break;
  }
}

}  // namespace dev
}  // namespace moc
