// Per-target profile summary: the summary row and histogram of every (record, target) pair's target profile (gfx950,
// wave64). Definitions: moc/cpu_engine.hpp targets_summary_batch_cpu; group sizes, cut-overs and the histogram's LDS
// rule: moc/kernel_bounds.hpp.
//
// The kernels read a chunk's catalog profile where targets_select_kernel reads it (prof[poffsets[r] - base + o],
// written by offset_profile_kernel just before on the same stream) and reduce, per pair, the target's slice of it
// plus at most one un-mutated boundary entry summed from the letters: the pair view of targets_pair.hpp, from which
// both kernels start (its group reductions and launch splitter too; the bin function is kernel_common.hpp's). No
// atomics on global memory, no kernel waits on another block; ordering is launch order:
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
#include "targets_pair.hpp"

namespace moc {
namespace dev {

using namespace kc;
using namespace tp;

namespace {
constexpr int kBlock = bounds::kTargetsThreads;
constexpr int kCols = 7;  // kSummaryCols: count, sum, sumsq, min, max, n, k
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
  int bsum = boundary_part(p, pv, sub, G);
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
    const int b = summary_bin_dev(ta.view.prof[at].score, sa.lo, sa.width, bins);
    MOC_DCHECK(b >= 0 && b < bins);
    atomicAdd(&mine[b], 1);  // LDS add: lanes on one bin serialise and stay exact
  }
  // every lane of the wave reaches the shuffles
  const int bsum = group_sum_i32<G>(boundary_part(p, pv, sub, G));
  if (p.boundary && sub == 0) {
    const int b = summary_bin_dev(bsum, sa.lo, sa.width, bins);
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
  const int64_t n_pairs = sa.ta.view.n_rec * sa.ta.T;
  for_each_launch<G>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_summary_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, sa, pv, bv, pair0, n_pairs);
  });
}

template <int G>
void launch_hist_g(const TargetsSummaryArgs& sa, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  constexpr int kMaxBins = G == 4 ? bounds::kTargetsHistGroup4MaxBins : bounds::kSummaryMaxBins;
  const int64_t n_pairs = sa.ta.view.n_rec * sa.ta.T;
  for_each_launch<G>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_hist_kernel<G, kMaxBins>), dim3(blocks), dim3(kBlock), 0, stream, sa, pv, bv, pair0,
                       n_pairs);
  });
}
}  // namespace

void launch_targets_summary(const TargetsSummaryArgs& sa, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  if (sa.ta.view.n_rec <= 0 || sa.ta.T <= 0) return;
  with_group(sa.ta.group, [&](auto g) { launch_summary_g<g()>(sa, pv, bv, stream); });
  if (sa.bins <= 0 || !sa.hist) return;
  const int hist_group = bounds::targets_hist_group(sa.ta.group == 4 || sa.ta.group == 16 ? sa.ta.group : 64, sa.bins);
  with_group(hist_group, [&](auto g) { launch_hist_g<g()>(sa, pv, bv, stream); });
}

}  // namespace dev
}  // namespace moc
