// Per-target top-K and threshold hits: the K best entries, or every entry at or above a threshold, of every (record,
// target) pair's target profile (gfx950, wave64). Definitions: moc/cpu_engine.hpp targets_topk_batch_cpu /
// targets_hits_batch_cpu; group sizes and cut-overs: moc/kernel_bounds.hpp (targets_group).
//
// The kernels read a chunk's catalog profile where targets_select_kernel reads it (prof[poffsets[r] - base + o],
// written by offset_profile_kernel just before on the same stream). A pair's target profile is the target's slice of
// it plus at most one un-mutated boundary entry summed from the letters, which has the largest local offset: the
// pair view of targets_pair.hpp, from which all three kernels start (its group reductions and launch splitter too).
// No atomics on global memory, no kernel waits on another block, no LDS; ordering is launch order:
//   targets_topk_kernel<G>          targets_select_kernel's ownership: a group of G consecutive lanes (4, 16 or 64;
//                                   aligned to G, so __shfl_xor steps below G stay inside it) owns pair p = li * T + t
//                                   of the chunk (64-bit). The group sums the boundary entry first; it is one more
//                                   key, final_key(bsum, len_t - L2), held by one lane. K rounds of a group maximum
//                                   over the keys strictly below the previous winner (topk_select_kernel's rounds; a
//                                   lane keeps its first kHeld slice keys in registers, so slices of up to kHeld * G
//                                   entries are read once); the group's first lane stores round j's row — a slice
//                                   winner's k re-read from the profile, the boundary winner as (bsum, len_t - L2, 0),
//                                   rounds past the pair's entries as the empty row. Every lane of a wave reaches
//                                   every shuffle: K is a kernel argument, and groups without a pair, with an empty
//                                   profile or out of keys carry 0. No rank-by-counting path for short profiles.
//   targets_hits_count_kernel<G>    the same ownership: slice entries at or above the pair's threshold plus the
//                                   boundary entry, a group sum, the count to toffsets[p + 1] (batch-wide p); pair 0
//                                   of the batch also stores toffsets[0] = 0.
//   (prefix sum)                    hits_kernels.hip's launch_hits_scan over pairs in place of records, unchanged.
//   targets_hits_compact_kernel<G>  the same ownership: the group strides its slice G entries per pass; a lane's rank
//                                   is the popcount of its group's G bits of the 64-bit ballot below its own position
//                                   on top of a group-uniform running base; a hit goes to rows[toffsets[p] + base +
//                                   rank] when that is < cap, the boundary entry last. The groups of one wave have
//                                   slices of different lengths: the trip count is PADDED to the wave's longest slice
//                                   (a wave maximum before the loop), so the loop is wave-uniform and every lane
//                                   reaches every ballot; a group past its own slice, with a pair that starts at or
//                                   past cap or without hits contributes no bits and stores nothing.
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
constexpr int kHeld = 4;  // slice keys a lane keeps in registers (topk_select_kernel's held[])
}  // namespace

// pairs [pair0, pair0 + gridDim.x * (kBlock / G)) of the chunk's n_pairs = n_rec * T
template <int G>
__global__ __launch_bounds__(256) void targets_topk_kernel(TargetsArgs ta, int K, ProblemView pv, BatchView bv,
                                                           int64_t pair0, int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets rows: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  const int sub = threadIdx.x & (G - 1);
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G), n_pairs);
  // every lane of the wave reaches the shuffles (the loops are the only divergent parts)
  const int bsum = group_sum_i32<G>(boundary_part(p, pv, sub, G));
  const int C = p.slice + (p.boundary ? 1 : 0);
  // the boundary entry's key: one more key of the lane the stride would give its offset to
  const unsigned long long bkey =
      p.boundary && sub == (p.slice & (G - 1)) ? final_key(bsum, static_cast<uint32_t>(p.slice)) : 0ull;
  unsigned long long held[kHeld];  // 0: no entry (a real key is never 0: o < 2^31)
#pragma unroll
  for (int q = 0; q < kHeld; ++q) {
    const int o = sub + G * q;
    held[q] = o < p.slice ? final_key(slice_entry(ta, p, o).score, static_cast<uint32_t>(o)) : 0ull;
  }
  Result* out = ta.out + p.p * K;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < K; ++j) {  // K is wave-uniform
    unsigned long long m = 0ull;
    if (j < C) {  // group-uniform: min(K, C) rounds have a winner
#pragma unroll
      for (int q = 0; q < kHeld; ++q) m = (j == 0 || held[q] < prev) ? max_u64(m, held[q]) : m;
      for (int o = sub + G * kHeld; o < p.slice; o += G) {
        const unsigned long long k = final_key(slice_entry(ta, p, o).score, static_cast<uint32_t>(o));
        m = (j == 0 || k < prev) ? max_u64(m, k) : m;
      }
      m = (j == 0 || bkey < prev) ? max_u64(m, bkey) : m;
    }
    m = group_max_u64<G>(m);
    if (p.active && sub == 0) {
      Result row{INT32_MIN, 0, 0};
      if (m != 0ull) {
        const int o = static_cast<int>(0xffffffffu - static_cast<uint32_t>(m));
        MOC_DCHECK(o >= 0 && o < C);
        if (o < p.slice) {
          const ProfileEntry e = slice_entry(ta, p, o);
          row = Result{e.score, o, e.k};
        } else {
          row = Result{bsum, p.slice, 0};
        }
      }
      MOC_DCHECK(p.p * K + j >= 0 && p.p * K + j < ta.view.n_total * ta.T * K);
      out[j] = row;
    }
    prev = m;
  }
}

template <int G>
__global__ __launch_bounds__(256) void targets_hits_count_kernel(TargetsHitsArgs ha, ProblemView pv, BatchView bv,
                                                                 int64_t pair0, int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets rows: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  const TargetsArgs& ta = ha.ta;
  const int sub = threadIdx.x & (G - 1);
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G), n_pairs);
  const int thr = pair_threshold(ha, p);
  int count = 0;  // slice < 2^31
  for (int o = sub; o < p.slice; o += G) count += slice_entry(ta, p, o).score >= thr ? 1 : 0;
  // every lane of the wave reaches the shuffles
  const int bsum = group_sum_i32<G>(boundary_part(p, pv, sub, G));
  count = group_sum_i32<G>(count);
  if (p.active && sub == 0) {
    MOC_DCHECK(p.p >= 0 && p.p + 1 <= ta.view.n_total * ta.T);
    ha.toffsets[p.p + 1] = count + (p.boundary && bsum >= thr ? 1 : 0);
    if (p.p == 0) ha.toffsets[0] = 0;
  }
}

template <int G>
__global__ __launch_bounds__(256) void targets_hits_compact_kernel(TargetsHitsArgs ha, ProblemView pv, BatchView bv,
                                                                   int64_t pair0, int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets rows: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  constexpr unsigned long long kGroupBits = G == 64 ? ~0ull : (1ull << G) - 1ull;
  const TargetsArgs& ta = ha.ta;
  const int sub = threadIdx.x & (G - 1);
  const int gfirst = (threadIdx.x & 63) & ~(G - 1);  // the group's first lane of the wave
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G), n_pairs);
  int64_t out0 = 0, out1 = 0;
  if (p.active) {
    MOC_DCHECK(p.p >= 0 && p.p + 1 <= ta.view.n_total * ta.T);
    out0 = ha.toffsets[p.p];
    out1 = ha.toffsets[p.p + 1];
  }
  const bool work = p.active && out0 < ha.cap && out1 > out0;  // group-uniform: something of this pair lands below cap
  const int thr = pair_threshold(ha, p);
  const int slice = work ? p.slice : 0;
  // the wave's longest slice, in a scalar register: the loop is wave-uniform and every lane reaches every ballot
  const int trips = __builtin_amdgcn_readfirstlane(wave_max_i32(slice));
  int bpart = 0;
  if (work) bpart = boundary_part(p, pv, sub, G);
  const int bsum = group_sum_i32<G>(bpart);
  int base = 0;  // hits of the passes before this one (group-uniform)
  for (int o0 = 0; o0 < trips; o0 += G) {
    const int o = o0 + sub;
    ProfileEntry e{0, 0};
    bool hit = false;
    if (o < slice) {
      e = slice_entry(ta, p, o);
      hit = e.score >= thr;
    }
    const unsigned long long m = (__builtin_amdgcn_ballot_w64(hit) >> gfirst) & kGroupBits;  // the group's G bits
    if (hit) {
      const int rank = __popcll(m & ((1ull << sub) - 1ull));  // set bits of the group below this lane
      const int64_t at = out0 + base + rank;
      MOC_DCHECK(at >= out0 && at < out1);
      if (at < ha.cap) ha.rows[at] = Result{e.score, o, e.k};
    }
    base += __popcll(m);
  }
  if (work && sub == 0) {
    if (p.boundary && bsum >= thr) {  // the largest local offset: the pair's last row
      const int64_t at = out0 + base;
      MOC_DCHECK(at >= out0 && at + 1 == out1);
      if (at < ha.cap) ha.rows[at] = Result{bsum, p.slice, 0};
    } else {
      MOC_DCHECK(out0 + base == out1);
    }
  }
}

void preload_targets_rows_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&targets_topk_kernel<4>));
}

namespace {
template <int G>
void launch_topk_g(const TargetsArgs& ta, int K, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  const int64_t n_pairs = ta.view.n_rec * ta.T;
  for_each_launch<G>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_topk_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, ta, K, pv, bv, pair0, n_pairs);
  });
}

template <int G>
void launch_hits_g(const TargetsHitsArgs& ha, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  const int64_t n_pairs = ha.ta.view.n_rec * ha.ta.T;
  for_each_launch<G>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_hits_count_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, ha, pv, bv, pair0, n_pairs);
  });
  // the prefix sum over pairs: launch_hits_scan reads view.rec0, view.n_rec, hoffsets and sums only
  HitsArgs scan;
  scan.view.rec0 = ha.ta.view.rec0 * ha.ta.T;
  scan.view.n_rec = n_pairs;
  scan.hoffsets = ha.toffsets;
  scan.sums = ha.sums;
  launch_hits_scan(scan, stream);
  if (ha.cap <= 0 || !ha.rows) return;
  for_each_launch<G>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_hits_compact_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, ha, pv, bv, pair0, n_pairs);
  });
}
}  // namespace

void launch_targets_topk(const TargetsArgs& ta, int K, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  if (ta.view.n_rec <= 0 || ta.T <= 0) return;
  with_group(ta.group, [&](auto g) { launch_topk_g<g()>(ta, K, pv, bv, stream); });
}

void launch_targets_hits(const TargetsHitsArgs& ha, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  if (ha.ta.view.n_rec <= 0 || ha.ta.T <= 0) return;
  with_group(ha.ta.group, [&](auto g) { launch_hits_g<g()>(ha, pv, bv, stream); });
}

}  // namespace dev
}  // namespace moc
