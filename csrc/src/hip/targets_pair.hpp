// The (record, target) pair of the per-target kernels (gfx950, wave64): the one place that says which profile entries
// are a pair's slice, whether its boundary entry takes part and how many entries it has, with the lane-group
// reductions and the host-side launch plumbing those kernels share. Included only by the targets_*.hip files.
#pragma once

#include <algorithm>
#include <type_traits>

#include "kernel_common.hpp"
#include "moc/kernel_bounds.hpp"

namespace moc {
namespace dev {
namespace tp {

// ---- reductions over a group of G consecutive lanes aligned to G (xor steps below G stay inside it) ----------------
template <int G>
__device__ __forceinline__ unsigned long long group_max_u64(unsigned long long v) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) {
    const int lo = __shfl_xor(static_cast<int>(v), d, 64);
    const int hi = __shfl_xor(static_cast<int>(v >> 32), d, 64);
    v = kc::max_u64(v, (static_cast<unsigned long long>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo));
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

// ---- the pair view -------------------------------------------------------------------------------------------------
// What a group knows about its pair: every per-target kernel starts from it.
struct Pair {
  int64_t r = 0, pb = 0, b = 0;  // batch-wide record, its profile's first entry in `prof`, the target's start
  int64_t p = 0;                 // batch-wide pair index r * T + t
  int t = 0, L2 = 0;
  int slice = 0;          // entries of the pair's slice; local offset of its boundary entry
  bool active = false;    // the group has a pair (uniform over the group)
  bool fits = false;
  bool boundary = false;  // the boundary entry takes part
  const uint8_t* rec = nullptr;
};

// pair: index within the chunk's n_pairs = n_rec * T, never negative (no compare is spent on that)
__device__ __forceinline__ Pair pair_of(const TargetsArgs& ta, const ProblemView& pv, const BatchView& bv, int64_t pair,
                                        int64_t n_pairs) {
  MOC_DCHECK(pair >= 0);
  Pair p;
  p.active = pair < n_pairs;
  int len = 0;
  if (p.active) {
    const int64_t li = pair / ta.T;
    p.t = static_cast<int>(pair - li * ta.T);
    p.r = ta.view.rec0 + li;
    p.p = p.r * ta.T + p.t;
    MOC_DCHECK(li >= 0 && li < ta.view.n_rec && p.r >= 0 && p.r < bv.n && p.t >= 0 && p.t < ta.T);
    p.rec = bv.codes + (bv.offsets[p.r] - bv.offsets[0]);
    p.L2 = static_cast<int>(bv.offsets[p.r + 1] - bv.offsets[p.r]);
    p.b = ta.starts[p.t];
    len = static_cast<int>(ta.starts[p.t + 1] - p.b);
    p.pb = kc::chunk_first(ta.view, p.r);
    MOC_DCHECK(p.b >= 0 && len >= 1 && p.b + len <= pv.L1);
  }
  p.fits = p.active && p.L2 >= 1 && p.L2 <= len && p.L2 <= pv.L1;
  p.slice = p.fits ? len - p.L2 : 0;
  p.boundary = p.fits && (pv.semantics == static_cast<int>(Semantics::Spec) || p.slice == 0);
  return p;
}

// entries of the pair's profile (0: no pair, or it does not fit)
__device__ __forceinline__ int pair_count(const Pair& p) { return p.slice + (p.boundary ? 1 : 0); }

// this thread's share of the boundary entry's score, letters sub, sub + stride, ... (0 where the entry does not take part)
__device__ __forceinline__ int boundary_part(const Pair& p, const ProblemView& pv, int sub, int stride) {
  int bsum = 0;
  if (p.boundary) {
    const int64_t a0 = p.b + p.slice;  // the entry's first Seq1 letter; its last is b + len - 1 < L1
    for (int l = sub; l < p.L2; l += stride) {
      const int c = p.rec[l];
      MOC_DCHECK(c >= 0 && c < kLutStride);
      MOC_DCHECK(a0 + l >= 0 && a0 + l < pv.L1);
      bsum += pv.lut[(c << 5) + pv.seq1[a0 + l]];
    }
  }
  return bsum;
}

// entry o of the pair's slice
__device__ __forceinline__ ProfileEntry slice_entry(const TargetsArgs& ta, const Pair& p, int o) {
  MOC_DCHECK(o >= 0 && o < p.slice);
  MOC_DCHECK(p.b + o < kc::chunk_count(ta.view, p.r));  // the slice lies inside the record's entries
  return ta.view.prof[p.pb + p.b + o];
}

__device__ __forceinline__ int pair_threshold(const TargetsHitsArgs& ha, const Pair& p) {
  if (!p.active || !ha.thresholds) return ha.min_score;
  MOC_DCHECK(p.p >= 0 && p.p < ha.ta.view.n_total * ha.ta.T);
  return ha.thresholds[p.p];
}

// ---- host side -----------------------------------------------------------------------------------------------------
constexpr int64_t kMaxBlocksPerLaunch = int64_t{1} << 30;  // below the 2^31 - 1 grid limit

// fn(blocks, item0) for every launch over n_items items (pairs, records) with G lanes of a kTargetsThreads block
// each, split below the grid limit
template <int G, class Fn>
void for_each_launch(int64_t n_items, Fn&& fn) {
  constexpr int64_t kGroupsPerBlock = bounds::kTargetsThreads / G;
  for (int64_t item0 = 0; item0 < n_items;) {
    const int64_t blocks = std::min<int64_t>((n_items - item0 + kGroupsPerBlock - 1) / kGroupsPerBlock, kMaxBlocksPerLaunch);
    fn(static_cast<unsigned>(blocks), item0);
    item0 += blocks * kGroupsPerBlock;
  }
}

// fn(g) with g() == 4, 16 or 64 a constant expression: the planner's lane-group size as a template argument
// (anything else means 64)
template <class Fn>
void with_group(int group, Fn&& fn) {
  switch (group) {
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 16: fn(std::integral_constant<int, 16>{}); break;
    default: fn(std::integral_constant<int, 64>{}); break;
  }
}

}  // namespace tp
}  // namespace dev
}  // namespace moc
