// Per-target top-K and threshold hits: the K best entries, or every entry at or above a threshold, of every (record,
// target) pair's target profile (gfx950, wave64). Definitions: moc/cpu_engine.hpp targets_topk_batch_cpu /
// targets_hits_batch_cpu; group sizes and cut-overs: moc/kernel_bounds.hpp (targets_group).
//
// The kernels read a chunk's catalog profile where targets_select_kernel reads it (prof[poffsets[r] - base + o],
// written by offset_profile_kernel just before on the same stream). A pair's target profile is the target's slice of
// it plus at most one un-mutated boundary entry summed from the letters, which has the largest local offset. No
// atomics on global memory, no kernel waits on another block, no LDS; ordering is launch order:
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

namespace moc {
namespace dev {

using namespace kc;

namespace {
constexpr int kBlock = bounds::kTargetsThreads;
constexpr int64_t kMaxBlocksPerLaunch = int64_t{1} << 30;  // below the 2^31 - 1 grid limit
constexpr int kHeld = 4;  // slice keys a lane keeps in registers (topk_select_kernel's held[])

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
__device__ __forceinline__ int group_sum_i32(int v) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// What a group knows about its pair (targets_summary_kernels.hip's): all three kernels start from it.
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

__device__ __forceinline__ Pair pair_of(const TargetsArgs& ta, const ProblemView& pv, const BatchView& bv, int64_t pair,
                                        int64_t n_pairs) {
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

// entry o of the pair's slice
__device__ __forceinline__ ProfileEntry slice_entry(const TargetsArgs& ta, const Pair& p, int o) {
  MOC_DCHECK(o >= 0 && o < p.slice);
  MOC_DCHECK(p.b + o < chunk_count(ta.view, p.r));  // the slice lies inside the record's entries
  return ta.view.prof[p.pb + p.b + o];
}

__device__ __forceinline__ int pair_threshold(const TargetsHitsArgs& ha, const Pair& p) {
  if (!p.active || !ha.thresholds) return ha.min_score;
  MOC_DCHECK(p.p >= 0 && p.p < ha.ta.view.n_total * ha.ta.T);
  return ha.thresholds[p.p];
}
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
  const int bsum = group_sum_i32<G>(boundary_part<G>(p, pv, sub));
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
  const int bsum = group_sum_i32<G>(boundary_part<G>(p, pv, sub));
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
  if (work) bpart = boundary_part<G>(p, pv, sub);
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
// fn(blocks, pair0) for every launch over n_pairs pairs with G lanes each, split below the grid limit
template <int G, class Fn>
void for_each_launch(int64_t n_pairs, Fn&& fn) {
  constexpr int64_t kGroupsPerBlock = kBlock / G;
  for (int64_t pair0 = 0; pair0 < n_pairs;) {
    const int64_t blocks = std::min<int64_t>((n_pairs - pair0 + kGroupsPerBlock - 1) / kGroupsPerBlock, kMaxBlocksPerLaunch);
    fn(static_cast<unsigned>(blocks), pair0);
    pair0 += blocks * kGroupsPerBlock;
  }
}

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
  switch (ta.group) {
    case 4: launch_topk_g<4>(ta, K, pv, bv, stream); break;
    case 16: launch_topk_g<16>(ta, K, pv, bv, stream); break;
    default: launch_topk_g<64>(ta, K, pv, bv, stream); break;
  }
}

void launch_targets_hits(const TargetsHitsArgs& ha, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  if (ha.ta.view.n_rec <= 0 || ha.ta.T <= 0) return;
  switch (ha.ta.group) {
    case 4: launch_hits_g<4>(ha, pv, bv, stream); break;
    case 16: launch_hits_g<16>(ha, pv, bv, stream); break;
    default: launch_hits_g<64>(ha, pv, bv, stream); break;
  }
}

}  // namespace dev
}  // namespace moc
