// Per-target distinct placements: the peak filter over every (record, target) pair's OWN profile, and the per-target
// top-K and hits kernels over the peaks only (gfx950, wave64). Definitions: moc/cpu_engine.hpp targets_topk_batch_cpu /
// targets_hits_batch_cpu with radius > 0; geometry and segment widths: moc/kernel_bounds.hpp (targets_peaks_seg).
//
// A pair's profile is what targets_rows_kernels.hip ranks: its target's slice of the chunk's catalog profile
// (prof[poffsets[r] - base + starts[t] + o], written by offset_profile_kernel just before on the same stream) plus,
// when it takes part, one un-mutated boundary entry summed from the letters at local offset `slice`; C entries in
// all. Local entry o is a peak of radius R iff its order-free key (score ^ 2^31) << 32 | (2^32 - 1 - o) is the
// maximum of the keys at local offsets [o - R, o + R] clipped to [0, C): the windows never hold a straddling catalog
// entry, the catalog's own value at the boundary offset or a neighbouring target's entry — a key outside [0, C) is 0,
// the maximum's identity. Every entry decides from its own window: no atomics, no kernel waits on another block, no
// state crosses a chunk; ordering is launch order.
//
// Marks: one byte per entry in the catalog's own layout, peak[poffsets[r] - base + starts[t] + o] for o <= slice.
// Slices of different targets are disjoint and a boundary entry's byte is that of a straddling catalog entry that no
// pair owns. The one edge of this layout — under the reference semantics a last target of exactly the record's
// length puts its boundary byte one past the record's entries — is a pair of C == 1, and for C == 1 NO MARK IS EVER
// STORED OR READ: its one entry is a peak at every radius. Every other byte a consumer reads was stored by this
// chunk's pass (the scratch is reused across chunks and calls): the pass stores all C marks of every fitting pair of
// C >= 2, the segment kernel those of 2 .. S entries, the tile kernel the longer ones.
//   targets_peaks_seg_kernel<S>   pairs of 2 .. S entries: a segment of S consecutive lanes (4, 8, 16, 32 or 64; aligned to
//                                 S) owns pair p = li * T + t of the chunk, a lane per entry, lane `slice` of the
//                                 segment the boundary entry, its score a segment sum over the letters. The window
//                                 maximum is peaks_wave_kernel's log-step construction with the shuffles clipped to
//                                 the segment (a source lane outside it contributes 0, and so do the segment's lanes
//                                 at and past C); R >= S - 1 is the segment maximum. The segments of a wave hold pairs
//                                 of different C, no pair, or one that does not fit or is the tile kernel's: those
//                                 carry key 0 and store nothing, and every lane of the wave reaches every shuffle
//                                 (the trip counts depend on S and the radius, a kernel argument, alone).
//   targets_peaks_tile_kernel     pairs of more than S entries: a workgroup per (pair, tile of kPeaksTile entries)
//                                 work item, peaks_tile_kernel's LDS scheme — the tile and a halo of min(R, C - 1) keys
//                                 on each side, 0 outside [0, C), doubling steps with a barrier between every read and
//                                 write phase, two overlapping power-of-two windows over [o - R, o + R]. The boundary
//                                 key is summed once per work item by the block, before the keys are built, and only
//                                 when the tile's key range holds it.
//   targets_topk_peaks_kernel<G> / targets_hits_count_peaks_kernel<G> / targets_hits_compact_peaks_kernel<G>
//                                 targets_topk_kernel, targets_hits_count_kernel and targets_hits_compact_kernel over
//                                 the peaks: the same lane groups and ownership, a non-peak has key 0 or hit = false,
//                                 the boundary entry is masked like any other. They are kernels of their own beside
//                                 the unmasked ones and share only the pair view, group reductions and launch
//                                 splitter of targets_pair.hpp, from which every kernel here starts; the prefix sum is
//                                 launch_hits_scan, the compaction's padded wave-uniform trip count stays.
#include <hip/hip_runtime.h>

#include <algorithm>

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
constexpr int kHeld = 4;  // slice keys a lane keeps in registers (targets_topk_kernel's held[])
constexpr int kTile = bounds::kPeaksTile;
constexpr int kKeysPerThread = bounds::kPeaksKeysPerThread;
constexpr int kMaxKeys = kTile + 2 * bounds::kPeaksMaxRadius;
static_assert(bounds::kPeaksThreads == kBlock, "targets peaks: the tile kernel's keys per thread are kPeaksThreads'");

// v of lane `src` of this lane's segment of S lanes, or 0 when src is no lane of the segment
template <int S>
__device__ __forceinline__ unsigned long long shfl_seg_u64_or0(unsigned long long v, int seg0, int src) {
  const int s = seg0 + (src & (S - 1));
  const int lo = __shfl(static_cast<int>(v), s, 64);
  const int hi = __shfl(static_cast<int>(v >> 32), s, 64);
  const unsigned long long r = (static_cast<unsigned long long>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo);
  return src >= 0 && src < S ? r : 0ull;
}

// index of the mark of local entry o (o <= slice) of a pair of C >= 2 entries: inside the record's entries
__device__ __forceinline__ int64_t mark_at(const TargetsArgs& ta, const Pair& p, int o) {
  MOC_DCHECK(pair_count(p) >= 2 && o >= 0 && o < pair_count(p));
  MOC_DCHECK(p.b + o < chunk_count(ta.view, p.r) && p.pb + p.b + o < ta.view.prof_entries);
  return p.pb + p.b + o;
}

// whether local entry o of the pair is a peak: the stored mark, or true for the pair of one entry (never stored)
__device__ __forceinline__ bool is_peak(const TargetsArgs& ta, const uint8_t* __restrict__ peak, const Pair& p, int C, int o) {
  return C <= 1 || peak[mark_at(ta, p, o)] != 0;
}
}  // namespace

// pairs [pair0, pair0 + gridDim.x * (kBlock / S)) of the chunk's n_pairs = n_rec * T; marks of those of 2 .. S entries
template <int S>
__global__ __launch_bounds__(256) void targets_peaks_seg_kernel(TargetsPeaksArgs a, ProblemView pv, BatchView bv,
                                                                int64_t pair0, int64_t n_pairs) {
  static_assert(bounds::kTargetsPeaksMinSeg <= S && S <= 64 && (S & (S - 1)) == 0, "targets peaks: a segment is 4, 8, 16, 32 or 64 lanes");
  constexpr int kSegsPerBlock = kBlock / S;
  const TargetsArgs& ta = a.ta;
  const int sub = threadIdx.x & (S - 1);
  const int seg0 = (threadIdx.x & 63) & ~(S - 1);  // the segment's first lane of the wave
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kSegsPerBlock + (threadIdx.x / S), n_pairs);
  const int C = pair_count(p);
  const bool mine = C >= 2 && C <= S;  // segment-uniform: the pair's marks are this kernel's
  // every lane of the wave reaches the shuffles; a segment without such a pair sums nothing and carries key 0
  const int bsum = group_sum_i32<S>(mine ? boundary_part(p, pv, sub, S) : 0);
  unsigned long long key = 0ull;  // lanes at and past C hold 0, the maximum's identity (a key is never 0)
  if (mine) {
    if (sub < p.slice)
      key = final_key(slice_entry(ta, p, sub).score, static_cast<uint32_t>(sub));
    else if (sub == p.slice && p.boundary)
      key = final_key(bsum, static_cast<uint32_t>(sub));
  }
  unsigned long long m;
  if (a.radius >= S - 1) {  // wave-uniform: the window is the segment
    m = group_max_u64<S>(key);
  } else {
    // peaks_wave_kernel's halves: bl / br the maximum of the 2^p keys ending / starting at this lane, the R + 1 keys
    // ending (starting) here the windows of R + 1's set bits laid end to end — inside the segment
    const int W = a.radius + 1;  // 2 .. S - 1
    unsigned long long bl = key, br = key, ml = 0, mr = 0;
    int pl = sub, pr = sub;
#pragma unroll
    for (int d = 1; d < S; d <<= 1) {
      if (d > W) break;  // wave-uniform: no set bit of W is left, the wider windows would not be read
      if (W & d) {  // wave-uniform
        ml = max_u64(ml, shfl_seg_u64_or0<S>(bl, seg0, pl));
        mr = max_u64(mr, shfl_seg_u64_or0<S>(br, seg0, pr));
        pl -= d;
        pr += d;
      }
      bl = max_u64(bl, shfl_seg_u64_or0<S>(bl, seg0, sub - d));
      br = max_u64(br, shfl_seg_u64_or0<S>(br, seg0, sub + d));
    }
    m = max_u64(ml, mr);
  }
  if (mine && sub < C) a.peak[mark_at(ta, p, sub)] = m == key ? 1 : 0;  // every key is unique
}

// work items w = pair * max_tiles + tile of the chunk; marks of the pairs of more than `seg` entries
__global__ __launch_bounds__(256) void targets_peaks_tile_kernel(TargetsPeaksArgs a, ProblemView pv, BatchView bv,
                                                                 int64_t n_pairs) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
  __shared__ int bparts[kBlock / 64];
  const TargetsArgs& ta = a.ta;
  const int tid = threadIdx.x;
  const int64_t total = n_pairs * a.max_tiles;
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {  // block-uniform
    const Pair p = pair_of(ta, pv, bv, w / a.max_tiles, n_pairs);
    const int t0 = static_cast<int>(w % a.max_tiles) * kTile;
    const int C = pair_count(p);
    if (C <= a.seg || C < 2 || t0 >= C) continue;  // block-uniform: the segment kernel's, unmarked, or no such tile
    const int R = min(a.radius, C - 1);  // beyond C - 1 the window is the pair's profile either way
    const int Tn = min(kTile, C - t0);
    const int E = Tn + 2 * R;            // keys[x] = the key of local offset lo + x
    const int lo = t0 - R;
    MOC_DCHECK(E > 0 && E <= kMaxKeys && E <= a.lds_keys);
    // the boundary entry's key, once per work item and only when [lo, lo + E) holds its offset (block-uniform)
    unsigned long long bkey = 0ull;
    if (p.boundary && p.slice >= lo && p.slice < lo + E) {
      int part = boundary_part(p, pv, tid, kBlock);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
      if ((tid & 63) == 0) bparts[tid >> 6] = part;
      __syncthreads();
      int bsum = 0;
#pragma unroll
      for (int q = 0; q < kBlock / 64; ++q) bsum += bparts[q];
      bkey = final_key(bsum, static_cast<uint32_t>(p.slice));
      __syncthreads();  // the next work item's stores to bparts come after these reads
    }
    auto key_of = [&](int o) {  // local offset o in [0, C)
      return o < p.slice ? final_key(slice_entry(ta, p, o).score, static_cast<uint32_t>(o)) : bkey;
    };
    unsigned long long own[kKeysPerThread];
#pragma unroll
    for (int q = 0; q < kKeysPerThread; ++q) {
      const int x = tid + kBlock * q;
      own[q] = 0;
      if (x < E) {
        const int o = lo + x;
        if (o >= 0 && o < C) own[q] = key_of(o);
        keys[x] = own[q];
      }
    }
    __syncthreads();
    // after the step with d: keys[x] = the maximum of keys [x, x + 2d) of the tile's range (absent ones count 0)
    const int W = 2 * R + 1;
    const int P = 1 << (31 - __clz(W));  // largest power of two <= W
    for (int d = 1; d < P; d <<= 1) {    // block-uniform
      unsigned long long other[kKeysPerThread];
#pragma unroll
      for (int q = 0; q < kKeysPerThread; ++q) {
        const int x = tid + kBlock * q;
        other[q] = x + d < E ? keys[x + d] : 0ull;
      }
      __syncthreads();  // every read of this step is done
#pragma unroll
      for (int q = 0; q < kKeysPerThread; ++q) {
        const int x = tid + kBlock * q;
        own[q] = max_u64(own[q], other[q]);
        if (x < E) keys[x] = own[q];
      }
      __syncthreads();
    }
    // local offset o = t0 + j sits at x = j + R; its window [x - R, x + R] = [j, j + P) and [j + W - P, j + W)
    for (int j = tid; j < Tn; j += kBlock) {
      MOC_DCHECK(j + W - P >= 0 && j + W - P < E);
      const unsigned long long m = max_u64(keys[j], keys[j + W - P]);
      const int o = t0 + j;
      a.peak[mark_at(ta, p, o)] = m == key_of(o) ? 1 : 0;
    }
    __syncthreads();  // the next work item's stores come after these reads
  }
}

// targets_topk_kernel over the peaks: an entry that is no peak has key 0, which no round picks; rounds past the
// pair's peaks store the empty row.
template <int G>
__global__ __launch_bounds__(256) void targets_topk_peaks_kernel(TargetsArgs ta, const uint8_t* __restrict__ peak, int K,
                                                                 ProblemView pv, BatchView bv, int64_t pair0,
                                                                 int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets rows: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  const int sub = threadIdx.x & (G - 1);
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G), n_pairs);
  // every lane of the wave reaches the shuffles (the loops are the only divergent parts)
  const int bsum = group_sum_i32<G>(boundary_part(p, pv, sub, G));
  const int C = pair_count(p);
  auto key_at = [&](int o) {  // o < slice
    return is_peak(ta, peak, p, C, o) ? final_key(slice_entry(ta, p, o).score, static_cast<uint32_t>(o)) : 0ull;
  };
  // the boundary entry's key: one more key of the lane the stride would give its offset to
  const unsigned long long bkey = p.boundary && sub == (p.slice & (G - 1)) && is_peak(ta, peak, p, C, p.slice)
                                      ? final_key(bsum, static_cast<uint32_t>(p.slice))
                                      : 0ull;
  unsigned long long held[kHeld];  // 0: no entry, or no peak (a real key is never 0: o < 2^31)
#pragma unroll
  for (int q = 0; q < kHeld; ++q) {
    const int o = sub + G * q;
    held[q] = o < p.slice ? key_at(o) : 0ull;
  }
  Result* out = ta.out + p.p * K;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < K; ++j) {  // K is wave-uniform
    unsigned long long m = 0ull;
    if (j < C && prev != 0ull) {  // group-uniform: at most min(K, C) rounds have a winner, none after an empty one
#pragma unroll
      for (int q = 0; q < kHeld; ++q) m = (j == 0 || held[q] < prev) ? max_u64(m, held[q]) : m;
      for (int o = sub + G * kHeld; o < p.slice; o += G) {
        const unsigned long long k = key_at(o);
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
__global__ __launch_bounds__(256) void targets_hits_count_peaks_kernel(TargetsHitsArgs ha, const uint8_t* __restrict__ peak,
                                                                       ProblemView pv, BatchView bv, int64_t pair0,
                                                                       int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets rows: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  const TargetsArgs& ta = ha.ta;
  const int sub = threadIdx.x & (G - 1);
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G), n_pairs);
  const int C = pair_count(p);
  const int thr = pair_threshold(ha, p);
  int count = 0;  // slice < 2^31
  for (int o = sub; o < p.slice; o += G) count += slice_entry(ta, p, o).score >= thr && is_peak(ta, peak, p, C, o) ? 1 : 0;
  // every lane of the wave reaches the shuffles
  const int bsum = group_sum_i32<G>(boundary_part(p, pv, sub, G));
  count = group_sum_i32<G>(count);
  if (p.active && sub == 0) {
    MOC_DCHECK(p.p >= 0 && p.p + 1 <= ta.view.n_total * ta.T);
    ha.toffsets[p.p + 1] = count + (p.boundary && bsum >= thr && is_peak(ta, peak, p, C, p.slice) ? 1 : 0);
    if (p.p == 0) ha.toffsets[0] = 0;
  }
}

template <int G>
__global__ __launch_bounds__(256) void targets_hits_compact_peaks_kernel(TargetsHitsArgs ha, const uint8_t* __restrict__ peak,
                                                                         ProblemView pv, BatchView bv, int64_t pair0,
                                                                         int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets rows: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  constexpr unsigned long long kGroupBits = G == 64 ? ~0ull : (1ull << G) - 1ull;
  const TargetsArgs& ta = ha.ta;
  const int sub = threadIdx.x & (G - 1);
  const int gfirst = (threadIdx.x & 63) & ~(G - 1);  // the group's first lane of the wave
  const Pair p = pair_of(ta, pv, bv, pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G), n_pairs);
  const int C = pair_count(p);
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
      hit = e.score >= thr && is_peak(ta, peak, p, C, o);
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
    if (p.boundary && bsum >= thr && is_peak(ta, peak, p, C, p.slice)) {  // the largest local offset: the pair's last row
      const int64_t at = out0 + base;
      MOC_DCHECK(at >= out0 && at + 1 == out1);
      if (at < ha.cap) ha.rows[at] = Result{bsum, p.slice, 0};
    } else {
      MOC_DCHECK(out0 + base == out1);
    }
  }
}

void preload_targets_peaks_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&targets_peaks_tile_kernel));
}

namespace {
template <int S>
void launch_seg_s(const TargetsPeaksArgs& a, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  const int64_t n_pairs = a.ta.view.n_rec * a.ta.T;
  for_each_launch<S>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_peaks_seg_kernel<S>), dim3(blocks), dim3(kBlock), 0, stream, a, pv, bv, pair0, n_pairs);
  });
}

template <int G>
void launch_topk_g(const TargetsArgs& ta, const uint8_t* peak, int K, const ProblemView& pv, const BatchView& bv,
                   hipStream_t stream) {
  const int64_t n_pairs = ta.view.n_rec * ta.T;
  for_each_launch<G>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_topk_peaks_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, ta, peak, K, pv, bv, pair0,
                       n_pairs);
  });
}

template <int G>
void launch_hits_g(const TargetsHitsArgs& ha, const uint8_t* peak, const ProblemView& pv, const BatchView& bv,
                   hipStream_t stream) {
  const int64_t n_pairs = ha.ta.view.n_rec * ha.ta.T;
  for_each_launch<G>(n_pairs, [&](unsigned blocks, int64_t pair0) {
    hipLaunchKernelGGL((targets_hits_count_peaks_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, ha, peak, pv, bv, pair0,
                       n_pairs);
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
    hipLaunchKernelGGL((targets_hits_compact_peaks_kernel<G>), dim3(blocks), dim3(kBlock), 0, stream, ha, peak, pv, bv,
                       pair0, n_pairs);
  });
}
}  // namespace

void launch_targets_peaks(const TargetsPeaksArgs& a, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  if (a.ta.view.n_rec <= 0 || a.ta.T <= 0 || a.radius <= 0) return;
  if (a.any_short) {
    switch (a.seg) {
      case 4: launch_seg_s<4>(a, pv, bv, stream); break;
      case 8: launch_seg_s<8>(a, pv, bv, stream); break;
      case 16: launch_seg_s<16>(a, pv, bv, stream); break;
      case 32: launch_seg_s<32>(a, pv, bv, stream); break;
      default: launch_seg_s<64>(a, pv, bv, stream); break;
    }
  }
  if (a.max_tiles > 0) {
    const int64_t n_pairs = a.ta.view.n_rec * a.ta.T;
    const int64_t total = n_pairs * a.max_tiles;
    const int64_t blocks = std::min<int64_t>(total, static_cast<int64_t>(std::max(a.num_cus, 1)) * 64);
    hipLaunchKernelGGL(targets_peaks_tile_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock),
                       sizeof(unsigned long long) * static_cast<size_t>(a.lds_keys), stream, a, pv, bv, n_pairs);
  }
}

void launch_targets_topk_peaks(const TargetsArgs& ta, const uint8_t* peak, int K, const ProblemView& pv,
                               const BatchView& bv, hipStream_t stream) {
  if (ta.view.n_rec <= 0 || ta.T <= 0) return;
  with_group(ta.group, [&](auto g) { launch_topk_g<g()>(ta, peak, K, pv, bv, stream); });
}

void launch_targets_hits_peaks(const TargetsHitsArgs& ha, const uint8_t* peak, const ProblemView& pv, const BatchView& bv,
                               hipStream_t stream) {
  if (ha.ta.view.n_rec <= 0 || ha.ta.T <= 0) return;
  with_group(ha.ta.group, [&](auto g) { launch_hits_g<g()>(ha, peak, pv, bv, stream); });
}

}  // namespace dev
}  // namespace moc
