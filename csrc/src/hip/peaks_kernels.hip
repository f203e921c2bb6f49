// Distinct placements: the peak filter between the profile kernel and the select / hits kernels, and the masked
// forms of those (gfx950, wave64). Definitions: moc/cpu_engine.hpp peaks_filter; geometry: moc/kernel_bounds.hpp.
//
// Entry o of a record's profile is a peak of radius R iff its order-free key (score ^ 2^31) << 32 | (2^32 - 1 - o)
// is the maximum of the keys in [o - R, o + R] clipped to the record: local-maximum suppression, every entry from
// its own window, so there is no ordering between entries, no atomics, nothing waits on another block, and no state
// crosses a chunk (chunks are whole records). The kernels read a chunk's profile where topk_select_kernel reads it
// (prof[poffsets[r] - base + o], written by offset_profile_kernel just before on the same stream), never alter it,
// and store one byte per entry, peak[poffsets[r] - base + o] = 1 or 0 — every entry of the chunk is stored.
//   peaks_wave_kernel   records of 1 .. kPeaksWaveEntries entries: one wave per record, a lane per entry. The
//                       window maximum is a left and a right half, each put together from power-of-two windows
//                       (log-step shifts; a lane past either end of the wave contributes nothing); R >= 63 is the
//                       wave maximum.
//   peaks_tile_kernel   longer records: a workgroup per tile of kPeaksTile entries. The tile and a halo of
//                       min(R, C - 1) entries on each side go to LDS as keys (0 outside the record), log2 steps
//                       of F[x] = max(F[x], F[x + d]) turn them into maxima of 2^p consecutive keys, 2^p the
//                       largest power of two <= 2R + 1 (a thread keeps its own keys in registers; a barrier
//                       between every read and write phase), and two overlapping such windows cover [o - R, o + R].
//   topk_select_peaks_kernel / hits_count_peaks_kernel / hits_compact_peaks_kernel
//                       topk_select_kernel, hits_count_kernel and hits_compact_kernel over the peaks only. The
//                       unmasked kernels and their code objects are untouched; the prefix sum between count and
//                       compaction is theirs (launch_hits_scan).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernel_common.hpp"
#include "moc/kernel_bounds.hpp"
#include "moc/runtime/hip_check.hpp"

namespace moc {
namespace dev {

using namespace kc;

namespace {
constexpr int kBlock = bounds::kPeaksThreads;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kTile = bounds::kPeaksTile;
constexpr int kKeysPerThread = bounds::kPeaksKeysPerThread;
constexpr int kMaxKeys = kTile + 2 * bounds::kPeaksMaxRadius;

// v of lane `src`, or 0 when src is no lane of the wave
__device__ __forceinline__ unsigned long long shfl_u64_or0(unsigned long long v, int src) {
  const int s = src & 63;
  const int lo = __shfl(static_cast<int>(v), s, 64);
  const int hi = __shfl(static_cast<int>(v >> 32), s, 64);
  const unsigned long long r = (static_cast<unsigned long long>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo);
  return src >= 0 && src < 64 ? r : 0ull;
}
}  // namespace

__global__ __launch_bounds__(256) void peaks_wave_kernel(PeaksArgs a) {
  const int64_t li = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (li >= a.view.n_rec) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int64_t r = a.view.rec0 + li;
  const int64_t pb = chunk_first(a.view, r);
  const int C = __builtin_amdgcn_readfirstlane(chunk_count(a.view, r));
  if (C <= 0 || C > bounds::kPeaksWaveEntries) return;  // wave-uniform: none, or the tile kernel's
  unsigned long long key = 0;  // lanes past the record hold 0, the maximum's identity (a key is never 0)
  if (lane < C) {
    key = final_key(a.view.prof[pb + lane].score, static_cast<uint32_t>(lane));
  }
  unsigned long long m;
  if (a.radius >= 63) {  // wave-uniform: the window is the record
    m = wave_max_u64(key);
  } else {
    // bl / br: the maximum of the 2^p keys ending / starting at this lane. The R + 1 keys ending (starting) here
    // are the windows of R + 1's set bits, laid end to end from this lane leftwards (rightwards).
    const int W = a.radius + 1;  // 2 .. 63
    unsigned long long bl = key, br = key, ml = 0, mr = 0;
    int pl = lane, pr = lane;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      if (W & d) {  // wave-uniform
        ml = max_u64(ml, shfl_u64_or0(bl, pl));
        mr = max_u64(mr, shfl_u64_or0(br, pr));
        pl -= d;
        pr += d;
      }
      bl = max_u64(bl, shfl_u64_or0(bl, lane - d));
      br = max_u64(br, shfl_u64_or0(br, lane + d));
    }
    m = max_u64(ml, mr);
  }
  if (lane < C) a.peak[pb + lane] = m == key ? 1 : 0;  // every key is unique: the maximum is this entry or another
}

__global__ __launch_bounds__(256) void peaks_tile_kernel(PeaksArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
  const int tid = threadIdx.x;
  const int64_t total = a.view.n_rec * a.max_tiles;
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {  // block-uniform
    const int64_t li = w / a.max_tiles;
    const int t0 = static_cast<int>(w % a.max_tiles) * kTile;
    const int64_t r = a.view.rec0 + li;
    const int64_t pb = chunk_first(a.view, r);
    const int C = chunk_count(a.view, r);
    if (C <= bounds::kPeaksWaveEntries || t0 >= C) continue;  // block-uniform: the wave kernel's, or no such tile
    const int R = min(a.radius, C - 1);  // beyond C - 1 the window is the record either way
    const int Tn = min(kTile, C - t0);
    const int E = Tn + 2 * R;            // keys[x] = the key of offset lo + x
    const int lo = t0 - R;
    MOC_DCHECK(E > 0 && E <= kMaxKeys && E <= a.lds_keys);
    unsigned long long own[kKeysPerThread];
#pragma unroll
    for (int q = 0; q < kKeysPerThread; ++q) {
      const int x = tid + kBlock * q;
      own[q] = 0;
      if (x < E) {
        const int o = lo + x;
        if (o >= 0 && o < C) {
          own[q] = final_key(a.view.prof[pb + o].score, static_cast<uint32_t>(o));
        }
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
    // offset o = t0 + j sits at x = j + R; its window [x - R, x + R] = [j, j + P) and [j + W - P, j + W)
    for (int j = tid; j < Tn; j += kBlock) {
      MOC_DCHECK(j + W - P >= 0 && j + W - P < E);
      const unsigned long long m = max_u64(keys[j], keys[j + W - P]);
      const int o = t0 + j;
      a.peak[pb + o] = m == final_key(a.view.prof[pb + o].score, static_cast<uint32_t>(o)) ? 1 : 0;
    }
    __syncthreads();  // the next tile's stores come after these reads
  }
}

// topk_select_kernel over the peaks: an entry that is no peak has key 0, which no round picks.
__global__ __launch_bounds__(256) void topk_select_peaks_kernel(ChunkView v, const uint8_t* __restrict__ peak, int K,
                                                                Result* __restrict__ out) {
  const int64_t li = static_cast<int64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (li >= v.n_rec) return;
  const int lane = threadIdx.x & 63;
  const int64_t r = v.rec0 + li;
  const ProfileEntry* __restrict__ e = v.prof + chunk_first(v, r);
  const uint8_t* pk = peak + chunk_first(v, r);
  const int C = __builtin_amdgcn_readfirstlane(chunk_count(v, r));
  auto key_at = [&](int o) { return pk[o] ? final_key(e[o].score, static_cast<uint32_t>(o)) : 0ull; };
  if (C <= 64) {
    // a lane per entry: the number of larger keys is a peak's row; rows #peaks .. K-1 are padding
    const unsigned long long key = lane < C ? key_at(lane) : 0ull;
    const uint32_t lo = static_cast<uint32_t>(key), hi = static_cast<uint32_t>(key >> 32);
    const int peaks = __popcll(__builtin_amdgcn_ballot_w64(key != 0ull));
    int rank = 0;
    for (int i = 0; i < C; ++i) {  // wave-uniform i: two v_readlane per entry
      const uint32_t ohi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hi), i));
      const uint32_t olo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lo), i));
      const unsigned long long other = (static_cast<unsigned long long>(ohi) << 32) | olo;
      rank += other > key ? 1 : 0;
    }
    MOC_DCHECK(key == 0ull || rank < peaks);
    if (key != 0ull && rank < K) out[r * K + rank] = Result{e[lane].score, lane, e[lane].k};
    if (lane >= peaks && lane < K) out[r * K + lane] = Result{INT32_MIN, 0, 0};  // K <= 64 lanes
    return;
  }
  constexpr int kHeld = 4;
  unsigned long long held[kHeld];
#pragma unroll
  for (int q = 0; q < kHeld; ++q) held[q] = lane + 64 * q < C ? key_at(lane + 64 * q) : 0ull;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < K; ++j) {
    unsigned long long m = 0;
    if (j < C && prev != 0ull) {  // wave-uniform: a round without a winner ends the peaks
#pragma unroll
      for (int q = 0; q < kHeld; ++q) m = (j == 0 || held[q] < prev) ? max_u64(m, held[q]) : m;
      for (int o = lane + 64 * kHeld; o < C; o += 64) {
        const unsigned long long k = key_at(o);
        m = (j == 0 || k < prev) ? max_u64(m, k) : m;
      }
      m = wave_max_u64(m);
    }
    if (lane == 0) {
      Result row{INT32_MIN, 0, 0};
      if (m != 0ull) {
        const int o = static_cast<int>(0xffffffffu - static_cast<uint32_t>(m));
        MOC_DCHECK(o >= 0 && o < C);
        row = Result{e[o].score, o, e[o].k};
      }
      out[r * K + j] = row;
    }
    prev = m;
  }
}

// hits_count_kernel over the peaks
__global__ __launch_bounds__(256) void hits_count_peaks_kernel(HitsArgs ha, const uint8_t* __restrict__ peak) {
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
      hit = peak[pb + o] != 0 && ha.view.prof[pb + o].score >= t;
    }
    count += __popcll(__builtin_amdgcn_ballot_w64(hit));
  }
  if (lane == 0) {
    ha.hoffsets[r + 1] = count;
    if (r == 0) ha.hoffsets[0] = 0;
  }
}

// hits_compact_kernel over the peaks
__global__ __launch_bounds__(256) void hits_compact_peaks_kernel(HitsArgs ha, const uint8_t* __restrict__ peak) {
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
      hit = peak[pb + o] != 0 && e.score >= t;
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
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

void preload_peaks_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&peaks_wave_kernel));
}

void launch_peaks(const PeaksArgs& a, hipStream_t stream) {
  if (a.view.n_rec <= 0 || a.radius <= 0) return;
  if (a.any_short) {
    const unsigned blocks = static_cast<unsigned>((a.view.n_rec + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(peaks_wave_kernel, dim3(blocks), dim3(kBlock), 0, stream, a);
  }
  if (a.max_tiles > 0) {
    const int64_t total = a.view.n_rec * a.max_tiles;
    const int64_t blocks = std::min<int64_t>(total, static_cast<int64_t>(std::max(a.num_cus, 1)) * 64);
    hipLaunchKernelGGL(peaks_tile_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock),
                       sizeof(unsigned long long) * static_cast<size_t>(a.lds_keys), stream, a);
  }
}

void launch_topk_select_peaks(const ChunkView& view, const uint8_t* peak, int K, Result* out, hipStream_t stream) {
  if (view.n_rec <= 0) return;
  const int64_t blocks = (view.n_rec + 3) / 4;
  hipLaunchKernelGGL(topk_select_peaks_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, view, peak,
                     K, out);
}

void launch_hits_peaks(const HitsArgs& ha, const uint8_t* peak, hipStream_t stream) {
  if (ha.view.n_rec <= 0) return;
  const unsigned wave_blocks = static_cast<unsigned>((ha.view.n_rec + kWavesPerBlock - 1) / kWavesPerBlock);
  hipLaunchKernelGGL(hits_count_peaks_kernel, dim3(wave_blocks), dim3(kBlock), 0, stream, ha, peak);
  launch_hits_scan(ha, stream);
  if (ha.cap > 0 && ha.rows)
    hipLaunchKernelGGL(hits_compact_peaks_kernel, dim3(wave_blocks), dim3(kBlock), 0, stream, ha, peak);
}

}  // namespace dev
}  // namespace moc
