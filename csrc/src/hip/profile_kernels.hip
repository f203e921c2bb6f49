// Per-offset score profile and top-K selection (gfx950, wave64).
//
// offset_profile_kernel keeps what the search kernels reduce away: every offset's own best candidate
// {score, k} (moc/cpu_engine.hpp: the maximum of score(o, 0) and score(o, k), k = 1..L2-1; ties -> k = 0, then
// the smallest k). Work decomposition and sweep are the LUT tile kernel's (align_kernels.hip): a wave tile =
// (record, 63·U consecutive offsets) as U sub-tiles of 63 owned offsets + 1 helper lane, persistent waves
// walking host-planned, cost-balanced runs of the record-major tile list — here over EVERY record of the
// batch, short ones as single tiles. Per lane (= one offset o) and Seq2 position i:
//     P  += LUT[Seq2[i]][Seq1[o+i]]
//     Pn  = P of lane+1                        (DPP wave_shl:1, the neighbouring diagonal)
//     d   = P - Pn;  if (d > bd) bd = d, bk = i+1     (strict: the smallest k wins ties)
// and at the end of the tile the lane stores its own candidate — Tot_o with k = 0, or bd + Tot_{o+1} with bk
// when that is strictly larger — to prof[poffsets[r] - base + o] with one 8-byte vector store. No cross-lane
// reduction, no atomics; the running best is two plain int32 registers, so the arithmetic is the CPU
// engine's for any weights.
//
// topk_select_kernel: one wave per record over that record's profile entries, K rounds of a wave maximum of
// the order-free key (score ^ 2^31) << 32 | (2^32 - 1 - o) over the keys strictly below the previous round's
// winner (the profile is read-only; every key is unique, so every round has one winner). A record whose
// profile fits the wave's lanes (C <= 64) is ranked in one pass instead — same rows.
#include <hip/hip_runtime.h>

#include "kernel_common.hpp"
#include "moc/runtime/hip_check.hpp"

namespace moc {
namespace dev {

using namespace kc;

template <bool Seq1Lds, int U>
__global__ __launch_bounds__(256) void offset_profile_kernel(ProblemView pv, BatchView bv, ProfileArgs pa) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* lut = reinterpret_cast<int*>(smem);
  uint8_t* s1l = smem + kLutInts * sizeof(int);
  const int L1 = pv.L1;
  stage_lut(lut, pv.lut);
  if (Seq1Lds) stage_bytes(s1l, pv.seq1, L1 + kSeq1Pad);
  __syncthreads();
  const int64_t w = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= pa.n_waves) return;  // wave-uniform; no barrier follows
  const uint8_t* s1 = Seq1Lds ? s1l : pv.seq1;
  const int s1_last = L1 + kSeq1Pad - 1;

  const int lane = threadIdx.x & 63;
  constexpr int kSpan = kTileOffsets * U;  // offsets per wave tile

  const WaveStart ws = pa.starts[w], we = pa.starts[w + 1];
  int li = __builtin_amdgcn_readfirstlane(ws.li), t = __builtin_amdgcn_readfirstlane(ws.t);
  const int end_li = __builtin_amdgcn_readfirstlane(we.li), end_t = __builtin_amdgcn_readfirstlane(we.t);
  while (li < end_li || (li == end_li && t < end_t)) {  // wave-uniform
    // ---- one record of the chunk: its first letters stay in a register across the run's tiles of it
    const int64_t r = pa.view.rec0 + li;
    MOC_DCHECK(r >= 0 && r < bv.n);
    const uint8_t* rec = bv.codes + (bv.offsets[r] - bv.offsets[0]);
    const int L2 = __builtin_amdgcn_readfirstlane(static_cast<int>(bv.offsets[r + 1] - bv.offsets[r]));
    const int64_t pbase = chunk_first(pa.view, r);
    const int C = __builtin_amdgcn_readfirstlane(chunk_count(pa.view, r));
    const int steps = L2 <= L1 ? L2 : 0;
    const int need = L2 <= L1 ? L1 - L2 + 1 : 1;
    const int ntiles = (need + kSpan - 1) / kSpan;
    const int t_stop = li == end_li ? min(end_t, ntiles) : ntiles;
    const int last = L1 - L2;  // mutated candidates exist at o < last
    const int cv_first = lane < steps ? static_cast<int>(rec[lane]) : 0;
    for (; t < t_stop; ++t) {
      const int o0 = t * kSpan;
      MOC_DCHECK(o0 >= 0 && o0 <= L1);
      // sub-tile u: lanes 0..62 own offsets o0 + 63u + lane, lane 63 is its helper diagonal
      int x[U], P[U], bd[U], bk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        MOC_DCHECK(o0 + kTileOffsets * u + lane >= 0);
        x[u] = s1[min(o0 + kTileOffsets * u + lane, s1_last)];
        P[u] = 0;
        bd[u] = INT32_MIN;
        bk[u] = 0;
      }
      // Seq2 letters and the helper lanes' Seq1 feeds arrive 64 steps at a time as one coalesced load per
      // wave (lane j holds step j's value), each step pulls its values out with v_readlane
      auto step = [&](int cv, const int (&fv)[U], int j, int k, bool key) {
        const int c = __builtin_amdgcn_readlane(cv, j);
        const int* row = lut + (c << 5);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          P[u] += row[x[u]];
          if (key) {
            const int d = P[u] - wave_shl1(P[u]);
            const bool up = d > bd[u];
            bd[u] = up ? d : bd[u];
            bk[u] = up ? k : bk[u];
            x[u] = wave_shl1_fill(x[u], __builtin_amdgcn_readlane(fv[u], j));
          }
        }
      };
      int cv = cv_first;
      int i0 = 0;
      for (; i0 + 64 < steps; i0 += 64) {  // full chunks (the record's last letter lies beyond)
        const int cv_next = i0 + 64 + lane < steps ? static_cast<int>(rec[i0 + 64 + lane]) : 0;
        int fv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) fv[u] = s1[min(o0 + kTileOffsets * u + 64 + i0 + lane, s1_last)];
#pragma unroll 8
        for (int j = 0; j < 64; ++j) step(cv, fv, j, i0 + j + 1, true);
        cv = cv_next;
      }
      if (steps > 0) {  // last chunk: 1..64 steps; no hyphen after the final letter
        const int m = steps - i0;
        int fv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) fv[u] = s1[min(o0 + kTileOffsets * u + 64 + i0 + lane, s1_last)];
        for (int j = 0; j < m - 1; ++j) step(cv, fv, j, i0 + j + 1, true);
        step(cv, fv, m - 1, 0, false);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int o = o0 + kTileOffsets * u + lane;
        const int Pn = wave_shl1(P[u]);  // Tot_{o+1}
        if (lane < kTileOffsets && o < C) {  // C = 0 for L2 > L1; o < C makes score(o, 0) a candidate
          ProfileEntry e{P[u], 0};
          if (o < last && L2 >= 2 && bd[u] + Pn > e.score) e = ProfileEntry{bd[u] + Pn, bk[u]};
          pa.prof[pbase + o] = e;
        }
      }
    }
    ++li;
    t = 0;
  }
}

// One wave per record r = rec0 + li of a chunk whose profile lies at prof[poffsets[r] - base ..): K rounds,
// round j's winner -> out[r * K + j] = (score, o, k of that offset); rounds past the record's C entries pad
// with no_candidate(). A lane keeps its first four keys in registers (C <= 256 reads the profile once). Records
// with C <= 64 take no rounds: a lane per entry ranks its key against the others (same rows).
__global__ __launch_bounds__(256) void topk_select_kernel(ChunkView v, int K, Result* __restrict__ out) {
  const int64_t li = static_cast<int64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (li >= v.n_rec) return;
  const int lane = threadIdx.x & 63;
  const int64_t r = v.rec0 + li;
  const ProfileEntry* __restrict__ e = v.prof + chunk_first(v, r);
  const int C = __builtin_amdgcn_readfirstlane(chunk_count(v, r));
  auto key_at = [&](int o) {
    return final_key(e[o].score, static_cast<uint32_t>(o));  // never 0: o < 2^31
  };
  if (C <= 64) {
    // a lane per entry (the short-record regime: K rounds of wave reductions would cost more than the profile
    // itself): every key is unique, so the number of larger keys is the entry's row — the same rows as the
    // rounds below give
    const unsigned long long key = lane < C ? key_at(lane) : 0ull;
    const uint32_t lo = static_cast<uint32_t>(key), hi = static_cast<uint32_t>(key >> 32);
    int rank = 0;
    for (int i = 0; i < C; ++i) {  // wave-uniform i: two v_readlane per entry
      const uint32_t ohi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hi), i));
      const uint32_t olo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lo), i));
      const unsigned long long other = (static_cast<unsigned long long>(ohi) << 32) | olo;
      rank += other > key ? 1 : 0;
    }
    if (lane < C && rank < K) out[r * K + rank] = Result{e[lane].score, lane, e[lane].k};
    if (lane >= C && lane < K) out[r * K + lane] = Result{INT32_MIN, 0, 0};  // K <= 64 lanes: rows C .. K-1
    return;
  }
  constexpr int kHeld = 4;
  unsigned long long held[kHeld];
#pragma unroll
  for (int q = 0; q < kHeld; ++q) held[q] = lane + 64 * q < C ? key_at(lane + 64 * q) : 0ull;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < K; ++j) {
    unsigned long long m = 0;
    if (j < C) {  // wave-uniform: min(K, C) rounds have a winner
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

void preload_profile_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&topk_select_kernel));
}

namespace {
constexpr int kBlock = 256;
constexpr int kMaxSeq1Lds = 56 * 1024;  // Seq1 staged in LDS up to this size (keeps dyn. LDS < 64 KiB)

template <int U>
void launch_profile_u(const ProblemView& pv, const BatchView& bv, const ProfileArgs& pa, hipStream_t stream) {
  const size_t lds_lut = kLutInts * sizeof(int);
  const size_t lds_s1 = static_cast<size_t>(pv.L1 + kSeq1Pad + 3) & ~size_t{3};
  const int64_t blocks = (pa.n_waves * 64 + kBlock - 1) / kBlock;
  if (pv.L1 + kSeq1Pad <= kMaxSeq1Lds)
    hipLaunchKernelGGL((offset_profile_kernel<true, U>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock),
                       lds_lut + lds_s1, stream, pv, bv, pa);
  else
    hipLaunchKernelGGL((offset_profile_kernel<false, U>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), lds_lut,
                       stream, pv, bv, pa);
}
}  // namespace

void launch_offset_profile(const ProblemView& pv, const BatchView& bv, const ProfileArgs& pa, hipStream_t stream) {
  if (pa.n_waves <= 0) return;
  switch (pa.u) {
    case 1: launch_profile_u<1>(pv, bv, pa, stream); break;
    case 4: launch_profile_u<4>(pv, bv, pa, stream); break;
    default: launch_profile_u<2>(pv, bv, pa, stream); break;
  }
}

void launch_topk_select(const ChunkView& view, int K, Result* out, hipStream_t stream) {
  if (view.n_rec <= 0) return;
  const int64_t blocks = (view.n_rec + 3) / 4;
  hipLaunchKernelGGL(topk_select_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, view, K, out);
}

}  // namespace dev
}  // namespace moc
