// Multi-target search: every record's best alignment against each target of a catalog (gfx950, wave64).
// Definitions: moc/cpu_engine.hpp targets_batch_cpu; group sizes and cut-overs: moc/kernel_bounds.hpp.
//
// The kernel reads a chunk's catalog profile where hits_count_kernel reads it (prof[poffsets[r] - base + o], written
// by offset_profile_kernel just before on the same stream) and reduces, per (record, target) pair, the target's slice
// of it plus at most one un-mutated boundary diagonal to one row. No atomics on global memory, no kernel waits on
// another block, no LDS; ordering is launch order.
//   targets_select_kernel<G>  a group of G consecutive lanes (4, 16 or 64; aligned to G, so __shfl_xor steps below G
//                             stay inside it) owns pair p = li * T + t of the chunk (64-bit). The group strides over
//                             the slice's len_t - L2 entries keeping the largest order-free key (topk_select_kernel's
//                             final_key over the LOCAL offset, so the better() tie-break is top-K's), then — under the
//                             spec semantics or with len_t == L2 — over the record's L2 letters, summing
//                             LUT[s2[l]][Seq1[starts[t] + len_t - L2 + l]]; xor-shuffle reductions; the group's first
//                             lane re-reads the winning entry's k, merges the boundary entry (it has the largest
//                             offset: it wins only with a strictly higher score) and stores the row at
//                             out[(r - out_rec0) * T + t] — the batch's rows, or (the target ranking) the chunk's
//                             alone in the profile scratch behind the chunk's entries. Every lane of a
//                             wave reaches every shuffle: groups without a pair or with an empty slice carry key 0.
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
}  // namespace

// pairs [pair0, pair0 + gridDim.x * (kBlock / G)) of the chunk's n_pairs = n_rec * T
template <int G>
__global__ __launch_bounds__(256) void targets_select_kernel(TargetsArgs ta, ProblemView pv, BatchView bv, int64_t pair0,
                                                             int64_t n_pairs) {
  static_assert(G == 4 || G == 16 || G == 64, "targets: a group is 4, 16 or 64 lanes");
  constexpr int kGroupsPerBlock = kBlock / G;
  const int sub = threadIdx.x & (G - 1);
  const int64_t pair = pair0 + static_cast<int64_t>(blockIdx.x) * kGroupsPerBlock + (threadIdx.x / G);
  const bool active = pair < n_pairs;  // uniform over the group; an idle group still reaches every shuffle
  const int L1 = pv.L1;
  int64_t r = 0, pb = 0, b = 0;
  int t = 0, L2 = 0, len = 0;
  const uint8_t* rec = nullptr;
  if (active) {
    const int64_t li = pair / ta.T;
    t = static_cast<int>(pair - li * ta.T);
    r = ta.view.rec0 + li;
    MOC_DCHECK(li >= 0 && li < ta.view.n_rec && r >= 0 && r < bv.n && t >= 0 && t < ta.T);
    rec = bv.codes + (bv.offsets[r] - bv.offsets[0]);
    L2 = static_cast<int>(bv.offsets[r + 1] - bv.offsets[r]);
    b = ta.starts[t];
    len = static_cast<int>(ta.starts[t + 1] - b);
    pb = chunk_first(ta.view, r);
    MOC_DCHECK(b >= 0 && len >= 1 && b + len <= L1);
  }
  const bool fits = active && L2 >= 1 && L2 <= len && L2 <= L1;
  const int slice = fits ? len - L2 : 0;  // entries of the pair's slice; local offset of its boundary diagonal
  unsigned long long key = 0ull;          // 0: no entry (a real key is never 0: o < 2^31)
  for (int o = sub; o < slice; o += G) {
    const int64_t at = pb + b + o;
    MOC_DCHECK(b + o < chunk_count(ta.view, r));  // the slice lies inside the record's entries
    key = max_u64(key, final_key(ta.view.prof[at].score, static_cast<uint32_t>(o)));
  }
  const bool boundary = fits && (pv.semantics == static_cast<int>(Semantics::Spec) || slice == 0);
  int bsum = 0;
  if (boundary) {
    const int64_t a0 = b + slice;  // the diagonal's first Seq1 letter; its last is b + len - 1 < L1
    for (int l = sub; l < L2; l += G) {
      const int c = rec[l];
      MOC_DCHECK(c >= 0 && c < kLutStride);
      MOC_DCHECK(a0 + l >= 0 && a0 + l < L1);
      bsum += pv.lut[(c << 5) + pv.seq1[a0 + l]];
    }
  }
  // every lane of the wave reaches the shuffles (the two loops above are the only divergent parts)
  key = group_max_u64<G>(key);
  bsum = group_sum_i32<G>(bsum);
  if (active && sub == 0) {
    Result row{INT32_MIN, 0, 0};
    if (key != 0ull) {
      const int o = static_cast<int>(0xffffffffu - static_cast<uint32_t>(key));
      MOC_DCHECK(o >= 0 && o < slice);
      const int64_t at = pb + b + o;
      const ProfileEntry e = ta.view.prof[at];
      row = Result{e.score, o, e.k};
    }
    if (boundary && (key == 0ull || bsum > row.score)) row = Result{bsum, slice, 0};
    const int64_t at = (r - ta.out_rec0) * ta.T + t;  // 64-bit; out_rec0 is 0 or the chunk's first record
    MOC_DCHECK(at >= 0 && at < (ta.out_rec0 ? ta.view.n_rec : ta.view.n_total) * ta.T);
    ta.out[at] = row;
  }
}

void preload_targets_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&targets_select_kernel<4>));
}

namespace {
template <int G>
void launch_targets_g(const TargetsArgs& ta, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  constexpr int64_t kGroupsPerBlock = kBlock / G;
  const int64_t n_pairs = ta.view.n_rec * ta.T;
  for (int64_t pair0 = 0; pair0 < n_pairs;) {
    const int64_t blocks = std::min<int64_t>((n_pairs - pair0 + kGroupsPerBlock - 1) / kGroupsPerBlock, kMaxBlocksPerLaunch);
    hipLaunchKernelGGL((targets_select_kernel<G>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, ta, pv,
                       bv, pair0, n_pairs);
    pair0 += blocks * kGroupsPerBlock;
  }
}
}  // namespace

void launch_targets(const TargetsArgs& ta, const ProblemView& pv, const BatchView& bv, hipStream_t stream) {
  if (ta.view.n_rec <= 0 || ta.T <= 0) return;
  switch (ta.group) {
    case 4: launch_targets_g<4>(ta, pv, bv, stream); break;
    case 16: launch_targets_g<16>(ta, pv, bv, stream); break;
    default: launch_targets_g<64>(ta, pv, bv, stream); break;
  }
}

}  // namespace dev
}  // namespace moc
