// Clipped n-gram statistics of BLEU over integer sequences (dn_bleu_stats).  Definitions and the reference lines they replace:
// include/diffnorm_hip.h.
//   bleu_stats_kernel  ONE WORKGROUP PER PAIR.  The hypothesis's and the reference's tokens are staged in LDS one behind the other, so
//                     that position p of the joint row (p < hyp_len: the hypothesis's, otherwise the reference's) starts the n-gram
//                     tok[p .. p + n) and has rem(p) = (end of its side) - p tokens left.  The N = hyp_len + ref_len positions are
//                     sorted ONCE (bitonic network over 16-bit position indices in LDS, padded to the next power of two with an
//                     index that sorts last) by their 4-token key, compared lexicographically token by token as signed integers,
//                     a position with fewer than 4 tokens left carrying a below-every-token mark in the missing places.  In that
//                     one order the positions whose n-grams are equal are contiguous for every n <= 4 (they share an n-prefix, and
//                     nothing with another n-prefix sorts between them), and a position that has no n-gram (rem < n) carries the
//                     mark inside its n-prefix, so it never lies inside a run of real ones.  One pass then serves all four orders:
//                     every thread walks a contiguous chunk of the sorted positions, knows for each how many leading key places it
//                     shares with its predecessor (a new run of order n starts where fewer than n are shared) and keeps, per order,
//                     the counts of hypothesis / reference positions of the run that is open: a run that closes adds
//                     min(hypothesis count, reference count) to match_n.  A chunk's leading and trailing part-runs are joined by an
//                     associative combine of per-thread summaries (wave: 6 lane-shift steps; workgroup: the waves' summaries in LDS,
//                     folded in order by one thread per order).
// Integer arithmetic, full comparisons of the tokens (no hash), no atomics: a pair's ten numbers depend on its own tokens and lengths
// only -- not on B, the pair's place, the leading dimensions (which set the workgroup's size and LDS, not a count) or the padding.
#include "common.h"
#include "engine.h"

using namespace dn;

namespace dn {
namespace {

constexpr int BL_MAX_LEN = DN_EDIT_DISTANCE_MAX_LEN;  // 8192 tokens a side: 16384 positions, 16-bit indices
constexpr int BL_ORDER = DN_BLEU_ORDER;
constexpr int BL_THREADS_MAX = 1024;
constexpr int BL_PAD = 0xffff;  // index of the network's padding: no position (N <= 16384), sorts behind every position

// a key place as one unsigned number: 0 = no token there, otherwise 1 + the token's rank among all int32 values
__device__ __forceinline__ uint64_t bl_place(const int32_t* tok, int p, int k, int rem) {
  return k < rem ? (uint64_t)((uint32_t)tok[p + k] ^ 0x80000000u) + 1u : 0u;
}

__device__ __forceinline__ int bl_rem(int p, int hl, int N) { return (p < hl ? hl : N) - p; }

// key(a) > key(b); the padding is above every position and equal to itself
__device__ __forceinline__ bool bl_greater(const int32_t* tok, int a, int b, int hl, int N) {
  if (a == BL_PAD || b == BL_PAD) return a == BL_PAD && b != BL_PAD;
  const int ra = bl_rem(a, hl, N), rb = bl_rem(b, hl, N);
#pragma unroll
  for (int k = 0; k < BL_ORDER; ++k) {
    const uint64_t x = bl_place(tok, a, k, ra), y = bl_place(tok, b, k, rb);
    if (x != y) return x > y;
    if (x == 0) return false;  // both rows ended: the remaining places are equal
  }
  return false;
}

// What a stretch of the sorted order knows about one order n: the counts (hypothesis | reference << 16) before its first run start
// (all of them when it has none), the matches of the runs that start and end inside it, and the counts of the run still open.
struct BlSum {
  int head, pre, match, open;
};
__device__ __forceinline__ int bl_min2(int packed) { return min(packed & 0xffff, packed >> 16); }
// a = a followed by b
__device__ __forceinline__ void bl_combine(BlSum& a, const BlSum& b) {
  if (!b.head) {
    if (a.head) a.open += b.pre;
    else a.pre += b.pre;
  } else if (a.head) {
    a.match += b.match + bl_min2(a.open + b.pre);
    a.open = b.open;
  } else {
    a.pre += b.pre;
    a.match = b.match;
    a.open = b.open;
    a.head = 1;
  }
}

__global__ __launch_bounds__(BL_THREADS_MAX) void bleu_stats_kernel(const int32_t* __restrict__ hyp, int ld_hyp, const int32_t* __restrict__ hyp_len,
                                                                    const int32_t* __restrict__ ref, int ld_ref, const int32_t* __restrict__ ref_len,
                                                                    int32_t* __restrict__ stats) {
  extern __shared__ int32_t bl_lds[];
  __shared__ BlSum wave_sum[BL_THREADS_MAX / 64][BL_ORDER];
  const int pair = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
  int hl = hyp_len[pair], rl = ref_len[pair];
  hl = hl < 0 ? 0 : hl > ld_hyp ? ld_hyp : hl;
  rl = rl < 0 ? 0 : rl > ld_ref ? ld_ref : rl;
  const int N = hl + rl;  // <= ld_hyp + ld_ref
  int P = 1;              // the network's width
  while (P < N) P <<= 1;  // <= the power of two the host sized the index array for
  int32_t* tok = bl_lds;
  uint16_t* idx = reinterpret_cast<uint16_t*>(bl_lds + ld_hyp + ld_ref);
  const int32_t* ph = hyp + (int64_t)pair * ld_hyp;
  const int32_t* pr = ref + (int64_t)pair * ld_ref;
  for (int i = tid; i < hl; i += nthreads) tok[i] = ph[i];
  for (int i = tid; i < rl; i += nthreads) tok[hl + i] = pr[i];
  for (int i = tid; i < P; i += nthreads) idx[i] = (uint16_t)(i < N ? i : BL_PAD);
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += nthreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const int a = idx[lo], b = idx[hi];
        const bool up = (lo & k) == 0;
        if (up ? bl_greater(tok, a, b, hl, N) : bl_greater(tok, b, a, hl, N)) {
          idx[lo] = (uint16_t)b;
          idx[hi] = (uint16_t)a;
        }
      }
      __syncthreads();
    }
  }
  // the thread's chunk of the sorted positions
  const int chunk = (N + nthreads - 1) / nthreads;
  const int c0 = min(tid * chunk, N), c1 = min(c0 + chunk, N);
  BlSum sum[BL_ORDER];
#pragma unroll
  for (int n = 0; n < BL_ORDER; ++n) sum[n] = BlSum{0, 0, 0, 0};
  uint64_t prev[BL_ORDER] = {0, 0, 0, 0};
  if (c0 > 0 && c0 < c1) {
    const int p = idx[c0 - 1], rem = bl_rem(p, hl, N);
#pragma unroll
    for (int k = 0; k < BL_ORDER; ++k) prev[k] = bl_place(tok, p, k, rem);
  }
  for (int i = c0; i < c1; ++i) {
    const int p = idx[i], rem = bl_rem(p, hl, N);
    const int add = p < hl ? 1 : 0x10000;
    uint64_t cur[BL_ORDER];
    int shared = 0;  // leading key places equal to the predecessor's
    bool same = i > 0;
#pragma unroll
    for (int k = 0; k < BL_ORDER; ++k) {
      cur[k] = bl_place(tok, p, k, rem);
      same = same && cur[k] == prev[k];
      shared += same ? 1 : 0;
      prev[k] = cur[k];
    }
#pragma unroll
    for (int n = 0; n < BL_ORDER; ++n) {
      if (rem > n) {           // the position has an (n + 1)-gram
        if (shared <= n) {     // and it is not its predecessor's: a run starts
          if (sum[n].head) sum[n].match += bl_min2(sum[n].open);
          sum[n].head = 1;
          sum[n].open = 0;
        }
        if (sum[n].head) sum[n].open += add;
        else sum[n].pre += add;
      }
    }
  }
  // wave: lane l <- lanes l .. l + 2 off - 1, in order
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int n = 0; n < BL_ORDER; ++n) {
    for (int off = 1; off < 64; off <<= 1) {
      BlSum o;
      o.head = __shfl_down(sum[n].head, off);
      o.pre = __shfl_down(sum[n].pre, off);
      o.match = __shfl_down(sum[n].match, off);
      o.open = __shfl_down(sum[n].open, off);
      if (lane + off < 64) bl_combine(sum[n], o);
    }
    if (lane == 0) wave_sum[wave][n] = sum[n];
  }
  __syncthreads();
  if (tid < BL_ORDER) {
    BlSum s = wave_sum[0][tid];
    for (int w = 1; w < (nthreads >> 6); ++w) bl_combine(s, wave_sum[w][tid]);
    int32_t* out = stats + (int64_t)pair * DN_BLEU_STATS;
    out[2 + 2 * tid] = bl_min2(s.pre) + s.match + (s.head ? bl_min2(s.open) : 0);
    out[3 + 2 * tid] = hl > tid ? hl - tid : 0;
    if (tid == 0) {
      out[0] = hl;
      out[1] = rl;
    }
  }
}

inline int bl_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace
}  // namespace dn

// One path covers every pair (tokens and indices of 8192 + 8192 take 96 KiB of the CU's 160 KiB of LDS): the workspace is a token.
extern "C" size_t dn_bleu_stats_workspace_bytes(int32_t B, int32_t ld_hyp, int32_t ld_ref) {
  if (B <= 0 || ld_hyp < 1 || ld_ref < 1 || ld_hyp > BL_MAX_LEN || ld_ref > BL_MAX_LEN) return 0;
  return 16;
}

extern "C" int dn_bleu_stats(const int32_t* hyp, int32_t ld_hyp, const int32_t* hyp_len, const int32_t* ref, int32_t ld_ref, const int32_t* ref_len,
                             int32_t B, int32_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(hyp && hyp_len && ref && ref_len && stats, "dn_bleu_stats: null argument");
  DN_CHECK_ARG(B > 0, "dn_bleu_stats: B=%d (at least 1)", B);
  DN_CHECK_ARG(ld_hyp >= 1 && ld_hyp <= BL_MAX_LEN, "dn_bleu_stats: ld_hyp=%d: rows of hyp hold 1 .. %d tokens", ld_hyp, BL_MAX_LEN);
  DN_CHECK_ARG(ld_ref >= 1 && ld_ref <= BL_MAX_LEN, "dn_bleu_stats: ld_ref=%d: rows of ref hold 1 .. %d tokens", ld_ref, BL_MAX_LEN);
  const size_t need = dn_bleu_stats_workspace_bytes(B, ld_hyp, ld_ref);
  DN_CHECK_ARG(workspace != nullptr && workspace_bytes >= need, "dn_bleu_stats: workspace of %zu bytes, dn_bleu_stats_workspace_bytes(B, ld_hyp, ld_ref) = %zu",
               workspace_bytes, need);
  const int width = bl_pow2(ld_hyp + ld_ref);  // the widest network a pair of this batch can need
  // 8 compare-exchanges per thread and step at most; whole waves
  const int threads = width / 16 < 64 ? 64 : width / 16 > BL_THREADS_MAX ? BL_THREADS_MAX : width / 16;
  const size_t lds = (size_t)(ld_hyp + ld_ref) * sizeof(int32_t) + (size_t)width * sizeof(uint16_t);  // <= 96 KiB
  // once (thread-safe static): the dynamic LDS may go beyond the 64 KiB a launch gets unasked
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(bleu_stats_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     2 * BL_MAX_LEN * (int)(sizeof(int32_t) + sizeof(uint16_t)));
  if (attr != hipSuccess) {
    dn_set_error("dn_bleu_stats: %zu bytes of LDS refused: %s", lds, hipGetErrorString(attr));
    return DN_ELAUNCH;
  }
  hipLaunchKernelGGL(bleu_stats_kernel, dim3(B), dim3(threads), lds, (hipStream_t)stream, hyp, ld_hyp, hyp_len, ref, ld_ref, ref_len, stats);
  DN_CHECK_LAUNCH("dn_bleu_stats");
  return DN_OK;
}
