// Scores over integer sequences: batched unit-cost Levenshtein distance (dn_edit_distance) and batched run-length de-duplication
// (dn_reduce_units).  Definitions and the reference lines they replace: include/diffnorm_hip.h.
//   edit_distance_kernel  ONE WAVEFRONT PER PAIR, ED_WAVES_MAX pairs per workgroup at most.  Both sequences are staged in LDS once; the
//                     shorter one becomes the columns (the distance is symmetric).  The columns are swept in panels of `panel`
//                     (at most 2048) columns; inside a panel lane l owns the strip of w = ceil(panel columns / 64) consecutive
//                     columns l w + 1 .. l w + w and keeps the previous row's values of its strip and the strip's tokens in
//                     registers.  The rows sweep through the lanes skewed by one step per lane: at step t lane l computes row
//                     t - l + 1, whose left neighbour D[row][l w] lane l - 1 produced one step earlier and hands over with one
//                     DPP wave shift (no LDS, no memory); the diagonal D[row - 1][l w] is the value it received the step before.
//                     The row's token comes from the LDS copy (lanes read consecutive words).  A pair whose shorter side fits one
//                     panel never touches memory between its loads and its one store.  A longer pair (both sides above the panel)
//                     writes each panel's last column -- one value per row, by lane 63 -- to a row of the workspace and the next
//                     panel's lane 0 reads it back 64 rows at a time (one coalesced load per 64 steps, then v_readlane); the two
//                     rows of the workspace alternate, and a fence separates a panel's stores from the next one's loads.
//                     Cells right of the pair's last column are computed and never read: a cell depends on its left, upper and
//                     upper-left neighbours only.
//   reduce_units_kernel   one wavefront per row, chunks of 64 units in ascending order: run-start flags -> ballot -> prefix count of
//                     the lanes below + the carry of the chunks before.  A run's length is written by the lane that finds the NEXT run's
//                     start (the last one's after the loop), so the row is read once.
// Integer arithmetic, no atomics, nothing that depends on the launch order: a pair's / row's result depends on its own tokens and
// lengths only.
#include "common.h"
#include "engine.h"

using namespace dn;

namespace dn {
namespace {

constexpr int ED_MAX_LEN = DN_EDIT_DISTANCE_MAX_LEN;  // 8192
constexpr int ED_STRIP_MAX = 32;                      // columns a lane holds in registers
constexpr int ED_PANEL_MAX = 64 * ED_STRIP_MAX;       // 2048
constexpr int ED_WAVES_MAX = 4;                       // pairs of a workgroup
constexpr int ED_LDS_WORDS = 16384;                   // 64 KiB of staged tokens per workgroup

// lane l <- lane l - 1 (lane 0 keeps `self`): DPP wave_shr:1
__device__ __forceinline__ int wave_shr1(int self, int v) { return __builtin_amdgcn_update_dpp(self, v, 0x138, 0xf, 0xf, false); }

// One panel of one pair.  rows [na] and cols (the panel's, [pw]) are LDS copies; col_in / col_out are workspace rows indexed by the row
// number 1 .. na (null: the panel is the first / the last).  Returns D[na][c_lo + pw] in every lane.
template <int S>
__device__ __forceinline__ int ed_panel(const int32_t* rows, int na, const int32_t* cols, int c_lo, int pw, int w, const int32_t* col_in,
                                        int32_t* col_out, int lane) {
  int prev[S], tok[S];
  const int j0 = lane * w;  // columns c_lo + j0 + 1 .. c_lo + j0 + w
#pragma unroll
  for (int k = 0; k < S; ++k) {
    prev[k] = c_lo + j0 + k + 1;  // D[0][column]
    tok[k] = k < w && j0 + k < pw ? cols[j0 + k] : 0;
  }
  const int last_lane = (pw - 1) / w;  // the lane that holds the panel's last column, in cell (pw - 1) - last_lane * w
  const int steps = na + last_lane;
  int diag = c_lo + j0;  // D[row - 1][c_lo + j0], row = 1
  int out = 0;           // the strip's last value of the row this lane computed last
  int colbuf = 0;        // col_in[64 m + lane + 1]
  for (int t = 0; t < steps; ++t) {
    if (col_in != nullptr && (t & 63) == 0) colbuf = t + lane < na ? col_in[t + lane + 1] : 0;
    // lane 0's left neighbour of row t + 1 is the boundary column: its own index in the first panel
    const int edge = col_in != nullptr ? __builtin_amdgcn_readlane(colbuf, t & 63) : t + 1;
    int left = wave_shr1(edge, out);
    const int r = t - lane;  // row r + 1
    if (r >= 0 && r < na) {
      const int a = rows[r];
      const int d0 = left;
#pragma unroll
      for (int k = 0; k < S; ++k) {
        if (k >= w) break;  // wave-uniform
        const int up = prev[k];
        const int sub = diag + (a != tok[k] ? 1 : 0);
        const int best = min(min(up + 1, sub), left + 1);
        diag = up;
        prev[k] = best;
        left = best;
      }
      diag = d0;
      out = left;
      if (col_out != nullptr && lane == 63) col_out[r + 1] = out;
    }
  }
  // D[na][last column]: lane last_lane's cell (pw - 1) - last_lane * w
  const int cell = pw - 1 - last_lane * w;
  int res = 0;
#pragma unroll
  for (int k = 0; k < S; ++k)
    if (k == cell) res = prev[k];
  return __builtin_amdgcn_readlane(res, last_lane);
}

__global__ __launch_bounds__(64 * ED_WAVES_MAX) void edit_distance_kernel(const int32_t* __restrict__ a, int lda, const int32_t* __restrict__ a_len,
                                                                         const int32_t* __restrict__ b, int ldb, const int32_t* __restrict__ b_len, int B,
                                                                         int32_t* __restrict__ dist, int32_t* ws, int ws_ld, int panel, int waves) {
  extern __shared__ int32_t ed_lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: lengths and strip widths stay scalar
  const int pair = blockIdx.x * waves + wave;
  if (pair >= B) return;  // whole waves leave; no workgroup barrier follows
  int la = a_len[pair], lb = b_len[pair];
  la = la < 0 ? 0 : la > lda ? lda : la;
  lb = lb < 0 ? 0 : lb > ldb ? ldb : lb;
  const int32_t* pa = a + (int64_t)pair * lda;
  const int32_t* pb = b + (int64_t)pair * ldb;
  if (lb > la) {  // the shorter sequence becomes the columns
    const int32_t* p = pa; pa = pb; pb = p;
    const int n = la; la = lb; lb = n;
  }
  if (lb == 0) {
    if (lane == 0) dist[pair] = la;
    return;
  }
  int32_t* rows = ed_lds + (size_t)wave * (lda + ldb);  // la + lb <= lda + ldb
  int32_t* cols = rows + la;
  for (int i = lane; i < la; i += 64) rows[i] = pa[i];
  for (int i = lane; i < lb; i += 64) cols[i] = pb[i];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the wave's own LDS stores, read by its other lanes below
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  int32_t* col = ws + (int64_t)pair * 2 * ws_ld;  // the pair's two boundary columns
  int res = 0;
  int p = 0;
  for (int c_lo = 0; c_lo < lb; c_lo += panel, ++p) {
    const int pw = lb - c_lo < panel ? lb - c_lo : panel;
    const int w = (pw + 63) >> 6;
    const int32_t* cin = c_lo > 0 ? col + ((p + 1) & 1) * ws_ld : nullptr;
    int32_t* cout = c_lo + panel < lb ? col + (p & 1) * ws_ld : nullptr;
    if (w <= 4)
      res = ed_panel<4>(rows, la, cols + c_lo, c_lo, pw, w, cin, cout, lane);
    else if (w <= 16)
      res = ed_panel<16>(rows, la, cols + c_lo, c_lo, pw, w, cin, cout, lane);
    else
      res = ed_panel<ED_STRIP_MAX>(rows, la, cols + c_lo, c_lo, pw, w, cin, cout, lane);
    if (cout != nullptr) __threadfence();  // lane 63's column stores before the next panel's loads by the other lanes
  }
  if (lane == 0) dist[pair] = res;
}

constexpr int RU_WAVES = 4;  // rows of a workgroup

__global__ __launch_bounds__(64 * RU_WAVES) void reduce_units_kernel(const int32_t* __restrict__ units, const int32_t* __restrict__ lengths, int B, int ld,
                                                                    int32_t* __restrict__ reduced, int32_t* __restrict__ reduced_len,
                                                                    int32_t* __restrict__ durations, int32_t* __restrict__ first) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * RU_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= B) return;
  int len = lengths[row];
  len = len < 0 ? 0 : len > ld ? ld : len;
  const int32_t* u = units + (int64_t)row * ld;
  int32_t* red = reduced + (int64_t)row * ld;
  int32_t* dur = durations ? durations + (int64_t)row * ld : nullptr;
  int32_t* fst = first ? first + (int64_t)row * ld : nullptr;
  int count = 0;       // runs that start in the chunks before
  int last_start = 0;  // first frame of the latest of them
  int tail = 0;        // the last unit of the chunk before
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    const bool in = i < len;
    const int v = in ? u[i] : 0;
    const int before = wave_shr1(tail, v);  // lane 0: the chunk before's last unit
    const bool start = in && (i == 0 || v != before);
    const unsigned long long mask = __ballot(start);
    const unsigned long long below = mask & ((1ull << lane) - 1ull);
    if (start) {
      const int r = count + __popcll(below);
      red[r] = v;
      if (fst) fst[r] = i;
      if (dur && r > 0) dur[r - 1] = i - (below ? base + 63 - __clzll(below) : last_start);
    }
    count += __popcll(mask);
    if (mask) last_start = base + 63 - __clzll(mask);
    tail = __builtin_amdgcn_readlane(v, 63);
  }
  if (lane == 0) {
    reduced_len[row] = count;
    if (dur && count > 0) dur[count - 1] = len - last_start;
  }
  for (int j = count + lane; j < ld; j += 64) {
    red[j] = 0;
    if (dur) dur[j] = 0;
    if (fst) fst[j] = 0;
  }
}

inline int ed_waves(int lda, int ldb) {
  const int per = lda + ldb;
  const int n = ED_LDS_WORDS / per;
  return n < 1 ? 1 : n > ED_WAVES_MAX ? ED_WAVES_MAX : n;
}

}  // namespace
}  // namespace dn

extern "C" size_t dn_edit_distance_workspace_bytes(int32_t B, int32_t max_len_a, int32_t max_len_b) {
  if (B <= 0 || max_len_a < 0 || max_len_b < 0 || max_len_a > ED_MAX_LEN || max_len_b > ED_MAX_LEN) return 0;
  const int longer = max_len_a > max_len_b ? max_len_a : max_len_b;
  // two boundary columns per pair, rows 0 .. longer, each padded to 64 words
  return (size_t)B * 2 * (size_t)((longer + 1 + 63) & ~63) * sizeof(int32_t);
}

extern "C" int dn_edit_distance(const int32_t* a, int32_t lda, const int32_t* a_len, const int32_t* b, int32_t ldb, const int32_t* b_len, int32_t B,
                                int32_t* dist, int32_t panel_cols, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(a && a_len && b && b_len && dist, "dn_edit_distance: null argument");
  DN_CHECK_ARG(B > 0, "dn_edit_distance: B=%d (at least 1)", B);
  DN_CHECK_ARG(lda >= 1 && lda <= ED_MAX_LEN, "dn_edit_distance: lda=%d: rows of a hold 1 .. %d tokens", lda, ED_MAX_LEN);
  DN_CHECK_ARG(ldb >= 1 && ldb <= ED_MAX_LEN, "dn_edit_distance: ldb=%d: rows of b hold 1 .. %d tokens", ldb, ED_MAX_LEN);
  DN_CHECK_ARG(panel_cols == 0 || (panel_cols >= 64 && panel_cols <= ED_PANEL_MAX && panel_cols % 64 == 0),
               "dn_edit_distance: panel_cols=%d (0, or a multiple of 64 up to %d)", panel_cols, ED_PANEL_MAX);
  const size_t need = dn_edit_distance_workspace_bytes(B, lda, ldb);
  DN_CHECK_ARG(workspace != nullptr && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
               "dn_edit_distance: workspace of %zu bytes, dn_edit_distance_workspace_bytes(B, lda, ldb) = %zu", workspace_bytes, need);
  const int waves = ed_waves(lda, ldb);
  const int longer = lda > ldb ? lda : ldb;
  const int ws_ld = (longer + 1 + 63) & ~63;
  const size_t lds = (size_t)waves * (lda + ldb) * sizeof(int32_t);  // <= 64 KiB
  hipLaunchKernelGGL(edit_distance_kernel, dim3((B + waves - 1) / waves), dim3(64 * waves), lds, (hipStream_t)stream, a, lda, a_len, b, ldb, b_len, B, dist,
                     (int32_t*)workspace, ws_ld, panel_cols ? panel_cols : ED_PANEL_MAX, waves);
  DN_CHECK_LAUNCH("dn_edit_distance");
  return DN_OK;
}

extern "C" int dn_reduce_units(const int32_t* units, const int32_t* lengths, int32_t B, int32_t ld, int32_t* reduced, int32_t* reduced_len,
                               int32_t* durations, int32_t* first, void* stream) {
  DN_CHECK_ARG(units && lengths && reduced && reduced_len, "dn_reduce_units: null argument");
  DN_CHECK_ARG(B > 0 && ld >= 1, "dn_reduce_units: B=%d ld=%d (each at least 1)", B, ld);
  DN_CHECK_ARG(reduced != units && durations != units && first != units, "dn_reduce_units: an output aliases the units");
  hipLaunchKernelGGL(reduce_units_kernel, dim3((B + RU_WAVES - 1) / RU_WAVES), dim3(64 * RU_WAVES), 0, (hipStream_t)stream, units, lengths, B, ld, reduced,
                     reduced_len, durations, first);
  DN_CHECK_LAUNCH("dn_reduce_units");
  return DN_OK;
}
