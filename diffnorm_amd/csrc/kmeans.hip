// Learning the unit quantizer (examples/textless_nlp/gslm/speech2unit/clustering/cluster_kmeans.py, examples/hubert/simple_kmeans/
// learn_kmeans.py: sklearn.cluster.MiniBatchKMeans) on the device, and applying it (ApplyKmeans, examples/hubert/simple_kmeans/
// dump_km_label.py:20-53).  One mini-batch step is assign -> accumulate -> update.  Here:
//   dn_kmeans_assign       the nearest centre of every row: scores x . c_j - |c_j|^2 / 2 by one DN_F32 contraction, then the first
//                          maximum of each row (dn_argmax_units)
//   dn_kmeans_accumulate   per-cluster column sums, member counts and the inertia of a labelled batch, without floating-point atomics
//                          and without a one-hot contraction: a stable counting sort of the row indices by label
//                            km_hist_kernel   histogram of the labels of KM_ROWS rows per workgroup (LDS integer atomics)
//                            km_scan_kernel   one workgroup: cluster totals, their exclusive scan, and every workgroup's first slot in
//                                             every cluster (workgroups in index order)
//                            km_rank_kernel   a row's slot = its workgroup's first slot + the rows of the same label in front of it in
//                                             the workgroup: every cluster lists its rows in ascending row index
//                          then km_sum_kernel: one wave per (cluster, 256 columns) adds its rows in that order, 16 bytes per lane and
//                          row, into double accumulators, and sums |x - c|^2 from the differences; km_reduce_kernel adds the waves'
//                          inertia parts in index order.  The order of every sum is a function of (labels, n, D) alone: two calls
//                          give the same bits, and so does any position of M against KM_ROWS.
//   dn_kmeans_update       scikit-learn's dense mini-batch rule c <- (c w + sum) / (w + count), w += count, in double, one rounding
//                          to fp32; -|c|^2 / 2 of the rounded centre in double, one rounding
//   dn_kmeans_min_dist     the step of k-means++ seeding: squared distances of every row to <= 16 candidates (differences, double
//                          accumulation, one rounding to fp32), the potentials sum_m min(mind2[m], d2[m][j]) in double in a fixed
//                          order (rows in order inside a wave, waves in order inside a workgroup, workgroups strided over the lanes of
//                          one wave per candidate), and optionally mind2 <- min(mind2, d2[:, commit])
#include <algorithm>

#include "common.h"
#include "engine.h"
#include "nar_common.h"

using namespace dn;

namespace dn {
namespace {

constexpr int KM_ROWS = 256;    // rows per workgroup of the counting sort, one per thread
constexpr int KM_NMAX = 8192;   // clusters: the workgroup's histogram is n ints of LDS
constexpr int KM_COLS = 256;    // columns per wave of the row sum: 16 bytes per lane
constexpr int KM_CHUNKS = 16;   // D <= KM_COLS * KM_CHUNKS
constexpr int KM_KMAX = 16;     // candidates per dn_kmeans_min_dist call
constexpr int MD_WROWS = 16;    // rows per wave there
constexpr int MD_ROWS = 4 * MD_WROWS;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a label outside [0, n) owns no slot: the row is left out of every sum (the binding refuses such labels before the launch)
__device__ __forceinline__ int label_of(const int32_t* labels, int m, int M, int n) {
  if (m >= M) return -1;
  const int l = labels[m];
  return (unsigned)l < (unsigned)n ? l : -1;
}

__global__ __launch_bounds__(KM_ROWS) void km_hist_kernel(const int32_t* __restrict__ labels, int M, int n, int32_t* __restrict__ hist) {
  extern __shared__ int32_t bins[];
  for (int j = threadIdx.x; j < n; j += KM_ROWS) bins[j] = 0;
  __syncthreads();
  const int l = label_of(labels, blockIdx.x * KM_ROWS + threadIdx.x, M, n);
  if (l >= 0) atomicAdd(&bins[l], 1);
  __syncthreads();
  int32_t* h = hist + (size_t)blockIdx.x * n;
  for (int j = threadIdx.x; j < n; j += KM_ROWS) h[j] = bins[j];
}

// hist [nblk][n] counts -> first slots; start [n + 1]; counts [n]
__global__ __launch_bounds__(256) void km_scan_kernel(int32_t* __restrict__ hist, int nblk, int n, int32_t* __restrict__ start, int32_t* __restrict__ counts) {
  __shared__ int32_t sc[256];
  const int t = threadIdx.x;
  int32_t carry = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int j = c0 + t;
    int32_t c = 0;
    if (j < n)
      for (int b = 0; b < nblk; ++b) c += hist[(size_t)b * n + j];
    sc[t] = c;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int32_t v = t >= o ? sc[t - o] : 0;
      __syncthreads();
      sc[t] += v;
      __syncthreads();
    }
    const int32_t incl = sc[t], total = sc[255];
    __syncthreads();
    if (j < n) {
      counts[j] = c;
      int32_t run = carry + incl - c;
      start[j] = run;
      for (int b = 0; b < nblk; ++b) {
        const int32_t h = hist[(size_t)b * n + j];
        hist[(size_t)b * n + j] = run;
        run += h;
      }
    }
    carry += total;
  }
  if (t == 0) start[n] = carry;
}

__global__ __launch_bounds__(KM_ROWS) void km_rank_kernel(const int32_t* __restrict__ labels, int M, int n, const int32_t* __restrict__ first,
                                                          int32_t* __restrict__ order) {
  __shared__ int32_t lab[KM_ROWS];
  const int t = threadIdx.x, m = blockIdx.x * KM_ROWS + t;
  const int l = label_of(labels, m, M, n);
  lab[t] = l;
  __syncthreads();
  if (l < 0) return;
  int r = 0;
  for (int i = 0; i < t; ++i) r += lab[i] == l;
  const int slot = first[(size_t)blockIdx.x * n + l] + r;
  if (slot < M) order[slot] = m;
}

__device__ __forceinline__ void km_add_row(double (&a)[4], double& q, const float4& x, const float4& c) {
  a[0] += (double)x.x; a[1] += (double)x.y; a[2] += (double)x.z; a[3] += (double)x.w;
  const double d0 = (double)x.x - (double)c.x, d1 = (double)x.y - (double)c.y, d2 = (double)x.z - (double)c.z, d3 = (double)x.w - (double)c.w;
  q += d0 * d0; q += d1 * d1; q += d2 * d2; q += d3 * d3;
}

// grid (n, ceil(D / KM_COLS)), one wave each
__global__ __launch_bounds__(64) void km_sum_kernel(const float* __restrict__ feats, const float* __restrict__ centers, const int32_t* __restrict__ order,
                                                    const int32_t* __restrict__ start, int D, double* __restrict__ sums, double* __restrict__ part) {
  const int j = blockIdx.x, col = blockIdx.y * KM_COLS + threadIdx.x * 4;
  const bool on = col < D;
  const int s = start[j], e = start[j + 1];
  double a[4] = {0.0, 0.0, 0.0, 0.0}, q = 0.0;
  if (on) {
    const float4 c = *reinterpret_cast<const float4*>(centers + (size_t)j * D + col);
    const float* x = feats + col;
    int i = s;
    for (; i + 4 <= e; i += 4) {
      const int r0 = order[i], r1 = order[i + 1], r2 = order[i + 2], r3 = order[i + 3];
      const float4 x0 = *reinterpret_cast<const float4*>(x + (size_t)r0 * D), x1 = *reinterpret_cast<const float4*>(x + (size_t)r1 * D);
      const float4 x2 = *reinterpret_cast<const float4*>(x + (size_t)r2 * D), x3 = *reinterpret_cast<const float4*>(x + (size_t)r3 * D);
      km_add_row(a, q, x0, c);
      km_add_row(a, q, x1, c);
      km_add_row(a, q, x2, c);
      km_add_row(a, q, x3, c);
    }
    for (; i < e; ++i) km_add_row(a, q, *reinterpret_cast<const float4*>(x + (size_t)order[i] * D), c);
    double* o = sums + (size_t)j * D + col;
    *reinterpret_cast<double2*>(o) = make_double2(a[0], a[1]);
    *reinterpret_cast<double2*>(o + 2) = make_double2(a[2], a[3]);
  }
  q = wave_sum_f64(q);
  if (threadIdx.x == 0) part[(size_t)j * gridDim.y + blockIdx.y] = q;
}

// out = sum of part[0 : count], thread t taking t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void km_reduce_kernel(const double* __restrict__ part, int count, double* __restrict__ out) {
  __shared__ double sh[256];
  double v = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) v += part[i];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

// one wave per cluster
__global__ __launch_bounds__(64) void km_update_kernel(float* __restrict__ centers, float* __restrict__ half_norm, double* __restrict__ weight_sums,
                                                       const double* __restrict__ sums, const int32_t* __restrict__ counts, int D) {
  const int j = blockIdx.x, cnt = counts[j];
  if (cnt <= 0) return;
  const double w = weight_sums[j], wn = w + (double)cnt;
  double h = 0.0;
  for (int d = threadIdx.x * 4; d < D; d += 256) {
    float4 c = *reinterpret_cast<const float4*>(centers + (size_t)j * D + d);
    const double2 s0 = *reinterpret_cast<const double2*>(sums + (size_t)j * D + d), s1 = *reinterpret_cast<const double2*>(sums + (size_t)j * D + d + 2);
    c.x = (float)(((double)c.x * w + s0.x) / wn);
    c.y = (float)(((double)c.y * w + s0.y) / wn);
    c.z = (float)(((double)c.z * w + s1.x) / wn);
    c.w = (float)(((double)c.w * w + s1.y) / wn);
    *reinterpret_cast<float4*>(centers + (size_t)j * D + d) = c;
    h += (double)c.x * (double)c.x + (double)c.y * (double)c.y + (double)c.z * (double)c.z + (double)c.w * (double)c.w;
  }
  h = wave_sum_f64(h);
  if (threadIdx.x == 0) {
    weight_sums[j] = wn;
    half_norm[j] = (float)(-0.5 * h);
  }
}

// grid ceil(M / MD_ROWS), 4 waves of MD_WROWS rows each; part [blocks][KM_KMAX]
__global__ __launch_bounds__(256) void km_min_dist_kernel(const float* __restrict__ feats, int M, int D, const float* __restrict__ cands, int k, int commit,
                                                          float* __restrict__ mind2, double* __restrict__ part) {
  __shared__ double ws[4][KM_KMAX];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double pot[KM_KMAX];
#pragma unroll
  for (int j = 0; j < KM_KMAX; ++j) pot[j] = 0.0;
  const int r0 = blockIdx.x * MD_ROWS + wave * MD_WROWS, r1 = min(r0 + MD_WROWS, M);
  for (int r = r0; r < r1; ++r) {
    const float* x = feats + (size_t)r * D;
    const float cur = mind2[r];
    float keep = cur;
#pragma unroll
    for (int j = 0; j < KM_KMAX; ++j) {
      if (j < k) {
        const float* c = cands + (size_t)j * D;
        double d = 0.0;
        for (int col = lane * 4; col < D; col += 256) {
          const float4 xv = *reinterpret_cast<const float4*>(x + col), cv = *reinterpret_cast<const float4*>(c + col);
          const double d0 = (double)xv.x - (double)cv.x, d1 = (double)xv.y - (double)cv.y, d2 = (double)xv.z - (double)cv.z, d3 = (double)xv.w - (double)cv.w;
          d += d0 * d0; d += d1 * d1; d += d2 * d2; d += d3 * d3;
        }
        const float m2 = fminf(cur, (float)wave_sum_f64(d));
        pot[j] += (double)m2;
        if (j == commit) keep = m2;
      }
    }
    if (commit >= 0 && lane == 0) mind2[r] = keep;
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < KM_KMAX; ++j) ws[wave][j] = pot[j];
  }
  __syncthreads();
  if ((int)threadIdx.x < KM_KMAX) part[(size_t)blockIdx.x * KM_KMAX + threadIdx.x] = ((ws[0][threadIdx.x] + ws[1][threadIdx.x]) + ws[2][threadIdx.x]) + ws[3][threadIdx.x];
}

// grid k, one wave each: lane l adds workgroups l, l + 64, ... in order, then the wave's fixed tree
__global__ __launch_bounds__(64) void km_pot_kernel(const double* __restrict__ part, int blocks, double* __restrict__ pot) {
  double v = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 64) v += part[(size_t)b * KM_KMAX + blockIdx.x];
  v = wave_sum_f64(v);
  if (threadIdx.x == 0) pot[blockIdx.x] = v;
}

struct TrainPlan {
  int32_t *hist, *order, *start;
  double* part;
  size_t bytes;
};
inline TrainPlan train_plan(void* ws, size_t cap, int M, int n) {
  Arena ar{static_cast<char*>(ws), 0, cap};
  TrainPlan p;
  const size_t nblk = (size_t)(M + KM_ROWS - 1) / KM_ROWS;
  p.hist = (int32_t*)ar.take(nblk * n * sizeof(int32_t));
  p.order = (int32_t*)ar.take((size_t)M * sizeof(int32_t));
  p.start = (int32_t*)ar.take((size_t)(n + 1) * sizeof(int32_t));
  p.part = (double*)ar.take((size_t)n * KM_CHUNKS * sizeof(double));
  p.bytes = ar.off;
  return p;
}
inline size_t min_dist_bytes(int M) { return (size_t)((M + MD_ROWS - 1) / MD_ROWS) * KM_KMAX * sizeof(double); }

}  // namespace
}  // namespace dn

extern "C" size_t dn_kmeans_workspace_bytes(int32_t M, int32_t n_centroids) {
  if (M <= 0 || n_centroids <= 0) return 0;
  return (size_t)M * round_up(n_centroids, 4) * sizeof(float) + 512;
}

extern "C" int dn_kmeans_assign(const float* feats, const float* centroids, const float* half_norm, int32_t M, int32_t D, int32_t n_centroids,
                                int32_t* units, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(feats && centroids && half_norm && units && workspace, "dn_kmeans_assign: null argument");
  DN_CHECK_ARG(M > 0 && D > 0 && D % 32 == 0 && n_centroids > 0, "dn_kmeans_assign: M=%d D=%d (a multiple of 32) centroids=%d", M, D, n_centroids);
  const int N = round_up(n_centroids, 4);
  DN_CHECK_ARG((int64_t)M * std::max(N, D) < (int64_t)1 << 31, "dn_kmeans_assign: M=%d: a buffer exceeds 2^31 elements", M);
  DN_TRY(check_workspace("dn_kmeans_assign", workspace, workspace_bytes, (size_t)M * N * sizeof(float)));
  hipStream_t s = (hipStream_t)stream;
  float* scores = (float*)workspace;
  DN_TRY(linear(Rows{DN_F32, M, M, 0, s}, feats, D, centroids, half_norm, N, DN_EPI_BIAS, scores, DN_F32));  // x . c_j - |c_j|^2 / 2
  return dn_argmax_units(scores, N, M, n_centroids, 0, units, stream);  // the first maximum wins: ties go to the lowest index
}

extern "C" size_t dn_kmeans_workspace_bytes_train(int32_t M, int32_t n_clusters) {
  if (M <= 0 || n_clusters <= 0 || n_clusters > KM_NMAX) return 0;
  return std::max(train_plan(nullptr, 0, M, n_clusters).bytes, min_dist_bytes(M));
}

extern "C" int dn_kmeans_accumulate(const float* feats, const int32_t* labels, const float* centers, int32_t M, int32_t D, int32_t n_clusters, double* sums,
                                    int32_t* counts, double* inertia, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(feats && labels && centers && sums && counts && inertia && workspace, "dn_kmeans_accumulate: null argument");
  DN_CHECK_ARG(M > 0 && D > 0 && D % 32 == 0 && D <= KM_COLS * KM_CHUNKS && n_clusters > 0 && n_clusters <= KM_NMAX,
               "dn_kmeans_accumulate: M=%d D=%d (a multiple of 32, <= %d) clusters=%d (<= %d)", M, D, KM_COLS * KM_CHUNKS, n_clusters, KM_NMAX);
  const int n = n_clusters, nblk = (M + KM_ROWS - 1) / KM_ROWS;
  DN_CHECK_ARG((int64_t)M * D < (int64_t)1 << 31 && (int64_t)nblk * n < (int64_t)1 << 31, "dn_kmeans_accumulate: M=%d: a buffer exceeds 2^31 elements", M);
  DN_CHECK_ARG((((uintptr_t)feats | (uintptr_t)centers | (uintptr_t)sums) & 15) == 0, "dn_kmeans_accumulate: feats, centers and sums must be 16-byte aligned");
  const TrainPlan p = train_plan(workspace, workspace_bytes, M, n);
  DN_TRY(check_workspace("dn_kmeans_accumulate", workspace, workspace_bytes, p.bytes));
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (D + KM_COLS - 1) / KM_COLS;
  hipLaunchKernelGGL(km_hist_kernel, dim3(nblk), dim3(KM_ROWS), (size_t)n * sizeof(int32_t), s, labels, M, n, p.hist);
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(256), 0, s, p.hist, nblk, n, p.start, counts);
  hipLaunchKernelGGL(km_rank_kernel, dim3(nblk), dim3(KM_ROWS), 0, s, labels, M, n, p.hist, p.order);
  hipLaunchKernelGGL(km_sum_kernel, dim3(n, chunks), dim3(64), 0, s, feats, centers, p.order, p.start, D, sums, p.part);
  hipLaunchKernelGGL(km_reduce_kernel, dim3(1), dim3(256), 0, s, p.part, n * chunks, inertia);
  DN_CHECK_LAUNCH("dn_kmeans_accumulate");
  return DN_OK;
}

extern "C" int dn_kmeans_update(float* centers, float* half_norm, double* weight_sums, const double* sums, const int32_t* counts, int32_t n_clusters, int32_t D,
                                void* stream) {
  DN_CHECK_ARG(centers && half_norm && weight_sums && sums && counts, "dn_kmeans_update: null argument");
  DN_CHECK_ARG(n_clusters > 0 && n_clusters <= KM_NMAX && D > 0 && D % 32 == 0, "dn_kmeans_update: clusters=%d (<= %d) D=%d (a multiple of 32)", n_clusters, KM_NMAX, D);
  DN_CHECK_ARG((((uintptr_t)centers | (uintptr_t)sums) & 15) == 0, "dn_kmeans_update: centers and sums must be 16-byte aligned");
  hipLaunchKernelGGL(km_update_kernel, dim3(n_clusters), dim3(64), 0, (hipStream_t)stream, centers, half_norm, weight_sums, sums, counts, D);
  DN_CHECK_LAUNCH("dn_kmeans_update");
  return DN_OK;
}

extern "C" int dn_kmeans_min_dist(const float* feats, int32_t M, int32_t D, const float* cands, int32_t k, int32_t commit, float* mind2, double* pot,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(feats && cands && mind2 && pot && workspace, "dn_kmeans_min_dist: null argument");
  DN_CHECK_ARG(M > 0 && D > 0 && D % 32 == 0 && (int64_t)M * D < (int64_t)1 << 31, "dn_kmeans_min_dist: M=%d D=%d (a multiple of 32; M * D < 2^31)", M, D);
  DN_CHECK_ARG(k >= 1 && k <= KM_KMAX && commit >= -1 && commit < k, "dn_kmeans_min_dist: %d candidates (1 .. %d), commit %d (-1 or one of them)", k, KM_KMAX, commit);
  DN_CHECK_ARG((((uintptr_t)feats | (uintptr_t)cands) & 15) == 0, "dn_kmeans_min_dist: feats and cands must be 16-byte aligned");
  DN_TRY(check_workspace("dn_kmeans_min_dist", workspace, workspace_bytes, min_dist_bytes(M)));
  const int blocks = (M + MD_ROWS - 1) / MD_ROWS;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(km_min_dist_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, feats, M, D, cands, k, commit, mind2, part);
  hipLaunchKernelGGL(km_pot_kernel, dim3(k), dim3(64), 0, (hipStream_t)stream, part, blocks, pot);
  DN_CHECK_LAUNCH("dn_kmeans_min_dist");
  return DN_OK;
}
