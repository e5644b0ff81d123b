// dn_repack_weights: the inference engines' packed tensors from a training engine's flat fp32 master buffer, on the device.
//
// The master buffer holds the packed fp32 tensors of diffnorm_amd/packing.py's entry tables (rows padded to 128, K to 64, GEGLU
// interleave, stacked conditioning projections); what the inference lists add is a dtype conversion, the per-tensor stacking of
// the transformer's layers, the K-blocked copies and the summed skip bias (packing.repack_plan builds the descriptors).  One
// launch: grid.y = descriptor, grid.x strides over its 16-byte units.  A pure stream: every lane loads 32 (COPY / SUM: 16)
// contiguous bytes, consecutive lanes consecutive addresses; every store is one 16-byte vector store per lane (the only
// exception: an fp32 COPY whose length is no multiple of 4 elements, or whose slice of a stacked destination is not 16-byte
// aligned -- the few-hundred-element frequency and gamma vectors -- goes element by element).
#include "common.h"

namespace dn {
namespace {

constexpr int kRepackBlocks = 1024;  // grid.x: workgroups striding over one descriptor (the 470 MB conditioning matrix keeps 4 per CU busy)

template <int DT>
__device__ __forceinline__ uint4 to16(const float4& a, const float4& b) {
  if constexpr (DT == DN_F16)
    return make_uint4(pack_f16x2_sat(a.x, a.y), pack_f16x2_sat(a.z, a.w), pack_f16x2_sat(b.x, b.y), pack_f16x2_sat(b.z, b.w));
  else
    return make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
}

// 8 consecutive fp32 elements starting at element `e` of the destination (e a multiple of 8), row-major as they lie
template <int DT>
__device__ __forceinline__ void store8(void* dst, int64_t e, const float4& a, const float4& b) {
  if constexpr (DT == DN_F32) {
    float4* p = reinterpret_cast<float4*>(reinterpret_cast<float*>(dst) + e);
    p[0] = a;
    p[1] = b;
  } else if constexpr (DT == DN_BF16X3) {  // weight order: [lo | hi] per 32 elements (packing.split_rows(weight=True))
    uint32_t h0, l0, h1, l1, h2, l2, h3, l3;
    split_pair(a.x, a.y, h0, l0);
    split_pair(a.z, a.w, h1, l1);
    split_pair(b.x, b.y, h2, l2);
    split_pair(b.z, b.w, h3, l3);
    char* p = reinterpret_cast<char*>(dst) + split_byte(e);
    *reinterpret_cast<uint4*>(p) = make_uint4(l0, l1, l2, l3);
    *reinterpret_cast<uint4*>(p + 64) = make_uint4(h0, h1, h2, h3);
  } else {
    *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(dst) + e) = to16<DT>(a, b);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void repack_kernel(const float* __restrict__ master, const DnRepackDesc* __restrict__ descs) {
  const DnRepackDesc d = descs[blockIdx.y];  // wave-uniform
  const float* __restrict__ src = master + d.src;
  const int64_t n = (int64_t)d.mats * d.rows * d.K;
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (d.kind == DN_REPACK_CONVERT) {
    for (int64_t u = first; u < n / 8; u += step) {
      const float4* p = reinterpret_cast<const float4*>(src + u * 8);
      store8<DT>(d.dst, u * 8, p[0], p[1]);
    }
  } else if (d.kind == DN_REPACK_KBLOCK) {
    // destination [mats][K/32][rows][32] (packing.kblock), walked in destination order: a lane's 8 elements are 8 consecutive k of
    // one row, four lanes cover a row's 128 source bytes of the K-tile, the next four the next row's
    if constexpr (DT == DN_BF16 || DT == DN_F16) {
      const int64_t per_mat = (int64_t)d.rows * d.K / 8, per_kb = (int64_t)d.rows * 4;
      for (int64_t u = first; u < n / 8; u += step) {
        const int64_t m = u / per_mat, rem = u - m * per_mat;
        const int64_t kb = rem / per_kb, in_kb = rem - kb * per_kb;
        const int64_t r = in_kb >> 2, q = in_kb & 3;
        const float4* p = reinterpret_cast<const float4*>(src + (m * d.rows + r) * d.K + kb * 32 + q * 8);
        *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(d.dst) + u * 8) = to16<DT>(p[0], p[1]);
      }
    }
  } else if (d.kind == DN_REPACK_COPY) {
    float* __restrict__ out = reinterpret_cast<float*>(d.dst);
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      for (int64_t u = first; u < n / 4; u += step) reinterpret_cast<float4*>(out)[u] = reinterpret_cast<const float4*>(src)[u];
    } else {
      for (int64_t i = first; i < n; i += step) out[i] = src[i];
    }
  } else {  // DN_REPACK_SUM: out[c] = ((0 + row_0[c]) + row_1[c]) + ..., the order of the host packer's sum()
    float4* __restrict__ out = reinterpret_cast<float4*>(d.dst);
    for (int64_t u = first; u < n / 4; u += step) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int j = 0; j < d.count; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(src + j * d.stride + u * 4);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
      out[u] = acc;
    }
  }
}

// dn_ffn_fold: the feed-forward block's CausalConv1d(inner, inner, 3) and the Linear(inner, dim) after it as ONE causal conv of three
// taps inner -> dim (nothing but the identity sits between the two at inference): W'_j = W_out . W_conv_j, b' = W_out . b_conv + b_out.
// fp32 products summed over k = 0 .. inner-1 in that order by one lane per output, so a refreshed engine and a freshly built one
// get the same bits from the same sources; the result is rounded once, into the engine's operand format.  A lane owns 4 rows x 8
// consecutive columns of one (layer, tap): W_out's elements are wave-uniform loads, W_conv's row pieces 32 contiguous bytes per lane.
struct FoldArgs {
  const float *conv_W, *conv_b, *out_W, *out_b;
  int64_t conv_W_ls, conv_b_ls, out_W_ls, out_b_ls;  // elements between the layers' sources
  int dim, inner, ip, in_n, Dp, Dn;
  void* W;   // [depth][3][Dn][ip] in the operand format
  void* Wkb; // [depth][3][ip/32][Dn][32], 2-byte types, or NULL: the same values K-blocked (packing.kblock's layout)
  float* b;  // [depth][Dp]
};

template <int DT>
__global__ __launch_bounds__(64) void ffn_fold_w_kernel(FoldArgs a) {
  const int u = blockIdx.x * 64 + threadIdx.x, n0 = blockIdx.y * 4, l = blockIdx.z / 3, tap = blockIdx.z % 3;
  if (u * 8 >= a.ip) return;
  const int c = u * 8;
  const float* __restrict__ wc = a.conv_W + l * a.conv_W_ls + (int64_t)tap * a.in_n * a.ip + c;
  const float* __restrict__ wo = a.out_W + l * a.out_W_ls + (int64_t)n0 * a.ip;
  float acc[4][8];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
  for (int k = 0; k < a.inner; ++k) {
    const float4 x0 = *reinterpret_cast<const float4*>(wc + (int64_t)k * a.ip), x1 = *reinterpret_cast<const float4*>(wc + (int64_t)k * a.ip + 4);
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float w = wo[(int64_t)r * a.ip + k];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[r][i] = fmaf(w, x[i], acc[r][i]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // padding rows and columns are zeros whatever the sources' padding holds
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (n0 + r < a.dim && c + i < a.inner) ? acc[r][i] : 0.f;
    store8<DT>(a.W, (((int64_t)blockIdx.z * a.Dn) + n0 + r) * a.ip + c, make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]));
    if constexpr (DT == DN_BF16 || DT == DN_F16) {  // the lane's 8 columns lie inside one 32-column block
      if (a.Wkb) store8<DT>(a.Wkb, ((((int64_t)blockIdx.z * (a.ip / 32)) + (c >> 5)) * a.Dn + n0 + r) * 32 + (c & 31), make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]));
    }
  }
}

__global__ __launch_bounds__(64) void ffn_fold_b_kernel(FoldArgs a) {
  const int n = blockIdx.x * 64 + threadIdx.x, l = blockIdx.y;
  if (n >= a.Dp) return;
  float acc = 0.f;
  if (n < a.dim) {
    const float* __restrict__ wo = a.out_W + l * a.out_W_ls + (int64_t)n * a.ip;
    const float* __restrict__ bc = a.conv_b + l * a.conv_b_ls;
    for (int k = 0; k < a.inner; ++k) acc = fmaf(wo[k], bc[k], acc);
    acc += a.out_b[l * a.out_b_ls + n];
  }
  a.b[(int64_t)l * a.Dp + n] = acc;
}

}  // namespace
}  // namespace dn

// see include/diffnorm_hip.h
extern "C" int dn_repack_weights(const float* master, const DnRepackDesc* descs, int32_t n, int32_t dtype, void* stream) {
  DN_CHECK_ARG(master && descs, "dn_repack_weights: null argument");
  DN_CHECK_ARG(n >= 1 && n <= 65535, "dn_repack_weights: n=%d descriptors (1 .. 65535)", n);
  DN_CHECK_ARG(dtype == DN_F32 || dtype == DN_BF16 || dtype == DN_BF16X3 || dtype == DN_F16, "dn_repack_weights: dtype=%d", dtype);
  DN_CHECK_ARG(((uintptr_t)master & 15) == 0 && ((uintptr_t)descs & 7) == 0, "dn_repack_weights: master 16-byte, descs 8-byte aligned");
  const dim3 grid(dn::kRepackBlocks, n), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DN_F32) hipLaunchKernelGGL(dn::repack_kernel<DN_F32>, grid, block, 0, s, master, descs);
  else if (dtype == DN_BF16) hipLaunchKernelGGL(dn::repack_kernel<DN_BF16>, grid, block, 0, s, master, descs);
  else if (dtype == DN_F16) hipLaunchKernelGGL(dn::repack_kernel<DN_F16>, grid, block, 0, s, master, descs);
  else hipLaunchKernelGGL(dn::repack_kernel<DN_BF16X3>, grid, block, 0, s, master, descs);
  DN_CHECK_LAUNCH("dn_repack_weights");
  return DN_OK;
}

// see include/diffnorm_hip.h
extern "C" int dn_ffn_fold(const float* conv_W, const float* conv_b, const float* out_W, const float* out_b, int64_t conv_W_stride,
                           int64_t conv_b_stride, int64_t out_W_stride, int64_t out_b_stride, int32_t depth, int32_t dim, int32_t inner,
                           int32_t dtype, void* fold_W, float* fold_b, void* stream) {
  return dn_ffn_fold_kblocked(conv_W, conv_b, out_W, out_b, conv_W_stride, conv_b_stride, out_W_stride, out_b_stride, depth, dim, inner, dtype,
                              fold_W, fold_b, nullptr, stream);
}

// see include/diffnorm_hip.h
extern "C" int dn_ffn_fold_kblocked(const float* conv_W, const float* conv_b, const float* out_W, const float* out_b, int64_t conv_W_stride,
                                    int64_t conv_b_stride, int64_t out_W_stride, int64_t out_b_stride, int32_t depth, int32_t dim,
                                    int32_t inner, int32_t dtype, void* fold_W, float* fold_b, void* fold_Wkb, void* stream) {
  DN_CHECK_ARG(conv_W && conv_b && out_W && out_b && fold_W && fold_b, "dn_ffn_fold: null argument");
  DN_CHECK_ARG(depth >= 1 && 3 * depth <= 65535 && dim >= 1 && inner >= 1, "dn_ffn_fold: depth=%d dim=%d inner=%d", depth, dim, inner);
  DN_CHECK_ARG(dtype == DN_F32 || dtype == DN_BF16 || dtype == DN_BF16X3 || dtype == DN_F16, "dn_ffn_fold: dtype=%d", dtype);
  DN_CHECK_ARG((conv_W_stride | out_W_stride) % 4 == 0 && (((uintptr_t)conv_W | (uintptr_t)out_W) & 15) == 0 && ((uintptr_t)fold_W & 127) == 0,
               "dn_ffn_fold: the weight sources must be 16-byte aligned (strides multiples of 4), the folded weights 128-byte aligned");
  DN_CHECK_ARG(!fold_Wkb || ((dtype == DN_BF16 || dtype == DN_F16) && ((uintptr_t)fold_Wkb & 127) == 0),
               "dn_ffn_fold_kblocked: the K-blocked copy is for DN_BF16 / DN_F16 (dtype=%d), 128-byte aligned", dtype);
  dn::FoldArgs a;
  a.conv_W = conv_W; a.conv_b = conv_b; a.out_W = out_W; a.out_b = out_b;
  a.conv_W_ls = conv_W_stride; a.conv_b_ls = conv_b_stride; a.out_W_ls = out_W_stride; a.out_b_ls = out_b_stride;
  a.dim = dim; a.inner = inner; a.ip = (inner + 63) / 64 * 64; a.in_n = (inner + 127) / 128 * 128; a.Dp = (dim + 63) / 64 * 64; a.Dn = (dim + 127) / 128 * 128;
  a.W = fold_W; a.b = fold_b; a.Wkb = fold_Wkb;
  const dim3 grid((a.ip / 8 + 63) / 64, a.Dn / 4, 3 * depth), block(64);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DN_F32) hipLaunchKernelGGL(dn::ffn_fold_w_kernel<DN_F32>, grid, block, 0, s, a);
  else if (dtype == DN_BF16) hipLaunchKernelGGL(dn::ffn_fold_w_kernel<DN_BF16>, grid, block, 0, s, a);
  else if (dtype == DN_F16) hipLaunchKernelGGL(dn::ffn_fold_w_kernel<DN_F16>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(dn::ffn_fold_w_kernel<DN_BF16X3>, grid, block, 0, s, a);
  hipLaunchKernelGGL(dn::ffn_fold_b_kernel, dim3((a.Dp + 63) / 64, depth), block, 0, s, a);
  DN_CHECK_LAUNCH("dn_ffn_fold");
  return DN_OK;
}
