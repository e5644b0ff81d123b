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
