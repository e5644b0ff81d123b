// Key-masked multi-head self-attention with Transformer-XL relative positions, flash-style: RelPositionMultiHeadedAttention.forward
// (fairseq/modules/espnet_multihead_attention.py:109-196) between linear_q/k/v (+ linear_pos) and linear_out, zero_triu False.
//   score[i, j] = ((q_i + u_h) . k_j + (q_i + v_h) . P_h(i - j)) * scale,   keys j >= lengths[b] masked,   out = softmax(score) V
// The reference forms matrix_bd = (q + v) P^T over all 2T - 1 offsets ([B, H, T, 2T - 1]) and skews it with rel_shift (:120-145); here
// a (64-query, 64-key) tile pair needs only the band of 127 offsets i - j it spans.  Per workgroup (4 waves, 16 queries each):
//   * K tile [64][dk], V tile transposed [dk][64] and the band [128][dk] (row r = offset i0 - j0 - 63 + r) staged in LDS;
//   * wave w contracts its (q + u) rows with the K tile (4 MFMA column blocks) and its (q + v) rows with rows 16 w .. 16 w + 79 of
//     the band (5 column blocks) -- the 79 offsets its 16 x 64 scores touch;
//   * the skew: the band products go to a wave-private LDS patch bd[16][81] and come back as bd[ri][ri - cj + 63] for the score at
//     (query ri, key cj) of the tile;
//   * online softmax in fp32 over the key tiles, P rounded once to the operand type, P V on the MFMA pipe.
// Nothing of size O(T^2) exists anywhere.  Operand types: fp32 (DN_F32, and DN_BF16X3 -- whose q / k / v / pos arrive as plain fp32),
// bf16, IEEE half; accumulation and softmax fp32; q + u and q + v formed in fp32 and rounded once.
#include "common.h"
#include "engine.h"

using namespace dn;

namespace dn {
namespace {

template <typename E> struct Frag;  // the 16 bytes a lane holds of a k-step <-> floats
template <> struct Frag<F32> {
  static constexpr int N = 4;
  typedef float elem_t;
  static __device__ __forceinline__ void unpack(const uint4& v, float* f) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
  }
  static __device__ __forceinline__ uint4 pack(const float* f) {
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
  }
  static __device__ __forceinline__ elem_t one(float v) { return v; }
};
template <bool H16> struct FragH {
  static constexpr int N = 8;
  typedef uint16_t elem_t;
  static __device__ __forceinline__ void unpack(const uint4& v, float* f) {
    const float2 a = unpack_h2<H16>(v.x), b = unpack_h2<H16>(v.y), c = unpack_h2<H16>(v.z), d = unpack_h2<H16>(v.w);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y; f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
  }
  static __device__ __forceinline__ uint4 pack(const float* f) {
    return make_uint4(pack_h2<H16>(f[0], f[1]), pack_h2<H16>(f[2], f[3]), pack_h2<H16>(f[4], f[5]), pack_h2<H16>(f[6], f[7]));
  }
  static __device__ __forceinline__ elem_t one(float v) { return (uint16_t)(pack_h2<H16>(v, 0.f) & 0xffff); }
};
template <> struct Frag<BF16> : FragH<false> {};
template <> struct Frag<F16> : FragH<true> {};

constexpr int TQ = 64, TK = 64, BAND = 128, BDLD = 81;
constexpr int kWaveScratch = 16 * BDLD * 4;  // bytes: the band products [16][81] fp32; later the P tile, at the end the O tile

template <typename E, int DK> struct RelCfg {
  static constexpr int ES = Elem<E>::bytes;
  static constexpr int KS = 64 / ES;                    // k per k-step
  static constexpr int DKP = (DK + KS - 1) / KS * KS;   // head width padded to whole k-steps (zeros)
  static constexpr int NKS = DKP / KS;                  // k-steps over the head width
  static constexpr int RSB = DKP * ES + 16;             // row stride of the K tile and the band, bytes
  static constexpr int VSB = TK * ES + 16;              // row stride of V^T and of a wave's P tile, bytes
  static constexpr int NKV = TK / KS;                   // k-steps over the keys of a tile
  static constexpr int NBO = DK / 16;                   // output column blocks
  static constexpr int K_OFF = 0, V_OFF = K_OFF + TK * RSB, P_OFF = V_OFF + DK * VSB, W_OFF = P_OFF + BAND * RSB;
  static constexpr int LDS = W_OFF + 4 * kWaveScratch;
  static_assert(16 * VSB <= kWaveScratch && 16 * (DK + 1) * 4 <= kWaveScratch, "a wave's P and O tiles fit its scratch patch");
};

template <typename E, int DK>
__global__ __launch_bounds__(256) void rel_attn_kernel(DnRelAttnParams p) {
  typedef RelCfg<E, DK> Cf;
  typedef Frag<E> Fr;
  typedef typename Fr::elem_t elem_t;
  constexpr int N = Fr::N, ES = Cf::ES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if constexpr (Elem<E>::kDtype == DN_F16) f16_saturate();  // q + u, q + v and P beyond 65504 clamp instead of becoming inf (common.h)
  char* const Ks = smem + Cf::K_OFF;
  char* const Vt = smem + Cf::V_OFF;
  char* const Ps = smem + Cf::P_OFF;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lg = l >> 4;
  char* const Ws = smem + Cf::W_OFF + w * kWaveScratch;
  float* const bd = reinterpret_cast<float*>(Ws);
  const int T = p.T, h = blockIdx.y, b = blockIdx.z, i0 = blockIdx.x * TQ;
  int len = p.lengths ? p.lengths[b] : T;
  len = len < 1 ? 1 : (len > T ? T : len);  // (the host refuses empty sequences; this only keeps the reads inside the tensors)
  const int64_t row0 = (int64_t)b * T;
  const int hc = h * DK;

  // ---- this lane's (q + u) and (q + v) fragments: query row i0 + 16 w + lr, 16-byte chunk lg of every k-step
  uint4 qu[Cf::NKS], qv[Cf::NKS];
  {
    int qi = i0 + 16 * w + lr;
    qi = qi < T ? qi : T - 1;  // rows behind the end are computed on the last row and not stored
    const char* qrow = reinterpret_cast<const char*>(p.q) + ((row0 + qi) * p.ldq + hc) * ES;
#pragma unroll
    for (int ks = 0; ks < Cf::NKS; ++ks) {
      const int c = ks * Cf::KS + lg * N;
      float fu[N], fv[N];
      if (c < DK) {
        float f[N];
        Fr::unpack(*reinterpret_cast<const uint4*>(qrow + c * ES), f);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          fu[e] = f[e] + p.bias_u[hc + c + e];
          fv[e] = f[e] + p.bias_v[hc + c + e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < N; ++e) fu[e] = fv[e] = 0.f;
      }
      qu[ks] = Fr::pack(fu);
      qv[ks] = Fr::pack(fv);
    }
  }

  f32x4 acc_o[Cf::NBO];
#pragma unroll
  for (int n = 0; n < Cf::NBO; ++n) acc_o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }

  constexpr int FPR = Cf::DKP / N;  // fragments per staged row
  const int n_tiles = (len + TK - 1) / TK;
  for (int kt = 0; kt < n_tiles; ++kt) {
    const int j0 = kt * TK;
    __syncthreads();  // the previous tile's reads of K, V^T, the band and the scratch patches are done
    // ---- stage the K tile (rows = keys), V transposed (rows = head columns) and the band of offsets
    for (int idx = tid; idx < TK * FPR; idx += 256) {
      const int r = idx / FPR, c = (idx - r * FPR) * N;
      int kj = j0 + r;
      kj = kj < T ? kj : T - 1;
      uint4 kv = make_uint4(0, 0, 0, 0);
      if (c < DK) {
        kv = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(p.k) + ((row0 + kj) * p.ldk + hc + c) * ES);
        const uint4 vv = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(p.v) + ((row0 + kj) * p.ldv + hc + c) * ES);
        const elem_t* ve = reinterpret_cast<const elem_t*>(&vv);
#pragma unroll
        for (int e = 0; e < N; ++e) *reinterpret_cast<elem_t*>(Vt + (c + e) * Cf::VSB + r * ES) = ve[e];
      }
      *reinterpret_cast<uint4*>(Ks + r * Cf::RSB + c * ES) = kv;
    }
    const int dmin = i0 - j0 - (TK - 1);
    for (int idx = tid; idx < BAND * FPR; idx += 256) {
      const int r = idx / FPR, c = (idx - r * FPR) * N;
      int d = dmin + r;
      d = d < -(T - 1) ? -(T - 1) : (d > T - 1 ? T - 1 : d);  // offsets no (query < T, key < T) pair has: any row of the table will do
      uint4 pv = make_uint4(0, 0, 0, 0);
      if (c < DK) pv = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(p.pos) + ((int64_t)(p.pos_zero_row + d) * p.ldp + hc + c) * ES);
      *reinterpret_cast<uint4*>(Ps + r * Cf::RSB + c * ES) = pv;
    }
    __syncthreads();
    // ---- content term (q + u) K^T: 16 x 64, and the band term (q + v) P^T: 16 x 80
    f32x4 acc_s[4], acc_b[5];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc_s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < 5; ++n) acc_b[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < Cf::NKS; ++ks) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const uint4 kb = *reinterpret_cast<const uint4*>(Ks + (16 * n + lr) * Cf::RSB + ks * 64 + lg * 16);
        mma_kstep<E>(acc_s[n], qu[ks], kb);
      }
#pragma unroll
      for (int n = 0; n < 5; ++n) {
        const uint4 pb = *reinterpret_cast<const uint4*>(Ps + (16 * w + 16 * n + lr) * Cf::RSB + ks * 64 + lg * 16);
        mma_kstep<E>(acc_b[n], qv[ks], pb);
      }
    }
#pragma unroll
    for (int n = 0; n < 5; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) bd[(4 * lg + r) * BDLD + 16 * n + lr] = acc_b[n][r];
    __syncthreads();
    // ---- skewed read-back, mask, online softmax (rows 4 lg + r of the wave, keys 16 n + lr of the tile)
    float s[4][4];
    float mx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mx[r] = -INFINITY;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int ri = 4 * lg + r, cj = 16 * n + lr;
        const float v = (acc_s[n][r] + bd[ri * BDLD + ri - cj + (TK - 1)]) * p.scale;
        s[r][n] = (j0 + cj < len) ? v : -INFINITY;
        mx[r] = fmaxf(mx[r], s[r][n]);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o, 64));
    }
    float alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float m_new = fmaxf(m_run[r], mx[r]);  // finite from the first tile on: key 0 is valid
      alpha[r] = expf(m_run[r] - m_new);
      float sum = 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        s[r][n] = expf(s[r][n] - m_new);
        sum += s[r][n];
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
      l_run[r] = l_run[r] * alpha[r] + sum;
      m_run[r] = m_new;
    }
#pragma unroll
    for (int n = 0; n < Cf::NBO; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc_o[n][r] *= alpha[r];
    __syncthreads();  // every lane has read its band products: the patch now takes P in the operand type
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int n = 0; n < 4; ++n) *reinterpret_cast<elem_t*>(Ws + (4 * lg + r) * Cf::VSB + (16 * n + lr) * ES) = Fr::one(s[r][n]);
    __syncthreads();
    // ---- O += P V
#pragma unroll
    for (int ks = 0; ks < Cf::NKV; ++ks) {
      const uint4 pa = *reinterpret_cast<const uint4*>(Ws + lr * Cf::VSB + ks * 64 + lg * 16);
#pragma unroll
      for (int n = 0; n < Cf::NBO; ++n) {
        const uint4 vb = *reinterpret_cast<const uint4*>(Vt + (16 * n + lr) * Cf::VSB + ks * 64 + lg * 16);
        mma_kstep<E>(acc_o[n], pa, vb);
      }
    }
  }
  // ---- normalise and store: through the wave's patch, so that a lane writes 4 consecutive columns
  __syncthreads();
  float* const ot = reinterpret_cast<float*>(Ws);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = 1.0f / l_run[r];
#pragma unroll
    for (int n = 0; n < Cf::NBO; ++n) ot[(4 * lg + r) * (DK + 1) + 16 * n + lr] = acc_o[n][r] * inv;
  }
  __syncthreads();
  for (int idx = l; idx < 16 * (DK / 4); idx += 64) {
    const int r = idx / (DK / 4), c = (idx - r * (DK / 4)) * 4;
    const int qi = i0 + 16 * w + r;
    if (qi < T) {
      const float* o = ot + r * (DK + 1) + c;
      store4(p.out, (row0 + qi) * p.ldo + hc + c, p.dtype, o[0], o[1], o[2], o[3]);
    }
  }
}

template <typename E, int DK>
int launch_rel(const DnRelAttnParams& p, hipStream_t s) {
  const int lds = RelCfg<E, DK>::LDS;
  // once per instantiation (thread-safe static): the kernel's dynamic LDS goes beyond the 64 KB a launch gets unasked
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(rel_attn_kernel<E, DK>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (attr != hipSuccess) {
    dn_set_error("dn_rel_attention: %d bytes of LDS refused: %s", lds, hipGetErrorString(attr));
    return DN_ELAUNCH;
  }
  hipLaunchKernelGGL((rel_attn_kernel<E, DK>), dim3((p.T + TQ - 1) / TQ, p.heads, p.B), dim3(256), lds, s, p);
  return DN_OK;
}
template <typename E>
int launch_rel_dk(const DnRelAttnParams& p, hipStream_t s) {
  switch (p.dim_head) {
    case 16: return launch_rel<E, 16>(p, s);
    case 32: return launch_rel<E, 32>(p, s);
    case 64: return launch_rel<E, 64>(p, s);
  }
  return DN_EINVAL;
}

}  // namespace
}  // namespace dn

extern "C" int dn_rel_attention(const DnRelAttnParams* pp, void* stream) {
  DN_CHECK_ARG(pp != nullptr, "dn_rel_attention: null params");
  const DnRelAttnParams& p = *pp;
  DN_CHECK_ARG(p.q && p.k && p.v && p.out && p.pos && p.bias_u && p.bias_v, "dn_rel_attention: null tensor");
  DN_CHECK_ARG(p.dtype == DN_F32 || p.dtype == DN_BF16 || p.dtype == DN_BF16X3 || p.dtype == DN_F16, "dn_rel_attention: bad dtype %d", p.dtype);
  DN_CHECK_ARG(p.B > 0 && p.heads > 0 && p.T >= 1, "dn_rel_attention: B=%d heads=%d T=%d (an empty sequence has no softmax)", p.B, p.heads, p.T);
  DN_CHECK_ARG(p.dim_head == 16 || p.dim_head == 32 || p.dim_head == 64, "dn_rel_attention: dim_head %d (16, 32 or 64)", p.dim_head);
  DN_CHECK_ARG(p.B <= 65535 && p.heads <= 65535, "dn_rel_attention: B=%d heads=%d exceed the grid", p.B, p.heads);
  const int es = esize(p.dtype), al = 16 / es, hd = p.heads * p.dim_head;
  DN_CHECK_ARG(p.ldq >= hd && p.ldk >= hd && p.ldv >= hd && p.ldo >= hd && p.ldp >= hd && p.ldq % al == 0 && p.ldk % al == 0 && p.ldv % al == 0 &&
                   p.ldp % al == 0 && p.ldo % (p.dtype == DN_BF16X3 ? 32 : 4) == 0,
               "dn_rel_attention: row strides must cover heads * dim_head = %d and keep 16-byte fragments aligned", hd);
  DN_CHECK_ARG((((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.pos | (uintptr_t)p.out) & 15) == 0 &&
                   (p.dtype != DN_BF16X3 || ((uintptr_t)p.out & 127) == 0),
               "dn_rel_attention: q, k, v, pos and out must be 16-byte aligned (out 128 in split rows)");
  DN_CHECK_ARG(p.pos_zero_row >= p.T - 1 && p.pos_zero_row + p.T <= p.pos_rows,
               "dn_rel_attention: a table of %d rows with offset 0 at row %d does not hold the offsets -%d .. %d", p.pos_rows, p.pos_zero_row, p.T - 1, p.T - 1);
  DN_CHECK_ARG(p.scale > 0.f, "dn_rel_attention: scale must be positive");
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (p.dtype == DN_BF16) rc = launch_rel_dk<BF16>(p, s);
  else if (p.dtype == DN_F16) rc = launch_rel_dk<F16>(p, s);
  else rc = launch_rel_dk<F32>(p, s);  // DN_BF16X3: the fp32 form on the fp32 q / k / v / pos that mode keeps beside its split rows
  DN_TRY(rc);
  DN_CHECK_LAUNCH("dn_rel_attention");
  return DN_OK;
}
