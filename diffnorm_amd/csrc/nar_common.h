// What the NAR decoder, the two speech encoders and the HuBERT front end share (nar_decoder.hip, nar_encoder.hip,
// conformer_encoder.hip, hubert.hip; kmeans.hip takes `linear` for the assignment's scores): the LayerNorm kernel, the
// Conv1dSubsampler, and the few host helpers their passes are written in.  Internal linkage, one copy per unit.
#pragma once
#include <algorithm>

#include "common.h"
#include "engine.h"

namespace dn {
namespace {

// nn.GELU() (erf form) in fp32
__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// LayerNorm (eps 1e-5, biased variance, affine): x fp32 [M, ldx] -> y [M, ldy] in out_dtype (pad columns zeroed); GELU: the exact
// GELU behind the affine.  One wave per row, D <= 1024 in registers.  y may be x itself (fp32, ldy == ldx): a wave holds its whole
// row before it stores, and neither pointer is __restrict__.
template <bool GELU>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* x, int ldx, void* y, int ldy, int out_dtype, int M, int D,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* xr = x + (int64_t)row * ldx;
  float4 v[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = c < D ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0, 0, 0, 0);
    s += v[i].x + v[i].y + v[i].z + v[i].w;
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) {
      const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
      q += a * a + b * b + cc * cc + d * d;
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + 1e-5f);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c >= ldy) continue;
    float o[4] = {0, 0, 0, 0};
    if (c < D) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
      o[0] = (v[i].x - mean) * rstd * g.x + be.x; o[1] = (v[i].y - mean) * rstd * g.y + be.y;
      o[2] = (v[i].z - mean) * rstd * g.z + be.z; o[3] = (v[i].w - mean) * rstd * g.w + be.w;
      if (GELU) { o[0] = gelu_exact(o[0]); o[1] = gelu_exact(o[1]); o[2] = gelu_exact(o[2]); o[3] = gelu_exact(o[3]); }
    }
    store4(y, (int64_t)row * ldy + c, out_dtype, o[0], o[1], o[2], o[3]);
  }
}

// ---- the Conv1dSubsampler's gathers, shared by the two speech encoders (nar_encoder.hip, conformer_encoder.hip)
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// Rows of the contraction that IS a Conv1d(k, stride 2, padding k / 2) over [B, Lin, C]: cols[b * Lout + t][j * C + c] = in[b][2 t + j - k / 2][c]
// (zero outside [0, Lin); columns >= k * C zero: the K padding).  GLU: `in` is the previous conv's output [B, Lin, 2 C] and the gathered
// value is a * sigmoid(g) with a = in[..][c], g = in[..][C + c] (F.glu over the channels, convolution.py:56).  The whole PADDED batch is
// convolved, frames behind an utterance's end included, as upstream.
template <bool GLU>
__global__ __launch_bounds__(256) void strided_rows_kernel(const float* __restrict__ in, int B, int Lin, int Lout, int C, int k, int Kp,
                                                           void* __restrict__ cols, int dtype) {
  const int64_t n = (int64_t)B * Lout * Kp;
  const int ld_in = GLU ? 2 * C : C;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int col = (int)(i % Kp);
    const int64_t row = i / Kp;
    const int t = (int)(row % Lout), b = (int)(row / Lout);
    float v = 0.f;
    if (col < k * C) {
      const int j = col / C, c = col - j * C;
      const int src = 2 * t + j - k / 2;
      if (src >= 0 && src < Lin) {
        const float* r = in + ((int64_t)b * Lin + src) * ld_in;
        v = GLU ? r[c] * sigmoidf_(r[C + c]) : r[c];
      }
    }
    store_act(cols, i, dtype, v);
  }
}

// Frames behind n_conv stride-2 convolutions with padding k / 2 (any odd k): floor((len - 1) / 2 + 1) each (convolution.py:45-49)
__host__ __device__ __forceinline__ int subsampled_len(int len, int n_conv) {
  for (int l = 0; l < n_conv; ++l) len = len <= 0 ? 0 : (len - 1) / 2 + 1;
  return len;
}

// ---------------------------------------------------------------------------------------------- host helpers of the passes
// layer l of a stacked packed weight [layers][padn(N)][K]
inline const void* layer_mat(const void* W, int l, int N, int K, int es) { return eoff(W, (size_t)l * padn(N) * K, es); }

// What the launches of a pass share: the arithmetic, M rows of T per sequence, the width D of the fp32 residual stream, the stream.
struct Rows { int dtype, M, T, D; hipStream_t s; };

inline void layernorm(const Rows& r, const float* x, const float* gamma, const float* beta, void* y, int out_dtype) {
  hipLaunchKernelGGL((layernorm_kernel<false>), dim3((r.M + 3) / 4), dim3(256), 0, r.s, x, r.D, y, r.D, out_dtype, r.M, r.D, gamma, beta);
}
// y = gelu(LayerNorm(x)); in place when y == x and out_dtype is DN_F32
inline void layernorm_gelu(const Rows& r, const float* x, const float* gamma, const float* beta, void* y, int out_dtype) {
  hipLaunchKernelGGL((layernorm_kernel<true>), dim3((r.M + 3) / 4), dim3(256), 0, r.s, x, r.D, y, r.D, out_dtype, r.M, r.D, gamma, beta);
}

// out[M, N] = epilogue(A[M, K] W^T + bias) in out_dtype; A and out dense
inline int linear(const Rows& r, const void* A, int K, const void* W, const float* bias, int N, int epilogue, void* out, int out_dtype) {
  DnGemmParams p = gemm_base(r.dtype, r.M, N, K, r.T);
  p.terms[0].A = A; p.terms[0].lda = K; p.terms[0].W = W;
  p.bias = bias; p.epilogue = epilogue; p.out = out; p.ldo = N; p.out_dtype = out_dtype;
  return dn_conv_gemm(&p, r.s);
}

// x[M, D] += A[M, K] W^T + bias on the fp32 residual stream
inline int linear_resadd(const Rows& r, const void* A, int K, const void* W, const float* bias, float* x) {
  DnGemmParams p = gemm_base(r.dtype, r.M, r.D, K, r.T);
  p.terms[0].A = A; p.terms[0].lda = K; p.terms[0].W = W;
  p.bias = bias; p.epilogue = DN_EPI_RESADD; p.res = x; p.ldr = r.D; p.out = x; p.ldo = r.D; p.out_dtype = DN_F32;
  return dn_conv_gemm(&p, r.s);
}

// x += W2 act(W1 LayerNorm(x) + b1) + b2 through xn [M, D] and h [M, F]: the FFN of a fairseq layer (act = DN_EPI_RELU,
// transformer_layer.py:210-215 and :495-508) and of a Conformer layer (DN_EPI_SILU; FeedForwardModule.forward, conformer_layer.py:132-144)
inline int ffn_block(const Rows& r, float* x, void* xn, void* h, int F, const float* gamma, const float* beta, const void* W1, const float* b1,
                     const void* W2, const float* b2, int act) {
  layernorm(r, x, gamma, beta, xn, r.dtype);
  DN_TRY(linear(r, xn, r.D, W1, b1, F, act, h, r.dtype));
  return linear_resadd(r, h, F, W2, b2, x);
}

// The fields DnAttnParams and DnRelAttnParams share: B sequences of T queries, `heads` heads of width dh, k and v with one leading
// dimension, out [B * T, heads * dh]; scale = head_dim^-0.5 (multihead_attention.py)
template <class P>
inline P attn_params(int dtype, int heads, int dh, const void* q, int ldq, const void* k, const void* v, int ldkv, int B, int T, const int32_t* lengths,
                     void* out) {
  P a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.out = out;
  a.ldq = ldq; a.ldk = a.ldv = ldkv; a.ldo = heads * dh;
  a.B = B; a.T = T; a.heads = heads; a.dim_head = dh; a.dtype = dtype; a.lengths = lengths;
  a.scale = 1.0f / sqrtf((float)dh);
  return a;
}
// Tk keys per sequence, `lengths` of them valid; Tk = 0: the keys are the queries' own frames
inline int attention(int dtype, int heads, int dh, const void* q, int ldq, const void* k, const void* v, int ldkv, int B, int T, int Tk,
                     const int32_t* lengths, void* out, hipStream_t s) {
  DnAttnParams a = attn_params<DnAttnParams>(dtype, heads, dh, q, ldq, k, v, ldkv, B, T, lengths, out);
  a.Tk = Tk;
  return dn_attention(&a, s);
}

// x += out_W attention(qkv_W xn + qkv_b) + out_b: the self-attention of a layer on the normalised rows xn [M, D] and the fp32
// residual stream x, through qkv [M, 3 D] (q ; k ; v) and ao [M, D]; the keys are the sequence's own frames, lengths[b] of them valid
inline int self_attention_block(const Rows& r, int heads, int dh, const void* xn, const void* qkv_W, const float* qkv_b, const void* out_W,
                                const float* out_b, void* qkv, void* ao, const int32_t* lengths, float* x) {
  const int D = r.D, sdt = side_dtype(r.dtype), ses = esize(sdt);
  DN_TRY(linear(r, xn, D, qkv_W, qkv_b, 3 * D, DN_EPI_BIAS, qkv, sdt));
  DN_TRY(attention(r.dtype, heads, dh, qkv, 3 * D, eoff(qkv, D, ses), eoff(qkv, 2 * D, ses), 3 * D, r.M / r.T, r.T, 0, lengths, ao, r.s));
  return linear_resadd(r, ao, D, out_W, out_b, x);
}

// What every *_create here asks of its arguments and of the fields the three configs share
template <class Cfg>
inline int check_create(const char* who, const Cfg* cfg, const void* const* w, int n, int expected, const void* out) {
  DN_CHECK_ARG(cfg && w && out, "%s: null argument", who);
  DN_CHECK_ARG(n == expected, "%s: expected %d packed tensors, got %d", who, expected, n);
  DN_CHECK_ARG(cfg->dtype == DN_F32 || cfg->dtype == DN_BF16 || cfg->dtype == DN_BF16X3 || cfg->dtype == DN_F16, "%s: bad dtype", who);
  DN_CHECK_ARG(cfg->dim > 0 && cfg->dim % 64 == 0 && cfg->dim <= 1024 && cfg->heads > 0 && cfg->dim % cfg->heads == 0 && (cfg->dim / cfg->heads) % 4 == 0,
               "%s: embed dim %d must be a multiple of 64 (<= 1024) and of the head count", who, cfg->dim);
  DN_CHECK_ARG(cfg->ffn > 0 && cfg->ffn % 64 == 0 && cfg->layers >= 1, "%s: ffn %% 64, at least one layer", who);
  for (int i = 0; i < n; ++i) DN_CHECK_ARG(w[i] != nullptr, "%s: packed tensor %d is null", who, i);
  return DN_OK;
}

struct TableCursor {  // over a packed tensor table, in table order
  const void* const* w;
  int i;
  const void* next_mat() { return w[i++]; }                 // a contraction operand, in the engine's arithmetic
  const float* next_vec() { return (const float*)w[i++]; }  // fp32
};

// Conv1dSubsampler (convolution.py:13-57): two Conv1d(k, stride 2, padding k / 2), a GLU behind each.  A strided conv is a contraction over
// gathered rows; the first GLU is applied by the second gather, the second is left to the caller's embedding kernel.
struct Subsampler {
  int input_dim, conv_channels, kernel, dim;
  const void* conv0_W;  // (members in table order: both encoders' tables open with these four)
  const float* conv0_b;
  const void* conv1_W;
  const float* conv1_b;
  struct Bufs { void *cols0, *cols1; float *y0, *y1; };

  int K0() const { return padk(kernel * input_dim); }
  int K1() const { return kernel * (conv_channels / 2); }
  int check(const char* who) const {
    DN_CHECK_ARG(input_dim > 0 && conv_channels > 0 && conv_channels % 8 == 0 && K1() % 64 == 0 && kernel >= 1 && kernel % 2 == 1,
                 "%s: conv_channels %% 8, odd kernel, kernel * conv_channels / 2 a multiple of 64", who);
    return DN_OK;
  }
  Bufs plan(int dtype, int B, int L, Arena& ar) const {
    const int es = esize(dtype), S1 = subsampled_len(L, 1), S = subsampled_len(L, 2);
    Bufs b;
    b.cols0 = ar.take((size_t)B * S1 * K0() * es);
    b.y0 = (float*)ar.take((size_t)B * S1 * conv_channels * 4);
    b.cols1 = ar.take((size_t)B * S * K1() * es);
    b.y1 = (float*)ar.take((size_t)B * S * 2 * dim * 4);
    return b;
  }
  // feats fp32 [B, L, input_dim] -> b.y1 fp32 [B, S, 2 dim]: the second conv's output, its GLU not yet applied
  int run(int dtype, const float* feats, int B, int L, const Bufs& b, hipStream_t s) const {
    const int S1 = subsampled_len(L, 1), S = subsampled_len(L, 2), Ch = conv_channels / 2;
    hipLaunchKernelGGL((strided_rows_kernel<false>), dim3(ew_grid((int64_t)B * S1 * K0())), dim3(256), 0, s, feats, B, L, S1, input_dim, kernel, K0(), b.cols0,
                       dtype);
    DN_TRY(linear(Rows{dtype, B * S1, S1, 0, s}, b.cols0, K0(), conv0_W, conv0_b, conv_channels, DN_EPI_BIAS, b.y0, DN_F32));
    hipLaunchKernelGGL((strided_rows_kernel<true>), dim3(ew_grid((int64_t)B * S * K1())), dim3(256), 0, s, b.y0, B, S1, S, Ch, kernel, K1(), b.cols1, dtype);
    return linear(Rows{dtype, B * S, S, 0, s}, b.cols1, K1(), conv1_W, conv1_b, 2 * dim, DN_EPI_BIAS, b.y1, DN_F32);
  }
};

}  // namespace
}  // namespace dn
