// The Conformer speech encoder of the NAR S2UT recipe (scripts/s2ut/train.sh:19-31: --arch nar_s2ut_conformer --attn-type espnet
// --pos-enc-type rel_pos): S2SConformerEncoder (research/TranSpeech/nar_conformer.py:42-74, no speaker embedding) over
// S2TConformerEncoder._forward (fairseq/models/speech_to_text/s2t_conformer.py:91-137), eval mode: Conv1dSubsampler -> sqrt(D) scaling
// -> linear -> ConformerEncoderLayers (fairseq/modules/conformer_layer.py:229-284: half-step FFN, relative-position self-attention,
// convolution module, half-step FFN, LayerNorm); no final LayerNorm.  The subsampler's gathers and the LayerNorm are the kernels of
// nar_common.h; every projection is a dn_conv_gemm launch, the attention dn_rel_attention (rel_attention.hip), the middle of the
// convolution module (GLU -> depthwise conv -> BatchNorm -> swish) dn_glu_dwconv below.  All B * S rows are computed, frames behind an
// utterance's end included: the convolution module is not masked upstream, so those frames reach the valid ones.
#include <new>

#include <algorithm>

#include "common.h"
#include "engine.h"
#include "nar_common.h"

using namespace dn;

namespace dn {
namespace {

// out[b, t, c] = swish(sum_j w[c][j] * glu(x)[b, t + j - k / 2, c] + shift[c]),  glu(x)[.., c] = x[.., c] * sigmoid(x[.., C + c]), taps
// outside [0, S) zero (ConvolutionModule.forward, conformer_layer.py:77-99: glu, depthwise_conv, batch_norm folded into w / shift,
// activation).  A block takes DW_TT frames x 64 channels: the DW_TT + k - 1 rows it reads are staged ONCE in LDS as fp32 GLU values.
constexpr int DW_TT = 32, DW_TC = 64, DW_KMAX = 63;
__global__ __launch_bounds__(256) void glu_dwconv_kernel(const void* __restrict__ x, int in_dtype, const float* __restrict__ w,
                                                          const float* __restrict__ shift, void* __restrict__ out, int out_dtype, int S, int C, int k) {
  __shared__ __attribute__((aligned(16))) float gl[(DW_TT + DW_KMAX - 1) * DW_TC];
  __shared__ __attribute__((aligned(16))) float wl[DW_KMAX * DW_TC];  // [tap][channel]
  const int tid = threadIdx.x, t0 = blockIdx.x * DW_TT, c0 = blockIdx.y * DW_TC, b = blockIdx.z, half = k / 2;
  const int rows = DW_TT + k - 1;
  for (int i = tid; i < rows * (DW_TC / 4); i += 256) {
    const int r = i / (DW_TC / 4), c = (i - r * (DW_TC / 4)) * 4;
    const int t = t0 + r - half;
    float4 v = make_float4(0, 0, 0, 0);
    if (t >= 0 && t < S) {
      const int64_t off = ((int64_t)b * S + t) * 2 * C + c0 + c;
      const float4 a = load4(x, off, in_dtype), g = load4(x, off + C, in_dtype);
      v = make_float4(a.x * sigmoidf_(g.x), a.y * sigmoidf_(g.y), a.z * sigmoidf_(g.z), a.w * sigmoidf_(g.w));
    }
    *reinterpret_cast<float4*>(gl + r * DW_TC + c) = v;
  }
  for (int i = tid; i < k * DW_TC; i += 256) {
    const int c = i / k, j = i - c * k;
    wl[j * DW_TC + c] = w[(int64_t)(c0 + c) * k + j];
  }
  __syncthreads();
  const int c = (tid & 15) * 4;
  const float4 sh = *reinterpret_cast<const float4*>(shift + c0 + c);
#pragma unroll
  for (int i = 0; i < DW_TT / 16; ++i) {
    const int r = (tid >> 4) + 16 * i, t = t0 + r;
    if (t >= S) continue;
    float4 acc = make_float4(0, 0, 0, 0);
    for (int j = 0; j < k; ++j) {
      const float4 g = *reinterpret_cast<const float4*>(gl + (r + j) * DW_TC + c), ww = *reinterpret_cast<const float4*>(wl + j * DW_TC + c);
      acc.x = fmaf(ww.x, g.x, acc.x); acc.y = fmaf(ww.y, g.y, acc.y); acc.z = fmaf(ww.z, g.z, acc.z); acc.w = fmaf(ww.w, g.w, acc.w);
    }
    store4(out, ((int64_t)b * S + t) * C + c0 + c, out_dtype, silu(acc.x + sh.x), silu(acc.y + sh.y), silu(acc.z + sh.z), silu(acc.w + sh.w));
  }
}

// xs[b, t, :] = sqrt(D) * glu(y[b, t, :]) in the activation dtype: the A operand of `linear` (s2t_conformer.py:105-120; nothing is added
// for rel_pos).  Also writes the subsampled lengths.
__global__ __launch_bounds__(256) void conf_embed_kernel(const float* __restrict__ y, const int32_t* __restrict__ src_len, int n_conv, int B, int S, int D,
                                                         float scale, void* __restrict__ xs, int dtype, int32_t* __restrict__ out_len) {
  const int64_t n = (int64_t)B * S * D;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int d = (int)(i % D);
    const int64_t row = i / D;
    const int t = (int)(row % S), b = (int)(row / S);
    if (t == 0 && d == 0) {
      int len = src_len[b];
      for (int l = 0; l < n_conv; ++l) len = subsampled_len(len);
      out_len[b] = len < S ? len : S;
    }
    const float* r = y + row * 2 * D;
    store_act(xs, i, dtype, scale * (r[d] * sigmoidf_(r[D + d])));
  }
}

}  // namespace
}  // namespace dn

extern "C" int dn_glu_dwconv(const void* x, const float* w, const float* shift, void* out, int32_t B, int32_t S, int32_t C, int32_t k, int32_t dtype,
                             void* stream) {
  DN_CHECK_ARG(x && w && shift && out, "dn_glu_dwconv: null argument");
  DN_CHECK_ARG(dtype == DN_F32 || dtype == DN_BF16 || dtype == DN_BF16X3 || dtype == DN_F16, "dn_glu_dwconv: bad dtype %d", dtype);
  DN_CHECK_ARG(B > 0 && B <= 65535 && S > 0, "dn_glu_dwconv: B=%d S=%d", B, S);
  DN_CHECK_ARG(C > 0 && C % 64 == 0, "dn_glu_dwconv: C=%d must be a multiple of 64", C);
  DN_CHECK_ARG(k >= 1 && k <= DW_KMAX && k % 2 == 1, "dn_glu_dwconv: kernel %d must be odd and <= %d (an even depthwise kernel is not 'same'-padded upstream)", k, DW_KMAX);
  DN_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)shift) & 15) == 0 && (dtype != DN_BF16X3 || ((uintptr_t)out & 127) == 0),
               "dn_glu_dwconv: x, shift and out must be 16-byte aligned (out 128 in split rows)");
  const int in_dtype = dtype == DN_BF16X3 ? DN_F32 : dtype;
  hipLaunchKernelGGL(glu_dwconv_kernel, dim3((S + DW_TT - 1) / DW_TT, C / DW_TC, B), dim3(256), 0, (hipStream_t)stream, x, in_dtype, w, shift, out, dtype, S, C, k);
  DN_CHECK_LAUNCH("dn_glu_dwconv");
  return DN_OK;
}

struct DnConformerEnc {
  DnConformerEncConfig cfg;
  const void *conv0_W, *conv1_W, *lin_W, *pe, *f1w1_W, *f1w2_W, *f2w1_W, *f2w2_W, *qkv_W, *pos_W, *out_W, *pw1_W, *pw2_W;
  const float *conv0_b, *conv1_b, *lin_b, *f1w1_b, *f1w2_b, *f2w1_b, *f2w2_b, *qkv_b, *out_b, *bias_u, *bias_v, *dw_w, *dw_shift, *ln_g, *ln_b, *zeros;
};
static const int kConformerEncTensors = 29;

extern "C" int dn_conformer_encoder_create(const DnConformerEncConfig* cfg, const void* const* w, int32_t n, DnConformerEnc** out) {
  DN_CHECK_ARG(cfg && w && out, "dn_conformer_encoder_create: null argument");
  DN_CHECK_ARG(n == kConformerEncTensors, "dn_conformer_encoder_create: expected %d packed tensors, got %d", kConformerEncTensors, n);
  DN_CHECK_ARG(cfg->dtype == DN_F32 || cfg->dtype == DN_BF16 || cfg->dtype == DN_BF16X3 || cfg->dtype == DN_F16, "dn_conformer_encoder_create: bad dtype");
  DN_CHECK_ARG(cfg->dim > 0 && cfg->dim % 64 == 0 && cfg->dim <= 1024 && cfg->heads > 0 && cfg->dim % cfg->heads == 0,
               "dn_conformer_encoder_create: embed dim %d must be a multiple of 64 (<= 1024) and of the head count", cfg->dim);
  const int dh = cfg->dim / cfg->heads;
  DN_CHECK_ARG(dh == 16 || dh == 32 || dh == 64, "dn_conformer_encoder_create: head width %d (16, 32 or 64)", dh);
  DN_CHECK_ARG(cfg->ffn > 0 && cfg->ffn % 64 == 0 && cfg->layers >= 1 && cfg->input_dim > 0 && cfg->conv_channels > 0 && cfg->conv_channels % 8 == 0 &&
                   (cfg->kernel * (cfg->conv_channels / 2)) % 64 == 0 && cfg->kernel >= 1 && cfg->kernel % 2 == 1,
               "dn_conformer_encoder_create: ffn %% 64, conv_channels %% 8, odd kernel, kernel * conv_channels / 2 a multiple of 64");
  DN_CHECK_ARG(cfg->depthwise_kernel >= 1 && cfg->depthwise_kernel <= DW_KMAX && cfg->depthwise_kernel % 2 == 1,
               "dn_conformer_encoder_create: depthwise kernel %d must be odd and <= %d", cfg->depthwise_kernel, DW_KMAX);
  DN_CHECK_ARG(cfg->max_frames >= 1, "dn_conformer_encoder_create: max_frames %d", cfg->max_frames);
  for (int i = 0; i < n; ++i) DN_CHECK_ARG(w[i] != nullptr, "dn_conformer_encoder_create: packed tensor %d is null", i);
  DnConformerEnc* m = new (std::nothrow) DnConformerEnc();
  DN_CHECK_ARG(m != nullptr, "dn_conformer_encoder_create: out of host memory");
  m->cfg = *cfg;
  int i = 0;
  auto f = [&]() { return (const float*)w[i++]; };
  m->conv0_W = w[i++]; m->conv0_b = f(); m->conv1_W = w[i++]; m->conv1_b = f(); m->lin_W = w[i++]; m->lin_b = f(); m->pe = w[i++];
  m->f1w1_W = w[i++]; m->f1w1_b = f(); m->f1w2_W = w[i++]; m->f1w2_b = f();
  m->f2w1_W = w[i++]; m->f2w1_b = f(); m->f2w2_W = w[i++]; m->f2w2_b = f();
  m->qkv_W = w[i++]; m->qkv_b = f(); m->pos_W = w[i++]; m->out_W = w[i++]; m->out_b = f(); m->bias_u = f(); m->bias_v = f();
  m->pw1_W = w[i++]; m->dw_w = f(); m->dw_shift = f(); m->pw2_W = w[i++]; m->ln_g = f(); m->ln_b = f(); m->zeros = f();
  *out = m;
  return DN_OK;
}

extern "C" void dn_conformer_encoder_destroy(DnConformerEnc* m) { delete m; }

namespace {
inline int conf_side_dt(int dtype) { return dtype == DN_BF16X3 ? DN_F32 : dtype; }
inline int conf_frames(int L) {
  const int s1 = L <= 0 ? 0 : (L - 1) / 2 + 1;
  return s1 <= 0 ? 0 : (s1 - 1) / 2 + 1;
}

struct ConfBufs { void *cols0, *cols1, *xn, *qkv, *posb, *ao, *h; float *y0, *y1, *xa, *xb; };
ConfBufs plan_conf(const DnConformerEnc* m, int B, int L, Arena& ar) {
  const DnConformerEncConfig& c = m->cfg;
  const int es = esize(c.dtype), D = c.dim, S1 = L <= 0 ? 0 : (L - 1) / 2 + 1, S = conf_frames(L);
  const int K0 = padk(c.kernel * c.input_dim), K1 = c.kernel * (c.conv_channels / 2);
  ConfBufs b;
  b.cols0 = ar.take((size_t)B * S1 * K0 * es);
  b.y0 = (float*)ar.take((size_t)B * S1 * c.conv_channels * 4);
  b.cols1 = ar.take((size_t)B * S * K1 * es);
  b.y1 = (float*)ar.take((size_t)B * S * 2 * D * 4);
  b.xa = (float*)ar.take((size_t)B * S * D * 4);
  b.xb = (float*)ar.take((size_t)B * S * D * 4);
  b.xn = ar.take((size_t)B * S * D * es);
  b.qkv = ar.take((size_t)B * S * 3 * D * es);     // also the 2 D-wide input of the GLU
  b.posb = ar.take((size_t)(2 * S - 1) * D * es);  // linear_pos(pe) of the layer at hand
  b.ao = ar.take((size_t)B * S * D * es);
  b.h = ar.take((size_t)B * S * c.ffn * es);
  return b;
}
inline int conf_ew(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 4096); }
}  // namespace

extern "C" size_t dn_conformer_encoder_workspace_bytes(const DnConformerEnc* m, int32_t B, int32_t L) {
  if (!m || B <= 0 || L <= 0) return 0;
  Arena a{nullptr, 0, 0};
  (void)plan_conf(m, B, L, a);
  return a.off + 512;
}

extern "C" int dn_conformer_encoder_forward(DnConformerEnc* m, const float* feats, const int32_t* src_lengths, int32_t B, int32_t L, float* enc_out,
                                            int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && feats && src_lengths && enc_out && out_lengths && workspace, "dn_conformer_encoder_forward: null argument");
  const DnConformerEncConfig& c = m->cfg;
  const int S1 = L <= 0 ? 0 : (L - 1) / 2 + 1, S = conf_frames(L);
  DN_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && S >= 1 && S <= c.max_frames,
               "dn_conformer_encoder_forward: B=%d L=%d (%d frames after the subsampler; the position table holds %d)", B, L, S, c.max_frames);
  DN_CHECK_ARG((int64_t)B * S1 * std::max(padk(c.kernel * c.input_dim), c.conv_channels) < (int64_t)1 << 31 && (int64_t)B * S * std::max(c.ffn, 3 * c.dim) < (int64_t)1 << 31,
               "dn_conformer_encoder_forward: B=%d L=%d: a buffer exceeds 2^31 elements", B, L);
  DN_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "dn_conformer_encoder_forward: workspace must be 256-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  const ConfBufs b = plan_conf(m, B, L, ar);
  if (ar.off > workspace_bytes) {
    dn_set_error("dn_conformer_encoder_forward: workspace %zu < required %zu", workspace_bytes, ar.off);
    return DN_EWORKSPACE;
  }
  const int dtype = c.dtype, es = esize(dtype), D = c.dim, F = c.ffn, H = c.heads, dh = D / H, Ch = c.conv_channels / 2, k = c.kernel;
  const int K0 = padk(k * c.input_dim), K1 = k * Ch, M = B * S, P = 2 * S - 1;
  const int sdt = conf_side_dt(dtype), ses = esize(sdt);
  // ---- Conv1dSubsampler, as dn_nar_encoder_forward
  hipLaunchKernelGGL((strided_rows_kernel<false>), dim3(conf_ew((int64_t)B * S1 * K0)), dim3(256), 0, s, feats, B, L, S1, c.input_dim, k, K0, b.cols0, dtype);
  {
    DnGemmParams p = gemm_base(dtype, B * S1, c.conv_channels, K0, S1);
    p.terms[0].A = b.cols0; p.terms[0].lda = K0; p.terms[0].W = m->conv0_W;
    p.bias = m->conv0_b; p.out = b.y0; p.ldo = c.conv_channels; p.out_dtype = DN_F32;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  hipLaunchKernelGGL((strided_rows_kernel<true>), dim3(conf_ew((int64_t)M * K1)), dim3(256), 0, s, b.y0, B, S1, S, Ch, k, K1, b.cols1, dtype);
  {
    DnGemmParams p = gemm_base(dtype, M, 2 * D, K1, S);
    p.terms[0].A = b.cols1; p.terms[0].lda = K1; p.terms[0].W = m->conv1_W;
    p.bias = m->conv1_b; p.out = b.y1; p.ldo = 2 * D; p.out_dtype = DN_F32;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  // ---- x = linear(sqrt(D) * glu(conv))  (s2t_conformer.py:108-120)
  hipLaunchKernelGGL(conf_embed_kernel, dim3(conf_ew((int64_t)M * D)), dim3(256), 0, s, b.y1, src_lengths, 2, B, S, D, sqrtf((float)D), b.xn, dtype, out_lengths);
  float *cur = b.xa, *other = b.xb;
  {
    DnGemmParams p = gemm_base(dtype, M, D, D, S);
    p.terms[0].A = b.xn; p.terms[0].lda = D; p.terms[0].W = m->lin_W;
    p.bias = m->lin_b; p.out = cur; p.ldo = D; p.out_dtype = DN_F32;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  auto ln = [&](const float* x, const float* g, const float* be, void* y, int odt) {
    hipLaunchKernelGGL(layernorm_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, D, y, D, odt, M, D, g, be);
  };
  auto proj = [&](const void* A, int rows, int T, int N, int K, const void* W, const float* bias, int epi, void* out, int odt) -> int {
    DnGemmParams p = gemm_base(dtype, rows, N, K, T);
    p.terms[0].A = A; p.terms[0].lda = K; p.terms[0].W = W;
    p.bias = bias; p.epilogue = epi; p.out = out; p.ldo = N; p.out_dtype = odt;
    return dn_conv_gemm(&p, s);
  };
  auto resadd = [&](const void* A, int K, const void* W, const float* bias) -> int {  // x += A W^T + bias
    DnGemmParams p = gemm_base(dtype, M, D, K, S);
    p.terms[0].A = A; p.terms[0].lda = K; p.terms[0].W = W;
    p.bias = bias; p.epilogue = DN_EPI_RESADD; p.res = cur; p.ldr = D; p.out = cur; p.ldo = D; p.out_dtype = DN_F32;
    return dn_conv_gemm(&p, s);
  };
  auto ffn = [&](const float* g, const float* be, const void* w1, const float* b1, const void* w2, const float* b2) -> int {
    ln(cur, g, be, b.xn, dtype);  // FeedForwardModule.forward (conformer_layer.py:132-144): layer_norm, w_1, swish, w_2; the 0.5 is in w2 / b2
    DN_TRY(proj(b.xn, M, S, F, D, w1, b1, DN_EPI_SILU, b.h, dtype));
    return resadd(b.h, F, w2, b2);
  };
  // rows of the packed positional encodings for this S: offset d at row (max_frames - 1) + d
  const void* pe = eoff(m->pe, (size_t)(c.max_frames - S) * D, es);
  for (int l = 0; l < c.layers; ++l) {
    const float* g = m->ln_g + (size_t)l * 5 * D;
    const float* be = m->ln_b + (size_t)l * 5 * D;
    const size_t wDD = (size_t)l * padn(D) * D;
    DN_TRY(ffn(g, be, eoff(m->f1w1_W, (size_t)l * padn(F) * D, es), m->f1w1_b + (size_t)l * F, eoff(m->f1w2_W, (size_t)l * padn(D) * F, es),
               m->f1w2_b + (size_t)l * D));                                                                                    // :243-245
    ln(cur, g + D, be + D, b.xn, dtype);                                                                                        // :247
    DN_TRY(proj(b.xn, M, S, 3 * D, D, eoff(m->qkv_W, (size_t)l * padn(3 * D) * D, es), m->qkv_b + (size_t)l * 3 * D, DN_EPI_BIAS, b.qkv, sdt));
    DN_TRY(proj(pe, P, P, D, D, eoff(m->pos_W, wDD, es), m->zeros, DN_EPI_BIAS, b.posb, sdt));  // linear_pos(pe), no bias
    {
      DnRelAttnParams a;
      memset(&a, 0, sizeof(a));
      a.q = b.qkv; a.k = eoff(b.qkv, D, ses); a.v = eoff(b.qkv, 2 * D, ses); a.out = b.ao;
      a.ldq = a.ldk = a.ldv = 3 * D; a.ldo = D;
      a.B = B; a.T = S; a.heads = H; a.dim_head = dh; a.dtype = dtype; a.lengths = out_lengths;
      a.scale = 1.0f / sqrtf((float)dh);
      a.pos = b.posb; a.ldp = D; a.pos_zero_row = S - 1; a.pos_rows = P;
      a.bias_u = m->bias_u + (size_t)l * D; a.bias_v = m->bias_v + (size_t)l * D;
      DN_TRY(dn_rel_attention(&a, s));
    }
    DN_TRY(resadd(b.ao, D, eoff(m->out_W, wDD, es), m->out_b + (size_t)l * D));                                                  // :248-266
    ln(cur, g + 2 * D, be + 2 * D, b.xn, dtype);  // ConvolutionModule (:77-99), unmasked
    DN_TRY(proj(b.xn, M, S, 2 * D, D, eoff(m->pw1_W, (size_t)l * padn(2 * D) * D, es), m->zeros, DN_EPI_BIAS, b.qkv, sdt));
    DN_TRY(dn_glu_dwconv(b.qkv, m->dw_w + (size_t)l * D * c.depthwise_kernel, m->dw_shift + (size_t)l * D, b.ao, B, S, D, c.depthwise_kernel, dtype, s));
    DN_TRY(resadd(b.ao, D, eoff(m->pw2_W, wDD, es), m->zeros));                                                                 // :268-274
    DN_TRY(ffn(g + 3 * D, be + 3 * D, eoff(m->f2w1_W, (size_t)l * padn(F) * D, es), m->f2w1_b + (size_t)l * F, eoff(m->f2w2_W, (size_t)l * padn(D) * F, es),
               m->f2w2_b + (size_t)l * D));                                                                                    // :276-281
    float* dst = l == c.layers - 1 ? enc_out : other;  // final_layer_norm (:283); the last layer's is the encoder's output
    ln(cur, g + 4 * D, be + 4 * D, dst, DN_F32);
    other = cur;
    cur = dst;
  }
  DN_CHECK_LAUNCH("dn_conformer_encoder_forward");
  return DN_OK;
}
