// The Conformer speech encoder of the NAR S2UT recipe (scripts/s2ut/train.sh:19-31: --arch nar_s2ut_conformer --attn-type espnet
// --pos-enc-type rel_pos): S2SConformerEncoder (research/TranSpeech/nar_conformer.py:42-74, no speaker embedding) over
// S2TConformerEncoder._forward (fairseq/models/speech_to_text/s2t_conformer.py:91-137), eval mode: Conv1dSubsampler -> sqrt(D) scaling
// -> linear -> ConformerEncoderLayers (fairseq/modules/conformer_layer.py:229-284: half-step FFN, relative-position self-attention,
// convolution module, half-step FFN, LayerNorm); no final LayerNorm.  The subsampler and the LayerNorm are nar_common.h's; every
// projection is a dn_conv_gemm launch, the attention dn_rel_attention (rel_attention.hip), the middle of the
// convolution module (GLU -> depthwise conv -> BatchNorm -> swish) dn_glu_dwconv below.  All B * S rows are computed, frames behind an
// utterance's end included: the convolution module is not masked upstream, so those frames reach the valid ones.
#include <new>

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
      const int len = subsampled_len(src_len[b], n_conv);
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
  Subsampler sub;
  const void *lin_W, *pe, *f1w1_W, *f1w2_W, *f2w1_W, *f2w2_W, *qkv_W, *pos_W, *out_W, *pw1_W, *pw2_W;
  const float *lin_b, *f1w1_b, *f1w2_b, *f2w1_b, *f2w2_b, *qkv_b, *out_b, *bias_u, *bias_v, *dw_w, *dw_shift, *ln_g, *ln_b, *zeros;
};
static const int kConformerEncTensors = 29;

extern "C" int dn_conformer_encoder_create(const DnConformerEncConfig* cfg, const void* const* w, int32_t n, DnConformerEnc** out) {
  DN_TRY(check_create("dn_conformer_encoder_create", cfg, w, n, kConformerEncTensors, out));
  const int dh = cfg->dim / cfg->heads;
  DN_CHECK_ARG(dh == 16 || dh == 32 || dh == 64, "dn_conformer_encoder_create: head width %d (16, 32 or 64)", dh);
  TableCursor t{w, 0};
  const Subsampler sub{cfg->input_dim, cfg->conv_channels, cfg->kernel, cfg->dim, t.next_mat(), t.next_vec(), t.next_mat(), t.next_vec()};
  DN_TRY(sub.check("dn_conformer_encoder_create"));
  DN_CHECK_ARG(cfg->depthwise_kernel >= 1 && cfg->depthwise_kernel <= DW_KMAX && cfg->depthwise_kernel % 2 == 1,
               "dn_conformer_encoder_create: depthwise kernel %d must be odd and <= %d", cfg->depthwise_kernel, DW_KMAX);
  DN_CHECK_ARG(cfg->max_frames >= 1, "dn_conformer_encoder_create: max_frames %d", cfg->max_frames);
  DnConformerEnc* m = new (std::nothrow) DnConformerEnc();
  DN_CHECK_ARG(m != nullptr, "dn_conformer_encoder_create: out of host memory");
  m->cfg = *cfg;
  m->sub = sub;
  m->lin_W = t.next_mat(); m->lin_b = t.next_vec(); m->pe = t.next_mat();
  m->f1w1_W = t.next_mat(); m->f1w1_b = t.next_vec(); m->f1w2_W = t.next_mat(); m->f1w2_b = t.next_vec();
  m->f2w1_W = t.next_mat(); m->f2w1_b = t.next_vec(); m->f2w2_W = t.next_mat(); m->f2w2_b = t.next_vec();
  m->qkv_W = t.next_mat(); m->qkv_b = t.next_vec(); m->pos_W = t.next_mat(); m->out_W = t.next_mat(); m->out_b = t.next_vec();
  m->bias_u = t.next_vec(); m->bias_v = t.next_vec();
  m->pw1_W = t.next_mat(); m->dw_w = t.next_vec(); m->dw_shift = t.next_vec(); m->pw2_W = t.next_mat();
  m->ln_g = t.next_vec(); m->ln_b = t.next_vec(); m->zeros = t.next_vec();
  *out = m;
  return DN_OK;
}

extern "C" void dn_conformer_encoder_destroy(DnConformerEnc* m) { delete m; }

namespace {
struct ConfBufs { Subsampler::Bufs sub; void *xn, *qkv, *posb, *ao, *h; float *xa, *xb; };
ConfBufs plan_conf(const DnConformerEnc* m, int B, int L, Arena& ar) {
  const DnConformerEncConfig& c = m->cfg;
  const int es = esize(c.dtype), D = c.dim, S = subsampled_len(L, 2);
  ConfBufs b;
  b.sub = m->sub.plan(c.dtype, B, L, ar);
  b.xa = (float*)ar.take((size_t)B * S * D * 4);
  b.xb = (float*)ar.take((size_t)B * S * D * 4);
  b.xn = ar.take((size_t)B * S * D * es);
  b.qkv = ar.take((size_t)B * S * 3 * D * es);     // also the 2 D-wide input of the GLU
  b.posb = ar.take((size_t)(2 * S - 1) * D * es);  // linear_pos(pe) of the layer at hand
  b.ao = ar.take((size_t)B * S * D * es);
  b.h = ar.take((size_t)B * S * c.ffn * es);
  return b;
}
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
  const int S1 = subsampled_len(L, 1), S = subsampled_len(L, 2);
  DN_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && S >= 1 && S <= c.max_frames,
               "dn_conformer_encoder_forward: B=%d L=%d (%d frames after the subsampler; the position table holds %d)", B, L, S, c.max_frames);
  DN_CHECK_ARG((int64_t)B * S1 * std::max(m->sub.K0(), c.conv_channels) < (int64_t)1 << 31 && (int64_t)B * S * std::max(c.ffn, 3 * c.dim) < (int64_t)1 << 31,
               "dn_conformer_encoder_forward: B=%d L=%d: a buffer exceeds 2^31 elements", B, L);
  hipStream_t s = (hipStream_t)stream;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  const ConfBufs b = plan_conf(m, B, L, ar);
  DN_TRY(check_workspace("dn_conformer_encoder_forward", workspace, workspace_bytes, ar.off));
  const int dtype = c.dtype, es = esize(dtype), D = c.dim, F = c.ffn, H = c.heads, dh = D / H, P = 2 * S - 1;
  const int sdt = side_dtype(dtype), ses = esize(sdt);
  const Rows r{dtype, B * S, S, D, s};
  DN_TRY(m->sub.run(dtype, feats, B, L, b.sub, s));
  // ---- x = linear(sqrt(D) * glu(conv))  (s2t_conformer.py:108-120)
  hipLaunchKernelGGL(conf_embed_kernel, dim3(ew_grid((int64_t)r.M * D)), dim3(256), 0, s, b.sub.y1, src_lengths, 2, B, S, D, sqrtf((float)D), b.xn, dtype,
                     out_lengths);
  float *cur = b.xa, *other = b.xb;
  DN_TRY(linear(r, b.xn, D, m->lin_W, m->lin_b, D, DN_EPI_BIAS, cur, DN_F32));
  // rows of the packed positional encodings for this S: offset d at row (max_frames - 1) + d
  const void* pe = eoff(m->pe, (size_t)(c.max_frames - S) * D, es);
  for (int l = 0; l < c.layers; ++l) {  // ConformerEncoderLayer.forward (conformer_layer.py:229-284); the 0.5 of the half steps is in w_2 / its bias
    const float* g = m->ln_g + (size_t)l * 5 * D;
    const float* be = m->ln_b + (size_t)l * 5 * D;
    DN_TRY(ffn_block(r, cur, b.xn, b.h, F, g, be, layer_mat(m->f1w1_W, l, F, D, es), m->f1w1_b + (size_t)l * F, layer_mat(m->f1w2_W, l, D, F, es),
                     m->f1w2_b + (size_t)l * D, DN_EPI_SILU));  // ffn1 (:243-245)
    layernorm(r, cur, g + D, be + D, b.xn, dtype);  // self_attn_layer_norm (:247)
    DN_TRY(linear(r, b.xn, D, layer_mat(m->qkv_W, l, 3 * D, D, es), m->qkv_b + (size_t)l * 3 * D, 3 * D, DN_EPI_BIAS, b.qkv, sdt));
    DN_TRY(linear(Rows{dtype, P, P, D, s}, pe, D, layer_mat(m->pos_W, l, D, D, es), m->zeros, D, DN_EPI_BIAS, b.posb, sdt));  // linear_pos(pe), no bias
    DnRelAttnParams a = attn_params<DnRelAttnParams>(dtype, H, dh, b.qkv, 3 * D, eoff(b.qkv, D, ses), eoff(b.qkv, 2 * D, ses), 3 * D, B, S, out_lengths, b.ao);
    a.pos = b.posb; a.ldp = D; a.pos_zero_row = S - 1; a.pos_rows = P;
    a.bias_u = m->bias_u + (size_t)l * D; a.bias_v = m->bias_v + (size_t)l * D;
    DN_TRY(dn_rel_attention(&a, s));
    DN_TRY(linear_resadd(r, b.ao, D, layer_mat(m->out_W, l, D, D, es), m->out_b + (size_t)l * D, cur));  // self_attn (:248-266)
    layernorm(r, cur, g + 2 * D, be + 2 * D, b.xn, dtype);  // ConvolutionModule (:77-99), unmasked
    DN_TRY(linear(r, b.xn, D, layer_mat(m->pw1_W, l, 2 * D, D, es), m->zeros, 2 * D, DN_EPI_BIAS, b.qkv, sdt));
    DN_TRY(dn_glu_dwconv(b.qkv, m->dw_w + (size_t)l * D * c.depthwise_kernel, m->dw_shift + (size_t)l * D, b.ao, B, S, D, c.depthwise_kernel, dtype, s));
    DN_TRY(linear_resadd(r, b.ao, D, layer_mat(m->pw2_W, l, D, D, es), m->zeros, cur));  // conv_module (:268-274)
    DN_TRY(ffn_block(r, cur, b.xn, b.h, F, g + 3 * D, be + 3 * D, layer_mat(m->f2w1_W, l, F, D, es), m->f2w1_b + (size_t)l * F,
                     layer_mat(m->f2w2_W, l, D, F, es), m->f2w2_b + (size_t)l * D, DN_EPI_SILU));  // ffn2 (:276-281)
    float* dst = l == c.layers - 1 ? enc_out : other;  // final_layer_norm (:283); the last layer's is the encoder's output
    layernorm(r, cur, g + 4 * D, be + 4 * D, dst, DN_F32);
    other = cur;
    cur = dst;
  }
  DN_CHECK_LAUNCH("dn_conformer_encoder_forward");
  return DN_OK;
}
