// The model inside the mask-predict loop downstream of the normalised units: the DECODER side of the reference's
// NAR S2UT model, NARS2UTTransformerModel (research/TranSpeech/nar_transformer.py:569-976) -- TransformerUnitDecoder.forward
// (:321-420) = fairseq's TransformerDecoder with full context (fairseq/models/transformer/transformer_decoder.py:219-330): scaled
// token embedding + sinusoidal positions, pre-norm layers of self-attention, encoder attention and a ReLU FFN
// (fairseq/modules/transformer_layer.py:389-520), final LayerNorm, the 1004-way output projection; and the length predictor
// (:436-480).  The speech encoder is out of scope: its output is a given tensor.  Everything is a sequence of dn_conv_gemm /
// dn_attention launches plus the LayerNorm of nar_common.h and small kernels here (embedding, masked mean); the keys / values of the encoder
// attention depend on the encoder output only, so all layers' are one grouped contraction per utterance batch, reused by every
// refinement iteration (dn_nar_cross_kv).  Nothing allocates or synchronises.
#include <new>

#include "common.h"
#include "engine.h"
#include "nar_common.h"

using namespace dn;

namespace dn {

// x[b, t, :] = sqrt(D) * E[tok] + P[pos], pos = padding_idx + (rank of t among the non-pad tokens of its row), pad -> padding_idx
// (fairseq/utils.py:256-266; table row padding_idx is zero; transformer_decoder.py:254-275).  One workgroup per sequence; also
// writes the number of non-pad tokens (the self-attention's key mask: non-pad tokens are a prefix in this loop, :861-868).
__global__ __launch_bounds__(256) void nar_embed_kernel(const int32_t* __restrict__ tokens, int T, const float* __restrict__ emb,
                                                        const float* __restrict__ pos_table, int D, int Dp, int pad, float scale,
                                                        float* __restrict__ x, int32_t* __restrict__ tlen) {
  __shared__ int s_pos[2048];
  __shared__ int s_cnt;
  const int b = blockIdx.x;
  const int32_t* tk = tokens + (int64_t)b * T;
  if (threadIdx.x == 0) {
    int c = 0;
    for (int t = 0; t < T; ++t) {
      const bool np = tk[t] != pad;
      c += np ? 1 : 0;
      s_pos[t] = np ? c + pad : pad;
    }
    s_cnt = c;
    tlen[b] = c;
  }
  __syncthreads();
  const int q = Dp >> 2;
  for (int i = threadIdx.x; i < T * q; i += 256) {
    const int t = i / q, c = (i - t * q) * 4;
    float4 v = make_float4(0, 0, 0, 0);
    if (c < D) {
      const float4 e = *reinterpret_cast<const float4*>(emb + (int64_t)tk[t] * D + c);
      const float4 p = *reinterpret_cast<const float4*>(pos_table + (int64_t)s_pos[t] * D + c);
      v = make_float4(fmaf(scale, e.x, p.x), fmaf(scale, e.y, p.y), fmaf(scale, e.z, p.z), fmaf(scale, e.w, p.w));
    }
    *reinterpret_cast<float4*>(x + ((int64_t)b * T + t) * Dp + c) = v;
  }
}

// _mean_pooling (fairseq/models/nat/nonautoregressive_transformer.py:20-34): masked mean over the source frames; enc fp32 [B, S, D]
__global__ __launch_bounds__(256) void nar_mean_pool_kernel(const float* __restrict__ enc, const int32_t* __restrict__ slen, int S, int D, int Dp,
                                                            float* __restrict__ out) {
  const int b = blockIdx.x;
  const int n = min(slen[b], S);
  for (int c = threadIdx.x; c < Dp; c += 256) {
    float s = 0.f;
    if (c < D)
      for (int t = 0; t < n; ++t) s += enc[((int64_t)b * S + t) * D + c] / (float)n;  // the reference divides before it sums
    out[(int64_t)b * Dp + c] = s;
  }
}

// Classifier-free guidance (research/TranSpeech/nar_transformer.py:123-183, cg_forward): every source position of the null half is
// the one row e_null = embed_tokens.weight[bos] and no key is masked, so the encoder attention of every query returns the same row
// c_l = W_o,l (W_v,l e_null + b_v,l) + b_o,l (dn_nar_null_cross); the block is then x[m, :] += c_l over the null half's rows.
__global__ __launch_bounds__(256) void nar_add_row_kernel(float* __restrict__ x, const float* __restrict__ row, int64_t n4, int q) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 v = reinterpret_cast<float4*>(x)[i];
    const float4 c = reinterpret_cast<const float4*>(row)[i % q];
    v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w;
    reinterpret_cast<float4*>(x)[i] = v;
  }
}

// The literal form of the same block (option nar_cg_fold = 0): `rows` copies of e_null as an encoder output, every source length = S
// (cg_forward :144-158: torch.where(all-true mask, null_feature, src_features), zeros_like(src_mask)).
__global__ __launch_bounds__(256) void nar_null_rows_kernel(const float* __restrict__ e_null, int D, int64_t rows, float* __restrict__ out,
                                                            int32_t* __restrict__ lens, int B, int S) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i0 < B) lens[i0] = S;
  for (int64_t i = i0; i < rows * D; i += (int64_t)gridDim.x * 256) out[i] = e_null[i % D];
}

}  // namespace dn

struct DnNar {
  DnNarConfig cfg;
  float* null_tab;   // fp32 [layers][dim]: c_l of the null source (dn_nar_null_cross; nullptr until then), in the caller's buffer
  int32_t null_token;
  // packed tensors in table order
  const float *emb, *pos, *len_W;
  const void *qkv_W, *so_W, *cq_W, *ckv_W, *co_W, *fc1_W, *fc2_W, *out_W;
  const float *qkv_b, *so_b, *cq_b, *ckv_b, *co_b, *fc1_b, *fc2_b, *ln_g, *ln_b, *fin_g, *fin_b;
};
static const int kNarTensors = 22;

extern "C" int dn_nar_create(const DnNarConfig* cfg, const void* const* w, int32_t n, DnNar** out) {
  DN_TRY(check_create("dn_nar_create", cfg, w, n, kNarTensors, out));
  DN_CHECK_ARG(cfg->vocab % 4 == 0 && cfg->layers <= DN_MAX_TERMS, "dn_nar_create: vocab %% 4, at most %d layers", DN_MAX_TERMS);
  DnNar* m = new (std::nothrow) DnNar();
  DN_CHECK_ARG(m != nullptr, "dn_nar_create: out of host memory");
  m->cfg = *cfg;
  TableCursor t{w, 0};
  m->emb = t.next_vec(); m->pos = t.next_vec(); m->len_W = t.next_vec();
  m->qkv_W = t.next_mat(); m->qkv_b = t.next_vec(); m->so_W = t.next_mat(); m->so_b = t.next_vec();
  m->cq_W = t.next_mat(); m->cq_b = t.next_vec(); m->ckv_W = t.next_mat(); m->ckv_b = t.next_vec();
  m->co_W = t.next_mat(); m->co_b = t.next_vec(); m->fc1_W = t.next_mat(); m->fc1_b = t.next_vec();
  m->fc2_W = t.next_mat(); m->fc2_b = t.next_vec(); m->ln_g = t.next_vec(); m->ln_b = t.next_vec();
  m->fin_g = t.next_vec(); m->fin_b = t.next_vec(); m->out_W = t.next_mat();
  *out = m;
  return DN_OK;
}

extern "C" void dn_nar_destroy(DnNar* m) { delete m; }

namespace {
struct NarBufs { float* x; void *xn, *qkv, *cq, *ao, *h; int32_t* tlen; };
NarBufs plan_nar(const DnNar* m, int M, int B, Arena& ar) {
  const int es = esize(m->cfg.dtype), D = m->cfg.dim, F = m->cfg.ffn;
  NarBufs b;
  b.x = (float*)ar.take((size_t)M * D * 4);
  b.xn = ar.take((size_t)M * D * es);
  b.qkv = ar.take((size_t)M * 3 * D * es);
  b.cq = ar.take((size_t)M * D * es);
  b.ao = ar.take((size_t)M * D * es);
  b.h = ar.take((size_t)M * F * es);
  b.tlen = (int32_t*)ar.take((size_t)B * 4 + 64);
  return b;
}

// encoder_attn.{k,v}_proj of every layer (transformer_layer.py:455-470) on the rows of `src` ([rows, D] in the engine's arithmetic, T per
// sequence): one grouped contraction -> out [layers][rows][k(D) ; v(D)] in side_dt
int cross_kv_proj(const DnNar* m, const void* src, int rows, int T, void* out, hipStream_t s) {
  const int dtype = m->cfg.dtype, D = m->cfg.dim;
  DnGemmParams p = gemm_base(dtype, rows, 2 * D, D, T);
  p.groups = m->cfg.layers;
  p.terms[0].A = src; p.terms[0].lda = D; p.terms[0].a_gstride = 0;
  p.terms[0].W = m->ckv_W; p.terms[0].w_gstride = (int64_t)padn(2 * D) * D;
  p.bias = m->ckv_b; p.bias_gstride = 2 * D;
  p.out = out; p.ldo = 2 * D; p.out_gstride = (int64_t)rows * 2 * D; p.out_dtype = side_dtype(dtype);
  return dn_conv_gemm(&p, s);
}
}  // namespace

extern "C" size_t dn_nar_workspace_bytes(const DnNar* m, int32_t B, int32_t T, int32_t S) {
  if (!m || B <= 0 || T <= 0 || S <= 0) return 0;
  Arena a{nullptr, 0, 0};
  (void)plan_nar(m, B * T, B, a);
  const size_t pre = (size_t)B * S * m->cfg.dim * 4 + (size_t)B * (m->cfg.dim + 256) * 4 + 4096;  // dn_nar_cross_kv / dn_nar_predict_lengths staging
  return (a.off > pre ? a.off : pre) + 512;
}

extern "C" size_t dn_nar_cross_kv_bytes(const DnNar* m, int32_t B, int32_t S) {
  return m ? (size_t)m->cfg.layers * B * S * 2 * m->cfg.dim * esize(m->cfg.dtype) + 256 : 0;
}

extern "C" int dn_nar_cross_kv(DnNar* m, const float* enc_out, int32_t B, int32_t S, void* ckv, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && enc_out && ckv && workspace && B > 0 && S > 0, "dn_nar_cross_kv: bad argument");
  DN_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)ckv & 127) == 0, "dn_nar_cross_kv: buffers must be 256 / 128-byte aligned");
  const int dtype = m->cfg.dtype, D = m->cfg.dim;
  DN_CHECK_ARG(workspace_bytes >= (size_t)B * S * D * esize(dtype), "dn_nar_cross_kv: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  DN_TRY(dn_convert_rows(enc_out, DN_F32, D, workspace, dtype, D, B * S, D, s));
  return cross_kv_proj(m, workspace, B * S, S, ckv, s);
}

extern "C" int dn_nar_predict_lengths(DnNar* m, const float* enc_out, const int32_t* src_lengths, int32_t B, int32_t S, int32_t* lengths,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && enc_out && src_lengths && lengths && workspace && B > 0 && S > 0, "dn_nar_predict_lengths: bad argument");
  const int D = m->cfg.dim;
  DN_CHECK_ARG(workspace_bytes >= (size_t)B * (D + 256) * 4 + 256, "dn_nar_predict_lengths: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* pooled = (float*)workspace;
  float* logit = pooled + (size_t)B * D;
  hipLaunchKernelGGL(nar_mean_pool_kernel, dim3(B), dim3(256), 0, s, enc_out, src_lengths, S, D, D, pooled);
  // F.linear(enc_feats, embed_length.weight) (:443), exact fp32; arg-max of the log-softmax = of the logits
  DN_TRY(linear(Rows{DN_F32, B, 1, D, s}, pooled, D, m->len_W, nullptr, 256, DN_EPI_BIAS, logit, DN_F32));
  return dn_argmax_units(logit, 256, B, 256, 0, lengths, s);
}

// ------------------------------------------------------------------------------------------ classifier-free guidance (nar_cg)
// research/TranSpeech/nat_gen.py:196-236 runs the decoder twice per iteration: TransformerUnitDecoder.forward on the speech
// encoder's output and cg_forward (nar_transformer.py:123-183) on the "dropped" source.  Here: one pass over 2 B rows
// (decoder_pass below, halves == 2).
namespace {
inline int cg_fold() { return option_or(OPT_NAR_CG_FOLD, 1) != 0; }

struct NarNullBufs { float* tab; void *stage, *kv, *vst; };
NarNullBufs plan_null(const DnNar* m, Arena& ar) {
  const int D = m->cfg.dim, L = m->cfg.layers;
  NarNullBufs b;
  b.tab = (float*)ar.take((size_t)L * D * 4);  // first: the part the engine keeps reading
  b.stage = ar.take((size_t)D * 4);
  b.kv = ar.take((size_t)L * 2 * D * 4);
  b.vst = ar.take((size_t)L * D * 4);
  return b;
}

struct NarLiteralBufs { float* rows; void *stage, *kv; int32_t* lens; };
NarLiteralBufs plan_literal(const DnNar* m, int B, int S, Arena& ar) {
  const int D = m->cfg.dim;
  NarLiteralBufs b;
  b.rows = (float*)ar.take((size_t)B * S * D * 4);
  b.stage = ar.take((size_t)B * S * D * 4);
  b.kv = ar.take(dn_nar_cross_kv_bytes(m, B, S));
  b.lens = (int32_t*)ar.take((size_t)B * 4 + 64);
  return b;
}
}  // namespace

extern "C" size_t dn_nar_null_cross_bytes(const DnNar* m) {
  if (!m) return 0;
  Arena a{nullptr, 0, 0};
  (void)plan_null(m, a);
  return a.off + 256;
}

extern "C" int dn_nar_null_cross(DnNar* m, int32_t null_token, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && workspace, "dn_nar_null_cross: null argument");
  DN_CHECK_ARG(null_token >= 0 && null_token < m->cfg.vocab, "dn_nar_null_cross: null token %d outside the vocabulary of %d", null_token, m->cfg.vocab);
  const int dtype = m->cfg.dtype, D = m->cfg.dim, L = m->cfg.layers;
  const int sdt = side_dtype(dtype), ses = esize(sdt);
  Arena ar{(char*)workspace, 0, workspace_bytes};
  const NarNullBufs b = plan_null(m, ar);
  DN_TRY(check_workspace("dn_nar_null_cross", workspace, workspace_bytes, ar.off));
  hipStream_t s = (hipStream_t)stream;
  // null_feature = embed_tokens(bos) (cg_forward :144): the raw embedding row, neither scaled nor positioned
  DN_TRY(dn_convert_rows(m->emb + (size_t)null_token * D, DN_F32, D, b.stage, dtype, D, 1, D, s));
  DN_TRY(cross_kv_proj(m, b.stage, 1, 1, b.kv, s));  // on the one row, exactly as dn_nar_cross_kv forms a source row's (the k half is not used)
  // uniform softmax over S identical values = the value row itself: what the attention kernel would hand to out_proj, as its operand
  DN_TRY(dn_convert_rows(eoff(b.kv, D, ses), sdt, 2 * D, b.vst, dtype, D, L, D, s));
  {  // encoder_attn.out_proj (transformer_layer.py:455-470) -> c_l, fp32
    DnGemmParams p = gemm_base(dtype, 1, D, D, 1);
    p.groups = L;
    p.terms[0].A = b.vst; p.terms[0].lda = D; p.terms[0].a_gstride = D;
    p.terms[0].W = m->co_W; p.terms[0].w_gstride = (int64_t)padn(D) * D;
    p.bias = m->co_b; p.bias_gstride = D;
    p.out = b.tab; p.ldo = D; p.out_gstride = D; p.out_dtype = DN_F32;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  DN_CHECK_LAUNCH("dn_nar_null_cross");
  m->null_tab = b.tab;
  m->null_token = null_token;
  return DN_OK;
}

extern "C" const float* dn_nar_null_table(const DnNar* m) { return m ? m->null_tab : nullptr; }

extern "C" size_t dn_nar_guided_workspace_bytes(const DnNar* m, int32_t B, int32_t T, int32_t S) {
  if (!m || B <= 0 || T <= 0 || S <= 0) return 0;
  Arena a{nullptr, 0, 0};
  (void)plan_nar(m, 2 * B * T, 2 * B, a);
  if (!cg_fold()) (void)plan_literal(m, B, S, a);
  return a.off + 512;
}

// ------------------------------------------------------------------------------------------------------------ the decoder pass
// TransformerUnitDecoder.forward over `halves` copies of the B token rows.  halves == 1: the plain pass.  halves == 2: the guided one --
// both halves decode the same tokens (nat_gen.py:209-222), rows [0, M) against the speech encoder, rows [M, 2 M) against the null
// source: folded, they skip the encoder attention and receive c_l; literally (nar_cg_fold = 0), they attend to S copies of e_null per
// row of the batch with no key masked.
static int decoder_pass(const char* who, DnNar* m, int halves, const int32_t* tokens, const void* ckv, const int32_t* src_lengths, int B, int T, int S,
                        float* logits, void* workspace, size_t workspace_bytes, hipStream_t s) {
  const DnNarConfig& c = m->cfg;
  const int dtype = c.dtype, es = esize(dtype), M = B * T, D = c.dim, F = c.ffn, H = c.heads, dh = D / H;
  const bool fold = halves == 2 && cg_fold(), literal = halves == 2 && !fold;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  const NarBufs b = plan_nar(m, halves * M, halves * B, ar);
  NarLiteralBufs lit{nullptr, nullptr, nullptr, nullptr};
  if (literal) lit = plan_literal(m, B, S, ar);
  DN_TRY(check_workspace(who, workspace, workspace_bytes, ar.off));
  const int sdt = side_dtype(dtype), ses = esize(sdt);
  const Rows all{dtype, halves * M, T, D, s};
  const Rows cross = fold ? Rows{dtype, M, T, D, s} : all;  // the rows that run the encoder attention
  for (int h = 0; h < halves; ++h)
    hipLaunchKernelGGL(nar_embed_kernel, dim3(B), dim3(256), 0, s, tokens, T, m->emb, m->pos, D, D, c.pad, sqrtf((float)D), b.x + (size_t)h * M * D,
                       b.tlen + h * B);
  if (literal) {
    hipLaunchKernelGGL(nar_null_rows_kernel, dim3(256), dim3(256), 0, s, m->emb + (size_t)m->null_token * D, D, (int64_t)B * S, lit.rows, lit.lens, B, S);
    DN_TRY(dn_nar_cross_kv(m, lit.rows, B, S, lit.kv, lit.stage, (size_t)B * S * D * 4, s));
  }
  for (int l = 0; l < c.layers; ++l) {
    const float* g = m->ln_g + (size_t)l * 3 * D;
    const float* be = m->ln_b + (size_t)l * 3 * D;
    layernorm(all, b.x, g, be, b.xn, dtype);  // self_attn_layer_norm (pre-norm, :421-423)
    DN_TRY(self_attention_block(all, H, dh, b.xn, layer_mat(m->qkv_W, l, 3 * D, D, es), m->qkv_b + (size_t)l * 3 * D, layer_mat(m->so_W, l, D, D, es),
                                m->so_b + (size_t)l * D, b.qkv, b.ao, b.tlen, b.x));  // full context, keys = non-pad tokens
    layernorm(cross, b.x, g + D, be + D, b.xn, dtype);  // encoder_attn_layer_norm (:447-449)
    DN_TRY(linear(cross, b.xn, D, layer_mat(m->cq_W, l, D, D, es), m->cq_b + (size_t)l * D, D, DN_EPI_BIAS, b.cq, sdt));
    const void* kv = eoff(ckv, (size_t)l * B * S * 2 * D, ses);
    DN_TRY(attention(dtype, H, dh, b.cq, D, kv, eoff(kv, D, ses), 2 * D, B, T, S, src_lengths, b.ao, s));
    if (literal) {
      const void* nkv = eoff(lit.kv, (size_t)l * B * S * 2 * D, ses);
      DN_TRY(attention(dtype, H, dh, eoff(b.cq, (size_t)M * D, ses), D, nkv, eoff(nkv, D, ses), 2 * D, B, T, S, lit.lens, eoff(b.ao, (size_t)M * D, es), s));
    }
    DN_TRY(linear_resadd(cross, b.ao, D, layer_mat(m->co_W, l, D, D, es), m->co_b + (size_t)l * D, b.x));
    if (fold) {
      const int64_t n4 = (int64_t)M * D / 4;
      const int grid = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
      hipLaunchKernelGGL(nar_add_row_kernel, dim3(grid), dim3(256), 0, s, b.x + (size_t)M * D, m->null_tab + (size_t)l * D, n4, D / 4);
    }
    DN_TRY(ffn_block(all, b.x, b.xn, b.h, F, g + 2 * D, be + 2 * D, layer_mat(m->fc1_W, l, F, D, es), m->fc1_b + (size_t)l * F,
                     layer_mat(m->fc2_W, l, D, F, es), m->fc2_b + (size_t)l * D, DN_EPI_RELU));  // final_layer_norm, relu(fc1), fc2 (:495-508)
  }
  layernorm(all, b.x, m->fin_g, m->fin_b, b.xn, dtype);  // decoder.layer_norm (transformer_decoder.py:316-317)
  DN_TRY(linear(all, b.xn, D, m->out_W, nullptr, c.vocab, DN_EPI_BIAS, logits, DN_F32));  // output_projection (no bias)
  DN_CHECK_LAUNCH(who);
  return DN_OK;
}

extern "C" int dn_nar_decoder_forward(DnNar* m, const int32_t* tokens, const void* ckv, const int32_t* src_lengths, int32_t B, int32_t T, int32_t S,
                                      float* logits, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && tokens && ckv && src_lengths && logits && workspace, "dn_nar_decoder_forward: null argument");
  DN_CHECK_ARG(B > 0 && T > 0 && T <= 2048 && T + m->cfg.pad + 1 <= m->cfg.max_pos && S > 0, "dn_nar_decoder_forward: B=%d T=%d S=%d (T <= 2048 and within the positional table)", B, T, S);
  return decoder_pass("dn_nar_decoder_forward", m, 1, tokens, ckv, src_lengths, B, T, S, logits, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int dn_nar_decoder_forward_guided(DnNar* m, const int32_t* tokens, const void* ckv, const int32_t* src_lengths, int32_t B, int32_t T,
                                             int32_t S, float* logits2, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && tokens && ckv && src_lengths && logits2 && workspace, "dn_nar_decoder_forward_guided: null argument");
  DN_CHECK_ARG(m->null_tab != nullptr, "dn_nar_decoder_forward_guided: no null-source table: call dn_nar_null_cross on this engine first");
  DN_CHECK_ARG(B > 0 && T > 0 && T <= 2048 && T + m->cfg.pad + 1 <= m->cfg.max_pos && S > 0 && (int64_t)2 * B * T <= 0x7fffffff,
               "dn_nar_decoder_forward_guided: B=%d T=%d S=%d (T <= 2048 and within the positional table)", B, T, S);
  return decoder_pass("dn_nar_decoder_forward_guided", m, 2, tokens, ckv, src_lengths, B, T, S, logits2, workspace, workspace_bytes, (hipStream_t)stream);
}
