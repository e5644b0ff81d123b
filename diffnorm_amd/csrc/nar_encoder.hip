// The speech ENCODER of the NAR S2UT model behind the mask-predict loop: S2STransformerEncoder
// (research/TranSpeech/nar_transformer.py:40-76, no speaker embedding) = fairseq's S2TTransformerEncoder._forward
// (fairseq/models/speech_to_text/s2t_transformer.py:345-373): Conv1dSubsampler (fairseq/models/speech_to_text/modules/convolution.py:
// 13-57: two Conv1d(k, stride 2, padding k/2) + GLU over the channels) -> sqrt(D) scaling -> sinusoidal positions of the padding
// mask -> pre-norm TransformerEncoderLayers (fairseq/modules/transformer_layer.py:163-226: self-attention with the key-padding mask,
// ReLU FFN, all biases) -> LayerNorm.  One pass per utterance batch, in front of the loop: generate() of the research generator
// (research/TranSpeech/iterative_refinement_generator.py:131-160) then runs from [B, L, 80] features on this library alone.
// The subsampler (a strided conv as a contraction over gathered rows) and the LayerNorm kernel are nar_common.h's; the layers are
// dn_conv_gemm / dn_attention launches.
#include <new>

#include "common.h"
#include "engine.h"
#include "nar_common.h"

using namespace dn;

namespace dn {

// x[b, t, :] = sqrt(D) * glu(y[b, t, :]) + P[pos], pos = pad + 1 + t for t < len2[b] and `pad` (the zero row) behind it: make_positions on the
// padding mask itself (s2t_transformer.py:347-351; fairseq/utils.py:256-266).  Also writes the subsampled lengths.
__global__ __launch_bounds__(256) void enc_embed_kernel(const float* __restrict__ y, const int32_t* __restrict__ src_len, int n_conv, int B, int S, int D,
                                                        const float* __restrict__ pos_table, int pad, float scale, float* __restrict__ x,
                                                        int32_t* __restrict__ out_len) {
  const int64_t n = (int64_t)B * S * D;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int d = (int)(i % D);
    const int64_t row = i / D;
    const int t = (int)(row % S), b = (int)(row / S);
    const int len = subsampled_len(src_len[b], n_conv);
    if (t == 0 && d == 0) out_len[b] = len < S ? len : S;
    const float* r = y + row * 2 * D;
    const int pos = t < len ? pad + 1 + t : pad;
    x[i] = fmaf(scale, r[d] * sigmoidf_(r[D + d]), pos_table[(int64_t)pos * D + d]);
  }
}
}  // namespace dn

struct DnNarEnc {
  DnNarEncConfig cfg;
  Subsampler sub;
  const void *qkv_W, *so_W, *fc1_W, *fc2_W;
  const float *pos, *qkv_b, *so_b, *fc1_b, *fc2_b, *ln_g, *ln_b, *fin_g, *fin_b;
};
static const int kNarEncTensors = 17;

extern "C" int dn_nar_encoder_create(const DnNarEncConfig* cfg, const void* const* w, int32_t n, DnNarEnc** out) {
  DN_TRY(check_create("dn_nar_encoder_create", cfg, w, n, kNarEncTensors, out));
  TableCursor t{w, 0};
  const Subsampler sub{cfg->input_dim, cfg->conv_channels, cfg->kernel, cfg->dim, t.next_mat(), t.next_vec(), t.next_mat(), t.next_vec()};
  DN_TRY(sub.check("dn_nar_encoder_create"));
  DnNarEnc* m = new (std::nothrow) DnNarEnc();
  DN_CHECK_ARG(m != nullptr, "dn_nar_encoder_create: out of host memory");
  m->cfg = *cfg;
  m->sub = sub;
  m->pos = t.next_vec();
  m->qkv_W = t.next_mat(); m->qkv_b = t.next_vec(); m->so_W = t.next_mat(); m->so_b = t.next_vec();
  m->fc1_W = t.next_mat(); m->fc1_b = t.next_vec(); m->fc2_W = t.next_mat(); m->fc2_b = t.next_vec();
  m->ln_g = t.next_vec(); m->ln_b = t.next_vec(); m->fin_g = t.next_vec(); m->fin_b = t.next_vec();
  *out = m;
  return DN_OK;
}

extern "C" void dn_nar_encoder_destroy(DnNarEnc* m) { delete m; }

extern "C" int32_t dn_nar_encoder_out_frames(int32_t L) { return subsampled_len(L, 2); }

namespace {
struct EncBufs { Subsampler::Bufs sub; void *xn, *qkv, *ao, *h; float* x; };
EncBufs plan_enc(const DnNarEnc* m, int B, int L, Arena& ar) {
  const DnNarEncConfig& c = m->cfg;
  const int es = esize(c.dtype), D = c.dim, S = subsampled_len(L, 2);
  EncBufs b;
  b.sub = m->sub.plan(c.dtype, B, L, ar);
  b.x = (float*)ar.take((size_t)B * S * D * 4);
  b.xn = ar.take((size_t)B * S * D * es);
  b.qkv = ar.take((size_t)B * S * 3 * D * es);
  b.ao = ar.take((size_t)B * S * D * es);
  b.h = ar.take((size_t)B * S * c.ffn * es);
  return b;
}
}  // namespace

extern "C" size_t dn_nar_encoder_workspace_bytes(const DnNarEnc* m, int32_t B, int32_t L) {
  if (!m || B <= 0 || L <= 0) return 0;
  Arena a{nullptr, 0, 0};
  (void)plan_enc(m, B, L, a);
  return a.off + 512;
}

extern "C" int dn_nar_encoder_forward(DnNarEnc* m, const float* feats, const int32_t* src_lengths, int32_t B, int32_t L, float* enc_out,
                                      int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && feats && src_lengths && enc_out && out_lengths && workspace, "dn_nar_encoder_forward: null argument");
  const DnNarEncConfig& c = m->cfg;
  const int S = subsampled_len(L, 2);
  DN_CHECK_ARG(B > 0 && L > 0 && S >= 1 && S + c.pad + 1 <= c.max_pos, "dn_nar_encoder_forward: B=%d L=%d (%d frames after the subsampler; positional table %d)", B, L,
               S, c.max_pos);
  hipStream_t s = (hipStream_t)stream;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  const EncBufs b = plan_enc(m, B, L, ar);
  DN_TRY(check_workspace("dn_nar_encoder_forward", workspace, workspace_bytes, ar.off));
  const int dtype = c.dtype, es = esize(dtype), D = c.dim, F = c.ffn, H = c.heads, dh = D / H;
  const Rows r{dtype, B * S, S, D, s};
  DN_TRY(m->sub.run(dtype, feats, B, L, b.sub, s));
  hipLaunchKernelGGL(enc_embed_kernel, dim3(ew_grid((int64_t)r.M * D)), dim3(256), 0, s, b.sub.y1, src_lengths, 2, B, S, D, m->pos, c.pad, sqrtf((float)D), b.x,
                     out_lengths);
  // ---- pre-norm encoder layers
  for (int l = 0; l < c.layers; ++l) {
    const float* g = m->ln_g + (size_t)l * 2 * D;
    const float* be = m->ln_b + (size_t)l * 2 * D;
    layernorm(r, b.x, g, be, b.xn, dtype);  // self_attn_layer_norm (:194-196)
    DN_TRY(self_attention_block(r, H, dh, b.xn, layer_mat(m->qkv_W, l, 3 * D, D, es), m->qkv_b + (size_t)l * 3 * D, layer_mat(m->so_W, l, D, D, es),
                                m->so_b + (size_t)l * D, b.qkv, b.ao, out_lengths, b.x));  // key_padding_mask (:197-204)
    DN_TRY(ffn_block(r, b.x, b.xn, b.h, F, g + D, be + D, layer_mat(m->fc1_W, l, F, D, es), m->fc1_b + (size_t)l * F, layer_mat(m->fc2_W, l, D, F, es),
                     m->fc2_b + (size_t)l * D, DN_EPI_RELU));  // final_layer_norm, relu(fc1), fc2 (:210-215)
  }
  layernorm(r, b.x, m->fin_g, m->fin_b, enc_out, DN_F32);  // encoder.layer_norm (:361-362), fp32 [B, S, D]
  DN_CHECK_LAUNCH("dn_nar_encoder_forward");
  return DN_OK;
}
