// Whole-path engine: the eps-predictor `Model`, the speech VAE and the DDIM device loop, expressed as
// sequences of dn_conv_gemm / dn_attention / pointwise launches on one stream.  Nothing here
// allocates or synchronises; every intermediate lives in the caller's workspace (bump-allocated by
// the plan_* functions, which also serve the *_workspace_bytes queries).
#include <algorithm>
#include <functional>
#include <new>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "engine.h"

using namespace dn;

namespace {

// The residual-closing contractions can also emit the next block's RMSNorm (64 x 512 whole-row tile, dn_conv_gemm's
// norm_out).  Measured on [32,512] x dim 512 it loses to 256 x 128 tiles + a standalone norm kernel (one workgroup
// re-reads the whole weight for 64 rows): 6.85 vs 6.63 ms per denoising step.  Off unless DN_FUSE_NORM=1.
inline bool fuse_norm_enabled(int Dp, int dtype) {
  const bool on = option_or(OPT_FUSE_NORM, 0) != 0;  // dn_set_option("fuse_norm", 1)
  return on && Dp <= 512 && dtype != DN_BF16X3;  // (the whole-row tile is not built for split operands)
}

// Split RMSNorm (DnGemmParams.norm_split / row_ssq): every RMSNorm of the transformer is divided between the residual-
// closing contraction that produces its input and the projection that consumes its output, so the 2*depth+1 norm passes
// over the residual stream disappear (measured: -6 % per denoising step at [32,512] x dim 512).  DN_NO_SPLIT_NORM=1 runs
// the standalone norm kernel instead (A/B timing, and the reference point of the parity tests).
inline bool split_norm_enabled(int Dp, int dtype) {
  return option_or(OPT_NO_SPLIT_NORM, 0) == 0 && Dp % 64 == 0 && !fuse_norm_enabled(Dp, dtype);
}

// DN_KBLOCK: unset = K-blocked buffers where the consuming contraction lands on a tile that gains from them, 0 = never,
// 1 = always (the contraction then runs on a tile that takes them; tests).  Read per call (host side, once per capture).
int kblock_mode() {
  const int v = option(OPT_KBLOCK);  // dn_set_option("kblock", 0 / 1); DN_OPTION_DEFAULT = by tile
  return v == DN_OPT_UNSET ? -1 : (v != 0 ? 1 : 0);
}

// ------------------------------------------------------------------------------------------ WaveNet
struct WaveBufs { void *hw, *resb, *blk0, *blk1, *sk; };

WaveBufs plan_wave(const WavenetW& w, int M, int es, Arena& ar) {
  const size_t one = (size_t)M * padk(w.cout) * es;
  WaveBufs b;
  b.hw = ar.take(one);
  b.resb = ar.take(one * w.layers);
  b.blk0 = ar.take(one * w.layers);
  b.blk1 = ar.take(one * w.layers);
  b.sk = ar.take(one);
  return b;
}

// `fin` carries the destination of the final 1x1 conv (out, ldo, out_dtype, N, epilogue and its extras).  gemm_flags: DnGemmParams.flags
// of every contraction issued (DN_GEMM_TWIN from the two-stream sampler).
int run_wavenet(const WavenetW& w, int dtype, const void* in, int M, int T, const float* gb, int gb_ld, const WaveBufs& wb,
                DnGemmParams fin, hipStream_t s, int32_t gemm_flags = 0) {
  const int es = esize(dtype);
  const int cinp = padk(w.cin), cp = padk(w.cout), cn = padn(w.cout), L = w.layers, S = w.stacks;
  const size_t mat = (size_t)cn * cp;
  const int64_t plane = (int64_t)M * cp;
  // The hidden states between the init conv, the res convs and the dilated convs go K-blocked ([cp/32][M][32]) when both of
  // their consumers run on the 256 x 256 tile (large M): its 16-row staging pieces are then whole cache lines (-10 % on the
  // dilated conv, -11 % on the res conv at [32,512]).  The last stack's outputs stay row-major for the skip contraction.
  bool kb = false;
  if (kblock_mode() != 0 && dn::dn_is16(dtype) && w.conv_Wkb && w.res_Wkb) {
    DnGemmParams q = gemm_base(dtype, M, cp, cp, T, gemm_flags);
    q.groups = L;
    const int t_res = dn_conv_gemm_tile(&q);
    q.n_terms = 3; q.epilogue = DN_EPI_FILM_GATE;
    kb = kblock_mode() == 1 || (t_res == DN_TILE_256X256 && dn_conv_gemm_tile(&q) == DN_TILE_256X256);
  }
  const int a_layout = kb ? (DN_LAYOUT_A_KBLOCKED | DN_LAYOUT_W_KBLOCKED) : 0;
  {  // init conv, k=3, dilation 1 (latent_module.py:596,614 / 1014,1029)
    DnGemmParams p = gemm_base(dtype, M, cp, cinp, T, gemm_flags);
    p.n_terms = 3;
    for (int j = 0; j < 3; ++j) {
      p.terms[j].A = in; p.terms[j].lda = cinp; p.terms[j].shift = 2 - j;
      p.terms[j].W = eoff(w.init_W, (size_t)j * cn * cinp, es);
    }
    p.bias = w.init_b; p.out = wb.hw; p.ldo = cp;
    p.out_layout = kb ? DN_LAYOUT_OUT_KBLOCKED : 0;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  for (int st = 0; st < S; ++st) {
    const void* in_s = st == 0 ? wb.hw : ((st - 1) & 1 ? wb.blk1 : wb.blk0);
    const int64_t a_gs = st == 0 ? 0 : plane;  // stack 0 feeds one tensor to all blocks (:570-571)
    void* out_s = (st & 1) ? wb.blk1 : wb.blk0;
    {  // res_conv 1x1 of the L blocks (:510,521)
      DnGemmParams p = gemm_base(dtype, M, cp, cp, T, gemm_flags);
      p.groups = L;
      p.terms[0].A = in_s; p.terms[0].lda = cp; p.terms[0].a_gstride = a_gs;
      p.terms[0].W = eoff(kb ? w.res_Wkb : w.res_W, (size_t)st * L * mat, es); p.terms[0].w_gstride = (int64_t)mat;
      p.terms[0].layout = a_layout;
      p.bias = w.res_b + (size_t)st * L * cp; p.bias_gstride = cp;
      p.out = wb.resb; p.ldo = cp; p.out_gstride = plane; p.out_dtype = side_dtype(dtype);
      DN_TRY(dn_conv_gemm(&p, s));
    }
    {  // dilated conv k=3 (dilation 2^block) + FiLM + tanh*sigmoid + residual (:509,523-530)
      DnGemmParams p = gemm_base(dtype, M, cp, cp, T, gemm_flags);
      p.groups = L;
      p.n_terms = 3;
      for (int j = 0; j < 3; ++j) {
        p.terms[j].A = in_s; p.terms[j].lda = cp; p.terms[j].a_gstride = a_gs;
        p.terms[j].shift = 2 - j; p.terms[j].shift_by_group = 1;
        p.terms[j].W = eoff(kb ? w.conv_Wkb : w.conv_W, ((size_t)st * L * 3 + j) * mat, es); p.terms[j].w_gstride = (int64_t)(3 * mat);
        p.terms[j].layout = a_layout;
      }
      p.bias = w.conv_b + (size_t)st * L * cp; p.bias_gstride = cp;
      p.epilogue = DN_EPI_FILM_GATE;
      p.res = wb.resb; p.ldr = cp; p.res_gstride = plane; p.res_dtype = side_dtype(dtype);
      if (gb) {
        p.gamma_beta = gb + (size_t)st * L * 2 * cp; p.gb_ld = gb_ld; p.gb_half = cp; p.gb_gstride = 2 * cp;
      }
      p.out = out_s; p.ldo = cp; p.out_gstride = plane;
      p.out_layout = kb && st + 1 < S ? DN_LAYOUT_OUT_KBLOCKED : 0;
      p.flags |= DN_TAG_WN_DILATED << DN_GEMM_TAG_SHIFT;
      DN_TRY(dn_conv_gemm(&p, s));
    }
  }
  const void* last = ((S - 1) & 1) ? wb.blk1 : wb.blk0;
  {  // sum over blocks of skip_conv(out_i): one contraction with L terms (:511,534,617)
    DnGemmParams p = gemm_base(dtype, M, cp, cp, T, gemm_flags);
    p.n_terms = L;
    for (int i = 0; i < L; ++i) {
      p.terms[i].A = eoff(last, (size_t)i * plane, es); p.terms[i].lda = cp;
      p.terms[i].W = eoff(w.skip_W, (size_t)i * mat, es);
    }
    p.bias = w.skip_b; p.out = wb.sk; p.ldo = cp;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  fin.dtype = dtype; fin.M = M; fin.K = cp; fin.T = T; fin.groups = 1; fin.n_terms = 1; fin.flags |= gemm_flags;
  fin.terms[0].A = wb.sk; fin.terms[0].lda = cp; fin.terms[0].W = w.final_W;
  fin.bias = w.final_b;
  return dn_conv_gemm(&fin, s);
}

// ------------------------------------------------------------------------------------------ transformer
struct TfBufs { void *xn, *qkv, *ao, *gg, *fc; float* ssq; };
// row stride of the sums-of-squares buffer: one float per 64 columns, padded to >= 8 and a multiple of 4 so a consumer
// can fetch a row's partials with two 16-byte loads at kernel start
inline int ssq_ld(int Dp) { const int n = Dp / 64; return n <= 8 ? 8 : (n + 3) / 4 * 4; }

// Option ffn_fold (default on, off in DN_BF16: TransformerW.fold_default): with folded weights attached, the FFN's causal conv and output projection run as one contraction.
// 5: on the tile fold_route picks; 1: on the tile the route table chooses (term-outer: 128 x 128 at [32,512]); 2 / 3 / 4: forced to
// 256 x 128 / 256 x 256 / the 256 x 128 shared-row tile (A/B timing); 0: two stages.
enum { FOLD_OFF = 0, FOLD_TABLE = 1, FOLD_256X128 = 2, FOLD_256X256 = 3, FOLD_SR = 4, FOLD_ROUTED = 5 };
inline int ffn_fold_mode(const TransformerW& w) { return w.fold_W && w.fold_b ? option_or(OPT_FFN_FOLD, w.fold_default) : 0; }

// Does the folded contraction (M rows, N = Dp columns, K = 3 x ip) go to the 256 x 128 shared-row tile?  Long and at most 512
// columns wide -- one to four column tiles, where 256-column tiles leave CUs idle -- with enough 256 x 128 tiles to give every CU
// one; a half-batch launch of the two-stream chain counts double (its twin runs beside it).  With taps_inner = 2 whatever M is:
// a batch and its shards then sum every output in one order, as for the other tap-inner tiles.  Measured: DESIGN 11.
constexpr bool kFoldSrRouted = true;
inline bool fold_route(int dtype, int M, int Dp, int ip, int32_t gemm_flags) {
  if (!kFoldSrRouted || !dn::dn_is16(dtype) || Dp > 512 || 3L * ip < 1024) return false;
  if (option_or(OPT_TAPS_INNER, 1) == 2) return true;
  const long twin = (gemm_flags & DN_GEMM_TWIN) ? 2 : 1;
  return (long)((M + 255) / 256) * ((Dp + 127) / 128) * twin >= 256;
}

TfBufs plan_tf(const TransformerW& w, int M, int es, Arena& ar) {
  const int hd = w.heads * w.dim_head;
  TfBufs b;
  b.xn = ar.take((size_t)M * padk(w.dim) * es);
  b.qkv = ar.take((size_t)M * 3 * hd * es);
  b.ao = ar.take((size_t)M * hd * es);
  b.gg = ar.take((size_t)M * padk(w.inner) * es);
  b.fc = ffn_fold_mode(w) ? nullptr : ar.take((size_t)M * padk(w.inner) * es);  // (folded: the conv's output is never formed)
  b.ssq = (float*)ar.take((size_t)M * ssq_ld(padk(w.dim)) * 4);  // split RMSNorm: per-64-column sums of squares
  return b;
}

// Producer half of a split RMSNorm on a RESADD / POSEMB contraction: row * gamma -> xn, per-slab sums of squares -> ssq.
void set_split_norm(DnGemmParams& p, const TfBufs& tb, int Dp, int D, int dtype, const float* gamma, const float* gb, int gb_ld) {
  p.norm_out = tb.xn; p.norm_ld = Dp; p.norm_dtype = dtype; p.norm_D = D;
  p.norm_gamma = gamma; p.norm_gb = gb; p.norm_gb_ld = gb_ld; p.norm_gb_half = Dp;
  p.norm_split = 1; p.norm_ssq = tb.ssq; p.norm_ssq_ld = ssq_ld(Dp);
}
// Consumer half: scale the accumulators by sqrt(D)/|row| and add beta . W^T (rb: the consumer's columns of the row-bias
// block, NULL when the norm has no beta).
void set_row_scale(DnGemmParams& p, const TfBufs& tb, int Dp, int D, const float* rb, int rb_ld) {
  p.row_ssq = tb.ssq; p.row_ssq_ld = ssq_ld(Dp); p.row_ssq_parts = Dp / 64; p.row_D = (float)D;
  p.row_bias = rb; p.row_bias_ld = rb_ld;
}

// Fills the fused-RMSNorm fields of a RESADD / POSEMB contraction (see DnGemmParams.norm_out).
void set_norm(DnGemmParams& p, void* xn, int Dp, int D, int dtype, const float* gamma, const float* gb, int gb_ld) {
  p.norm_out = xn; p.norm_ld = Dp; p.norm_dtype = dtype; p.norm_D = D;
  p.norm_gamma = gamma; p.norm_gb = gb; p.norm_gb_ld = gb_ld; p.norm_gb_half = Dp;
}

// gamma / conditioning row of the norm in front of (layer l, sub-block j of nj): j = 0 attention, nj - 1 feed-forward (nj = 3: 1 is the
// cross-attention block of the prompt-conditioned model); l == depth selects to_pred's norm.
struct NormSrc { const float* gamma; const float* gb; };
NormSrc norm_src(const TransformerW& w, const float* gb, int l, int j, int nj = 2) {
  const int D = w.dim, Dp = padk(D);
  if (l == w.depth) return {w.pred_gamma, nullptr};
  const float* g = j == 0 ? w.g1 : w.g2;
  return {g ? g + (size_t)l * D : nullptr, gb ? gb + (size_t)(nj * l + j) * 2 * Dp : nullptr};
}

// The prompt-conditioned model's extra block per layer (latent_module.py:694-700): cross-attention from the frames to the resampled
// prompt latents, no mask.  kv: [depth][B * n_kv][2 hd] keys | values of every layer (they depend on the prompt only); q: [M, hd].
struct CrossAttn { const void* q_W; const void* out_W; const void* kv; int n_kv; void* q; };

// xres fp32 [M, padk(dim)] is updated in place; `pred` receives to_pred's output.  When the model width fits the
// whole-row tile (padk(dim) <= 512) every RMSNorm is fused into the contraction that produces its input: the caller
// supplies the first one (`xn_ready`: tb.xn already holds layer 0's attention norm) or it runs standalone once.
// `rb` (split RMSNorm with adaptive norms only): fp32 rows [Bc, rb_ld] of beta . W^T, layer l at columns
// l * (3 hd [+ hd] + 2 padk(inner)): first the q/kv projection's, [then the cross-attention query projection's,] then the GEGLU
// projection's (packed column order).  `cx`: the cross-attention block between the two (NULL: the unconditional model).  gemm_flags: as in
// run_wavenet.
int run_transformer(const TransformerW& w, int dtype, float* xres, int B, int T, const int32_t* lengths, const float* gb, int gb_ld,
                    const float* rb, int rb_ld, const TfBufs& tb, void* pred, int pred_ld, int pred_dtype, bool xn_ready, hipStream_t s,
                    const CrossAttn* cx = nullptr, int32_t gemm_flags = 0) {
  const int es = esize(dtype), M = B * T;
  const int D = w.dim, Dp = padk(D), Dn = padn(D), hd = w.heads * w.dim_head, ip = padk(w.inner), in_n = padn(w.inner);
  const bool fuse = fuse_norm_enabled(Dp, dtype);
  const bool split = split_norm_enabled(Dp, dtype);
  const int nj = cx ? 3 : 2, rb_layer = 3 * hd + (cx ? hd : 0) + 2 * ip;
  bool scaled = split && xn_ready;  // tb.xn holds row*gamma + tb.ssq its sums of squares (else: the finished norm)
  auto standalone_norm = [&](int l, int j) -> int {
    const NormSrc ns = norm_src(w, gb, l, j, nj);
    return dn_rmsnorm(xres, Dp, tb.xn, Dp, dtype, M, D, T, ns.gamma, ns.gb, gb_ld, Dp, s);
  };
  if (!((fuse || split) && xn_ready)) DN_TRY(standalone_norm(0, 0));
  // The GEGLU projection (K = dim: 16 K-tiles of 64-byte row pieces on the 256 x 256 tile) reads the feed-forward norm's output and
  // nothing else does: with the split norm its producer (the attention-out contraction) can write row * gamma K-blocked, and the
  // projection then stages whole cache lines from it and from a K-blocked copy of its weights.
  const int mid2 = dn::dn_is16(dtype) && M >= 2048 ? option_or(OPT_MID2, 0) : 0;  // option mid2: the K = dim projections on the 256 x 128 two-workgroup tile
  bool geglu_kb = false;
  static const bool geglu_kb_off = getenv("DN_GEGLU_KB") && atoi(getenv("DN_GEGLU_KB")) == 0;  // A/B timing
  if (!geglu_kb_off && split && !fuse && kblock_mode() != 0 && dn::dn_is16(dtype) && w.ffin_Wkb && Dp % 32 == 0) {
    DnGemmParams q = gemm_base(dtype, M, ip, Dp, T, gemm_flags);
    q.epilogue = DN_EPI_GEGLU;
    if (mid2 & 2) q.flags |= DN_TILE_256X128_2WG << DN_GEMM_TILE_SHIFT;
    const int gt = dn_conv_gemm_tile(&q);
    geglu_kb = kblock_mode() == 1 || gt == DN_TILE_256X256 || gt == DN_TILE_256X128_2WG;
  }
  // The same for the q/kv projection of layers >= 1 (layer 0's norm comes from the caller, row-major): its activations are the
  // attention norm's row * gamma, written by the previous layer's feed-forward-out contraction and read by nothing else.
  bool qkv_kb = false;
  static const bool qkv_kb_off = getenv("DN_QKV_KB") && atoi(getenv("DN_QKV_KB")) == 0;  // A/B timing
  if (!qkv_kb_off && split && !fuse && kblock_mode() != 0 && dn::dn_is16(dtype) && w.qkv_Wkb && Dp % 32 == 0) {
    DnGemmParams q = gemm_base(dtype, M, 3 * hd, Dp, T, gemm_flags);
    if (mid2 & 1) q.flags |= DN_TILE_256X128_2WG << DN_GEMM_TILE_SHIFT;
    const int qt = dn_conv_gemm_tile(&q);
    qkv_kb = kblock_mode() == 1 || qt == DN_TILE_256X256 || qt == DN_TILE_256X128_2WG;
  }
  // option qkv_192: the projection's 3 x 512 columns are 8 x 192 but 6 x 256 -- at [32,512] 512 tiles of 256 x 192 are two full rounds
  // of the chip, 384 tiles of 256 x 256 one and a half
  const int fold = ffn_fold_mode(w);
  // The folded contraction of layer l, row-major operands: three taps of the GEGLU output against W'_j, closing the residual.
  // Its tile: the route table's (128 x 128 at [32,512]: 512 workgroups over the two half-batch streams, two per CU), one forced by
  // the option, or -- FOLD_ROUTED, where fold_route says so -- the 256 x 128 shared-row tile; decided once per call.
  int fold_tile = fold == FOLD_256X128 ? DN_TILE_256X128 : fold == FOLD_256X256 ? DN_TILE_256X256 : fold == FOLD_SR ? DN_TILE_256X128_SR : 0;
  if (fold == FOLD_ROUTED && fold_route(dtype, M, Dp, ip, gemm_flags)) fold_tile = DN_TILE_256X128_SR;
  auto fold_params = [&](int l) {
    DnGemmParams p = gemm_base(dtype, M, Dp, ip, T, gemm_flags);
    p.n_terms = 3;
    for (int j = 0; j < 3; ++j) {
      p.terms[j].A = tb.gg; p.terms[j].lda = ip; p.terms[j].shift = 2 - j;
      p.terms[j].W = eoff(w.fold_W, ((size_t)l * 3 + j) * Dn * ip, es);
    }
    p.bias = w.fold_b + (size_t)l * Dp;
    p.flags |= DN_TAG_FFN_CONV << DN_GEMM_TAG_SHIFT;
    if (fold_tile && !fuse) p.flags |= fold_tile << DN_GEMM_TILE_SHIFT;
    return p;
  };
  // Where it lands on the shared-row tile (2-byte types, split norm, taps_inner not 0: dn_conv_gemm_tile says) its operands go
  // K-blocked when the engine has the K-blocked copy of the folded weights; DN_KBLOCK=0 keeps them row-major.
  bool fold_kb = false;
  if (fold && fold_tile == DN_TILE_256X128_SR && !fuse && w.fold_Wkb && kblock_mode() != 0 && dn::dn_is16(dtype)) {
    DnGemmParams q = fold_params(0);
    q.epilogue = DN_EPI_RESADD;
    if (split) { q.norm_out = tb.xn; q.norm_split = 1; }
    fold_kb = dn_conv_gemm_tile(&q) == DN_TILE_256X128_SR;
  }
  const bool qkv_192 = option_or(OPT_QKV_192, 0) != 0 && dn::dn_is16(dtype) && (3 * hd) % 192 == 0 && M >= 2048;
  for (int l = 0; l < w.depth; ++l) {
    {  // to_q ; to_kv in one contraction (:930-931,945)
      DnGemmParams p = gemm_base(dtype, M, 3 * hd, Dp, T, gemm_flags);
      p.terms[0].A = tb.xn; p.terms[0].lda = Dp; p.terms[0].W = eoff(w.qkv_W, (size_t)l * padn(3 * hd) * Dp, es);
      if (qkv_kb && l >= 1) {
        p.terms[0].W = eoff(w.qkv_Wkb, (size_t)l * padn(3 * hd) * Dp, es);
        p.terms[0].layout = DN_LAYOUT_A_KBLOCKED | DN_LAYOUT_W_KBLOCKED;
      }
      p.out = tb.qkv; p.ldo = 3 * hd; p.out_dtype = side_dtype(dtype);
      if (qkv_192) p.flags |= DN_TILE_256X192 << DN_GEMM_TILE_SHIFT;
      else if (mid2 & 1) p.flags |= DN_TILE_256X128_2WG << DN_GEMM_TILE_SHIFT;
      if (scaled) set_row_scale(p, tb, Dp, D, rb ? rb + (size_t)l * rb_layer : nullptr, rb_ld);
      DN_TRY(dn_conv_gemm(&p, s));
    }
    {
      DnAttnParams a;
      memset(&a, 0, sizeof(a));
      a.q = tb.qkv; a.k = eoff(tb.qkv, hd, es); a.v = eoff(tb.qkv, 2 * hd, es); a.out = tb.ao;
      a.ldq = a.ldk = a.ldv = 3 * hd; a.ldo = hd;
      a.B = B; a.T = T; a.heads = w.heads; a.dim_head = w.dim_head; a.dtype = dtype; a.lengths = lengths;
      a.scale = 1.0f / sqrtf((float)w.dim_head);
      DN_TRY(dn_attention(&a, s));
    }
    {  // to_out + residual (:932,692) [+ the feed-forward block's norm (:703)]
      DnGemmParams p = gemm_base(dtype, M, Dp, hd, T, gemm_flags);
      p.terms[0].A = tb.ao; p.terms[0].lda = hd; p.terms[0].W = eoff(w.out_W, (size_t)l * Dn * hd, es);
      p.epilogue = DN_EPI_RESADD; p.res = xres; p.ldr = Dp; p.out = xres; p.ldo = Dp; p.out_dtype = DN_F32;
      const NormSrc ns = norm_src(w, gb, l, 1, nj);
      if (fuse) set_norm(p, tb.xn, Dp, D, dtype, ns.gamma, ns.gb, gb_ld);
      else if (split) set_split_norm(p, tb, Dp, D, dtype, ns.gamma, ns.gb, gb_ld);
      if (geglu_kb && !cx) p.norm_split = 2;  // row * gamma goes out K-blocked: its only reader is the GEGLU projection below
      DN_TRY(dn_conv_gemm(&p, s));
    }
    if (!fuse && !split) DN_TRY(standalone_norm(l, 1));
    scaled = split;
    if (cx) {  // cross-attention to the resampled prompt latents, no mask (:694-700)
      {
        DnGemmParams p = gemm_base(dtype, M, hd, Dp, T, gemm_flags);
        p.terms[0].A = tb.xn; p.terms[0].lda = Dp; p.terms[0].W = eoff(cx->q_W, (size_t)l * padn(hd) * Dp, es);
        p.out = cx->q; p.ldo = hd; p.out_dtype = side_dtype(dtype);
        if (scaled) set_row_scale(p, tb, Dp, D, rb ? rb + (size_t)l * rb_layer + 3 * hd : nullptr, rb_ld);
        DN_TRY(dn_conv_gemm(&p, s));
      }
      {
        const void* kv = eoff(cx->kv, (size_t)l * B * cx->n_kv * 2 * hd, esize(side_dtype(dtype)));
        DnAttnParams a;
        memset(&a, 0, sizeof(a));
        a.q = cx->q; a.k = kv; a.v = eoff(kv, hd, esize(side_dtype(dtype))); a.out = tb.ao;
        a.ldq = hd; a.ldk = a.ldv = 2 * hd; a.ldo = hd;
        a.B = B; a.T = T; a.Tk = cx->n_kv; a.heads = w.heads; a.dim_head = w.dim_head; a.dtype = dtype; a.lengths = nullptr;
        a.scale = 1.0f / sqrtf((float)w.dim_head);
        DN_TRY(dn_attention(&a, s));
      }
      {
        DnGemmParams p = gemm_base(dtype, M, Dp, hd, T, gemm_flags);
        p.terms[0].A = tb.ao; p.terms[0].lda = hd; p.terms[0].W = eoff(cx->out_W, (size_t)l * Dn * hd, es);
        p.epilogue = DN_EPI_RESADD; p.res = xres; p.ldr = Dp; p.out = xres; p.ldo = Dp; p.out_dtype = DN_F32;
        const NormSrc ns = norm_src(w, gb, l, 2, nj);
        if (fuse) set_norm(p, tb.xn, Dp, D, dtype, ns.gamma, ns.gb, gb_ld);
        else if (split) set_split_norm(p, tb, Dp, D, dtype, ns.gamma, ns.gb, gb_ld);
        if (geglu_kb) p.norm_split = 2;
        DN_TRY(dn_conv_gemm(&p, s));
      }
      if (!fuse && !split) DN_TRY(standalone_norm(l, 2));
    }
    // The last contraction of the layer closes the residual [+ the next layer's attention norm (:691) or to_pred's norm (:677)]
    auto close_residual = [&](DnGemmParams& p) -> int {
      p.epilogue = DN_EPI_RESADD; p.res = xres; p.ldr = Dp; p.out = xres; p.ldo = Dp; p.out_dtype = DN_F32;
      const NormSrc ns = norm_src(w, gb, l + 1, 0, nj);
      if (fuse) set_norm(p, tb.xn, Dp, D, dtype, ns.gamma, ns.gb, gb_ld);
      else if (split) set_split_norm(p, tb, Dp, D, dtype, ns.gamma, ns.gb, gb_ld);
      if (qkv_kb && l + 1 < w.depth) p.norm_split = 2;  // the next layer's q/kv projection reads it K-blocked (to_pred: row-major)
      return dn_conv_gemm(&p, s);
    };
    if (fold) {
      // CausalConv1d(inner, inner, 3) and Linear(inner -> D) (:894,902) folded into one causal conv of three taps inner -> D
      // (dn_ffn_fold: nothing but the identity sits between them at inference): the conv's [M, inner] output is never formed
      {  // Linear(D -> 2*inner) + GEGLU (:899,881-884)
        DnGemmParams p = gemm_base(dtype, M, ip, Dp, T, gemm_flags);
        p.terms[0].A = tb.xn; p.terms[0].lda = Dp; p.terms[0].W = eoff(w.ffin_W, (size_t)l * 2 * ip * Dp, es);
        if (geglu_kb) {
          p.terms[0].W = eoff(w.ffin_Wkb, (size_t)l * 2 * ip * Dp, es);
          p.terms[0].layout = DN_LAYOUT_A_KBLOCKED | DN_LAYOUT_W_KBLOCKED;
        }
        p.bias = w.ffin_b + (size_t)l * 2 * ip;
        p.epilogue = DN_EPI_GEGLU; p.out = tb.gg; p.ldo = ip;
        if (mid2 & 2) p.flags |= DN_TILE_256X128_2WG << DN_GEMM_TILE_SHIFT;
        p.out_layout = fold_kb ? DN_LAYOUT_OUT_KBLOCKED : 0;
        if (scaled) set_row_scale(p, tb, Dp, D, rb ? rb + (size_t)l * rb_layer + 3 * hd + (cx ? hd : 0) : nullptr, rb_ld);
        DN_TRY(dn_conv_gemm(&p, s));
      }
      DnGemmParams p = fold_params(l);
      if (fold_kb)  // both operands as whole cache lines: the GEGLU output above, the weights from their K-blocked copy
        for (int j = 0; j < 3; ++j) {
          p.terms[j].W = eoff(w.fold_Wkb, ((size_t)l * 3 + j) * Dn * ip, es);
          p.terms[j].layout = DN_LAYOUT_A_KBLOCKED | DN_LAYOUT_W_KBLOCKED;
        }
      DN_TRY(close_residual(p));
    } else {
    // CausalConv1d(inner, inner, 3) (:894), set up first: when it runs on one of the two 256-row tiles its operands go K-blocked --
    // the GEGLU projection writes its output that way and the weights come from their K-blocked copy (the tile then stages
    // 1 KiB pieces of whole cache lines instead of sixteen half-lines: -5 % on this contraction; DN_KBLOCK=0 disables)
    DnGemmParams pc = gemm_base(dtype, M, ip, ip, T, gemm_flags);
    pc.n_terms = 3;
    for (int j = 0; j < 3; ++j) {
      pc.terms[j].A = tb.gg; pc.terms[j].lda = ip; pc.terms[j].shift = 2 - j;
      pc.terms[j].W = eoff(w.ffconv_W, ((size_t)l * 3 + j) * in_n * ip, es);
    }
    pc.bias = w.ffconv_b + (size_t)l * ip; pc.out = tb.fc; pc.ldo = ip;
    pc.flags |= DN_TAG_FFN_CONV << DN_GEMM_TAG_SHIFT;
    const int conv_tile = dn_conv_gemm_tile(&pc);  // 256 x 352 (the eps-predictor's width), 256 x 256 (the VAE's)
    const bool kblocked = kblock_mode() != 0 && dn::dn_is16(dtype) && w.ffconv_Wkb &&
                          (kblock_mode() == 1 || conv_tile == DN_TILE_256X352 || conv_tile == DN_TILE_256X256);
    if (kblocked)
      for (int j = 0; j < 3; ++j) {
        pc.terms[j].W = eoff(w.ffconv_Wkb, ((size_t)l * 3 + j) * in_n * ip, es);
        pc.terms[j].layout = DN_LAYOUT_A_KBLOCKED | DN_LAYOUT_W_KBLOCKED;
      }
    {  // Linear(D -> 2*inner) + GEGLU (:899,881-884)
      DnGemmParams p = gemm_base(dtype, M, ip, Dp, T, gemm_flags);
      p.terms[0].A = tb.xn; p.terms[0].lda = Dp; p.terms[0].W = eoff(w.ffin_W, (size_t)l * 2 * ip * Dp, es);
      if (geglu_kb) {
        p.terms[0].W = eoff(w.ffin_Wkb, (size_t)l * 2 * ip * Dp, es);
        p.terms[0].layout = DN_LAYOUT_A_KBLOCKED | DN_LAYOUT_W_KBLOCKED;
      }
      p.bias = w.ffin_b + (size_t)l * 2 * ip;
      p.epilogue = DN_EPI_GEGLU; p.out = tb.gg; p.ldo = ip;
      if (mid2 & 2) p.flags |= DN_TILE_256X128_2WG << DN_GEMM_TILE_SHIFT;
      p.out_layout = kblocked ? DN_LAYOUT_OUT_KBLOCKED : 0;
      if (scaled) set_row_scale(p, tb, Dp, D, rb ? rb + (size_t)l * rb_layer + 3 * hd + (cx ? hd : 0) : nullptr, rb_ld);
      DN_TRY(dn_conv_gemm(&p, s));
    }
    DN_TRY(dn_conv_gemm(&pc, s));
    {  // Linear(inner -> D) + residual (:902,704)
      DnGemmParams p = gemm_base(dtype, M, Dp, ip, T, gemm_flags);
      p.terms[0].A = tb.fc; p.terms[0].lda = ip; p.terms[0].W = eoff(w.ffout_W, (size_t)l * Dn * ip, es);
      p.bias = w.ffout_b + (size_t)l * Dp;
      DN_TRY(close_residual(p));
    }
    }
    if (!fuse && !split) DN_TRY(standalone_norm(l + 1, 0));
  }
  // to_pred = RMSNorm(gamma) + Linear(D, D, no bias) (:676-679); its norm came out of the last contraction above
  DnGemmParams p = gemm_base(dtype, M, Dp, Dp, T, gemm_flags);
  p.terms[0].A = tb.xn; p.terms[0].lda = Dp; p.terms[0].W = w.pred_W;
  p.out = pred; p.ldo = pred_ld; p.out_dtype = pred_dtype;
  if (pred_ld < Dp) p.N = pred_ld;  // dense fp32 destination narrower than the padded width
  if (split) set_row_scale(p, tb, Dp, D, nullptr, 0);  // learned gamma, no beta
  return dn_conv_gemm(&p, s);
}

const void* const* take_wavenet(WavenetW& w, const void* const* t) {
  w.init_W = t[0]; w.init_b = (const float*)t[1]; w.conv_W = t[2]; w.conv_b = (const float*)t[3];
  w.res_W = t[4]; w.res_b = (const float*)t[5]; w.skip_W = t[6]; w.skip_b = (const float*)t[7];
  w.final_W = t[8]; w.final_b = (const float*)t[9];
  w.conv_Wkb = t[10]; w.res_Wkb = t[11];
  return t + kWavenetTensors;
}

const void* const* take_transformer(TransformerW& w, const void* const* t) {
  w.qkv_W = t[0]; w.out_W = t[1]; w.ffin_W = t[2]; w.ffin_b = (const float*)t[3]; w.ffconv_W = t[4];
  w.ffconv_b = (const float*)t[5]; w.ffout_W = t[6]; w.ffout_b = (const float*)t[7];
  w.g1 = (const float*)t[8]; w.g2 = (const float*)t[9]; w.pred_gamma = (const float*)t[10]; w.pred_W = t[11];
  w.ffconv_Wkb = t[12]; w.ffin_Wkb = t[13]; w.qkv_Wkb = t[14];
  return t + kTransformerTensors;
}

int check_dims(const char* who, int dtype, int dim, int heads, int dim_head, int layers) {
  DN_CHECK_ARG(dtype == DN_F32 || dtype == DN_BF16 || dtype == DN_BF16X3 || dtype == DN_F16, "%s: bad dtype %d", who, dtype);
  DN_CHECK_ARG(dim > 0 && dim % 4 == 0, "%s: dim=%d must be a positive multiple of 4", who, dim);
  DN_CHECK_ARG((heads * dim_head) % 64 == 0, "%s: heads*dim_head=%d must be a multiple of 64", who, heads * dim_head);
  DN_CHECK_ARG(layers >= 1 && layers <= DN_MAX_TERMS, "%s: wavenet layers=%d must be in 1..%d", who, layers, DN_MAX_TERMS);
  return DN_OK;
}

// ------------------------------------------------------------------------------------------ eps plan
struct EpsBufs {
  float *cond, *gb, *xres;
  void *xin, *h0, *tp, *gbh;  // gbh: the conditioning rows in the arithmetic dtype (A operand of the beta . W^T contraction)
  WaveBufs wv;
  TfBufs tf;
};

EpsBufs plan_eps(const DnEps* m, int B, int T, int Bt, Arena& ar) {
  const int es = esize(m->cfg.dtype), M = B * T;
  const int C = m->cfg.dim * m->cfg.cond_mult, Dp = padk(m->cfg.dim), zp = padk(m->cfg.latent);
  EpsBufs b;
  b.cond = (float*)ar.take((size_t)Bt * C * 4);
  b.gb = (float*)ar.take((size_t)Bt * m->n_row * 4);
  b.gbh = m->cfg.dtype == DN_F32 ? nullptr : ar.take((size_t)Bt * m->n_cond * es);
  b.xin = ar.take((size_t)M * zp * es);
  b.h0 = ar.take((size_t)M * Dp * es);
  b.wv = plan_wave(m->wn, M, es, ar);
  b.xres = (float*)ar.take((size_t)M * Dp * 4);
  b.tf = plan_tf(m->tf, M, es, ar);
  b.tp = ar.take((size_t)M * Dp * es);
  return b;
}

__global__ void fill_t_kernel(int32_t* t, int n, const int32_t* counter) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) t[i] = *counter;
}
__global__ void set_counter_kernel(int32_t* counter, int v) { *counter = v; }
__global__ void dec_counter_kernel(int32_t* counter) { *counter -= 1; }
__global__ void inc_counter_kernel(int32_t* counter) { *counter += 1; }  // dn_ddim_sched_loop counts step indices upwards

}  // namespace

// =========================================================================================== eps
extern "C" int dn_eps_create(const DnEpsConfig* cfg, const void* const* weights, int32_t n_weights, DnEps** out) {
  DN_CHECK_ARG(cfg && weights && out, "dn_eps_create: null argument");
  const bool cond_model = cfg->dim_prompt > 0;
  const int expect_tensors = kEpsTensors + (cond_model ? kEpsCondTensors : 0);
  DN_CHECK_ARG(n_weights == expect_tensors, "dn_eps_create: expected %d packed tensors, got %d", expect_tensors, n_weights);
  DN_CHECK_ARG(!cond_model || (cfg->dim_prompt % 4 == 0 && cfg->num_latents >= 1 && cfg->resampler_depth >= 1),
               "dn_eps_create: conditional model needs dim_prompt %% 4 == 0, num_latents >= 1, resampler_depth >= 1");
  DN_TRY(check_dims("dn_eps_create", cfg->dtype, cfg->dim, cfg->heads, cfg->dim_head, cfg->wn_layers));
  DN_CHECK_ARG(cfg->dim % 2 == 0 && (cfg->dim * cfg->cond_mult) % 64 == 0, "dn_eps_create: dim*cond_mult must be a multiple of 64");
  DN_CHECK_ARG(cfg->latent % 4 == 0 && cfg->latent > 0, "dn_eps_create: latent=%d must be a multiple of 4", cfg->latent);
  for (int i = 0; i < n_weights; ++i) DN_CHECK_ARG(weights[i] != nullptr, "dn_eps_create: packed tensor %d is null", i);
  DnEps* m = new (std::nothrow) DnEps();
  DN_CHECK_ARG(m != nullptr, "dn_eps_create: out of host memory");
  memset(m, 0, sizeof(*m));
  m->cfg = *cfg;
  const void* const* t = weights;
  m->w_freq = (const float*)t[0]; m->tc_W = (const float*)t[1]; m->tc_b = (const float*)t[2];
  m->cond_W = t[3]; m->cond_b = (const float*)t[4]; m->init_W = t[5]; m->init_b = (const float*)t[6];
  t += 7;
  m->wn.cin = m->wn.cout = cfg->dim; m->wn.stacks = cfg->wn_stacks; m->wn.layers = cfg->wn_layers;
  t = take_wavenet(m->wn, t);
  m->tf.dim = cfg->dim; m->tf.depth = cfg->depth; m->tf.heads = cfg->heads; m->tf.dim_head = cfg->dim_head;
  m->tf.inner = (int)((double)cfg->dim * 4 * 2 / 3);  // int(dim*mult*2/3), latent_module.py:888
  t = take_transformer(m->tf, t);
  m->tf.g1 = m->tf.g2 = nullptr;  // time-conditioned norms carry no learned gamma (:662-663)
  m->final_W = t[0]; m->final_b = (const float*)t[1]; m->pos_table = (const float*)t[2];
  m->n_cond = (cfg->wn_stacks * cfg->wn_layers + (cond_model ? 3 : 2) * cfg->depth) * 2 * padk(cfg->dim);
  m->n_row = m->n_cond + cfg->depth * (3 * cfg->heads * cfg->dim_head + 2 * padk(m->tf.inner));
  if (cond_model) {
    const void* const* c = t + 3;
    m->tpc_W = (const float*)c[0]; m->tpc_b = (const float*)c[1]; m->null_pc = (const float*)c[2]; m->null_tok = c[3];
    m->proj_W = c[4]; m->proj_b = (const float*)c[5]; m->lat_pos = (const float*)c[6];
    m->rq_W = c[7]; m->rkv_W = c[8]; m->rout_W = c[9]; m->rffin_W = c[10]; m->rffin_b = (const float*)c[11];
    m->rffout_W = c[12]; m->rffout_b = (const float*)c[13]; m->rnorm_g = (const float*)c[14];
    m->cq_W = c[15]; m->ckv_W = c[16]; m->cout_W = c[17];
  }
  *out = m;
  return DN_OK;
}

// see include/diffnorm_hip.h
extern "C" int dn_eps_set_ffn_fold(DnEps* m, const void* fold_W, const float* fold_b) {
  DN_CHECK_ARG(m && (fold_W != nullptr) == (fold_b != nullptr), "dn_eps_set_ffn_fold: null engine, or one of the two buffers without the other");
  DN_CHECK_ARG(((uintptr_t)fold_W & 127) == 0 && ((uintptr_t)fold_b & 15) == 0, "dn_eps_set_ffn_fold: fold_W 128-byte, fold_b 16-byte aligned");
  m->tf.fold_W = fold_W; m->tf.fold_b = fold_b; m->tf.fold_Wkb = nullptr;
  m->tf.fold_default = m->cfg.dtype == DN_BF16 ? FOLD_OFF : FOLD_ROUTED;
  for (StepGraph* g : {&m->loop_graph, &m->guided_graph}) {  // a captured step holds the launches of the other form
    if (g->exec) (void)hipGraphExecDestroy((hipGraphExec_t)g->exec);
    g->exec = nullptr;
  }
  m->table_ws = nullptr;
  return DN_OK;
}

// see include/diffnorm_hip.h
extern "C" int dn_eps_set_ffn_fold_kblocked(DnEps* m, const void* fold_Wkb) {
  DN_CHECK_ARG(m && (!fold_Wkb || (m->tf.fold_W && dn::dn_is16(m->cfg.dtype))) && ((uintptr_t)fold_Wkb & 127) == 0,
               "dn_eps_set_ffn_fold_kblocked: null engine, no folded weights attached, not a 2-byte arithmetic, or fold_Wkb not 128-byte aligned");
  m->tf.fold_Wkb = fold_Wkb;
  for (StepGraph* g : {&m->loop_graph, &m->guided_graph}) {  // a captured step holds the other operand layout
    if (g->exec) (void)hipGraphExecDestroy((hipGraphExec_t)g->exec);
    g->exec = nullptr;
  }
  return DN_OK;
}

extern "C" void dn_eps_destroy(DnEps* m) {
  if (!m) return;
  for (StepGraph* g : {&m->loop_graph, &m->guided_graph})
    if (g->exec) (void)hipGraphExecDestroy((hipGraphExec_t)g->exec);
  if (m->ev_fork) (void)hipEventDestroy((hipEvent_t)m->ev_fork);
  if (m->ev_join) (void)hipEventDestroy((hipEvent_t)m->ev_join);
  if (m->side_stream) (void)hipStreamDestroy((hipStream_t)m->side_stream);
  delete m;
}

static size_t eps_ws_core(const DnEps* m, int B, int T) {
  Arena ar{nullptr, 0, 0};
  (void)plan_eps(m, B, T, B, ar);
  return ar.off + 256;
}

extern "C" size_t dn_eps_workspace_bytes(const DnEps* m, int32_t B, int32_t T) {
  if (!m || B <= 0 || T <= 0) return 0;
  return eps_ws_core(m, B, T);
}

namespace {

// Split RMSNorm: the beta of an adaptive norm reaches its consumer as beta . W^T, which depends on the conditioning row only -- one
// grouped contraction per consumer (one group per layer) writes it to rb [n, rb_ld]: per layer [q/kv columns | cross-attention query
// columns (prompt-conditioned model) | GEGLU columns (packed order)].  gb: the n conditioning rows (fp32, row stride gb_ld); gbh:
// room for them in the arithmetic dtype (unused in fp32).
int eps_beta_rows(const DnEps* m, const float* gb, int gb_ld, int n, void* gbh, float* rb, int rb_ld, hipStream_t s) {
  const int Dp = padk(m->cfg.dim), dtype = m->cfg.dtype, es = esize(dtype);
  const TransformerW& w = m->tf;
  const bool cx = m->cfg.dim_prompt > 0;
  const int hd = w.heads * w.dim_head, ip = padk(w.inner), nj = cx ? 3 : 2, rb_layer = 3 * hd + (cx ? hd : 0) + 2 * ip;
  const size_t tf_off = (size_t)m->cfg.wn_stacks * m->cfg.wn_layers * 2 * Dp;  // first transformer norm's [gamma ; beta]
  const void* A = gb;
  int lda = gb_ld;
  if (dtype != DN_F32) {  // operands in the arithmetic dtype
    DN_TRY(dn_convert_rows(gb, DN_F32, gb_ld, gbh, dtype, m->n_cond, n, m->n_cond, s));
    A = gbh; lda = m->n_cond;
  }
  int col = 0;
  for (int j = 0; j < nj; ++j) {  // j = 0: attention norm -> q/kv projection; nj - 1: feed-forward norm -> GEGLU projection
    const bool last = j == nj - 1;
    const int N = j == 0 ? 3 * hd : (last ? 2 * ip : hd);
    DnGemmParams q = gemm_base(dtype, n, N, Dp, 1);
    q.groups = w.depth;
    q.terms[0].A = eoff(A, tf_off + (size_t)j * 2 * Dp + Dp, es); q.terms[0].lda = lda; q.terms[0].a_gstride = (int64_t)nj * 2 * Dp;
    q.terms[0].W = j == 0 ? w.qkv_W : (last ? w.ffin_W : m->cq_W);
    q.terms[0].w_gstride = j == 0 ? (int64_t)padn(3 * hd) * Dp : (last ? (int64_t)2 * ip * Dp : (int64_t)padn(hd) * Dp);
    q.out = rb + col; q.ldo = rb_ld; q.out_dtype = DN_F32; q.out_gstride = rb_layer;
    DN_TRY(dn_conv_gemm(&q, s));
    col += N;
  }
  return DN_OK;
}

// Conditioning table: rows of [gamma ; beta] for the S*L FiLM blocks and the 2*depth adaptive norms,
// one row per entry of `times`.  Always fp32 (exact-f32 MFMA, fp32 weights): the raw integer timestep
// drives activations of O(100), so this tiny contraction is kept out of the bf16 budget.
int eps_cond_rows(const DnEps* m, const int32_t* times, int n, float* cond, float* gb, void* gbh, hipStream_t s) {
  const int D = m->cfg.dim, C = D * m->cfg.cond_mult, Dp = padk(D), dtype = m->cfg.dtype, es = esize(dtype);
  DN_TRY(dn_time_cond(times, n, m->w_freq, D / 2, m->tc_W, m->tc_b, C, cond, nullptr, DN_F32, C, s));
  DnGemmParams p = gemm_base(DN_F32, n, m->n_cond, C, 1);  // (:507,517) and (:624,637), all at once
  p.terms[0].A = cond; p.terms[0].lda = C; p.terms[0].W = m->cond_W;
  p.bias = m->cond_b; p.out = gb; p.ldo = m->n_row; p.out_dtype = DN_F32;
  DN_TRY(dn_conv_gemm(&p, s));
  if (!split_norm_enabled(Dp, dtype)) return DN_OK;
  return eps_beta_rows(m, gb, m->n_row, n, gbh, gb + m->n_cond, m->n_row, s);
}

// Model.forward after the conditioning (latent_module.py:861-876); gb_ld == 0 -> one row for the batch.  gemm_flags: as in run_wavenet.
int eps_core(const DnEps* m, const float* x, const float* gb, int gb_ld, const int32_t* lengths, int B, int T, float* eps_out,
             const EpsBufs& b, hipStream_t s, int32_t gemm_flags = 0) {
  const DnEpsConfig& c = m->cfg;
  const int dtype = c.dtype, M = B * T;
  const int D = c.dim, Dp = padk(D), z = c.latent, zp = padk(z);
  DN_TRY(dn_convert_rows(x, DN_F32, z, b.xin, dtype, zp, M, z, s));
  {  // init_conv 1x1: latent -> dim (:734,864)
    DnGemmParams p = gemm_base(dtype, M, Dp, zp, T, gemm_flags);
    p.terms[0].A = b.xin; p.terms[0].lda = zp; p.terms[0].W = m->init_W;
    p.bias = m->init_b; p.out = b.h0; p.ldo = Dp;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  {  // WaveNet; its final 1x1 conv also adds the positional embedding and opens the fp32 residual stream
    DnGemmParams fin = gemm_base(dtype, M, Dp, Dp, T, gemm_flags);
    fin.epilogue = DN_EPI_POSEMB; fin.pos_table = m->pos_table; fin.pos_ld = Dp; fin.lengths = lengths;
    fin.out = b.xres; fin.ldo = Dp; fin.out_dtype = DN_F32;
    // layer 0's attention norm rides on the contraction that opens the residual stream
    const float* gb0 = gb + (size_t)c.wn_stacks * c.wn_layers * 2 * Dp;
    if (fuse_norm_enabled(Dp, dtype)) set_norm(fin, b.tf.xn, Dp, D, dtype, nullptr, gb0, gb_ld);
    else if (split_norm_enabled(Dp, dtype)) set_split_norm(fin, b.tf, Dp, D, dtype, nullptr, gb0, gb_ld);
    DN_TRY(run_wavenet(m->wn, dtype, b.h0, M, T, gb, gb_ld, b.wv, fin, s, gemm_flags));
  }
  const float* gb_tf = gb + (size_t)c.wn_stacks * c.wn_layers * 2 * Dp;
  const bool xn_ready = fuse_norm_enabled(Dp, dtype) || split_norm_enabled(Dp, dtype);
  DN_TRY(run_transformer(m->tf, dtype, b.xres, B, T, lengths, gb_tf, gb_ld, gb + m->n_cond, gb_ld, b.tf, b.tp, Dp, dtype, xn_ready, s, nullptr,
                         gemm_flags));
  // final_proj: dim -> latent (:807,875), dense fp32 out
  DnGemmParams p = gemm_base(dtype, M, z, Dp, T, gemm_flags);
  p.terms[0].A = b.tp; p.terms[0].lda = Dp; p.terms[0].W = m->final_W;
  p.bias = m->final_b; p.out = eps_out; p.ldo = z; p.out_dtype = DN_F32;
  return dn_conv_gemm(&p, s);
}

__global__ void copy_cond_row_kernel(const float* __restrict__ table, int n_cond, const int32_t* __restrict__ counter,
                                     float* __restrict__ dst) {
  const float4* src = reinterpret_cast<const float4*>(table + (size_t)(*counter) * n_cond);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n_cond / 4; i += gridDim.x * 256) reinterpret_cast<float4*>(dst)[i] = src[i];
}

__global__ void iota_kernel(int32_t* t, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) t[i] = i;
}

}  // namespace

extern "C" int dn_eps_forward(DnEps* m, const float* x, const int32_t* t, const int32_t* lengths, int32_t B, int32_t T,
                              int32_t shared_t, float* eps_out, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && x && t && lengths && eps_out && workspace, "dn_eps_forward: null argument");
  DN_CHECK_ARG(m->cfg.dim_prompt == 0, "dn_eps_forward: this model is conditioned on a prompt: use dn_eps_forward_cond");
  DN_CHECK_ARG(B > 0 && T > 0, "dn_eps_forward: B=%d T=%d", B, T);
  DN_CHECK_ARG(T <= m->cfg.max_pos, "dn_eps_forward: T=%d exceeds the positional table (%d)", T, m->cfg.max_pos);
  hipStream_t s = (hipStream_t)stream;
  const int Bt = shared_t ? 1 : B;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  EpsBufs b = plan_eps(m, B, T, Bt, ar);
  DN_TRY(check_workspace("dn_eps_forward", workspace, workspace_bytes, ar.off));
  DN_TRY(eps_cond_rows(m, t, Bt, b.cond, b.gb, b.gbh, s));
  return eps_core(m, x, b.gb, shared_t ? 0 : m->n_row, lengths, B, T, eps_out, b, s);
}

extern "C" int dn_eps_weights_changed(DnEps* m) {
  DN_CHECK_ARG(m, "dn_eps_weights_changed: null engine");
  m->table_ws = nullptr;  // DN_LOOP_KEEP_TABLE: the next call rebuilds the conditioning table
  m->table_rows = 0;
  // dn_guided_ddim_loop and dn_guided_dpm_loop keep nothing derived from the weights across calls: every call rebuilds its time table, and
  // its eager first step recomputes the prompt-only state; a captured step holds addresses only
  return DN_OK;
}

static size_t ddim_extra_bytes(const DnEps* m, int B, int T, int start_step) {
  const size_t C = (size_t)m->cfg.dim * m->cfg.cond_mult;
  return (size_t)B * T * m->cfg.latent * 4 + (size_t)start_step * (m->n_row + C) * 4 + (size_t)start_step * m->n_cond * 4 +
         (size_t)(B + start_step) * 4 + 4096;
}

extern "C" size_t dn_ddim_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t start_step) {
  if (!m || B <= 0 || T <= 0 || start_step < 1) return 0;
  const size_t whole = eps_ws_core(m, B, T);
  const size_t halves = B >= 2 ? eps_ws_core(m, B / 2, T) + eps_ws_core(m, B - B / 2, T) : 0;  // DN_LOOP_SPLIT2
  return (whole > halves ? whole : halves) + ddim_extra_bytes(m, B, T, start_step);
}

namespace {
// Runs n steps of a chain on `s` as replays of one captured step.  A hit of `slot` replays all n.  A miss evicts the slot, captures
// `step` (recorded, not run), instantiates, stores the graph under `key` and replays it; with eager_first it runs one step eagerly
// before the capture (which also settles the per-kernel attributes outside capture) and replays n - 1.
template <class Step>
int replay_steps(StepGraph& slot, const StepKey& key, bool eager_first, int n, hipStream_t s, const char* who, Step&& step) {
  if (!slot.exec || key.injected || memcmp(&slot.key, &key, sizeof(key)) != 0) {
    if (eager_first) {
      DN_TRY(step());
      --n;
    }
    if (slot.exec) {
      (void)hipGraphExecDestroy((hipGraphExec_t)slot.exec);
      slot.exec = nullptr;
    }
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) {
      dn_set_error("%s: hipStreamBeginCapture failed", who);
      return DN_ELAUNCH;
    }
    int rc = step();
    hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc == DN_OK && (e != hipSuccess || !graph)) {
      dn_set_error("%s: hipStreamEndCapture: %s", who, hipGetErrorString(e));
      rc = DN_ELAUNCH;
    }
    hipGraphExec_t exec = nullptr;
    if (rc == DN_OK && (e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)) != hipSuccess) {
      dn_set_error("%s: hipGraphInstantiate: %s", who, hipGetErrorString(e));
      rc = DN_ELAUNCH;
    }
    if (graph) (void)hipGraphDestroy(graph);  // on every path: the executable graph keeps what it needs
    if (rc != DN_OK) return rc;
    slot.exec = exec;
    slot.key = key;
  }
  for (; n > 0; --n) {
    const hipError_t e = hipGraphLaunch((hipGraphExec_t)slot.exec, s);
    if (e != hipSuccess) {
      dn_set_error("%s: hipGraphLaunch: %s", who, hipGetErrorString(e));
      return DN_ELAUNCH;
    }
  }
  return DN_OK;
}

// what an update of the unconditional device loops works on: the whole batch's buffers (an update offsets them to its half itself)
struct StepBufs {
  float *x, *eps, *hist;
  const float* coef;  // what the captured step reads: the caller's table, or a schedule's rows in the workspace
  const int32_t *tvec, *steps, *counter;
  int T, z;
  int64_t all;    // elements of the whole batch: the row stride of injected noise
  int noise_top;  // injected ancestral noise: row (noise_top - t) belongs to step t
};

// One unconditional device loop: what sampler_loop needs to know beyond its arguments.
struct LoopDesc {
  const char* name;  // for messages (dn_ddpm_loop has always reported under dn_ddim_loop's)
  const char* ws_name;
  size_t (*ws_bytes)(const DnEps*, int32_t, int32_t, int32_t);
  // a loop over a timestep schedule (device int32 [n_steps], coefficient rows [n_steps, coef_cols]): the counter counts step indices
  // 0 .. n_steps-1 upwards and the conditioning table has one row per step; steps == NULL: timesteps start_step-1 downwards
  const int32_t* steps;
  int n_steps, coef_cols;
  bool history;  // one more persistent buffer of the latent's size (dn_dpm_loop: the previous step's data prediction)
  StepKey kind;  // ancestral, clip, scheduled, eta, dpm, seed, keys, injected: the loop's part of the graph key
  // the scheduler update after an evaluation, applied to batch rows [b0, b0 + nb) = half 0 or 1 on `stream`
  std::function<int(const StepBufs&, int half, int b0, int nb, hipStream_t stream)> update;
};
}  // namespace

static int sampler_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, int32_t start_step, int32_t max_evals,
                        const float* coef, int32_t timesteps, int32_t flags, void* workspace, size_t workspace_bytes, void* stream,
                        const LoopDesc& d) {
  DN_CHECK_ARG(m && m->cfg.dim_prompt == 0, "dn_ddim_loop: the device loop covers the unconditional model (prompted chains step through dn_eps_forward_cond)");
  int use_graph = flags & DN_LOOP_GRAPH;
  const bool split = (flags & DN_LOOP_SPLIT2) && B >= 2;
  DN_CHECK_ARG(m && x && lengths && coef && workspace, "dn_ddim_loop: null argument");
  const bool sched = d.steps != nullptr, ancestral = d.kind.ancestral;
  if (sched) {  // (a strictly descending list inside [0, timesteps-1] has at most `timesteps` entries)
    DN_CHECK_ARG(d.n_steps >= 1 && d.n_steps <= timesteps, "%s: n_steps=%d must be in [1, %d]", d.name, d.n_steps, timesteps);
    DN_CHECK_ARG(B > 0 && T > 0 && T <= m->cfg.max_pos, "%s: B=%d T=%d (positional table: %d)", d.name, B, T, m->cfg.max_pos);
    DN_CHECK_ARG(d.kind.eta || d.kind.generic || !d.kind.injected, "dn_ddim_sched_loop: injected noise needs eta_on (eta = 0 draws none)");
  } else
    DN_CHECK_ARG(start_step >= 1 && start_step <= timesteps - (ancestral ? 0 : 1), "dn_ddim_loop: start_step=%d must be in [1, %d]", start_step,
                 timesteps - (ancestral ? 0 : 1));
  if (sched) start_step = d.n_steps;  // rows of the conditioning table = evaluations of the chain
  hipStream_t s = (hipStream_t)stream;
  DN_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "dn_ddim_loop: workspace must be 256-byte aligned");
  const int z = m->cfg.latent, M = B * T, C = m->cfg.dim * m->cfg.cond_mult;
  // Two half-batches on two streams (a fork/join inside the captured step): the halves are independent chains, so the
  // fill / drain of one half's launches overlaps the other half's main loops (measured -5 % per step at [32,512]).
  const int B0 = split ? B / 2 : B, B1 = B - B0;
  const size_t core0 = eps_ws_core(m, B0, T), core1 = split ? eps_ws_core(m, B1, T) : 0, core = core0 + core1;
  // a schedule: the documented size, split or not (>= what this call lays out); a timestep loop: what this call lays out
  const size_t need = sched ? d.ws_bytes(m, B, T, start_step) : core + ddim_extra_bytes(m, B, T, start_step);
  if (need > workspace_bytes) {
    dn_set_error("%s: workspace %zu < required %zu (see %s)", d.name, workspace_bytes, need, d.ws_name);
    return DN_EWORKSPACE;
  }
  Arena core_ar{(char*)workspace, 0, core0};
  const EpsBufs bufs = plan_eps(m, B0, T, 1, core_ar);
  Arena core_ar1{(char*)workspace + core0, 0, core1};
  EpsBufs bufs1 = bufs;
  if (split) bufs1 = plan_eps(m, B1, T, 1, core_ar1);
  if (split && !m->side_stream) {
    if (hipStreamCreateWithFlags((hipStream_t*)&m->side_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags((hipEvent_t*)&m->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags((hipEvent_t*)&m->ev_join, hipEventDisableTiming) != hipSuccess) {
      dn_set_error("dn_ddim_loop: could not create the side stream");
      return DN_ELAUNCH;
    }
  }
  hipStream_t s2 = (hipStream_t)m->side_stream;
  Arena ar{(char*)workspace + core, 0, workspace_bytes - core};
  // fixed-size state first, so a cached graph stays valid when only start_step changes
  float* eps = (float*)ar.take((size_t)M * z * 4);
  float* hist = d.history ? (float*)ar.take((size_t)M * z * 4) : nullptr;  // (the whole batch's)
  int32_t* tvec = (int32_t*)ar.take((size_t)B * 4);
  int32_t* counter = (int32_t*)ar.take(64);
  float* table = (float*)ar.take((size_t)start_step * m->n_row * 4);  // conditioning rows for t = 0..start_step-1
  float* cond_all = (float*)ar.take((size_t)start_step * C * 4);
  void* table_h = m->cfg.dtype == DN_F32 ? nullptr : ar.take((size_t)start_step * m->n_cond * esize(m->cfg.dtype));
  int32_t* tall = (int32_t*)ar.take((size_t)start_step * 4);
  const int last = (start_step == 1 || ancestral || sched) ? 0 : 1;  // DDIM: the loop breaks after the t == 1 update (:1444-1445); p_sample_loop runs t = 0 too
  int n_eval = start_step - last;             // t = start_step-1 ... last (a schedule: every one of its steps)
  if (max_evals > 0 && max_evals < n_eval) n_eval = max_evals;  // partial chain (benchmarks, chunked sampling)
  // The 56 conditioning vectors depend only on t: build them for the whole chain once (fp32), so the
  // 117 M conditioning weights are not re-streamed at every step.
  const bool keep = (flags & DN_LOOP_KEEP_TABLE) && m->table_ws == workspace && m->table_at == table && m->table_B == B && m->table_T == T &&
                    m->table_split == (int)split && m->table_rows >= start_step;
  StepBufs sb = {x, eps, hist, coef, tvec, tall, counter, T, z, (int64_t)M * z, start_step - 1};
  if (sched) {
    // row i of the table belongs to steps[i].  The schedule and its coefficient rows move into the workspace, so a captured step
    // holds workspace addresses only: the steps where the other loops keep 0..start_step-1, the coefficients over `cond_all`
    // (dn_ddim_sched_workspace_bytes: dead once the table is built, and C >= 64 floats a row against DN_DDIM_SCHED_COLS).
    static_assert(DN_DDIM_SCHED_COLS <= 64 && DN_DPM_COLS <= 64 && DN_GD_COLS <= 64, "the coefficient rows live in cond_all");
    if (hipMemcpyAsync(tall, d.steps, (size_t)start_step * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      dn_set_error("%s: copying the schedule failed", d.name);
      return DN_ELAUNCH;
    }
    DN_TRY(eps_cond_rows(m, tall, start_step, cond_all, table, table_h, s));
    if (hipMemcpyAsync(cond_all, coef, (size_t)start_step * d.coef_cols * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      dn_set_error("%s: copying the coefficient rows failed", d.name);
      return DN_ELAUNCH;
    }
    sb.coef = cond_all;
    m->table_ws = nullptr;  // (not a table DN_LOOP_KEEP_TABLE could continue on)
    m->table_rows = 0;
  } else if (!keep) {
    hipLaunchKernelGGL(iota_kernel, dim3((start_step + 255) / 256), dim3(256), 0, s, tall, start_step);
    DN_TRY(eps_cond_rows(m, tall, start_step, cond_all, table, table_h, s));
    m->table_ws = workspace; m->table_at = table; m->table_B = B; m->table_T = T; m->table_split = (int)split; m->table_rows = start_step;
  }
  const int32_t twin = split ? DN_GEMM_TWIN : 0;  // every contraction of a half batch has its twin beside it (tile choice)
  auto one_step = [&]() -> int {
    if (!sched)  // (the scheduled update reads its row by the counter: no per-sample step vector)
      hipLaunchKernelGGL(fill_t_kernel, dim3((B + 255) / 256), dim3(256), 0, s, tvec, B, counter);
    hipLaunchKernelGGL(copy_cond_row_kernel, dim3(32), dim3(256), 0, s, table, m->n_row, counter, bufs.gb);
    if (split) {  // fork: the second half runs on the side stream behind the shared conditioning row
      const size_t off = (size_t)B0 * T * z;
      if (hipEventRecord((hipEvent_t)m->ev_fork, s) != hipSuccess || hipStreamWaitEvent(s2, (hipEvent_t)m->ev_fork, 0) != hipSuccess) {
        dn_set_error("dn_ddim_loop: fork failed");
        return DN_ELAUNCH;
      }
      DN_TRY(eps_core(m, x + off, bufs.gb, 0, lengths + B0, B1, T, eps + off, bufs1, s2, twin));
      DN_TRY(d.update(sb, 1, B0, B1, s2));
    }
    DN_TRY(eps_core(m, x, bufs.gb, 0, lengths, B0, T, eps, bufs, s, twin));
    DN_TRY(d.update(sb, 0, 0, B0, s));
    if (split) {  // join
      if (hipEventRecord((hipEvent_t)m->ev_join, s2) != hipSuccess || hipStreamWaitEvent(s, (hipEvent_t)m->ev_join, 0) != hipSuccess) {
        dn_set_error("dn_ddim_loop: join failed");
        return DN_ELAUNCH;
      }
    }
    if (sched)
      hipLaunchKernelGGL(inc_counter_kernel, dim3(1), dim3(1), 0, s, counter);
    else
      hipLaunchKernelGGL(dec_counter_kernel, dim3(1), dim3(1), 0, s, counter);
    DN_CHECK_LAUNCH("dn_ddim_loop step");
    return DN_OK;
  };
  hipLaunchKernelGGL(set_counter_kernel, dim3(1), dim3(1), 0, s, counter, sched ? 0 : start_step - 1);
  if (!s) use_graph = 0;  // the null stream cannot be captured
  if (use_graph && n_eval > 2) {
    // what the captured step bakes in, and no more: any start_step / max_evals is served (the fixed-size state is laid out first);
    // a dn_set_option since the capture may route the contractions differently, so the option generation is part of it
    StepKey key = d.kind;
    key.ws = workspace; key.x = x; key.len = lengths; key.coef = sb.coef;
    key.B = B; key.T = T; key.flags = flags & ~DN_LOOP_KEEP_TABLE; key.opt_gen = dn::option_generation();
    DN_TRY(replay_steps(m->loop_graph, key, true, n_eval, s, d.name, one_step));
  } else {
    for (int done = 0; done < n_eval; ++done) DN_TRY(one_step());
  }
  return n_eval;
}

// the loop's part of a graph key (memset first: the key is compared with memcmp).  A keyed chain carries the address of its keys and
// seed 0: the captured step bakes in that address, never the keys' contents.
static StepKey step_kind(uint64_t seed, const float* noise, const uint64_t* keys = nullptr) {
  StepKey k;
  memset(&k, 0, sizeof(k));
  k.seed = keys ? 0 : seed;
  k.keys = keys;
  k.injected = noise != nullptr;
  return k;
}

// what every keyed loop entry refuses before anything is written
static int check_keys(const char* who, const DnEps* m, const uint64_t* keys) {
  DN_CHECK_ARG(m && keys, "%s: null engine or keys", who);
  DN_CHECK_ARG(((uintptr_t)keys & 7) == 0, "%s: keys must be 8-byte aligned", who);
  DN_CHECK_ARG(m->cfg.latent % 4 == 0, "%s: the latent width %d must be a multiple of 4", who, m->cfg.latent);
  return DN_OK;
}

extern "C" int dn_ddim_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, int32_t start_step, int32_t max_evals,
                            const float* coef, int32_t timesteps, int32_t flags, void* workspace, size_t workspace_bytes,
                            void* stream) {
  // DDIM eta = 0 with `coef` [timesteps, 4], on the half's own rows
  LoopDesc d = {"dn_ddim_loop", "dn_ddim_workspace_bytes", dn_ddim_workspace_bytes, nullptr, 0, 0, false, step_kind(0, nullptr), nullptr};
  d.update = [](const StepBufs& b, int, int b0, int nb, hipStream_t st) {
    float* xh = b.x + (size_t)b0 * b.T * b.z;
    return dn_ddim_step(xh, b.eps + (size_t)b0 * b.T * b.z, xh, nullptr, DN_F32, b.z, nb * b.T, b.z, b.z, b.T, b.coef, b.tvec + b0, st);
  };
  return sampler_loop(m, x, lengths, B, T, start_step, max_evals, coef, timesteps, flags, workspace, workspace_bytes, stream, d);
}

// dn_ddpm_loop (keys == NULL) and dn_ddpm_loop_keyed
static int ddpm_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, int32_t start_step, int32_t max_evals, const float* table,
                     int32_t timesteps, int32_t clip_denoised, uint64_t seed, const float* noise, const uint64_t* keys, int32_t flags,
                     void* workspace, size_t workspace_bytes, void* stream) {
  // the ancestral step with `table` [timesteps, DN_GD_COLS], on the half's own rows; seed-drawn, the second half draws from its own
  // key; keyed, both halves draw under the utterances' keys (the launch is told its first batch row), so the chain is split-invariant
  LoopDesc d = {"dn_ddim_loop", "dn_ddim_workspace_bytes", dn_ddim_workspace_bytes, nullptr, 0, 0, false, step_kind(seed, noise, keys), nullptr};
  d.kind.ancestral = 1;
  d.kind.clip = clip_denoised != 0;
  d.update = [=](const StepBufs& b, int half, int b0, int nb, hipStream_t st) {
    const size_t off = (size_t)b0 * b.T * b.z;
    return dn_ddpm_step_launch(b.x + off, b.eps + off, nb * b.T, b.z, b.T, b.coef, b.tvec + b0, clip_denoised, noise ? noise + off : nullptr, b.all,
                               b.noise_top, half ? seed ^ 0x9E3779B97F4A7C15ull : seed, keys, b0, st);
  };
  return sampler_loop(m, x, lengths, B, T, start_step, max_evals, table, timesteps, flags, workspace, workspace_bytes, stream, d);
}

extern "C" int dn_ddpm_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, int32_t start_step, int32_t max_evals,
                            const float* table, int32_t timesteps, int32_t clip_denoised, uint64_t seed, const float* noise, int32_t flags,
                            void* workspace, size_t workspace_bytes, void* stream) {
  return ddpm_loop(m, x, lengths, B, T, start_step, max_evals, table, timesteps, clip_denoised, seed, noise, nullptr, flags, workspace,
                   workspace_bytes, stream);
}

extern "C" int dn_ddpm_loop_keyed(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, int32_t start_step, int32_t max_evals,
                                  const float* table, int32_t timesteps, int32_t clip_denoised, const uint64_t* keys, int32_t flags,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  DN_TRY(check_keys("dn_ddpm_loop_keyed", m, keys));
  return ddpm_loop(m, x, lengths, B, T, start_step, max_evals, table, timesteps, clip_denoised, 0, nullptr, keys, flags, workspace,
                   workspace_bytes, stream);
}

// rows of cond_all (C fp32 each) hold the chain's coefficient rows after the table is built: the same bytes as dn_ddim_loop's for
// start_step = n_steps
extern "C" size_t dn_ddim_sched_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t n_steps) {
  return dn_ddim_workspace_bytes(m, B, T, n_steps);
}

extern "C" int dn_ddim_sched_check(const int32_t* steps, int32_t n_steps, int32_t timesteps) {
  DN_CHECK_ARG(steps && timesteps >= 1, "dn_ddim_sched_check: null schedule or timesteps=%d", timesteps);
  DN_CHECK_ARG(n_steps >= 1, "dn_ddim_sched_check: the schedule is empty");
  DN_CHECK_ARG(n_steps <= timesteps, "dn_ddim_sched_check: %d steps do not fit into %d timesteps", n_steps, timesteps);
  for (int i = 0; i < n_steps; ++i) {
    DN_CHECK_ARG(steps[i] >= 0 && steps[i] < timesteps, "dn_ddim_sched_check: step %d = %d is outside [0, %d]", i, steps[i], timesteps - 1);
    DN_CHECK_ARG(i == 0 || steps[i] < steps[i - 1], "dn_ddim_sched_check: step %d = %d does not descend from %d", i, steps[i], steps[i - 1]);
  }
  return DN_OK;
}

// dn_ddim_sched_loop (keys == NULL) and dn_ddim_sched_loop_keyed (eta on)
static int ddim_sched_loop(const char* who, DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps,
                           const float* coef, int32_t n_steps, int32_t timesteps, int32_t eta_on, uint64_t seed, const float* noise,
                           const uint64_t* keys, int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(steps, "%s: null schedule", who);
  DN_CHECK_ARG(!(flags & ~(DN_LOOP_GRAPH | DN_LOOP_SPLIT2)), "%s: flags=%d (DN_LOOP_GRAPH | DN_LOOP_SPLIT2 only)", who, flags);
  eta_on = eta_on != 0;
  if (!eta_on) seed = 0;
  // the scheduled update on the half's element range of the whole batch: the whole batch's element index keys the draw (or finds the
  // utterance's key), so the halves share one stream of numbers
  LoopDesc d = {who, "dn_ddim_sched_workspace_bytes", dn_ddim_sched_workspace_bytes, steps, n_steps, DN_DDIM_SCHED_COLS,
                false, step_kind(seed, noise, keys), nullptr};
  d.kind.scheduled = 1;
  d.kind.eta = (uint16_t)eta_on;
  d.update = [=](const StepBufs& b, int, int b0, int nb, hipStream_t st) {
    SchedStep u = {SCHED_DDIM, b.x, (int64_t)b0 * b.T * b.z, (int64_t)nb * b.T * b.z, b.eps};
    u.coef = b.coef; u.steps = b.steps; u.counter = b.counter; u.eta_on = eta_on;
    u.src = sched_noise(noise, b.all, seed, keys, (int64_t)b.T * (b.z >> 2));
    return sched_step_launch("dn_ddim_sched_loop", u, st);
  };
  return sampler_loop(m, x, lengths, B, T, 0, 0, coef, timesteps, flags, workspace, workspace_bytes, stream, d);
}

extern "C" int dn_ddim_sched_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* coef,
                                  int32_t n_steps, int32_t timesteps, int32_t eta_on, uint64_t seed, const float* noise, int32_t flags,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  return ddim_sched_loop("dn_ddim_sched_loop", m, x, lengths, B, T, steps, coef, n_steps, timesteps, eta_on, seed, noise, nullptr, flags,
                         workspace, workspace_bytes, stream);
}

extern "C" int dn_ddim_sched_loop_keyed(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps,
                                        const float* coef, int32_t n_steps, int32_t timesteps, const uint64_t* keys, int32_t flags,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  DN_TRY(check_keys("dn_ddim_sched_loop_keyed", m, keys));
  return ddim_sched_loop("dn_ddim_sched_loop_keyed", m, x, lengths, B, T, steps, coef, n_steps, timesteps, 1, 0, nullptr, keys, flags,
                         workspace, workspace_bytes, stream);
}

// dn_ddim_sched_loop's layout with the history buffer taken beside eps (one more 256-byte aligned block of the latent's size)
extern "C" size_t dn_dpm_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t n_steps) {
  const size_t base = dn_ddim_workspace_bytes(m, B, T, n_steps);
  if (!base) return 0;
  return base + (((size_t)B * T * m->cfg.latent * 4 + 255) & ~size_t(255));
}

extern "C" int dn_dpm_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* coef,
                           int32_t n_steps, int32_t timesteps, int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m, "dn_dpm_loop: null engine");
  DN_CHECK_ARG(m->cfg.dim_prompt == 0, "dn_dpm_loop: the solver covers the unconditional model (the prompted, guided chain is dn_guided_ddim_loop)");
  DN_CHECK_ARG(steps, "dn_dpm_loop: null schedule");
  DN_CHECK_ARG(!(flags & ~(DN_LOOP_GRAPH | DN_LOOP_SPLIT2)), "dn_dpm_loop: flags=%d (DN_LOOP_GRAPH | DN_LOOP_SPLIT2 only)", flags);
  DN_CHECK_ARG(x && lengths && coef && workspace, "dn_dpm_loop: null argument");
  // DPM-Solver++(2M) on the half's element range of the shared x / eps / hist
  LoopDesc d = {"dn_dpm_loop", "dn_dpm_workspace_bytes", dn_dpm_workspace_bytes, steps, n_steps, DN_DPM_COLS, true, step_kind(0, nullptr), nullptr};
  d.kind.scheduled = d.kind.dpm = 1;
  d.update = [](const StepBufs& b, int, int b0, int nb, hipStream_t st) {
    SchedStep u = {SCHED_DPM2M, b.x, (int64_t)b0 * b.T * b.z, (int64_t)nb * b.T * b.z, b.eps};
    u.coef = b.coef; u.counter = b.counter; u.hist = b.hist;
    return sched_step_launch("dn_dpm_loop", u, st);
  };
  return sampler_loop(m, x, lengths, B, T, 0, 0, coef, timesteps, flags, workspace, workspace_bytes, stream, d);
}

// dn_ddim_sched_loop's layout: the DN_GD_COLS coefficients of a row fit where its DN_DDIM_SCHED_COLS do
extern "C" size_t dn_gaussian_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t n_steps) {
  return dn_ddim_sched_workspace_bytes(m, B, T, n_steps);
}

// dn_gaussian_loop (keys == NULL) and dn_gaussian_loop_keyed
static int gaussian_loop(const char* who, DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps,
                         const float* table, int32_t n_steps, int32_t timesteps, int32_t sampler, int32_t clip_denoised, float eta,
                         uint64_t seed, const float* noise, const uint64_t* keys, int32_t flags, void* workspace, size_t workspace_bytes,
                         void* stream) {
  DN_CHECK_ARG(m, "%s: null engine", who);
  DN_CHECK_ARG(m->cfg.dim_prompt == 0, "%s: the loop covers the unconditional model (the prompted, guided chain is dn_guided_ddim_loop)", who);
  DN_CHECK_ARG(steps, "%s: null schedule", who);
  DN_CHECK_ARG(!(flags & ~(DN_LOOP_GRAPH | DN_LOOP_SPLIT2)), "%s: flags=%d (DN_LOOP_GRAPH | DN_LOOP_SPLIT2 only)", who, flags);
  DN_CHECK_ARG(x && lengths && table && workspace, "%s: null argument", who);
  DN_TRY(dn_gaussian_sched_args(who, n_steps, sampler, eta));
  DN_CHECK_ARG(m->cfg.latent % 4 == 0, "%s: the latent width %d must be a multiple of 4", who, m->cfg.latent);
  DN_CHECK_ARG(((uintptr_t)noise & 15) == 0, "%s: noise must be 16-byte aligned", who);
  const int clip = clip_denoised != 0;
  const bool ddim = sampler == 1;
  if (ddim && eta == 0.0f) seed = 0;  // (nothing is drawn: one graph serves every seed)
  // the generic update on the half's element range of the whole batch: the whole batch's element index keys the draw (or finds the
  // utterance's key), so the halves share one stream of numbers
  LoopDesc d = {who, "dn_gaussian_workspace_bytes", dn_gaussian_workspace_bytes, steps, n_steps, DN_GD_COLS, false, step_kind(seed, noise, keys),
                nullptr};
  d.kind.scheduled = d.kind.generic = 1;
  d.kind.ancestral = !ddim;
  d.kind.clip = (uint16_t)clip;
  d.kind.eta = ddim && eta != 0.0f;
  if (ddim) memcpy(&d.kind.eta_bits, &eta, 4);
  d.update = [=](const StepBufs& b, int, int b0, int nb, hipStream_t st) {
    SchedStep u = {SCHED_GAUSSIAN, b.x, (int64_t)b0 * b.T * b.z, (int64_t)nb * b.T * b.z, b.eps};
    u.coef = b.coef; u.steps = b.steps; u.counter = b.counter;
    u.n_steps = n_steps; u.sampler = sampler; u.clip = clip; u.eta = eta;
    u.src = sched_noise(noise, b.all, seed, keys, (int64_t)b.T * (b.z >> 2));
    return sched_step_launch("dn_gaussian_loop", u, st);
  };
  return sampler_loop(m, x, lengths, B, T, 0, 0, table, timesteps, flags, workspace, workspace_bytes, stream, d);
}

extern "C" int dn_gaussian_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* table,
                                int32_t n_steps, int32_t timesteps, int32_t sampler, int32_t clip_denoised, float eta, uint64_t seed,
                                const float* noise, int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  return gaussian_loop("dn_gaussian_loop", m, x, lengths, B, T, steps, table, n_steps, timesteps, sampler, clip_denoised, eta, seed, noise, nullptr,
                       flags, workspace, workspace_bytes, stream);
}

extern "C" int dn_gaussian_loop_keyed(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* table,
                                      int32_t n_steps, int32_t timesteps, int32_t sampler, int32_t clip_denoised, float eta,
                                      const uint64_t* keys, int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  DN_TRY(check_keys("dn_gaussian_loop_keyed", m, keys));
  return gaussian_loop("dn_gaussian_loop_keyed", m, x, lengths, B, T, steps, table, n_steps, timesteps, sampler, clip_denoised, eta, 0, nullptr, keys,
                       flags, workspace, workspace_bytes, stream);
}


// =========================================================================================== conditional variant (f3)
namespace dn {
// pooled[b, c] = mean over ALL Tp positions of the masked prompt (masked_fill(~mask, 0) then Reduce 'b n d -> b d' mean,
// latent_module.py:844-845, 764); prompt fp32 [B, Tp, P] -> pooled fp32 [B, Pp] (pad columns zero)
__global__ __launch_bounds__(256) void prompt_pool_kernel(const float* __restrict__ prompt, const int32_t* __restrict__ plen, int B, int Tp, int P,
                                                          int Pp, float* __restrict__ pooled) {
  const int b = blockIdx.x;
  const int n = plen[b] < Tp ? plen[b] : Tp;
  for (int c = threadIdx.x; c < Pp; c += 256) {
    float s = 0.f;
    if (c < P)
      for (int t = 0; t < n; ++t) s += prompt[((int64_t)b * Tp + t) * P + c];
    pooled[(int64_t)b * Pp + c] = s / (float)Tp;
  }
}
// cond2[b] = [time_cond[b] | (drop[b] ? null_prompt_cond : prompt_cond[b])]  (:846-852)
__global__ __launch_bounds__(256) void assemble_cond2_kernel(const float* __restrict__ tc, const float* __restrict__ pc, const float* __restrict__ null_pc,
                                                             const int32_t* __restrict__ drop, int B, int C, float* __restrict__ out) {
  const int64_t n = (int64_t)B * 2 * C;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / (2 * C)), c = (int)(i - (int64_t)b * 2 * C);
    out[i] = c < C ? tc[(int64_t)b * C + c] : (drop[b] ? null_pc[c - C] : pc[(int64_t)b * C + c - C]);
  }
}
// gb[b] = table[t[b] - t0] + gbp[b]: the conditioning rows of a step from the chain's time table and the prompt half
__global__ __launch_bounds__(256) void cond_rows_from_table_kernel(const float* __restrict__ table, const int32_t* __restrict__ t, int t0, int n_t,
                                                                   const float* __restrict__ gbp, int B, int n, float* __restrict__ gb) {
  const int64_t tot = (int64_t)B * (n / 4);
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / (n / 4)), c = (int)(i - (int64_t)b * (n / 4)) * 4;
    int r = t[b] - t0;
    r = r < 0 ? 0 : (r >= n_t ? n_t - 1 : r);
    const float4 a = *reinterpret_cast<const float4*>(table + (int64_t)r * n + c);
    const float4 p = *reinterpret_cast<const float4*>(gbp + (int64_t)b * n + c);
    *reinterpret_cast<float4*>(gb + (int64_t)b * n + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
  }
}
// dst rows [b, row0 + j] (row stride of a sample: rows_total) <- src rows: sample-indexed [b, j] (src_bstride = rows * ld) or shared
// (src_bstride = 0); optional per-sample override by `alt` (shared rows) where flag[b] != 0.  fp32 or bf16 sources -> dst dtype.
__global__ __launch_bounds__(256) void place_rows_kernel(const void* __restrict__ src, int src_dtype, int64_t src_bstride, const void* __restrict__ alt,
                                                         const int32_t* __restrict__ flag, void* __restrict__ dst, int dst_dtype, int B, int rows,
                                                         int ld, int rows_total, int row0) {
  const int64_t n = (int64_t)B * rows * ld;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % ld);
    const int j = (int)((i / ld) % rows);
    const int b = (int)(i / ((int64_t)ld * rows));
    const bool use_alt = alt && flag && flag[b] != 0;
    const void* sp = use_alt ? alt : src;
    const int64_t so = (use_alt ? 0 : (int64_t)b * src_bstride) + (int64_t)j * ld + c;
    const float v = src_dtype == DN_BF16X3 ? load1_split(sp, so)
                    : dn_is16(src_dtype) ? from_h16(src_dtype, reinterpret_cast<const uint16_t*>(sp)[so]) : reinterpret_cast<const float*>(sp)[so];
    const int64_t o = ((int64_t)b * rows_total + row0 + j) * ld + c;
    if (dst_dtype == DN_BF16X3)
      store1_split(dst, o, v);
    else if (dn_is16(dst_dtype))
      reinterpret_cast<uint16_t*>(dst)[o] = to_h16(dst_dtype, v);
    else
      reinterpret_cast<float*>(dst)[o] = v;
  }
}
__global__ void iota_i32_kernel(int32_t first, int32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = first + i;
}
__global__ void add_const_i32_kernel(const int32_t* __restrict__ a, int32_t c, int32_t cap, int32_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (a[i] < cap ? a[i] : cap) + c;
}
}  // namespace dn

namespace {

struct CondBufs {
  float *cond, *pooled, *pc, *cond2, *gb, *gbp, *lat, *xres, *rb;
  void *prompt_act, *ctx, *kvsrc, *lat_act, *rq, *rkv, *rao, *rgg, *c_act, *ckv, *xin, *h0, *cq, *tp, *gbh;
  int32_t* klen;
  WaveBufs wv;
  TfBufs tf;
};

CondBufs plan_eps_cond(const DnEps* m, int B, int T, int Tp, Arena& ar) {
  const DnEpsConfig& c = m->cfg;
  const int es = esize(c.dtype);
  const size_t M = (size_t)B * T, Dp = padk(c.dim), zp = padk(c.latent), C = (size_t)c.dim * c.cond_mult, Pp = padk(c.dim_prompt);
  const size_t hd = (size_t)c.heads * c.dim_head, ip = padk(m->tf.inner), ml = c.num_latents, Lk = ml + Tp;
  CondBufs b;
  memset(&b, 0, sizeof(b));
  b.cond = (float*)ar.take(B * C * 4); b.pooled = (float*)ar.take(B * Pp * 4); b.pc = (float*)ar.take(B * C * 4);
  b.cond2 = (float*)ar.take(B * 2 * C * 4); b.gb = (float*)ar.take((size_t)B * m->n_cond * 4);
  b.gbp = (float*)ar.take((size_t)B * m->n_cond * 4);  // the prompt half of the conditioning rows (+ bias): prompt-only, kept across steps
  b.prompt_act = ar.take((size_t)B * Tp * Pp * es); b.ctx = ar.take((size_t)B * Tp * Dp * es);
  b.kvsrc = ar.take(B * Lk * Dp * es); b.lat = (float*)ar.take(B * ml * Dp * 4); b.lat_act = ar.take(B * ml * Dp * es);
  b.rq = ar.take(B * ml * hd * es); b.rkv = ar.take(B * Lk * 2 * hd * es); b.rao = ar.take(B * ml * hd * es);
  b.rgg = ar.take(B * ml * ip * es); b.c_act = ar.take(B * ml * Dp * es); b.ckv = ar.take((size_t)c.depth * B * ml * 2 * hd * es);
  b.klen = (int32_t*)ar.take((size_t)B * 4);
  b.xin = ar.take(M * zp * es); b.h0 = ar.take(M * Dp * es);
  b.wv = plan_wave(m->wn, (int)M, es, ar);
  b.xres = (float*)ar.take(M * Dp * 4);
  b.tf = plan_tf(m->tf, (int)M, es, ar);
  b.cq = ar.take(M * hd * es); b.tp = ar.take(M * Dp * es);
  b.rb = (float*)ar.take((size_t)B * c.depth * (4 * hd + 2 * ip) * 4);  // split RMSNorm: beta . W^T of every adaptive norm's consumer, per sample
  b.gbh = es == 4 && c.dtype == DN_F32 ? nullptr : ar.take((size_t)B * m->n_cond * es);
  return b;
}

int attn_call(int dtype, const void* q, int ldq, const void* k, const void* v, int ldkv, void* out, int ldo, int B, int T, int Tk, int heads,
              int dim_head, const int32_t* lengths, hipStream_t s) {
  DnAttnParams a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.out = out;
  a.ldq = ldq; a.ldk = a.ldv = ldkv; a.ldo = ldo;
  a.B = B; a.T = T; a.Tk = Tk; a.heads = heads; a.dim_head = dim_head; a.dtype = dtype; a.lengths = lengths;
  a.scale = 1.0f / sqrtf((float)dim_head);
  return dn_attention(&a, s);
}

}  // namespace

extern "C" size_t dn_eps_cond_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t Tp) {
  if (!m || m->cfg.dim_prompt <= 0 || B <= 0 || T <= 0 || Tp <= 0) return 0;
  Arena ar{nullptr, 0, 0};
  (void)plan_eps_cond(m, B, T, Tp, ar);
  return ar.off + 256;
}

extern "C" int dn_eps_forward_cond(DnEps* m, const float* x, const int32_t* t, const int32_t* lengths, const float* prompt,
                                   const int32_t* prompt_lengths, const int32_t* drop, int32_t B, int32_t T, int32_t Tp, float* eps_out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return dn_eps_forward_cond_ex(m, x, t, lengths, prompt, prompt_lengths, drop, B, T, Tp, eps_out, workspace, workspace_bytes, 0, nullptr, 0, 0, stream);
}

// The time half of the conditioning rows for timesteps t0 .. t0 + n_t - 1 of a chain: table[i] = W_c[:, :C] . time_cond(t0 + i)
// (no bias: it rides on the prompt half).  fp32 [n_t, n_cond].  workspace: n_t * (C + 1) * 4 bytes (+ 256).
extern "C" size_t dn_eps_cond_time_table_workspace_bytes(const DnEps* m, int32_t n_t) {
  if (!m || n_t <= 0) return 0;
  return (size_t)n_t * ((size_t)m->cfg.dim * m->cfg.cond_mult + 1) * 4 + 512;
}
// table[i] for the timesteps times[i] (device int32 [n_t]); cond: n_t * C floats of the workspace
static int cond_time_table_rows(const DnEps* m, const int32_t* times, int n_t, float* table, float* cond, hipStream_t s) {
  const int D = m->cfg.dim, C = D * m->cfg.cond_mult;
  DN_TRY(dn_time_cond(times, n_t, m->w_freq, D / 2, m->tc_W, m->tc_b, C, cond, nullptr, DN_F32, C, s));
  DnGemmParams p = gemm_base(DN_F32, n_t, m->n_cond, C, 1);
  p.terms[0].A = cond; p.terms[0].lda = C; p.terms[0].W = m->cond_W; p.terms[0].ldw = 2 * C;
  p.out = table; p.ldo = m->n_cond; p.out_dtype = DN_F32;
  return dn_conv_gemm(&p, s);
}
extern "C" int dn_eps_cond_time_table(DnEps* m, int32_t t0, int32_t n_t, float* table, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && table && workspace && n_t > 0 && t0 >= 0, "dn_eps_cond_time_table: bad argument");
  DN_CHECK_ARG(m->cfg.dim_prompt > 0, "dn_eps_cond_time_table: the model was created without a prompt branch");
  DN_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && workspace_bytes >= dn_eps_cond_time_table_workspace_bytes(m, n_t) - 256, "dn_eps_cond_time_table: workspace");
  hipStream_t s = (hipStream_t)stream;
  int32_t* times = (int32_t*)workspace;
  float* cond = (float*)((char*)workspace + (((size_t)n_t * 4 + 255) & ~(size_t)255));
  hipLaunchKernelGGL(dn::iota_i32_kernel, dim3((n_t + 255) / 256), dim3(256), 0, s, t0, times, n_t);
  DN_TRY(cond_time_table_rows(m, times, n_t, table, cond, s));
  DN_CHECK_LAUNCH("dn_eps_cond_time_table");
  return DN_OK;
}
// The same table for a device list of timesteps (row i for steps[i]: the schedule of dn_guided_ddim_loop); the workspace of
// dn_eps_cond_time_table_workspace_bytes(m, n_steps)
extern "C" int dn_eps_cond_time_table_steps(DnEps* m, const int32_t* steps, int32_t n_steps, float* table, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  DN_CHECK_ARG(m && steps && table && workspace && n_steps > 0, "dn_eps_cond_time_table_steps: bad argument");
  DN_CHECK_ARG(m->cfg.dim_prompt > 0, "dn_eps_cond_time_table_steps: the model was created without a prompt branch");
  DN_CHECK_ARG(((uintptr_t)workspace & 255) == 0 && workspace_bytes >= dn_eps_cond_time_table_workspace_bytes(m, n_steps) - 256,
               "dn_eps_cond_time_table_steps: workspace");
  float* cond = (float*)((char*)workspace + (((size_t)n_steps * 4 + 255) & ~(size_t)255));
  DN_TRY(cond_time_table_rows(m, steps, n_steps, table, cond, (hipStream_t)stream));
  DN_CHECK_LAUNCH("dn_eps_cond_time_table_steps");
  return DN_OK;
}

extern "C" int dn_eps_forward_cond_ex(DnEps* m, const float* x, const int32_t* t, const int32_t* lengths, const float* prompt,
                                      const int32_t* prompt_lengths, const int32_t* drop, int32_t B, int32_t T, int32_t Tp, float* eps_out,
                                      void* workspace, size_t workspace_bytes, int32_t flags, const float* time_table, int32_t table_t0,
                                      int32_t table_n, void* stream) {
  const bool reuse_prompt = (flags & DN_COND_REUSE_PROMPT) != 0;
  DN_CHECK_ARG(m && x && t && lengths && prompt && prompt_lengths && drop && eps_out && workspace, "dn_eps_forward_cond: null argument");
  DN_CHECK_ARG(!time_table || table_n > 0, "dn_eps_forward_cond: a time table needs its row count");
  DN_CHECK_ARG(m->cfg.dim_prompt > 0, "dn_eps_forward_cond: the model was created without a prompt branch (cfg.dim_prompt == 0)");
  DN_CHECK_ARG(B > 0 && T > 0 && Tp > 0 && T <= m->cfg.max_pos, "dn_eps_forward_cond: B=%d T=%d Tp=%d", B, T, Tp);
  hipStream_t s = (hipStream_t)stream;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  const CondBufs b = plan_eps_cond(m, B, T, Tp, ar);
  DN_TRY(check_workspace("dn_eps_forward_cond", workspace, workspace_bytes, ar.off));
  const DnEpsConfig& c = m->cfg;
  const int dtype = c.dtype, es = esize(dtype), M = B * T;
  const int D = c.dim, Dp = padk(D), Dn = padn(D), z = c.latent, zp = padk(z), C = D * c.cond_mult, P = c.dim_prompt, Pp = padk(P);
  const int hd = c.heads * c.dim_head, ip = padk(m->tf.inner), in_n = padn(m->tf.inner), ml = c.num_latents, Lk = ml + Tp, R = c.resampler_depth;
  // ---- conditioning rows: [time cond | pooled-prompt cond] -> FiLM / adaptive-norm [gamma ; beta] (:841-852), fp32.  The
  // projection is linear in its two halves, so the rows are formed as (time half) + (prompt half + bias): the prompt half and
  // everything else that depends on the prompt only -- the resampler and every layer's cross-attention keys / values -- is computed
  // once and kept in the workspace (DN_COND_REUSE_PROMPT: a later call on the same workspace and shapes skips it), and the time
  // half of a whole chain can come from dn_eps_cond_time_table (the 1.1 GB projection is then never streamed inside the loop).
  if (!time_table) DN_TRY(dn_time_cond(t, B, m->w_freq, D / 2, m->tc_W, m->tc_b, C, b.cond, nullptr, DN_F32, C, s));
  if (!reuse_prompt) {
  hipLaunchKernelGGL(dn::prompt_pool_kernel, dim3(B), dim3(256), 0, s, prompt, prompt_lengths, B, Tp, P, Pp, b.pooled);
  {  // to_prompt_cond: Linear(P -> C) + SiLU (:760-764)
    DnGemmParams p = gemm_base(DN_F32, B, C, Pp, 1);
    p.terms[0].A = b.pooled; p.terms[0].lda = Pp; p.terms[0].W = m->tpc_W;
    p.bias = m->tpc_b; p.epilogue = DN_EPI_SILU; p.out = b.pc; p.ldo = C; p.out_dtype = DN_F32;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  hipLaunchKernelGGL(dn::assemble_cond2_kernel, dim3(ew_grid((int64_t)B * 2 * C)), dim3(256), 0, s, b.pc, b.pc, m->null_pc, drop, B, C, b.cond2);  // (second half: pc or null_pc by drop)
  {  // prompt half + bias
    DnGemmParams p = gemm_base(DN_F32, B, m->n_cond, C, 1);
    p.terms[0].A = b.cond2 + C; p.terms[0].lda = 2 * C; p.terms[0].W = reinterpret_cast<const float*>(m->cond_W) + C; p.terms[0].ldw = 2 * C;
    p.bias = m->cond_b; p.out = b.gbp; p.ldo = m->n_cond; p.out_dtype = DN_F32;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  // ---- PerceiverResampler (:416-471): prompt -> ml latents per sample
  DN_TRY(dn_convert_rows(prompt, DN_F32, P, b.prompt_act, dtype, Pp, B * Tp, P, s));
  {  // proj_context
    DnGemmParams p = gemm_base(dtype, B * Tp, Dp, Pp, Tp);
    p.terms[0].A = b.prompt_act; p.terms[0].lda = Pp; p.terms[0].W = m->proj_W;
    p.bias = m->proj_b; p.out = b.ctx; p.ldo = Dp;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  // keys/values of every resampler layer = [latents ; projected prompt]: the prompt rows are placed once
  hipLaunchKernelGGL(dn::place_rows_kernel, dim3(ew_grid((int64_t)B * Tp * Dp)), dim3(256), 0, s, b.ctx, dtype, (int64_t)Tp * Dp, nullptr, nullptr, b.kvsrc,
                     dtype, B, Tp, Dp, Lk, ml);
  hipLaunchKernelGGL(dn::place_rows_kernel, dim3(ew_grid((int64_t)B * ml * Dp)), dim3(256), 0, s, m->lat_pos, DN_F32, (int64_t)0, nullptr, nullptr, b.lat,
                     DN_F32, B, ml, Dp, ml, 0);
  hipLaunchKernelGGL(dn::add_const_i32_kernel, dim3((B + 255) / 256), dim3(256), 0, s, prompt_lengths, ml, Tp, b.klen, B);  // mask = [ones(ml) ; prompt_mask]
  for (int l = 0; l < R; ++l) {
    DN_TRY(dn_convert_rows(b.lat, DN_F32, Dp, b.lat_act, dtype, Dp, B * ml, Dp, s));
    hipLaunchKernelGGL(dn::place_rows_kernel, dim3(ew_grid((int64_t)B * ml * Dp)), dim3(256), 0, s, b.lat_act, dtype, (int64_t)ml * Dp, nullptr, nullptr,
                       b.kvsrc, dtype, B, ml, Dp, Lk, 0);
    {
      DnGemmParams p = gemm_base(dtype, B * ml, hd, Dp, ml);
      p.terms[0].A = b.lat_act; p.terms[0].lda = Dp; p.terms[0].W = eoff(m->rq_W, (size_t)l * padn(hd) * Dp, es);
      p.out = b.rq; p.ldo = hd; p.out_dtype = side_dtype(dtype);
      DN_TRY(dn_conv_gemm(&p, s));
    }
    {
      DnGemmParams p = gemm_base(dtype, B * Lk, 2 * hd, Dp, Lk);
      p.terms[0].A = b.kvsrc; p.terms[0].lda = Dp; p.terms[0].W = eoff(m->rkv_W, (size_t)l * padn(2 * hd) * Dp, es);
      p.out = b.rkv; p.ldo = 2 * hd; p.out_dtype = side_dtype(dtype);
      DN_TRY(dn_conv_gemm(&p, s));
    }
    DN_TRY(attn_call(dtype, b.rq, hd, b.rkv, eoff(b.rkv, hd, es), 2 * hd, b.rao, hd, B, ml, Lk, c.heads, c.dim_head, b.klen, s));
    {
      DnGemmParams p = gemm_base(dtype, B * ml, Dp, hd, ml);
      p.terms[0].A = b.rao; p.terms[0].lda = hd; p.terms[0].W = eoff(m->rout_W, (size_t)l * Dn * hd, es);
      p.epilogue = DN_EPI_RESADD; p.res = b.lat; p.ldr = Dp; p.out = b.lat; p.ldo = Dp; p.out_dtype = DN_F32;
      DN_TRY(dn_conv_gemm(&p, s));
    }
    DN_TRY(dn_convert_rows(b.lat, DN_F32, Dp, b.lat_act, dtype, Dp, B * ml, Dp, s));
    {  // FeedForward without the causal conv: Linear -> GEGLU -> Linear (:887-903)
      DnGemmParams p = gemm_base(dtype, B * ml, ip, Dp, ml);
      p.terms[0].A = b.lat_act; p.terms[0].lda = Dp; p.terms[0].W = eoff(m->rffin_W, (size_t)l * 2 * ip * Dp, es);
      p.bias = m->rffin_b + (size_t)l * 2 * ip; p.epilogue = DN_EPI_GEGLU; p.out = b.rgg; p.ldo = ip;
      DN_TRY(dn_conv_gemm(&p, s));
    }
    {
      DnGemmParams p = gemm_base(dtype, B * ml, Dp, ip, ml);
      p.terms[0].A = b.rgg; p.terms[0].lda = ip; p.terms[0].W = eoff(m->rffout_W, (size_t)l * Dn * ip, es);
      p.bias = m->rffout_b + (size_t)l * Dp;
      p.epilogue = DN_EPI_RESADD; p.res = b.lat; p.ldr = Dp; p.out = b.lat; p.ldo = Dp; p.out_dtype = DN_F32;
      DN_TRY(dn_conv_gemm(&p, s));
    }
  }
  DN_TRY(dn_rmsnorm(b.lat, Dp, b.lat_act, Dp, dtype, B * ml, D, ml, m->rnorm_g, nullptr, 0, 0, s));
  // c = where(drop, null_prompt_tokens, resampled) (:855-859)
  hipLaunchKernelGGL(dn::place_rows_kernel, dim3(ew_grid((int64_t)B * ml * Dp)), dim3(256), 0, s, b.lat_act, dtype, (int64_t)ml * Dp, m->null_tok, drop, b.c_act,
                     dtype, B, ml, Dp, ml, 0);
  {  // keys / values of all cross-attention layers at once (they depend on the prompt only)
    DnGemmParams p = gemm_base(dtype, B * ml, 2 * hd, Dp, ml);
    p.groups = c.depth;
    p.terms[0].A = b.c_act; p.terms[0].lda = Dp; p.terms[0].a_gstride = 0;
    p.terms[0].W = m->ckv_W; p.terms[0].w_gstride = (int64_t)padn(2 * hd) * Dp;
    p.out = b.ckv; p.ldo = 2 * hd; p.out_gstride = (int64_t)B * ml * 2 * hd; p.out_dtype = side_dtype(dtype);
    DN_TRY(dn_conv_gemm(&p, s));
  }
  }  // !reuse_prompt
  // ---- the step's conditioning rows: time half (from the chain's table, or contracted here) + prompt half
  if (time_table) {
    hipLaunchKernelGGL(dn::cond_rows_from_table_kernel, dim3(ew_grid((int64_t)B * m->n_cond / 4)), dim3(256), 0, s, time_table, t, table_t0, table_n, b.gbp, B,
                       m->n_cond, b.gb);
  } else {
    DnGemmParams p = gemm_base(DN_F32, B, m->n_cond, C, 1);
    p.terms[0].A = b.cond; p.terms[0].lda = C; p.terms[0].W = m->cond_W; p.terms[0].ldw = 2 * C;
    p.epilogue = DN_EPI_RESADD; p.res = b.gbp; p.ldr = m->n_cond; p.out = b.gb; p.ldo = m->n_cond; p.out_dtype = DN_F32;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  const bool split = split_norm_enabled(Dp, dtype), xn_ready = split || fuse_norm_enabled(Dp, dtype);
  const int rb_ld = c.depth * (4 * hd + 2 * ip);
  if (split) DN_TRY(eps_beta_rows(m, b.gb, m->n_cond, B, b.gbh, b.rb, rb_ld, s));
  // ---- the eps-predictor proper (:861-876)
  DN_TRY(dn_convert_rows(x, DN_F32, z, b.xin, dtype, zp, M, z, s));
  {
    DnGemmParams p = gemm_base(dtype, M, Dp, zp, T);
    p.terms[0].A = b.xin; p.terms[0].lda = zp; p.terms[0].W = m->init_W;
    p.bias = m->init_b; p.out = b.h0; p.ldo = Dp;
    DN_TRY(dn_conv_gemm(&p, s));
  }
  {
    DnGemmParams fin = gemm_base(dtype, M, Dp, Dp, T);
    fin.epilogue = DN_EPI_POSEMB; fin.pos_table = m->pos_table; fin.pos_ld = Dp; fin.lengths = lengths;
    fin.out = b.xres; fin.ldo = Dp; fin.out_dtype = DN_F32;
    const float* gb0 = b.gb + (size_t)c.wn_stacks * c.wn_layers * 2 * Dp;  // layer 0's attention norm rides on it
    if (fuse_norm_enabled(Dp, dtype)) set_norm(fin, b.tf.xn, Dp, D, dtype, nullptr, gb0, m->n_cond);
    else if (split) set_split_norm(fin, b.tf, Dp, D, dtype, nullptr, gb0, m->n_cond);
    DN_TRY(run_wavenet(m->wn, dtype, b.h0, M, T, b.gb, m->n_cond, b.wv, fin, s));
  }
  // the transformer of the unconditional model with the cross-attention block between attention and feed-forward: every RMSNorm
  // split between the contraction that produces its input and the one that consumes it, K-blocked operands where a tile gains
  const float* gb_tf = b.gb + (size_t)c.wn_stacks * c.wn_layers * 2 * Dp;
  const CrossAttn cx = {m->cq_W, m->cout_W, b.ckv, ml, b.cq};
  DN_TRY(run_transformer(m->tf, dtype, b.xres, B, T, lengths, gb_tf, m->n_cond, split ? b.rb : nullptr, rb_ld, b.tf, b.tp, Dp, dtype, xn_ready, s, &cx));
  DnGemmParams p = gemm_base(dtype, M, z, Dp, T);
  p.terms[0].A = b.tp; p.terms[0].lda = Dp; p.terms[0].W = m->final_W;
  p.bias = m->final_b; p.out = eps_out; p.ldo = z; p.out_dtype = DN_F32;
  DN_TRY(dn_conv_gemm(&p, s));
  DN_CHECK_LAUNCH("dn_eps_forward_cond");
  return DN_OK;
}

// ------------------------------------------------------------------------------------------ guided chain over a timestep schedule
namespace {
// drop mask of the guided pass over n rows = [conditioned (first B) ; null]
__global__ void drop_mask_kernel(int32_t* drop, int n, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) drop[i] = i >= B ? 1 : 0;
}

// The workspace of a guided loop behind the model pass's own (`core` bytes at its start).  State whose size does not depend
// on n_steps first; the second halves exist for the guided (2B-row) pass only -- at cond_scale == 1 the model reads x itself and
// the caller's lengths / prompt / prompt lengths.  `history` (dn_guided_dpm_loop): one more B-row latent beside the prediction, the
// previous step's data prediction; without it and with DN_DDIM_SCHED_COLS columns the layout is dn_guided_ddim_loop's, byte for byte.
struct GuidedBufs {
  size_t core;
  float *both, *hist, *xin, *prompt2, *table, *coef;
  int32_t *tvec, *counter, *drop, *len2, *plen2, *steps;
  void* tt_ws;
  size_t tt_bytes;
};

GuidedBufs plan_guided(const DnEps* m, int B, int T, int Tp, int n_steps, bool guided, bool history, int coef_cols, Arena& ar) {
  const size_t n = guided ? 2 * (size_t)B : (size_t)B, Mz = (size_t)B * T * m->cfg.latent;
  GuidedBufs g;
  memset(&g, 0, sizeof(g));
  Arena core{nullptr, 0, 0};
  (void)plan_eps_cond(m, (int)n, T, Tp, core);
  g.core = (core.off + 255) & ~(size_t)255;
  (void)ar.take(g.core);
  g.both = (float*)ar.take(n * T * m->cfg.latent * 4);
  if (history) g.hist = (float*)ar.take(Mz * 4);
  g.tvec = (int32_t*)ar.take(n * 4);
  g.counter = (int32_t*)ar.take(64);
  g.drop = (int32_t*)ar.take(n * 4);
  if (guided) {
    g.xin = (float*)ar.take(2 * Mz * 4);
    g.len2 = (int32_t*)ar.take(n * 4);
    g.plen2 = (int32_t*)ar.take(n * 4);
    g.prompt2 = (float*)ar.take(n * Tp * m->cfg.dim_prompt * 4);
  }
  g.steps = (int32_t*)ar.take((size_t)n_steps * 4);
  g.table = (float*)ar.take((size_t)n_steps * m->n_cond * 4);  // row i: the time half of the conditioning rows of steps[i]
  g.coef = (float*)ar.take((size_t)n_steps * coef_cols * 4);
  g.tt_bytes = dn_eps_cond_time_table_workspace_bytes(m, n_steps);  // (dead once the table is built)
  g.tt_ws = ar.take(g.tt_bytes);
  return g;
}

size_t guided_ws_bytes(const DnEps* m, int32_t B, int32_t T, int32_t Tp, int32_t n_steps, int32_t guided, bool history, int coef_cols) {
  if (!m || m->cfg.dim_prompt <= 0 || B <= 0 || T <= 0 || Tp <= 0 || n_steps < 1) return 0;
  Arena ar{nullptr, 0, 0};
  (void)plan_guided(m, B, T, Tp, n_steps, guided != 0, history, coef_cols, ar);
  return ar.off + 256;
}

// One guided device loop: what guided_loop needs to know beyond its arguments.
struct GuidedDesc {
  const char *name, *ws_name, *uncond_name;  // for messages; uncond_name: the entry an unconditional model is sent to
  int coef_cols;
  bool history;  // GuidedBufs::hist
  StepKey kind;  // eta, dpm, seed, keys, injected: the loop's part of the graph key
  // the fused combination + update + refill of the model's input after a pass (n_elem = B T latent)
  std::function<int(const GuidedBufs&, float* x, float* xin, int64_t n_elem, int guided, float scale, hipStream_t stream)> update;
};
}  // namespace

// The body of the two guided loops: the argument checks, the chain-start copies, the drop mask, the time table, the step, the graph key
// and the replays.  The entries differ in the workspace plan (d.history, d.coef_cols), the update (d.update) and the key (d.kind).
static int guided_loop(DnEps* m, float* x, const int32_t* lengths, const float* prompt, const int32_t* prompt_lengths, int32_t B, int32_t T,
                       int32_t Tp, float cond_scale, const int32_t* steps, const float* coef, int32_t n_steps, int32_t timesteps, int32_t flags,
                       void* workspace, size_t workspace_bytes, void* stream, const GuidedDesc& d) {
  DN_CHECK_ARG(m && x && lengths && prompt && prompt_lengths && steps && coef && workspace, "%s: null argument", d.name);
  DN_CHECK_ARG(m->cfg.dim_prompt > 0, "%s: the model was created without a prompt branch (cfg.dim_prompt == 0): use %s", d.name, d.uncond_name);
  DN_CHECK_ARG(!(flags & DN_LOOP_SPLIT2), "%s: DN_LOOP_SPLIT2 is not offered (the prompt-only state lives in one workspace, and the "
               "guided pass already runs 2B rows)", d.name);
  DN_CHECK_ARG(!(flags & ~DN_LOOP_GRAPH), "%s: flags=%d (DN_LOOP_GRAPH only)", d.name, flags);
  DN_CHECK_ARG(n_steps >= 1 && n_steps <= timesteps, "%s: n_steps=%d must be in [1, %d]", d.name, n_steps, timesteps);
  DN_CHECK_ARG(B > 0 && T > 0 && Tp > 0 && T <= m->cfg.max_pos, "%s: B=%d T=%d Tp=%d (positional table: %d)", d.name, B, T, Tp, m->cfg.max_pos);
  DN_CHECK_ARG(cond_scale == cond_scale, "%s: cond_scale is not a number", d.name);
  DN_CHECK_ARG(d.kind.eta || !d.kind.injected, "%s: injected noise needs eta_on (eta = 0 draws none)", d.name);
  DN_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", d.name);
  const bool guided = cond_scale != 1.0f;
  const size_t need = guided_ws_bytes(m, B, T, Tp, n_steps, guided, d.history, d.coef_cols);
  if (need > workspace_bytes) {
    dn_set_error("%s: workspace %zu < required %zu (see %s)", d.name, workspace_bytes, need, d.ws_name);
    return DN_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  const GuidedBufs g = plan_guided(m, B, T, Tp, n_steps, guided, d.history, d.coef_cols, ar);
  const int n = guided ? 2 * B : B, z = m->cfg.latent;
  const size_t Mz = (size_t)B * T * z;
  // ---- chain start: the static inputs of the 2B-row pass, the model's first input, the schedule, its coefficient rows and its
  // time table, all in the workspace (a captured step holds workspace addresses and x only)
  auto copy = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess; };
  bool ok = copy(g.steps, steps, (size_t)n_steps * 4) && copy(g.coef, coef, (size_t)n_steps * d.coef_cols * 4);
  if (guided) {
    const size_t pb = (size_t)B * Tp * m->cfg.dim_prompt * 4;
    ok = ok && copy(g.len2, lengths, (size_t)B * 4) && copy(g.len2 + B, lengths, (size_t)B * 4) && copy(g.plen2, prompt_lengths, (size_t)B * 4) &&
         copy(g.plen2 + B, prompt_lengths, (size_t)B * 4) && copy(g.prompt2, prompt, pb) && copy((char*)g.prompt2 + pb, prompt, pb) &&
         copy(g.xin, x, Mz * 4) && copy(g.xin + Mz, x, Mz * 4);
  }
  if (!ok) {
    dn_set_error("%s: copying the chain's inputs into the workspace failed", d.name);
    return DN_ELAUNCH;
  }
  hipLaunchKernelGGL(drop_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, s, g.drop, n, B);
  hipLaunchKernelGGL(set_counter_kernel, dim3(1), dim3(1), 0, s, g.counter, 0);
  DN_TRY(dn_eps_cond_time_table_steps(m, g.steps, n_steps, g.table, g.tt_ws, g.tt_bytes, s));
  float* xin = guided ? g.xin : x;
  const int32_t *len = guided ? g.len2 : lengths, *plen = guided ? g.plen2 : prompt_lengths;
  const float* prm = guided ? g.prompt2 : prompt;
  // one step: the step-index vector (with a time table the pass uses `t` only to pick the table's row), the pass over n rows, the
  // fused combination + update + refill of the model's input, the counter.  `reuse`: every step but the chain's first
  auto one_step = [&](bool reuse) -> int {
    hipLaunchKernelGGL(fill_t_kernel, dim3((n + 255) / 256), dim3(256), 0, s, g.tvec, n, g.counter);
    DN_TRY(dn_eps_forward_cond_ex(m, xin, g.tvec, len, prm, plen, g.drop, n, T, Tp, g.both, workspace, g.core, reuse ? DN_COND_REUSE_PROMPT : 0,
                                  g.table, 0, n_steps, s));
    DN_TRY(d.update(g, x, xin, (int64_t)Mz, guided, cond_scale, s));
    hipLaunchKernelGGL(inc_counter_kernel, dim3(1), dim3(1), 0, s, g.counter);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      dn_set_error("%s step: %s", d.name, hipGetErrorString(e));
      return DN_ELAUNCH;
    }
    return DN_OK;
  };
  DN_TRY(one_step(false));  // eager: the prompt-only work, and the per-kernel attributes settle outside capture
  if ((flags & DN_LOOP_GRAPH) && s && n_steps > 2) {  // (the null stream cannot be captured)
    // (an injected-noise chain is never served from the cache; a dn_set_option since the capture may route the contractions differently)
    StepKey key = d.kind;
    key.ws = workspace; key.x = x; key.len = lengths; key.coef = g.coef; key.prompt = prompt; key.plen = prompt_lengths;
    key.B = B; key.T = T; key.Tp = Tp; key.n_steps = n_steps; key.flags = flags; key.opt_gen = dn::option_generation();
    memcpy(&key.scale_bits, &cond_scale, 4);
    DN_TRY(replay_steps(m->guided_graph, key, false, n_steps - 1, s, d.name, [&] { return one_step(true); }));
  } else {
    for (int done = 1; done < n_steps; ++done) DN_TRY(one_step(true));
  }
  return n_steps;
}

extern "C" size_t dn_guided_ddim_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t Tp, int32_t n_steps, int32_t guided) {
  return guided_ws_bytes(m, B, T, Tp, n_steps, guided, false, DN_DDIM_SCHED_COLS);
}

// dn_guided_ddim_loop (keys == NULL) and dn_guided_ddim_loop_keyed (eta on)
static int guided_ddim_loop(const char* who, DnEps* m, float* x, const int32_t* lengths, const float* prompt, const int32_t* prompt_lengths,
                            int32_t B, int32_t T, int32_t Tp, float cond_scale, const int32_t* steps, const float* coef, int32_t n_steps,
                            int32_t timesteps, int32_t eta_on, uint64_t seed, const float* noise, const uint64_t* keys, int32_t flags,
                            void* workspace, size_t workspace_bytes, void* stream) {
  eta_on = eta_on != 0;
  if (!eta_on) seed = 0;
  GuidedDesc d = {who, "dn_guided_ddim_workspace_bytes", "dn_ddim_sched_loop", DN_DDIM_SCHED_COLS, false, step_kind(seed, noise, keys), nullptr};
  d.kind.eta = (uint16_t)eta_on;
  d.update = [=](const GuidedBufs& g, float* xb, float* xin, int64_t n_elem, int guided, float scale, hipStream_t st) {
    SchedStep u = {SCHED_DDIM, xb, 0, n_elem, g.both, guided, scale, xin};
    u.coef = g.coef; u.steps = g.steps; u.counter = g.counter; u.eta_on = eta_on;
    u.src = sched_noise(noise, n_elem, seed, keys, n_elem / B / 4);
    return sched_step_launch("dn_guided_ddim_loop", u, st);
  };
  return guided_loop(m, x, lengths, prompt, prompt_lengths, B, T, Tp, cond_scale, steps, coef, n_steps, timesteps, flags, workspace,
                     workspace_bytes, stream, d);
}

extern "C" int dn_guided_ddim_loop(DnEps* m, float* x, const int32_t* lengths, const float* prompt, const int32_t* prompt_lengths, int32_t B,
                                   int32_t T, int32_t Tp, float cond_scale, const int32_t* steps, const float* coef, int32_t n_steps,
                                   int32_t timesteps, int32_t eta_on, uint64_t seed, const float* noise, int32_t flags, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return guided_ddim_loop("dn_guided_ddim_loop", m, x, lengths, prompt, prompt_lengths, B, T, Tp, cond_scale, steps, coef, n_steps, timesteps,
                          eta_on, seed, noise, nullptr, flags, workspace, workspace_bytes, stream);
}

extern "C" int dn_guided_ddim_loop_keyed(DnEps* m, float* x, const int32_t* lengths, const float* prompt, const int32_t* prompt_lengths,
                                         int32_t B, int32_t T, int32_t Tp, float cond_scale, const int32_t* steps, const float* coef,
                                         int32_t n_steps, int32_t timesteps, const uint64_t* keys, int32_t flags, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  DN_TRY(check_keys("dn_guided_ddim_loop_keyed", m, keys));
  return guided_ddim_loop("dn_guided_ddim_loop_keyed", m, x, lengths, prompt, prompt_lengths, B, T, Tp, cond_scale, steps, coef, n_steps,
                          timesteps, 1, 0, nullptr, keys, flags, workspace, workspace_bytes, stream);
}

// DPM-Solver++(2M) (Lu et al. 2022, "DPM-Solver++", the data-prediction multistep solver, eq. 11-12 / algorithm 2) on the guided
// prediction of forward_with_cond_scale (reference latent_module.py:813-826, which the fused step replaces together with the update):
// dn_guided_ddim_loop's body with dn_dpm_loop's rows, one more B-row latent (the previous step's data prediction) and a key bit of
// its own in the guided slot of the graph cache.
extern "C" size_t dn_guided_dpm_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t Tp, int32_t n_steps, int32_t guided) {
  return guided_ws_bytes(m, B, T, Tp, n_steps, guided, true, DN_DPM_COLS);
}

extern "C" int dn_guided_dpm_loop(DnEps* m, float* x, const int32_t* lengths, const float* prompt, const int32_t* prompt_lengths, int32_t B,
                                  int32_t T, int32_t Tp, float cond_scale, const int32_t* steps, const float* coef, int32_t n_steps,
                                  int32_t timesteps, int32_t flags, void* workspace, size_t workspace_bytes, void* stream) {
  GuidedDesc d = {"dn_guided_dpm_loop", "dn_guided_dpm_workspace_bytes", "dn_dpm_loop", DN_DPM_COLS, true, step_kind(0, nullptr), nullptr};
  d.kind.dpm = 1;
  d.update = [](const GuidedBufs& g, float* xb, float* xin, int64_t n_elem, int guided, float scale, hipStream_t st) {
    SchedStep u = {SCHED_DPM2M, xb, 0, n_elem, g.both, guided, scale, xin};
    u.coef = g.coef; u.counter = g.counter; u.hist = g.hist;
    return sched_step_launch("dn_guided_dpm_loop", u, st);
  };
  return guided_loop(m, x, lengths, prompt, prompt_lengths, B, T, Tp, cond_scale, steps, coef, n_steps, timesteps, flags, workspace,
                     workspace_bytes, stream, d);
}

// =========================================================================================== VAE
extern "C" int dn_vae_create(const DnVaeConfig* cfg, const void* const* weights, int32_t n_weights, DnVae** out) {
  DN_CHECK_ARG(cfg && weights && out, "dn_vae_create: null argument");
  DN_CHECK_ARG(cfg->n_mults >= 1 && cfg->n_mults <= 4, "dn_vae_create: n_mults=%d", cfg->n_mults);
  const int expect = 2 * cfg->n_mults * kWavenetTensors + kTransformerTensors + 2;
  DN_CHECK_ARG(n_weights == expect, "dn_vae_create: expected %d packed tensors, got %d", expect, n_weights);
  DN_TRY(check_dims("dn_vae_create", cfg->dtype, cfg->dim, cfg->heads, cfg->dim_head, cfg->layers));
  DN_CHECK_ARG(cfg->vocab % 4 == 0 && cfg->z % 4 == 0, "dn_vae_create: vocab and z must be multiples of 4");
  for (int i = 0; i < n_weights; ++i) DN_CHECK_ARG(weights[i] != nullptr, "dn_vae_create: packed tensor %d is null", i);
  DnVae* m = new (std::nothrow) DnVae();
  DN_CHECK_ARG(m != nullptr, "dn_vae_create: out of host memory");
  memset(m, 0, sizeof(*m));
  m->cfg = *cfg;
  m->n_wave = cfg->n_mults;
  const void* const* t = weights;
  int cur = cfg->dim;
  for (int n = 0; n < m->n_wave; ++n) {  // latent_module.py:1053-1065
    WavenetW& w = m->enc[n];
    w.cin = cur; w.cout = cur / cfg->mults[n]; w.stacks = cfg->stacks; w.layers = cfg->layers;
    cur = w.cout;
    t = take_wavenet(w, t);
  }
  DN_CHECK_ARG(cur == 2 * cfg->z, "dn_vae_create: encoder width %d != 2*z (%d)", cur, 2 * cfg->z);
  for (int n = 0; n < m->n_wave; ++n) {  // :1067-1081 (first decoder input halved by the posterior sample)
    WavenetW& w = m->dec[n];
    const int mult = cfg->mults[m->n_wave - 1 - n];
    w.cout = cur * mult; w.cin = n == 0 ? cur / 2 : cur; w.stacks = cfg->stacks; w.layers = cfg->layers;
    cur = w.cout;
    t = take_wavenet(w, t);
  }
  DN_CHECK_ARG(cur == cfg->dim, "dn_vae_create: decoder width %d != dim %d", cur, cfg->dim);
  m->tf.dim = cfg->dim; m->tf.depth = cfg->depth; m->tf.heads = cfg->heads; m->tf.dim_head = cfg->dim_head;
  m->tf.inner = (int)((double)cfg->dim * 4 * 2 / 3);
  t = take_transformer(m->tf, t);
  m->lm_W = t[0]; m->lm_b = (const float*)t[1];
  *out = m;
  return DN_OK;
}

extern "C" void dn_vae_destroy(DnVae* m) { delete m; }

// see include/diffnorm_hip.h
extern "C" int dn_vae_set_ffn_fold(DnVae* m, const void* fold_W, const float* fold_b) {
  DN_CHECK_ARG(m && (fold_W != nullptr) == (fold_b != nullptr), "dn_vae_set_ffn_fold: null engine, or one of the two buffers without the other");
  DN_CHECK_ARG(((uintptr_t)fold_W & 127) == 0 && ((uintptr_t)fold_b & 15) == 0, "dn_vae_set_ffn_fold: fold_W 128-byte, fold_b 16-byte aligned");
  m->tf.fold_W = fold_W; m->tf.fold_b = fold_b; m->tf.fold_Wkb = nullptr;
  m->tf.fold_default = m->cfg.dtype == DN_BF16 ? FOLD_OFF : FOLD_ROUTED;
  return DN_OK;
}

extern "C" int dn_vae_set_ffn_fold_kblocked(DnVae* m, const void* fold_Wkb) {
  DN_CHECK_ARG(m && (!fold_Wkb || (m->tf.fold_W && dn::dn_is16(m->cfg.dtype))) && ((uintptr_t)fold_Wkb & 127) == 0,
               "dn_vae_set_ffn_fold_kblocked: null engine, no folded weights attached, not a 2-byte arithmetic, or fold_Wkb not 128-byte aligned");
  m->tf.fold_Wkb = fold_Wkb;
  return DN_OK;
}

namespace {
struct VaeBufs {
  void *in_act, *mid[2];
  WaveBufs wv[4];
  float *xres, *recon, *logits;
  void* pred_act;
  TfBufs tf;
};

VaeBufs plan_vae_enc(const DnVae* m, int M, Arena& ar) {
  const int es = esize(m->cfg.dtype);
  VaeBufs b;
  memset(&b, 0, sizeof(b));
  b.in_act = ar.take((size_t)M * padk(m->cfg.dim) * es);
  int widest = 0;
  for (int n = 0; n < m->n_wave; ++n) widest = widest > m->enc[n].cout ? widest : m->enc[n].cout;
  b.mid[0] = ar.take((size_t)M * padk(widest) * es);
  b.mid[1] = ar.take((size_t)M * padk(widest) * es);
  for (int n = 0; n < m->n_wave; ++n) b.wv[n] = plan_wave(m->enc[n], M, es, ar);
  return b;
}

VaeBufs plan_vae_dec(const DnVae* m, int M, bool need_recon, bool need_logits, Arena& ar) {
  const int es = esize(m->cfg.dtype), Dp = padk(m->cfg.dim);
  VaeBufs b;
  memset(&b, 0, sizeof(b));
  b.in_act = ar.take((size_t)M * padk(m->cfg.z) * es);
  b.mid[0] = ar.take((size_t)M * Dp * es);
  b.mid[1] = ar.take((size_t)M * Dp * es);
  for (int n = 0; n < m->n_wave; ++n) b.wv[n] = plan_wave(m->dec[n], M, es, ar);
  b.xres = (float*)ar.take((size_t)M * Dp * 4);
  b.tf = plan_tf(m->tf, M, es, ar);
  b.recon = need_recon ? (float*)ar.take((size_t)M * Dp * 4) : nullptr;
  b.pred_act = ar.take((size_t)M * Dp * es);
  b.logits = need_logits ? (float*)ar.take((size_t)M * m->cfg.vocab * 4) : nullptr;
  return b;
}
}  // namespace

extern "C" size_t dn_vae_workspace_bytes(const DnVae* m, int32_t B, int32_t T) {
  if (!m || B <= 0 || T <= 0) return 0;
  Arena a{nullptr, 0, 0}, d{nullptr, 0, 0};
  (void)plan_vae_enc(m, B * T, a);
  (void)plan_vae_dec(m, B * T, true, true, d);
  return (a.off > d.off ? a.off : d.off) + 256;
}

extern "C" int dn_vae_encode_params(DnVae* m, const float* feat, int32_t B, int32_t T, float* params, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && feat && params && workspace && B > 0 && T > 0, "dn_vae_encode_params: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int dtype = m->cfg.dtype, M = B * T;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  VaeBufs b = plan_vae_enc(m, M, ar);
  DN_TRY(check_workspace("dn_vae_encode_params", workspace, workspace_bytes, ar.off));
  DN_TRY(dn_convert_rows(feat, DN_F32, m->cfg.dim, b.in_act, dtype, padk(m->cfg.dim), M, m->cfg.dim, s));
  const void* cur = b.in_act;
  for (int n = 0; n < m->n_wave; ++n) {
    const WavenetW& w = m->enc[n];
    const bool lastw = n == m->n_wave - 1;
    DnGemmParams fin = gemm_base(dtype, M, lastw ? w.cout : padk(w.cout), padk(w.cout), T);
    if (lastw) {  // posterior parameters [mean ; logvar], dense fp32
      fin.out = params; fin.ldo = w.cout; fin.out_dtype = DN_F32;
    } else {
      fin.out = b.mid[n & 1]; fin.ldo = padk(w.cout); fin.out_dtype = dtype;
    }
    DN_TRY(run_wavenet(w, dtype, cur, M, T, nullptr, 0, b.wv[n], fin, s));
    cur = b.mid[n & 1];
  }
  return DN_OK;
}

extern "C" int dn_vae_decode(DnVae* m, const float* latent, const int32_t* lengths, int32_t B, int32_t T, float* recon, float* logits,
                             int32_t* units, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && latent && lengths && workspace && B > 0 && T > 0, "dn_vae_decode: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int dtype = m->cfg.dtype, M = B * T, D = m->cfg.dim, Dp = padk(D), z = m->cfg.z, V = m->cfg.vocab;
  const bool want_lm = logits != nullptr || units != nullptr;
  const bool dense_recon = recon != nullptr && Dp == D;  // to_pred can write the caller's buffer directly
  Arena ar{(char*)workspace, 0, workspace_bytes};
  VaeBufs b = plan_vae_dec(m, M, !dense_recon, want_lm && !logits, ar);
  DN_TRY(check_workspace("dn_vae_decode", workspace, workspace_bytes, ar.off));
  DN_TRY(dn_convert_rows(latent, DN_F32, z, b.in_act, dtype, padk(z), M, z, s));
  const void* cur = b.in_act;
  for (int n = 0; n < m->n_wave; ++n) {
    const WavenetW& w = m->dec[n];
    const bool lastw = n == m->n_wave - 1;
    DnGemmParams fin = gemm_base(dtype, M, padk(w.cout), padk(w.cout), T);
    if (lastw) {  // opens the transformer's fp32 residual stream (no positional embedding, :1109-1114)
      fin.out = b.xres; fin.ldo = Dp; fin.out_dtype = DN_F32;
    } else {
      fin.out = b.mid[n & 1]; fin.ldo = padk(w.cout); fin.out_dtype = dtype;
    }
    DN_TRY(run_wavenet(w, dtype, cur, M, T, nullptr, 0, b.wv[n], fin, s));
    cur = b.mid[n & 1];
  }
  float* rec = dense_recon ? recon : b.recon;
  const int rec_ld = dense_recon ? D : Dp;
  DN_TRY(run_transformer(m->tf, dtype, b.xres, B, T, lengths, nullptr, 0, nullptr, 0, b.tf, rec, rec_ld, DN_F32, false, s));
  if (recon && !dense_recon) DN_TRY(dn_convert_rows(rec, DN_F32, Dp, recon, DN_F32, D, M, D, s));
  if (!want_lm) return DN_OK;
  DN_TRY(dn_convert_rows(rec, DN_F32, rec_ld, b.pred_act, dtype, Dp, M, D, s));
  float* lg = logits ? logits : b.logits;
  DnGemmParams p = gemm_base(dtype, M, V, Dp, T);  // decoder_lm (:1096,1115)
  p.terms[0].A = b.pred_act; p.terms[0].lda = Dp; p.terms[0].W = m->lm_W;
  p.bias = m->lm_b; p.out = lg; p.ldo = V; p.out_dtype = DN_F32;
  DN_TRY(dn_conv_gemm(&p, s));
  if (units) DN_TRY(dn_argmax_units(lg, V, M, V, 4, units, s));
  return DN_OK;
}
