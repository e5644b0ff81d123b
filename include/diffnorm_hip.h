/*
 * diffnorm_hip.h -- C ABI of libdiffnorm_hip.so: the MI355X (gfx950) implementation of DiffNorm's
 * latent-diffusion denoising hot path.
 *
 * The reference (steventan0110/DiffNorm) has no FFI on this path: its boundary is the fairseq Python
 * plugin API and everything below it is stock ATen.  The entry points here are what a binding for the
 * path would attach to; each cites the reference function it replaces (paths relative to
 * fairseq/models/text_to_speech/ in the reference).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, enums; no torch types.
 *   - every function returns 0 on success or a negative DN_E* code; dn_last_error() gives the text.
 *   - functions taking a `stream` only enqueue work on it (hipStream_t passed as void*); they never
 *     allocate device memory and never synchronise, so they are capturable into a hipGraph.
 *   - activations are channels-last row-major: row m = b*T + t, `ld` elements between rows.
 *   - `dtype` selects the arithmetic of the contractions: DN_BF16 = bf16 MFMA operands with fp32
 *     accumulation (activations that feed a contraction are stored bf16, the transformer residual
 *     stream stays fp32); DN_F32 = exact fp32 MFMA (v_mfma_f32_16x16x4_f32) end to end;
 *     DN_BF16X3 = split-operand bf16: every contraction operand is stored as a bf16 pair (hi, lo) with x ~ hi + lo
 *     (hi = bf16(x), lo = bf16(x - hi): 16 mantissa bits) and a product runs as three bf16 MFMAs into one fp32
 *     accumulator, a_hi b_hi + a_lo b_hi + a_hi b_lo (the dropped a_lo b_lo term is 2^-18 relative), i.e. fp32-class
 *     results (1e-3 budget of north_star's fp32 column) at a third of the bf16 MFMA rate instead of a sixteenth.
 *     Everything that is not a contraction operand is fp32 exactly as in DN_F32 mode.  Inference / sampling engines and the VAE
 *     training engine (dn_vae_train_*: work = the split image of master, made by dn_vae_train_refresh); the diffusion training
 *     engine runs DN_F32 / DN_BF16.
 *     DN_F16 = IEEE-half MFMA operands (v_mfma_f32_16x16x32_f16: the bf16 issue rate on gfx950) with fp32 accumulation --
 *     DN_BF16 with three more significand bits: the same 2-byte layouts, tiles and schedules, every tensor DN_BF16 stores as
 *     bf16 is stored as half, everything DN_BF16 keeps fp32 stays fp32.  The format ends at 65504: a value beyond it saturates
 *     (the kernels run with the MODE register's FP16_OVFL bit set) instead of becoming inf.  Inference engines only.
 *   - DN_BF16X3 storage ("split rows"): an element takes 4 bytes like fp32 and ld / K / column offsets count elements, but
 *     every group of 32 consecutive elements of a row is laid out as two 64-byte halves of 32 bf16 each: ACTIVATIONS
 *     (everything a kernel of this library writes, and every A operand) store [hi | lo], packed WEIGHTS (W operands)
 *     store [lo | hi].  A K-tile of 128 bytes per row then reads as two bf16 k-steps, and a kernel that walks a row in
 *     64-byte K-tiles meets (w_lo, a_hi) then (w_hi, a_lo): it keeps only a_hi across the pair for its three products.
 *     Row strides, K and column offsets of such tensors are multiples of 32 elements; bases are 128-byte aligned.
 */
#ifndef DIFFNORM_HIP_H
#define DIFFNORM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { DN_F32 = 0, DN_BF16 = 1, DN_BF16X3 = 2, DN_F16 = 3 };

enum {
  DN_OK = 0,
  DN_EINVAL = -1,   /* bad argument (shape/alignment/enum) */
  DN_ELAUNCH = -2,  /* HIP launch or runtime error */
  DN_EWORKSPACE = -3 /* workspace too small */
};

/* epilogues of dn_conv_gemm */
enum {
  DN_EPI_BIAS = 0,      /* out = acc + bias                                               (nn.Linear / CausalConv1d) */
  DN_EPI_SILU = 1,      /* out = silu(acc + bias)                                          latent_module.py:741-745 */
  DN_EPI_GEGLU = 2,     /* out[:, j] = gelu_erf(gate_j) * value_j (latent_module.py:881-884); W rows packed per 16-row tile:
                           packed row 16 t + i = value row 8 t + i (i < 8) or gate row 8 t + i - 8 (i >= 8)        */
  DN_EPI_FILM_GATE = 3, /* h=(acc+bias)[*gamma+beta]; out = tanh(h)*sigmoid(h) + res      latent_module.py:525-530 */
  DN_EPI_RESADD = 4,    /* out = res + acc + bias  (fp32 residual stream)                  latent_module.py:692,704 */
  DN_EPI_POSEMB = 5,    /* out = acc + bias + pe[pos(b,t)]                                 latent_module.py:867-868 */
  DN_EPI_RELU = 6       /* out = relu(acc + bias)   (the S2UT decoder's FFN, fairseq/modules/transformer_layer.py:505-508) */
};

#define DN_MAX_TERMS 8

/* One additive term of a causal-conv contraction: rows of A shifted back by `shift` frames inside
 * each sequence (rows with t < shift read zeros), times the packed weight W[Np][K].              */
typedef struct {
  const void* A;      /* [M, lda] activations, element type = dtype                                */
  const void* W;      /* [Np, K] packed weights (K contiguous), Np = N rounded up to 128           */
  int32_t lda;        /* elements between rows of A                                                 */
  int32_t shift;      /* causal shift in frames (tap j of a k-tap conv: (k-1-j)*dilation); negative = frames AFTER t
                         (zeros past the sequence end): the transposed conv of the backward data path (f2)   */
  int64_t a_gstride;  /* elements added to A per group (0 = all groups share A)                     */
  int64_t w_gstride;  /* elements added to W per group                                              */
  int32_t shift_by_group; /* 1: effective shift = shift * 2^group (WaveNet dilation 2^i)            */
  int32_t layout;     /* DN_LAYOUT_* bits; 0 = row-major A and W as described above                 */
  int32_t ldw;        /* elements between rows of W when it is not K (0 = K): a K-slice of a wider packed matrix -- with `groups`,
                         a_gstride and w_gstride = the slice width this is a split-K contraction whose groups write partial sums */
  int32_t pad_ldw_;
} DnGemmTerm;

/* K-blocked operand layout, bf16 only: [K/32][rows][32] instead of [rows][K] -- the 32 K-elements (64 bytes) a K-tile
 * takes from each row lie next to the same K-tile's elements of the neighbouring rows, so the 16-row pieces the
 * contraction stages are 1 KiB of whole cache lines (row-major pieces are sixteen half-lines; measured 2-4x the
 * L2 -> LDS fill rate, tools/dma_issue_cost.hip) and a causal shift is a plain row offset.  rows = M for A and for
 * out, Np for W.  K-blocked A / W are taken by the 256 x 352 tile and, where the shape does not route there, by the
 * 256 x 256 tile (the contraction then runs on that tile whatever the shape heuristic would have chosen; forcing
 * another tile is DN_EINVAL, except DN_TILE_256X192, DN_TILE_256X128_2WG and DN_TILE_256X128_SR where they
 * apply); dn_conv_gemm_kblocked_ok tells whether the shape routes to the 256 x 352 tile, where the
 * layout pays.  The GEGLU epilogue can emit K-blocked output (out_layout) on every tile.                          */
enum { DN_LAYOUT_A_KBLOCKED = 1, DN_LAYOUT_W_KBLOCKED = 2, DN_LAYOUT_OUT_KBLOCKED = 1 };

/* out[g] = epilogue( sum_terms shift(A_term[g]) @ W_term[g]^T ), g = 0..groups-1.
 * Replaces nn.Linear / CausalConv1d(k=1,3) and the ops the reference runs after them
 * (latent_module.py:476-488, 513-536, 613-617, 887-903, 930-950).                               */
typedef struct {
  DnGemmTerm terms[DN_MAX_TERMS];
  int32_t n_terms;
  int32_t dtype;       /* DN_F32 | DN_BF16 | DN_F16 | DN_BF16X3: element type of A and W            */
  int32_t M, N, K;     /* rows (B*T), stored output columns (multiple of 4), K per term (multiple of
                          64 for bf16 / 32 for f32)                                                 */
  int32_t T;           /* frames per sequence: row m -> (b = m / T, t = m % T)                      */
  int32_t groups;      /* independent problems in one launch (>= 1)                                 */
  int32_t epilogue;    /* DN_EPI_*                                                                  */
  const float* bias;   /* [N] fp32 or NULL                                                          */
  int64_t bias_gstride;
  void* out;           /* [M, ldo]                                                                  */
  int32_t ldo;
  int32_t out_dtype;   /* DN_F32 | dtype's 2-byte type | DN_BF16X3 (split rows: ldo, N offsets multiples of 32) */
  int64_t out_gstride;
  const void* res;     /* FILM_GATE: [M, ldr] in res_dtype; RESADD: fp32 [M, ldr] (may alias out)   */
  int32_t ldr;
  int32_t res_dtype;
  int64_t res_gstride;
  const float* gamma_beta; /* FILM_GATE: fp32 [Bc, gb_ld]: gamma at col 0.., beta at col gb_half..; NULL = no FiLM */
  int32_t gb_ld;       /* elements between batch rows (0 = one row shared by the whole batch)       */
  int32_t gb_half;     /* column offset of beta                                                     */
  int64_t gb_gstride;
  const float* pos_table; /* POSEMB: fp32 [T+1, pos_ld] sinusoidal table, row 0 = zeros             */
  int32_t pos_ld;
  int32_t flags;       /* DN_GEMM_* control bits: launch tag, twin launch, forced tile / K order / band (tests, A/B timing); 0 = the
                          library's choice for everything                                                              */
  const int32_t* lengths; /* POSEMB: [B] valid frames per sequence                                  */
  /* RESADD / POSEMB with N <= 512 only: when norm_out != NULL one workgroup owns whole output rows and also emits
   * the NEXT block's RMSNorm of the row it just produced (latent_module.py:620-639, 691, 703):
   * y = out_row / max(|out_row|, 1e-12) * sqrt(norm_D) [* norm_gamma] [* g + b], pad columns zeroed.            */
  void* norm_out;          /* [M, norm_ld] in norm_dtype                                             */
  int32_t norm_ld, norm_dtype, norm_D, norm_gb_ld; /* norm_gb_ld: 0 = one conditioning row for the batch */
  const float* norm_gamma; /* learned gamma [norm_D] or NULL                                         */
  const float* norm_gb;    /* adaptive rows [Bc, norm_gb_ld]: gamma at col 0.., beta at norm_gb_half.. or NULL */
  int32_t norm_gb_half;
  int32_t out_layout;      /* DN_LAYOUT_OUT_KBLOCKED: out is [N/32][M][32] (bf16, GEGLU epilogue, ldo ignored)      */
  /* Split RMSNorm: the norm of a row is divided between the contraction that produces the row and the one that consumes
   * it, so no separate pass over the residual stream remains (x/|x| * sqrt(D) * g + b feeding a Linear W equals
   * (sqrt(D)/|x|) * ((x*g) W^T) + b W^T).
   * Producer (RESADD / POSEMB, N a multiple of 64, any tile): norm_split != 0 makes norm_out receive out_row * gamma
   * (norm_split == 2: in the K-blocked layout [norm_ld/32][M][32], bf16 -- for a consumer that takes DN_LAYOUT_A_KBLOCKED)
   * (norm_gamma, or the gamma half of norm_gb per sample) WITHOUT the 1/|row| factor, and norm_ssq[m, n/64] the sum of
   * squares of the 64 output columns of row m that one wave produced (no atomics: the consumer adds the partials).
   * Consumer (BIAS / SILU / GEGLU): row_ssq != NULL makes out = acc * sqrt(row_D) / max(sqrt(sum_j row_ssq[m, j]), 1e-12)
   * + bias + row_bias[b], with row_bias = beta W^T (+ the layer bias) precomputed by the caller, NULL when there is no beta. */
  int32_t norm_split, norm_ssq_ld;
  float* norm_ssq;         /* [M, norm_ssq_ld]                                                       */
  const float* row_ssq;    /* [M, row_ssq_ld], row_ssq_parts partials per row                        */
  int32_t row_ssq_ld, row_ssq_parts;
  float row_D;             /* the norm's D (not padded)                                              */
  int32_t row_bias_ld;     /* elements between batch rows of row_bias (0 = one row for the batch)    */
  const float* row_bias;   /* [Bc, >= N (packed columns for GEGLU)] fp32 or NULL                     */
  /* GEGLU only (training forward, groups == 1): when pre_out != NULL the epilogue also stores the pre-activation it gates --
   * [M, pre_ld] in out_dtype, packed columns (what the BIAS epilogue would have written) -- for the backward pass.          */
  void* pre_out;
  int32_t pre_ld, pre_pad_;
} DnGemmParams;

/* DnGemmParams.flags.  Bits 0..3 are the compile-time K-loop ablations' (-DDN_GEMM_ABL builds only).                */
enum {
  DN_GEMM_NARROW_STORES = 1 << 4,    /* 4-column instead of 8-column 2-byte stores (A/B timing)                         */
  DN_GEMM_NO_RES_PREFETCH = 1 << 5,  /* no prefetch of the residual rows before the K loop (A/B timing)                 */
  DN_GEMM_RELU = 1 << 6,             /* set by the library: DN_EPI_RELU runs as the SILU kernels with this bit           */
  DN_GEMM_TWIN = 1 << 7,             /* an identical launch runs beside this one (the half batches of DN_LOOP_SPLIT2)    */
  DN_GEMM_TAG_SHIFT = 8,             /* bits 8..15: launch tag (DN_TAG_*) matched by dn_profile_start                     */
  DN_GEMM_TILE_SHIFT = 16,           /* bits 16..19: force a tile variant (DN_TILE_*); 0 = chosen from the shape          */
  DN_GEMM_FAT_STAMPS = 1 << 20,      /* in-kernel clock stamps of the 256 x 352 tile (-DDN_FAT_STAMPS builds only)        */
  DN_GEMM_NO_SHARED_ROWS = 1 << 21,  /* the taps of a causal conv do not share one staged copy of their rows               */
  DN_GEMM_TAPS_INNER = 1 << 22,      /* force the taps-innermost K order on the tiles with 32-deep K-tiles (3, 4, 6, 7)  */
  DN_GEMM_TERM_OUTER = 1 << 23,      /* force the term-outer K order (the summation order of every other tile)            */
  DN_GEMM_BAND_SHIFT = 24            /* bits 24..31: row-tile band of the tile order; 0 = chosen from the shape           */
};

/* Tile variants of dn_conv_gemm (rows x packed output columns per workgroup).                                         */
enum {
  DN_TILE_128X128 = 1,      /* two workgroups per CU, 128-byte K-tiles                                                 */
  DN_TILE_256X128 = 2,      /* one workgroup per CU, 128-byte K-tiles                                                  */
  DN_TILE_256X256 = 3,      /* one workgroup per CU, 64-byte K-tiles; takes K-blocked operands                        */
  DN_TILE_256X352 = 4,      /* one wave per SIMD, 2-byte types, BIAS / GEGLU, packed columns a multiple of 352        */
  DN_TILE_ROW = 5,          /* 64 whole output rows (the fused RMSNorm of RESADD / POSEMB with N <= 512)               */
  DN_TILE_256X256_W4 = 6,   /* forced only, bf16: the hand-scheduled 256 x 256 form, one wave per SIMD                 */
  DN_TILE_256X256_W8 = 7,   /* forced only, bf16: the same with two waves per SIMD                                     */
  DN_TILE_256X192 = 8,      /* the 256 x 256 kernel on 192 columns: widths a multiple of 192 but ragged on 256         */
  DN_TILE_256X128_2WG = 9,  /* forced only, 2-byte types: 256 x 128 with two workgroups per CU                         */
  DN_TILE_256X128_SR = 10   /* forced only, 2-byte types, RESADD, three taps (2d, d, 0): the 256 x 256 kernel on 128 columns,
                               taps innermost in K sharing one staged copy of their rows; takes K-blocked operands. The
                               engines force it for their folded feed-forward contraction (option "ffn_fold")            */
};

int dn_conv_gemm(const DnGemmParams* p, void* stream);

/* How dn_conv_gemm runs a contraction; reads the params and the run-time options only.                                */
typedef struct {
  int32_t tile;        /* DN_TILE_*; -1 = K-blocked operands with a tile forced that does not take them (dn_conv_gemm: DN_EINVAL) */
  int32_t taps_inner;  /* 1: the taps of a causal conv run innermost in K (tiles 3, 4, 6, 7, 10); 0: term-outer             */
  int32_t shared_rows; /* 1: the taps share one staged copy of the activation rows                                         */
  int32_t band;        /* row-tile band of the tile order (0 / 1 = column tiles fastest)                                   */
} DnGemmRoute;
int dn_conv_gemm_route(const DnGemmParams* p, DnGemmRoute* route);
/* 1 when dn_conv_gemm would run this contraction (M, N, K, groups, dtype, epilogue, n_terms are read) on the tile that
 * takes K-blocked A / W terms, else 0.                                                                            */
int dn_conv_gemm_kblocked_ok(const DnGemmParams* p);
/* The tile variant dn_conv_gemm would run this contraction on (DnGemmRoute.tile): lets a caller lay its buffers out
 * K-blocked only where the contraction lands on a tile that gains from it.                                        */
int dn_conv_gemm_tile(const DnGemmParams* p);

/* launch tags set by the engine on its dominant contractions */
enum { DN_TAG_FFN_CONV = 1, DN_TAG_WN_DILATED = 2,
       DN_TAG_FFN_CONV_WGRAD = 3 /* training: the weight-gradient contraction of the FFN causal conv */ };

/* Times the next `max_launches` eager dn_conv_gemm launches carrying `tag` with HIP events recorded on their
 * launch stream (not under graph capture); dn_profile_stop synchronises them and returns the average. */
int dn_profile_start(int32_t tag, int32_t max_launches);
int dn_profile_stop(float* avg_ms, int32_t* n_launches);

/* Fused key-masked multi-head self-attention, flash-style (no [B,H,T,T] tensor).
 * Replaces Attend.forward (non-flash branch) latent_module.py:299-343 between the to_q/to_kv and
 * to_out projections (:945-949).  q,k,v,out: row m = b*T+t, head h at columns [h*dh, (h+1)*dh).
 * Keys j >= lengths[b] are masked (lengths[b] == 0 -> uniform over all T keys, as masked_fill gives). */
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  int32_t ldq, ldk, ldv, ldo;
  int32_t B, T, heads, dim_head;
  int32_t dtype;      /* element type of q,k,v,out                                                 */
  int32_t Tk;         /* keys per sequence when they are not the queries' frames (cross-attention, latent_module.py:935-943:
                         k / v row = b*Tk + j); 0 = T (self-attention).  lengths then count valid KEYS (<= Tk)       */
  const int32_t* lengths; /* [B] or NULL (no mask)                                                  */
  float scale;        /* dim_head ** -0.5                                                           */
  int32_t pad2_;
  float* lse;         /* optional fp32 [B, heads, T]: log2-domain log-sum-exp of the scaled scores of every query
                         (max * scale * log2(e) + log2(sum)), what dn_attention_backward recomputes P from; NULL = not kept */
  float dropout_p;    /* training only (latent_module.py:338,668: nn.Dropout(0.1) on the attention probabilities): probability of
                         zeroing a probability; kept ones are scaled by 1 / (1 - p) AFTER the softmax normalisation.  0 = off.
                         The keep mask is a counter-based hash of (seed, batch, head, query, key) -- dn_attention_backward
                         regenerates it from the same seed; tests/test_hip_train_ops.py restates the hash on the host         */
  uint32_t seed_lo, seed_hi;
  int32_t pad3_;
} DnAttnParams;

int dn_attention(const DnAttnParams* p, void* stream);

/* RMSNorm (latent_module.py:620-639): y = x / max(|x|_2, 1e-12) * sqrt(D) [* gamma] [* g_c[b] + b_c[b]].
 * x fp32 [M, ldx]; y [M, ldy] in out_dtype; gamma fp32 [D] or NULL; gamma_beta fp32 [Bc, gb_ld] or NULL. */
int dn_rmsnorm(const float* x, int32_t ldx, void* y, int32_t ldy, int32_t out_dtype, int32_t M, int32_t D,
               int32_t T, const float* gamma, const float* gamma_beta, int32_t gb_ld, int32_t gb_half,
               void* stream);

/* LearnedSinusoidalPosEmb + Linear + SiLU (latent_module.py:104-116, 741-745).
 * times int32 [B]; w_freq fp32 [half]; W fp32 [C, 2*half+1]; bias fp32 [C]; out fp32 [B, ldo] and,
 * when out_act != NULL, a copy in act_dtype [B, ldo] for the conditioning contractions.            */
int dn_time_cond(const int32_t* times, int32_t B, const float* w_freq, int32_t half, const float* W,
                 const float* bias, int32_t C, float* out, void* out_act, int32_t act_dtype, int32_t ldo,
                 void* stream);

/* DDIM eta=0 update (latent_module.py:1419-1442, safe_div :958-959), elementwise over [B, T*z... rows].
 * coef fp32 [n_steps, 4] = {sqrt_abar, sqrt_1m_abar, sqrt(abar_prev), sqrt(1-abar_prev)} (fp32 casts
 * formed as the reference does); t int32 [B].  x, eps, x_out fp32 [M, ld]; x_act (optional, [M, ld_act])
 * receives x_out in act_dtype for the next step's first contraction.                                        */
int dn_ddim_step(const float* x, const float* eps, float* x_out, void* x_act, int32_t act_dtype,
                 int32_t ld_act, int32_t M, int32_t C, int32_t ld, int32_t T, const float* coef,
                 const int32_t* t, void* stream);

/* out = a[t_b]*x + b[t_b]*noise: q_sample / noise injection
 * (latent_module.py:1405-1409, 1538-1543; diffusion/gaussian_diffusion.py:215-230).               */
int dn_q_sample(const float* x, const float* noise, float* out, void* out_act, int32_t act_dtype,
                int32_t ld_act, int32_t M, int32_t C, int32_t ld, int32_t T, const float* coef_a,
                const float* coef_b, const int32_t* t, void* stream);

/* One reverse step of GaussianDiffusion for an eps-predicting model (diffusion/gaussian_diffusion.py:254-417 p_mean_variance
 * + p_sample, :513-560 ddim_sample): pred_xstart = sqrt_recip*x - sqrt_recipm1*eps [clamped to +-1], posterior mean,
 * FIXED_LARGE / FIXED_SMALL (table column 4) or LEARNED_RANGE variance (model_out has 2x channels on dim 1), then
 * sampler 0: mean + 1[t!=0]*exp(.5 logvar)*noise, sampler 1: DDIM with `eta`.  Tensors are fp32 [N, inner] (inner = C*L
 * contiguous; model_out [N, 2*inner] when learned_range).  table: fp32 [T, DN_GD_COLS].                              */
#define DN_GD_COLS 12
typedef struct {
  const float* x; const float* model_out; const float* noise; /* noise may be NULL (treated as 0) */
  float* sample; float* pred_xstart;                          /* pred_xstart may be NULL */
  const int32_t* t;                                           /* [N] */
  const float* table;
  int32_t N, inner, learned_range, clip_denoised, sampler;
  float eta;
  int32_t predict_xstart;   /* ModelMeanType.START_X (:317-318): model_out IS the x_0 prediction (clamped when clip_denoised) */
  const float* cond_grad;   /* optional fp32 [N, inner]: cond_fn(x, t), the gradient of a conditional log-probability -- sampler 0:
                               condition_mean (:346-358) mean += variance * grad; sampler 1: condition_score (:360-374)
                               eps -= sqrt(1 - abar) * grad, pred_xstart and the mean re-derived from it                        */
} DnGaussianStep;
int dn_gaussian_step(const DnGaussianStep* p, void* stream);

/* The moments and loss terms of GaussianDiffusion for an eps-predicting model, elementwise over fp32 [N, inner] tensors (every
 * output pointer optional):
 *   model_out != NULL: p_mean_variance (diffusion/gaussian_diffusion.py:254-332) -> mean, variance, log_variance, pred_xstart
 *     (_predict_xstart_from_eps :334-339, clipped to +-1 when clip_denoised); reverse_sample = the DDIM reverse-ODE step
 *     (ddim_reverse_sample :562-598); with x_start also vb = the per-element term of _vb_terms_bpd (:682-713) in bits:
 *     KL(q(x_{t-1}|x_t,x_0) || p) for t > 0, the discretised-Gaussian decoder NLL (diffusion_utils.py:66-88) at t = 0.
 *   model_out == NULL, x_start != NULL: q_posterior_mean_variance (:232-252) -> mean, variance, log_variance.
 * Table columns (fp32 casts of the float64 schedule): 0 sqrt_recip_abar, 1 sqrt_recipm1_abar, 2 post_coef1, 3 post_coef2,
 * 4 fixed log variance, 5 posterior_log_variance_clipped (= min_log), 6 log beta (= max_log), 7 abar, 8 abar_prev, 9 abar_next,
 * 10 posterior_variance, 11 fixed variance.                                                                              */
typedef struct {
  const float* x; const float* model_out; const float* x_start;
  const int32_t* t; const float* table;
  float *mean, *variance, *log_variance, *pred_xstart, *vb, *reverse_sample;
  int32_t N, inner, learned_range, clip_denoised;
  int32_t predict_xstart;   /* ModelMeanType.START_X: model_out is the x_0 prediction */
} DnGaussianMoments;
int dn_gaussian_moments(const DnGaussianMoments* p, void* stream);

/* DiagonalGaussianDistribution (distributions.py:24-41, 62-74): params fp32 [M, ldp] = [mean ; logvar];
 * z = mean + exp(0.5*clamp(logvar,-30,20))*noise; kl_rows (optional, fp32 [M]) = 0.5*sum_c(mean^2+var-1-logvar)
 * for valid frames, 0 for pads.                                                                    */
int dn_posterior_sample(const float* params, int32_t ldp, const float* noise, int32_t ldn, float* z,
                        void* z_act, int32_t act_dtype, int32_t ldz, int32_t M, int32_t Z, int32_t T,
                        const int32_t* lengths, float* kl_rows, void* stream);

/* argmax over the first V logits of each row minus `offset` (latent_module.py:1450-1451). */
int dn_argmax_units(const float* logits, int32_t ld, int32_t M, int32_t V, int32_t offset, int32_t* units,
                    void* stream);

/* Philox4x32-10 standard normal fill (Box-Muller), the build's own generator for throughput runs
 * (the reference draws with torch.randn, latent_module.py:1409, distributions.py:38).             */
int dn_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* One noise stream per utterance (chain-start noise that does not depend on how batches are formed): element (b, t, c) of a dense
 * fp32 [B, T, Z] tensor is normal c & 3 of the Philox4x32-10 call with key (keys[b] low, keys[b] high) and counter (q low, q high,
 * stream_id, 0x53545254), q = t * (Z / 4) + c / 4 as a 64-bit value; Box-Muller as dn_randn.  The draw depends on the key, the
 * frame and the channel only.  stream_id 0: posterior noise (distributions.py:24-41), 1: chain-start noise
 * (latent_module.py:1405-1409), 2 + t: the noise of the sampler update that leaves timestep t (the *_keyed loops below draw it in
 * their update kernels; this entry materialises the same numbers).  Z a multiple of 4, out 16-byte aligned.            */
int dn_randn_keyed(float* out, const uint64_t* keys, int32_t B, int32_t T, int32_t Z, uint32_t stream_id, void* stream);

/* Posterior sample + q_sample in one pass on those draws (distributions.py:24-41, latent_module.py:1405-1409): params fp32
 * [B*T, ldp] = [mean ; logvar], n0 / n1 = dn_randn_keyed's streams 0 / 1; z = mean + exp(0.5*clamp(logvar,-30,20))*n0,
 * x = coef_a[t_b]*z + coef_b[t_b]*n1 -- dn_posterior_sample's and dn_q_sample's statements, bit for bit.  x and z_out (may be
 * NULL) dense fp32 [B*T, Z]; Z and ldp multiples of 4, ldp >= 2 Z, params / x / z_out 16-byte aligned; t int32 [B].      */
int dn_chain_start(const float* params, int32_t ldp, const uint64_t* keys, int32_t B, int32_t T, int32_t Z,
                   const float* coef_a, const float* coef_b, const int32_t* t, float* x, float* z_out, void* stream);

/* dtype conversion / zero-padded row copy: dst[m, 0:C] = src[m, 0:C], dst[m, C:ldd] = 0. */
int dn_convert_rows(const void* src, int32_t src_dtype, int32_t lds, void* dst, int32_t dst_dtype,
                    int32_t ldd, int32_t M, int32_t C, void* stream);

/* ------------------------------------------------------------------ optimizer step */
/* The update of the reference's training recipe (scripts/diffusion/train.sh:29-31: Adam, betas (0.9, 0.98),
 * --clip-norm 2.0, inverse_sqrt schedule) over flat fp32 buffers; the schedule itself is host arithmetic
 * (diffnorm_amd/optim.py).  Backward kernels are not part of this round.                                      */

/* sumsq[0] (+)= sum_i grad[i]^2: the square of fairseq.utils.clip_grad_norm_'s total_norm (fairseq/utils.py:347-390;
 * call once per gradient buffer with accumulate != 0 after the first).  scratch: 1024 floats.  Two launches, fixed
 * summation order (bit-reproducible).                                                                          */
int dn_grad_sumsq(const float* grad, int64_t n, float* scratch, float* sumsq, int32_t accumulate, void* stream);

typedef struct {
  double lr, beta1, beta2, eps, weight_decay; /* doubles, as the reference's Python floats: 1 - beta and the step size
                                                 are formed in double and rounded to fp32 once                  */
  double max_norm;  /* --clip-norm; <= 0 or sumsq == NULL: no clipping                                          */
  int32_t step;     /* 1 for the first update (fairseq/optim/adam.py:212)                                       */
  int32_t pad_;
  double grad_scale; /* the trainer's multiply_grads (fairseq/trainer.py:918-933: world / sample_size after DDP's mean, i.e.
                        1 / sample_size on a summed gradient): applied to every gradient before the norm and the update;
                        0 is read as 1                                                                            */
  const float* grad_scale_dev; /* optional device scalar multiplied into grad_scale (a sample size that only exists on the
                                  device after the statistics all-reduce), NULL = 1                                */
} DnAdamParams;

/* Operand preparation for the weight gradient of a causal conv / Linear (the contraction over frames): bf16 [B*T, ld]
 * frames-major -> channels-major with `front` zero frames in front of every sequence and zeros up to Tp frames and in rows
 * >= C; the B*Tp columns are stored as [B*Tp / chunk][rows_total][chunk] (chunk a multiple of 64), one K-slice per group
 * of a split-K dn_conv_gemm; the call fills rows [row0, row0 + rows) (the taps of a conv stack their operands).  dW_j = dY^T . shift_j(X) is then that contraction with A = transposed dY (front 0), W =
 * transposed X with front = shift_j (the padding supplies the zeros of the causal left context), groups = K-slices spread
 * over the chip, fp32 partial outputs summed by the caller (diffnorm_amd/ops.py: conv_weight_grad).                    */
int dn_transpose_pad(const void* src, int32_t ld, int32_t B, int32_t T, int32_t C, int32_t front, int32_t Tp, void* dst,
                     int32_t rows, int32_t rows_total, int32_t row0, int32_t chunk, void* stream);

/* One fairseq Adam update (fairseq/optim/adam.py:159-239) of n fp32 parameters in place, with the gradient scaled by
 * s = grad_scale and then by min(1, max_norm / (s * sqrt(sumsq[0]) + 1e-6)) first (fairseq/trainer.py:918-933, fairseq/utils.py:
 * 392-396; sumsq is the sum of squares of the UNSCALED buffer, which is itself left untouched); param_bf16 != NULL also receives the updated parameters in bf16 (the forward kernels' operand type). */
int dn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const DnAdamParams* hp,
                 const float* sumsq, void* param_bf16, void* stream);

/* Exponential moving average of the parameters (fairseq/models/ema/ema.py:140-197, stepped after every update by fairseq/
 * trainer.py:1018-1025): one more flat fp32 buffer of n elements, ema = ema * decay + param * (1 - decay) per element, as
 * e = fma(p, (float)(1 - decay), e * (float)decay) with 1 - decay formed in double and rounded to fp32 once (the same bits from
 * both entry points).  0 <= decay < 1; decay == 0 (the reference's phase before --ema-start-update) is an exact copy that does
 * not read ema, which may hold anything before.  Buffers 16-byte aligned.
 *
 * dn_adam_step_ema: dn_adam_step (same arguments, same bits in param / exp_avg / exp_avg_sq / param_bf16) plus the EMA update of
 * the freshly updated parameter in the same pass -- 8 B more per element instead of the 12 B and the launch of a pass of its own.
 * ema == NULL is refused: the update without an EMA is dn_adam_step.
 * dn_ema_update: the pass of its own, after an optimizer that is not this library's, and for restores (decay 0).            */
int dn_adam_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const DnAdamParams* hp,
                     const float* sumsq, void* param_bf16, float* ema, double ema_decay, void* stream);
int dn_ema_update(float* ema, const float* param, int64_t n, double decay, void* stream);

/* ------------------------------------------------------------------ backward ops ---------- */
/* The contractions of a backward pass are dn_conv_gemm itself (data gradient: negative shifts + transposed packed weights from
 * dn_transpose_weights; weight gradient: dn_transpose_pad operands + split-K groups + dn_wgrad_reduce).  The entry points
 * below are the backward of everything that is not a contraction, the loss gradients and the reductions over frames.  All
 * reductions are two-stage with fixed block counts (no atomics): a training step is bit-reproducible.                     */

/* Gradient of dn_attention (Attend.forward non-flash branch, latent_module.py:299-343): P is recomputed from the forward's
 * per-query log-sum-exp (DnAttnParams.lse); dq / dk / dv have the layout of q / k / v (row m = b*T+t, head h at columns
 * [h*dh, (h+1)*dh)) with their own row strides, so they can be three column blocks of one [M, 3*heads*dh] buffer.
 * delta: fp32 scratch [B, heads, T] (sum_d dO*O per query, written by the call).  No atomics: dk/dv and dq each have one
 * writer.  Attention dropout (p = 0.1 in the reference's training mode, :338,668): dropout_p / seed as in the forward.        */
typedef struct {
  const void *q, *k, *v, *out, *dout;
  void *dq, *dk, *dv;
  int32_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  int32_t B, T, heads, dim_head;
  int32_t dtype;
  int32_t pad_;
  const int32_t* lengths; /* [B] or NULL */
  float scale;
  int32_t pad2_;
  const float* lse;       /* [B, heads, T] from the forward */
  float* delta;           /* [B, heads, T] scratch */
  float dropout_p;        /* must equal the forward's (with the same seed): the mask is regenerated, not stored */
  uint32_t seed_lo, seed_hi;
  int32_t pad3_;
} DnAttnBwdParams;
int dn_attention_backward(const DnAttnBwdParams* p, void* stream);

/* Gradient of dn_time_cond (latent_module.py:104-116, 741-745): dcond fp32 [B, ldd] -> ACCUMULATES dW [C, 2*half+1], dbias [C] and
 * dw_freq [half] (the learned Fourier frequencies: d/dw sin(2 pi w t) = 2 pi t cos(.)).  ds_scratch: fp32 [B, C].            */
int dn_time_cond_backward(const int32_t* times, int32_t B, const float* w_freq, int32_t half, const float* W, const float* bias, int32_t C,
                          const float* dcond, int32_t ldd, float* ds_scratch, float* dw_freq, float* dW, float* dbias, void* stream);

/* WaveNet gate as a stand-alone pass (the training forward keeps the pre-activation h that its derivative needs):
 * out = tanh(h') sigmoid(h') + res with h' = h * gamma[b] + beta[b] when gamma_beta != NULL (latent_module.py:525-530).
 * h, res, out, dout, dh: [M, ld] in `dtype`, same ld.  Backward: dh = dout * gate'(h') [* gamma]; with FiLM, dgb_rows
 * (fp32 [M, dgb_ld], optional) receives the per-frame terms of the conditioning gradient: [dg * h | dg] at [c | gb_half + c]. */
int dn_gate_forward(const void* h, const void* res, void* out, int32_t dtype, int32_t M, int32_t ld, int32_t T,
                    const float* gamma_beta, int32_t gb_ld, int32_t gb_half, void* stream);
int dn_gate_backward(const void* dout, const void* h, void* dh, int32_t dtype, int32_t M, int32_t ld, int32_t T,
                     const float* gamma_beta, int32_t gb_ld, int32_t gb_half, float* dgb_rows, int32_t dgb_ld, void* stream);

/* GEGLU (latent_module.py:881-884) on the packed column order of the GEGLU projection (DN_EPI_GEGLU: per 16 columns, 8 values
 * then the 8 gates of the same outputs): pre [M, 2*ip] -> out [M, ip] = gelu_erf(gate) * value; backward fills dpre [M, 2*ip]. */
int dn_geglu_forward(const void* pre, void* out, int32_t dtype, int32_t M, int32_t ip, void* stream);
int dn_geglu_backward(const void* dout, const void* pre, void* dpre, int32_t dtype, int32_t M, int32_t ip, void* stream);

/* Gradient of dn_rmsnorm (latent_module.py:620-639).  x fp32 [B*T, ldx] (the norm's input), dy [B*T, lddy] in dy_dtype;
 * dx fp32 [B*T, ldx] = norm gradient (+ dres, the gradient arriving on the residual branch, when not NULL; dx may alias dres);
 * dx_act (optional): dx once more in act_dtype [B*T, ld_act], pad columns zero (the next contraction's operand).
 * Parameter gradients are ACCUMULATED: dgamma fp32 [D] (learned gamma) or dgamma_beta fp32 [B, dgb_ld] = [d g_c | d b_c] at
 * [c | gb_half + c] per sample (adaptive norm).  scratch: dn_rmsnorm_backward_scratch_bytes(B, T, D).  D <= 1024.          */
size_t dn_rmsnorm_backward_scratch_bytes(int32_t B, int32_t T, int32_t D);
int dn_rmsnorm_backward(const float* x, int32_t ldx, const void* dy, int32_t lddy, int32_t dy_dtype, int32_t B, int32_t T, int32_t D,
                        const float* gamma, const float* gamma_beta, int32_t gb_ld, int32_t gb_half, const float* dres, float* dx,
                        void* dx_act, int32_t act_dtype, int32_t ld_act, float* dgamma, float* dgamma_beta, int32_t dgb_ld,
                        float* scratch, void* stream);

/* out[g, c] (+)= scale * sum over the rows of group g of src[row, c] (bias gradients, per-sample conditioning gradients,
 * loss sums): src [groups * rows_per_group, ld] in dtype, out fp32 [groups, out_ld].  scratch: dn_colsum_scratch_bytes.    */
size_t dn_colsum_scratch_bytes(int32_t groups, int32_t rows_per_group, int32_t C);
int dn_colsum(const void* src, int32_t ld, int32_t dtype, int32_t groups, int32_t rows_per_group, int32_t C, float* out,
              int32_t out_ld, float scale, int32_t accumulate, float* scratch, void* stream);

/* Gradient of dn_posterior_sample + the KL term (distributions.py:24-41, 62-74): dparams [M, ldo] (act_dtype, pad columns
 * zero) = [d mean ; d logvar] from dz fp32 [M, lddz] and kl_weight = (loss weight of the KL) / (B * Z * T); the clamp of
 * logvar to [-30, 20] passes no gradient outside the range, KL only counts valid frames.                                 */
int dn_posterior_backward(const float* params, int32_t ldp, const float* noise, int32_t ldn, const float* dz, int32_t lddz,
                          void* dparams, int32_t act_dtype, int32_t ldo, int32_t M, int32_t Z, int32_t T, const int32_t* lengths,
                          float kl_weight, void* stream);

/* Label-smoothed cross entropy over log_softmax(logits) and its gradient (fairseq/criterions/label_smoothed_cross_entropy.py:
 * 34-51 with ignore_index 0; speech_vae_decoder_loss.py:60-79): rows fp32 [M, 4] = {nll, smooth, correct, valid} per frame
 * (nll = -lprob[target], smooth = -sum lprobs; loss = (1 - eps - eps_i) nll + eps_i smooth, eps_i = eps / (V - 1));
 * dlogits (optional, act_dtype [M, ldd], pad columns zero) = grad_scale * d loss / d logits.  V <= 1024.                  */
int dn_lsce_loss_grad(const float* logits, int32_t ld, const int32_t* target, int32_t M, int32_t V, float epsilon, float grad_scale,
                      float* rows, void* dlogits, int32_t act_dtype, int32_t ldd, void* stream);

/* Masked MSE (latent_module.py:1135-1138, 1576-1577: mean over the elements of valid frames): sq_rows fp32 [M] = sum_c
 * (pred - target)^2 of valid frames (0 for pads); dpred fp32 [M, ldd] (+)= grad_scale * (pred - target), and dpred_act its
 * copy in act_dtype [M, ld_act] (both optional, pad columns and pad frames zero).                                          */
int dn_masked_mse_grad(const float* pred, int32_t ldp, const float* target, int32_t ldt, int32_t M, int32_t C, int32_t T,
                       const int32_t* lengths, float grad_scale, float* sq_rows, float* dpred, int32_t ldd, int32_t accumulate,
                       void* dpred_act, int32_t act_dtype, int32_t ld_act, void* stream);

/* out[0] (+)= sum_i v[i] (fixed two-stage order); scratch: 256 floats. */
int dn_vec_sum(const float* v, int64_t n, float* out, int32_t accumulate, float* scratch, void* stream);

/* dst[i] = sum_{k < count} src[k * stride + i], i < n (the gradients a tensor receives from several consumers). */
int dn_sum_groups(const void* src, int64_t stride, int32_t count, void* dst, int32_t dtype, int64_t n, void* stream);
/* out[b][c] = sum_n X[b][n] * W[n][c], fp32: a handful of rows (one stream of W per 32) against a huge ROW-MAJOR matrix W [N, ldw] (C valid columns), streamed once
 * as it lies -- the data gradient of the eps-predictor's conditioning projection (autograd of nn.Linear, latent_module.py:841-852),
 * without a transposed copy of its 470 MB.  Partial sums per row slice in `scratch` (dn_rows_times_weight_scratch_bytes), added in a
 * fixed order.                                                                                                                     */
size_t dn_rows_times_weight_scratch_bytes(int32_t B, int32_t N, int32_t C);
int dn_rows_times_weight(const float* X, int32_t ldx, int32_t B, const float* W, int32_t ldw, int32_t N, int32_t C, float* out,
                         float* scratch, void* stream);

/* Batched padded transpose of packed weights, the W operand of the data-gradient contraction: dst[n] [Cp][Rp] = (the first
 * R rows of src[n], [R][Cc])^T, zeros beyond; matrices src_stride / dst_stride elements apart.  DN_BF16X3: both sides are
 * weight-order split rows ([lo | hi]), dst = split(transpose(hi + lo)); Cc, Rp and the strides multiples of 32.            */
int dn_transpose_weights(const void* src, int32_t dtype, int32_t count, int64_t src_stride, int32_t R, int32_t Cc, void* dst,
                         int64_t dst_stride, int32_t Rp, int32_t Cp, void* stream);

/* fp32 [n] -> DN_BF16X3 split rows (n a multiple of 32; dst 128-byte aligned): weight_order != 0 stores [lo | hi] (packed
 * weights), 0 stores [hi | lo] (activations).  The split-operand training engine's work copy of its master parameters, the
 * operand type of the contractions that replace torch's fp32 autograd of nn.Linear / CausalConv1d (latent_module.py:476-488). */
int dn_split_rows(const float* src, int64_t n, void* dst, int32_t weight_order, void* stream);

/* The inference engines' packed tensors (dn_eps_create / dn_vae_create tables) from a training engine's flat fp32 master buffer,
 * on the device: what diffnorm_amd/packing.py::pack_eps / pack_vae make of the master's state dict, without the round trip through
 * the host.  One descriptor per destination tensor, or per layer slice of a tensor stacked over the transformer's layers
 * (packing.repack_plan); the array lives in device memory.  A descriptor covers `mats` matrices [rows][K] (padded sizes) that lie
 * one after the other in the master and in the destination:
 *   DN_REPACK_CONVERT  as they lie, in the arithmetic `dtype`: DN_F32 (copy), DN_BF16 / DN_F16 (round to nearest even; f16 saturates
 *                      at +-65504 like the host packer) or DN_BF16X3 weight-order split rows ([lo | hi] per 32 elements,
 *                      hi = bf16(x), lo = bf16(x - hi));  rows * K a multiple of 32, dst 128-byte aligned
 *   DN_REPACK_KBLOCK   the same values in the K-blocked layout [K/32][rows][32] (DN_LAYOUT_W_KBLOCKED); the 2-byte dtypes only
 *                      (the other modes have no K-blocked copies: such a descriptor writes nothing)
 *   DN_REPACK_COPY     fp32 as it lies whatever `dtype` (biases, gammas, the conditioning path, Fourier frequencies): any length
 *   DN_REPACK_SUM      fp32 dst[c] = ((0 + src[c]) + src[stride + c]) + ... over `count` rows of K elements (rows = mats = 1): the
 *                      summed skip bias of a WaveNet, in the host packer's order;  K a multiple of 4, dst 16-byte aligned
 * Stream-ordered, no allocation, no synchronisation.  The descriptors are trusted: the caller keeps src + mats * rows * K inside
 * the master and the destination inside its tensor.                                                                            */
enum { DN_REPACK_CONVERT = 0, DN_REPACK_KBLOCK = 1, DN_REPACK_COPY = 2, DN_REPACK_SUM = 3 };
typedef struct {
  int64_t src;        /* element offset of the source in the fp32 master (a multiple of 4)                        */
  void* dst;          /* device address of the destination tensor or slice                                        */
  int32_t kind;       /* DN_REPACK_*                                                                              */
  int32_t mats;       /* matrices [rows][K], contiguous on both sides                                             */
  int32_t rows, K;    /* padded sizes; COPY: rows * K * mats = number of elements                                 */
  int32_t count;      /* SUM: number of addends                                                                   */
  int32_t pad_;
  int64_t stride;     /* SUM: elements between the addends                                                        */
} DnRepackDesc;
int dn_repack_weights(const float* master, const DnRepackDesc* descs, int32_t n, int32_t dtype, void* stream);

/* The sampling engines' folded feed-forward weights.  FeedForward (latent_module.py:887-903) ends in CausalConv1d(inner, inner, 3)
 * -> Linear(inner, dim) with nothing but (at inference) the identity between them, and causal zero padding commutes with a linear
 * map: the two are one causal conv of three taps inner -> dim,
 *   W'_j = W_out . W_conv_j  (j = 0, 1, 2)      b' = W_out . b_conv + b_out
 * Sources: the packed fp32 tensors of `depth` layers (diffnorm_amd/packing.py: conv_W [3][padn(inner)][padk(inner)], conv_b
 * [padk(inner)], out_W [padn(dim)][padk(inner)], out_b [padk(dim)]), layer l at element l * its stride -- stacked tensors, or a
 * training engine's flat master / EMA buffer, whose layers lie a constant distance apart.  The products are fp32, summed over
 * k = 0 .. inner-1 in that order (one result per lane: the same sources give the same bits), and rounded once into the arithmetic
 * `dtype`'s weight format: fold_W [depth][3][padn(dim)][padk(inner)] (DN_F32 / DN_BF16 / DN_F16 row-major, DN_BF16X3 weight-order
 * split rows), 128-byte aligned; fold_b fp32 [depth][padk(dim)].  Padding rows and columns are written as zeros.  Stream-ordered,
 * no allocation, no synchronisation.  The training engines keep the two-stage form (their weights change every update and the
 * backward needs both stages).                                                                                                  */
int dn_ffn_fold(const float* conv_W, const float* conv_b, const float* out_W, const float* out_b, int64_t conv_W_stride,
                int64_t conv_b_stride, int64_t out_W_stride, int64_t out_b_stride, int32_t depth, int32_t dim, int32_t inner,
                int32_t dtype, void* fold_W, float* fold_b, void* stream);
/* The same, and from the same fp32 sums a second copy of the weights in the K-blocked layout, fold_Wkb
 * [depth][3][padk(inner)/32][padn(dim)][32] (DN_BF16 / DN_F16 only, 128-byte aligned): every element is rounded once and stored
 * twice, so the two copies hold the same bits, refreshed or fresh.  fold_Wkb NULL: dn_ffn_fold.                                 */
int dn_ffn_fold_kblocked(const float* conv_W, const float* conv_b, const float* out_W, const float* out_b, int64_t conv_W_stride,
                         int64_t conv_b_stride, int64_t out_W_stride, int64_t out_b_stride, int32_t depth, int32_t dim, int32_t inner,
                         int32_t dtype, void* fold_W, float* fold_b, void* fold_Wkb, void* stream);

/* The operand transpose of the training engines' weight gradient (autograd of CausalConv1d / nn.Linear, latent_module.py:476-485):
 * dst[j / chunk][row0 + c][j % chunk] = src[b * T + t, c] with j = b * Tp + front + t, zero for pad frames, channels >= C and the tail
 * columns [B * Tp, cols_total).  dtype DN_F32 / DN_BF16 / DN_BF16X3 (src split rows [hi | lo]; dst split rows in the order of its role:
 * weight_order 0 = [hi | lo], the A operand dY^T, 1 = [lo | hi], the W operand X^T).  chunk a multiple of 64 dividing cols_total.  */
int dn_transpose_slices(const void* src, int32_t dtype, int32_t ld, int32_t B, int32_t T, int32_t C, int32_t front, int32_t Tp,
                        int64_t cols_total, int32_t chunk, void* dst, int32_t rows, int32_t rows_total, int32_t row0, int32_t weight_order,
                        void* stream);

/* Last step of a weight gradient: grad[tap][n][k] += sum_s part[s][n][tap * rows_w + k] for n < cout, k < Kp; part is the fp32
 * split-K output [slices][cout][n_total] of the contraction over frames, grad the packed fp32 layout [n_taps][Np][Kp].    */
int dn_wgrad_reduce(const float* part, int32_t slices, int32_t cout, int32_t n_total, int32_t rows_w, int32_t n_taps, float* grad,
                    int32_t Np, int32_t Kp, void* stream);

/* dst[j * ld + c] += src[c], j < count (the L skip-conv biases of a WaveNet share one gradient). */
int dn_add_broadcast(const float* src, float* dst, int32_t C, int32_t ld, int32_t count, void* stream);

/* The same weight gradient straight from the row-major operands, no transposed copies (bf16; autograd of CausalConv1d
 * latent_module.py:476-485 / nn.Linear): sum over frames m of dY[m][n] * X_tap[m - shift_tap][k] (zero where the frame index of m
 * within its sequence is < shift_tap), the contraction over frames fed to the MFMA through transposing LDS reads
 * (csrc/wgrad_tn.hip).  dY [B*T][lddy], X_tap [B*T][ldx[tap]] bf16, rows 16-byte multiples (pad columns may hold anything).
 * slices == 1: grad[tap][padn(cout)][padk(cin)] += result (part == NULL); slices > 1:
 * part[slice][cout][n_taps * padn(cin)] = the partial sums of that slice of the frames (then dn_wgrad_reduce), grad unused.  */
int dn_conv_weight_grad_tn(const void* dy, int32_t lddy, int32_t cout, const void* const* x, const int32_t* ldx, const int32_t* shift,
                           int32_t n_taps, int32_t cin, int32_t B, int32_t T, int32_t slices, float* part, float* grad, void* stream);

/* The same from DN_BF16X3 split rows (autograd of CausalConv1d latent_module.py:476-485 / nn.Linear in split-operand arithmetic):
 * dY and every X_tap are split rows in activation order ([hi | lo] per 32 elements); lddy, ldx, cin and cout count 4-byte elements
 * and every ld is a multiple of 32 (pad columns may hold anything).  Per fragment pair three bf16 MFMAs into one fp32 accumulator,
 * x_lo dy_hi + x_hi dy_lo + x_hi dy_hi (lo lo dropped).  part / grad / slices as in dn_conv_weight_grad_tn (plain fp32).        */
int dn_conv_weight_grad_tn_x3(const void* dy, int32_t lddy, int32_t cout, const void* const* x, const int32_t* ldx, const int32_t* shift,
                              int32_t n_taps, int32_t cin, int32_t B, int32_t T, int32_t slices, float* part, float* grad, void* stream);

/* dn_transpose_pad for fp32 operands (exact-fp32 mode); chunk a multiple of 32. */
int dn_transpose_pad_f32(const float* src, int32_t ld, int32_t B, int32_t T, int32_t C, int32_t front, int32_t Tp, float* dst,
                         int32_t rows, int32_t rows_total, int32_t row0, int32_t chunk, void* stream);

/* ------------------------------------------------------------------ whole-path engine ---------- */

typedef struct {
  int32_t dim, latent, depth, heads, dim_head, wn_layers, wn_stacks, cond_mult;
  int32_t dtype;  /* DN_F32 | DN_BF16 */
  int32_t max_pos; /* rows in the positional table minus 1 */
  /* conditional variant (use_cond=True, latent_module.py:752-773): 0 = the unconditional model of the recipe */
  int32_t dim_prompt, num_latents, resampler_depth;
} DnEpsConfig;

typedef struct {
  int32_t dim, z, depth, heads, dim_head, stacks, layers, vocab;
  int32_t n_mults; int32_t mults[4];
  int32_t dtype;
} DnVaeConfig;

typedef struct DnEps DnEps;   /* eps-predictor `Model`        latent_module.py:709-876  */
typedef struct DnVae DnVae;   /* SpeechVAEEncoderDecoder      latent_module.py:1035-1142 */

/* Packed-weight tables: device pointers in the order produced by diffnorm_amd/packing.py
 * (documented in DESIGN.md "packed layout"); the library keeps the pointers, not copies.           */
int dn_eps_create(const DnEpsConfig* cfg, const void* const* weights, int32_t n_weights, DnEps** out);
void dn_eps_destroy(DnEps* m);
size_t dn_eps_workspace_bytes(const DnEps* m, int32_t B, int32_t T);
/* Model.forward (latent_module.py:828-876): x fp32 [B,T,latent] dense, t int32 [B], lengths int32 [B]
 * -> eps fp32 [B,T,latent].  shared_t != 0 promises all t[b] equal (sampling) so the 56 conditioning
 * projections run for one row.                                                                     */
int dn_eps_forward(DnEps* m, const float* x, const int32_t* t, const int32_t* lengths, int32_t B, int32_t T,
                   int32_t shared_t, float* eps_out, void* workspace, size_t workspace_bytes, void* stream);

/* Conditional variant (Model.forward with condition_on_prompt, latent_module.py:828-876, PerceiverResampler :416-471,
 * classifier-free guidance :813-826): prompt fp32 [B, Tp, dim_prompt] with prompt_lengths [B]; drop int32 [B] = the guidance drop
 * mask (1: the sample runs on null_prompt_cond / null_prompt_tokens).  The pooled-prompt condition is concatenated to the time
 * condition (2x conditioning width), the resampled prompt latents feed a cross-attention block in every transformer layer.
 * Needs a model created with cfg.dim_prompt > 0 (packed table: diffnorm_amd/packing.py::pack_eps).                        */
size_t dn_eps_cond_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t Tp);
int dn_eps_forward_cond(DnEps* m, const float* x, const int32_t* t, const int32_t* lengths, const float* prompt,
                        const int32_t* prompt_lengths, const int32_t* drop, int32_t B, int32_t T, int32_t Tp, float* eps_out,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same pass inside a CHAIN of steps (the prompted, guided sampling loop): everything that depends on the prompt only -- the
 * pooled-prompt half of the conditioning projection, the PerceiverResampler and every layer's cross-attention keys / values -- is
 * kept in the workspace, and with DN_COND_REUSE_PROMPT a later call on the SAME workspace and shapes skips it (the caller
 * guarantees nothing else wrote the workspace in between and that prompt / prompt_lengths / drop are unchanged).  time_table
 * (optional, fp32 [table_n, n_cond] from dn_eps_cond_time_table, first row = timestep table_t0): the time half of the conditioning
 * rows of every step of the chain, so the 2 C x n_cond projection is not streamed inside the loop.  flags = 0, time_table = NULL
 * is dn_eps_forward_cond.  With a time table `t` is used ONLY to pick the table's row, t[b] - table_t0 clamped into [0, table_n-1]
 * (the time-conditioning MLP is skipped): a chain whose table has one row per step (dn_eps_cond_time_table_steps) passes its step
 * index as `t` with table_t0 = 0, whatever timestep that step evaluates.                                                         */
#define DN_COND_REUSE_PROMPT 1
int dn_eps_forward_cond_ex(DnEps* m, const float* x, const int32_t* t, const int32_t* lengths, const float* prompt,
                           const int32_t* prompt_lengths, const int32_t* drop, int32_t B, int32_t T, int32_t Tp, float* eps_out,
                           void* workspace, size_t workspace_bytes, int32_t flags, const float* time_table, int32_t table_t0,
                           int32_t table_n, void* stream);
size_t dn_eps_cond_time_table_workspace_bytes(const DnEps* m, int32_t n_t);
int dn_eps_cond_time_table(DnEps* m, int32_t t0, int32_t n_t, float* table, void* workspace, size_t workspace_bytes, void* stream);
/* The same table for a device list of timesteps: row i = the time half of the conditioning rows of timestep steps[i] (device int32
 * [n_steps], any order; the schedule of dn_guided_ddim_loop).  Workspace: dn_eps_cond_time_table_workspace_bytes(m, n_steps).
 * steps = t0 .. t0 + n_t - 1 is dn_eps_cond_time_table's result (time conditioning latent_module.py:841-842, 846-852).          */
int dn_eps_cond_time_table_steps(DnEps* m, const int32_t* steps, int32_t n_steps, float* table, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* After the packed weights behind `m` were rewritten in place (dn_repack_weights): forgets what the engine derived from them --
 * the conditioning table a DN_LOOP_KEEP_TABLE call would reuse.  The captured hipGraph of the device loop stays: it holds
 * addresses only, and every table it reads is rebuilt from the weights by the next dn_ddim_loop / dn_ddpm_loop call.  The
 * guided loop (dn_guided_ddim_loop) needs nothing: every call rebuilds its time table and its first step the prompt-only state. */
int dn_eps_weights_changed(DnEps* m);
/* Attaches dn_ffn_fold's buffers (the engine keeps the pointers, like the table's; NULL, NULL detaches).  With them, and option
 * "ffn_fold" not 0, every transformer layer runs GEGLU projection -> ONE three-tap contraction (A = the GEGLU output, shifts 2/1/0,
 * RESADD into the residual stream with the split-norm producer, tagged DN_TAG_FFN_CONV) instead of conv + output projection, and
 * the conv's [M, padk(inner)] buffer leaves the workspace plan.  Captured steps are dropped.  After the packed weights were
 * rewritten, dn_ffn_fold into the same buffers refreshes them: the addresses stay attached.                                      */
int dn_eps_set_ffn_fold(DnEps* m, const void* fold_W, const float* fold_b);
/* Attaches dn_ffn_fold_kblocked's K-blocked copy (NULL detaches; dn_eps_set_ffn_fold detaches it too, so attach it after).  Where
 * the folded contraction runs on DN_TILE_256X128_SR (option "ffn_fold") the GEGLU projection then writes its output K-blocked and
 * the contraction stages whole cache lines of both operands; without the copy that tile reads row-major operands.              */
int dn_eps_set_ffn_fold_kblocked(DnEps* m, const void* fold_Wkb);

int dn_vae_create(const DnVaeConfig* cfg, const void* const* weights, int32_t n_weights, DnVae** out);
void dn_vae_destroy(DnVae* m);
int dn_vae_set_ffn_fold(DnVae* m, const void* fold_W, const float* fold_b); /* as dn_eps_set_ffn_fold, the decoder's transformer */
int dn_vae_set_ffn_fold_kblocked(DnVae* m, const void* fold_Wkb);           /* as dn_eps_set_ffn_fold_kblocked                    */
size_t dn_vae_workspace_bytes(const DnVae* m, int32_t B, int32_t T);
/* encoder WaveNets of encode_feature (latent_module.py:1099-1106): feat fp32 [B,T,dim] -> params fp32 [B,T,2z] */
int dn_vae_encode_params(DnVae* m, const float* feat, int32_t B, int32_t T, float* params, void* workspace,
                         size_t workspace_bytes, void* stream);
/* decode_feature (latent_module.py:1109-1116): latent fp32 [B,T,z] -> recon fp32 [B,T,dim], logits fp32
 * [B,T,vocab] (either may be NULL), units int32 [B,T] = argmax-4 (may be NULL)                     */
int dn_vae_decode(DnVae* m, const float* latent, const int32_t* lengths, int32_t B, int32_t T, float* recon,
                  float* logits, int32_t* units, void* workspace, size_t workspace_bytes, void* stream);

/* LatentDiscreteModel.ddim_sample's device loop (latent_module.py:1405-1445): starting from x (already
 * noised at start_step), evaluates the eps-predictor for t = start_step-1 .. 1 (t = 0 only when
 * start_step == 1) with the eta=0 update after each.  coef: fp32 [timesteps,4] as dn_ddim_step.
 * x fp32 [B,T,latent] is updated in place.  The conditioning rows of all steps are built once, in
 * fp32, before the loop.  max_evals > 0 stops after that many evaluations (the caller continues with
 * start_step - max_evals).  flags: DN_LOOP_* bits.  Workspace:
 * dn_ddim_workspace_bytes.  Returns the number of model evaluations (>= 0) or a negative error.                 */
enum { DN_LOOP_GRAPH = 1,  /* capture one step into a hipGraph and replay it */
       DN_LOOP_SPLIT2 = 2, /* run the two half-batches as parallel branches (side stream / forked graph) */
       DN_LOOP_KEEP_TABLE = 4 /* continuing a chain (after a max_evals stop): the caller guarantees that nothing wrote the
                                 workspace since the previous dn_ddim_loop call with the same B, T and split; the
                                 conditioning table built then (rows t < its start_step) is reused instead of rebuilt */ };
size_t dn_ddim_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t start_step);
int dn_ddim_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, int32_t start_step,
                 int32_t max_evals, const float* coef, int32_t timesteps, int32_t flags, void* workspace,
                 size_t workspace_bytes, void* stream);

/* The same device loop with the ancestral (DDPM) update of GaussianDiffusion.p_sample / p_sample_loop
 * (diffusion/gaussian_diffusion.py:376-417, 459-511) instead of DDIM eta = 0 -- BASELINE configs[2] read literally: for
 * t = start_step-1 .. 0 (t = 0 IS evaluated, its noise masked): eps = Model(x, t); x0 = sqrt_recip_abar x - sqrt_recipm1_abar eps
 * [clamped to +-1 when clip_denoised]; mean = coef1 x0 + coef2 x; x <- mean + 1[t != 0] exp(0.5 log_var_t) z.
 * table: fp32 [timesteps, DN_GD_COLS] as dn_gaussian_step takes it (column 4 = the fixed log-variance: FIXED_SMALL or
 * FIXED_LARGE).  z: injected -- noise fp32 [start_step, B*T*latent], row (start_step-1-t) used at step t (parity runs) -- or,
 * noise == NULL, drawn in the update kernel from Philox4x32-10 keyed by `seed` with the counter (t, element quad): the step
 * index is read from the loop's device counter, so a captured graph draws fresh noise at every replay.  Everything else
 * (conditioning table once per chain, hipGraph replay, two half-batch streams, max_evals / KEEP_TABLE) as dn_ddim_loop;
 * workspace: dn_ddim_workspace_bytes.  Returns the number of model evaluations or a negative error.                     */
int dn_ddpm_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, int32_t start_step, int32_t max_evals,
                 const float* table, int32_t timesteps, int32_t clip_denoised, uint64_t seed, const float* noise, int32_t flags,
                 void* workspace, size_t workspace_bytes, void* stream);

/* dn_ddpm_loop (diffusion/gaussian_diffusion.py:376-417, 459-511) with keyed per-step noise: z of element (b, frame, channel) at
 * step t is dn_randn_keyed's stream 2 + t under keys[b] (device uint64 [B], 8-byte aligned) -- it depends on the key, the timestep,
 * the frame and the channel only, not on the row, B, the padded T, graph or eager, or the half batch: BOTH halves of a
 * DN_LOOP_SPLIT2 chain draw under the keys, so, unlike the seed-drawn chain, the keyed one is split-invariant.  At t = 0 no draw
 * is applied.  The captured step bakes in the ADDRESS of keys (part of the graph key, with seed 0), never their contents.  Null or
 * misaligned keys and a latent width that is no multiple of 4 are refused before anything is written; everything else as
 * dn_ddpm_loop.                                                                                                              */
int dn_ddpm_loop_keyed(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, int32_t start_step, int32_t max_evals,
                       const float* table, int32_t timesteps, int32_t clip_denoised, const uint64_t* keys, int32_t flags,
                       void* workspace, size_t workspace_bytes, void* stream);

/* A DDIM chain over a timestep schedule: strided steps and eta (GaussianDiffusion.ddim_sample, diffusion/gaussian_diffusion.py:
 * 513-560, on a sub-sequence of the timesteps as SpacedDiffusion / space_timesteps select one, diffusion/respace.py:12-115; entered
 * like LatentDiscreteModel.ddim_sample's loop, latent_module.py:1405-1445).  The chain is a strictly descending list of evaluation
 * timesteps e_0 > ... > e_{n-1} >= 0 (steps: device int32 [n_steps]); x enters at level abar[e_0]; update i moves x from abar[e_i]
 * to abar_tgt(i) = abar[e_{i+1}], the last one to abar[0] (e_{n-1} >= 1) or to 1 (e_{n-1} == 0).  e = [s-1 .. 1] is dn_ddim_loop's
 * chain at start_step = s, bit for bit; e = [0] its start_step == 1.
 * coef: device fp32 [n_steps, DN_DDIM_SCHED_COLS], row i = {sqrt abar_e, sqrt(1-abar_e), sqrt abar_tgt, sqrt(1-abar_tgt-sigma^2),
 * sigma}, sigma = eta sqrt((1-abar_tgt)/(1-abar_e)) sqrt(1-abar_e/abar_tgt).  The update, fp32, safe-div form of dn_ddim_step:
 *   x1 = (x - s1 eps) / max(sa, 1e-10); pn = (x - sa x1) / max(s1, 1e-10); x <- x1 c2 + c3 pn [+ 1[e_i != 0] sigma z when eta_on].
 * z: injected -- noise fp32 [n_steps, B*T*latent], row i for update i -- or, noise == NULL, Philox4x32-10 keyed by `seed` with the
 * counter (element quad of the whole batch, step index i): the draw of an element depends on (seed, i, element) only, so eager,
 * graph replay and the two half-batch streams agree bit for bit.  eta_on == 0: no noise is drawn, `noise` must be NULL.
 * The conditioning table has n_steps rows (row i for e_i), and the workspace scales with n_steps: dn_ddim_sched_workspace_bytes
 * (= dn_ddim_workspace_bytes at start_step = n_steps).  steps and coef are copied into the workspace at chain start (device to
 * device, on the stream): a captured step holds workspace addresses only.  flags: DN_LOOP_GRAPH | DN_LOOP_SPLIT2.  Unconditional
 * model only.  Every argument check precedes the first HIP call; the CONTENT of `steps` is device memory the entry cannot read:
 * dn_ddim_sched_check validates a HOST copy (non-empty, inside [0, timesteps-1], strictly descending) before it is uploaded.
 * Returns the number of model evaluations (= n_steps) or a negative error.                                                       */
#define DN_DDIM_SCHED_COLS 5
size_t dn_ddim_sched_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t n_steps);
int dn_ddim_sched_check(const int32_t* steps_host, int32_t n_steps, int32_t timesteps);
int dn_ddim_sched_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* coef,
                       int32_t n_steps, int32_t timesteps, int32_t eta_on, uint64_t seed, const float* noise, int32_t flags,
                       void* workspace, size_t workspace_bytes, void* stream);

/* dn_ddim_sched_loop (diffusion/gaussian_diffusion.py:513-560, diffusion/respace.py:12-115, latent_module.py:1405-1445) with eta on
 * and keyed per-step noise: z of element (b, frame, channel) at update i is dn_randn_keyed's stream 2 + e_i under keys[b] (device
 * uint64 [B], 8-byte aligned).  The stream is the TIMESTEP e_i = steps[i], not the index i: the draw depends on (key, timestep,
 * frame, channel) only -- not on the row, B, the padded T, the half batch, the schedule's other members, graph or eager.  At
 * e_i == 0 no draw is applied.  The captured step bakes in the ADDRESS of keys (part of the graph key, with seed 0), never their
 * contents: new contents at that address give new draws, another address is a cache miss.  Null or misaligned keys and a latent
 * width that is no multiple of 4 are refused before anything is written; flags, workspace (dn_ddim_sched_workspace_bytes) and
 * everything else as dn_ddim_sched_loop.
 * dn_ddim_sched_step is the update alone on n (a multiple of 4) contiguous fp32 elements, x / eps / noise 16-byte aligned: row
 * *step_index (device int32) of coef and steps, z from `seed` (counter: element quad, step index) or the injected `noise` [n] of THIS
 * step; dn_ddim_sched_step_keyed the keyed update alone on dense x / eps [B, T, Z] (Z a multiple of 4), for host-stepped chains.  */
int dn_ddim_sched_loop_keyed(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* coef,
                             int32_t n_steps, int32_t timesteps, const uint64_t* keys, int32_t flags, void* workspace,
                             size_t workspace_bytes, void* stream);
int dn_ddim_sched_step(float* x, const float* eps, int64_t n, const float* coef, const int32_t* steps, const int32_t* step_index,
                       int32_t eta_on, uint64_t seed, const float* noise, void* stream);
int dn_ddim_sched_step_keyed(float* x, const float* eps, const uint64_t* keys, int32_t B, int32_t T, int32_t Z, const float* coef,
                             const int32_t* steps, const int32_t* step_index, void* stream);

/* DPM-Solver++(2M) over a timestep schedule, as a device loop (Lu et al. 2022, "DPM-Solver++", the data-prediction multistep solver,
 * eq. 11-12 / algorithm 2): dn_ddim_sched_loop's chain -- the strictly descending evaluation timesteps e_0 > ... > e_{n-1}, the level
 * x enters at, the target level abar_tgt(i) of update i, one evaluation per step -- with a second-order deterministic update.  With
 * alpha = sqrt abar, sigma = sqrt(1 - abar), lambda = log(alpha / sigma), s = e_i, t = the target of update i, h_i = lambda_t - lambda_s:
 *   x0_i = (x - sigma_s eps) / max(alpha_s, 1e-10)
 *   x <- a x + b (c1 x0_i + c0 x0_{i-1}),  a = sigma_t / sigma_s,  b = -alpha_t expm1(-h_i)
 * first-order rows (the first row, order 1, the last row under lower_order_final, a target level of 1 where a = 0, b = 1): c1 = 1,
 * c0 = 0 -- DDIM at eta = 0 in another arithmetic; second-order rows: r = (lambda_{e_i} - lambda_{e_{i-1}}) / h_i, c1 = 1 + 1/(2r),
 * c0 = -1/(2r).  coef: device fp32 [n_steps, DN_DPM_COLS], row i = {alpha_s, sigma_s, a, b, c1, c0}, formed in float64 on the host
 * (scheduler.dpm_schedule).  No noise is drawn: the solver is deterministic.
 * dn_dpm2m_step is the update alone on n (a multiple of 4) contiguous fp32 elements, 16-byte aligned: row *step_index (device int32) of
 * coef; hist holds x0_{i-1} on entry -- read only when the row's c0 != 0 -- and x0_i on return.
 * dn_dpm_loop keeps hist in its workspace beside eps: dn_dpm_workspace_bytes = dn_ddim_workspace_bytes(m, B, T, n_steps) + B T latent
 * fp32 rounded up to 256 bytes.  Row 0 is first order, so a chain never reads what an earlier call left there.  steps and coef are
 * copied into the workspace at chain start; flags: DN_LOOP_GRAPH | DN_LOOP_SPLIT2 (the captured step is cached under a key bit of its
 * own: a dn_ddim_sched_loop step is never replayed for this loop nor the other way round; the two half-batch streams each update their
 * own element range of the shared x / eps / hist).  Unconditional model only (the prompted chain is dn_guided_ddim_loop).  Every
 * argument check precedes the first HIP call; dn_ddim_sched_check validates a host copy of the steps.  Returns the number of model
 * evaluations (= n_steps) or a negative error.                                                                                    */
#define DN_DPM_COLS 6
int dn_dpm2m_step(float* x, const float* eps, float* hist, int64_t n, const float* coef, const int32_t* step_index, void* stream);
size_t dn_dpm_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t n_steps);
int dn_dpm_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* coef, int32_t n_steps,
                int32_t timesteps, int32_t flags, void* workspace, size_t workspace_bytes, void* stream);

/* The generic Gaussian scheduler as a device loop: GaussianDiffusion.p_sample_loop / ddim_sample_loop (diffusion/gaussian_diffusion.py:
 * 419-511, 600-680) of a diffusion create_diffusion builds for an eps-predicting model with a fixed variance, respaced or not
 * (SpacedDiffusion, diffusion/respace.py:63-129: the model sees timestep_map[i], the coefficients are row i of the RESPACED tables) --
 * in place of a host loop that builds a timestep tensor, evaluates the model, draws randn_like and launches dn_gaussian_step per step.
 * steps: device int32 [n_steps], the ORIGINAL timesteps the model is evaluated at, strictly descending (dn_ddim_sched_check validates
 * a host copy).  table: device fp32 [n_steps, DN_GD_COLS], the rows of the respaced diffusion's dn_gaussian_step table IN CHAIN ORDER:
 * row i belongs to steps[i], i.e. to respaced index n_steps-1-i, so the LAST row is respaced index 0.  A chain that starts part-way
 * passes the tail of both.  The update of row i is dn_gaussian_step's on eps = Model(x, steps[i]), bit for bit:
 *   x0 = sqrt_recip_abar x - sqrt_recipm1_abar eps [clamped to +-1 when clip_denoised]
 *   sampler 0, p_sample (:376-417):     x <- coef1 x0 + coef2 x + 1[i != n_steps-1] exp(0.5 log_var) z
 *   sampler 1, ddim_sample (:513-560):  e = (sqrt_recip_abar x - x0) / sqrt_recipm1_abar,
 *       sigma = eta sqrt((1-abar_prev)/(1-abar)) sqrt(1-abar/abar_prev),
 *       x <- x0 sqrt(abar_prev) + sqrt(1-abar_prev-sigma^2) e + 1[i != n_steps-1] sigma z
 * The noise switch is the respaced index (t != 0 of :404-407, :551-554), not the timestep's value: the last row adds none even where
 * steps[n_steps-1] != 0 (a use_timesteps without 0).
 * z: injected -- noise fp32 [n_steps, B*T*latent], row i for update i, 16-byte aligned -- or, noise == NULL, Philox4x32-10 keyed by
 * `seed` with the counter (element quad of the whole batch, i), as dn_ddim_sched_loop draws: eager, graph replay and the two
 * half-batch streams agree bit for bit.  dn_gaussian_loop_keyed: z of element (b, frame, channel) at update i is dn_randn_keyed's
 * stream 2 + steps[i] under keys[b] (device uint64 [B], 8-byte aligned) -- the ORIGINAL timestep, so a draw depends on (key, timestep,
 * frame, channel) only: not on the respacing's other members, the row, B, the padded T, the half batch, graph or eager.
 * Chain state, conditioning table (n_steps rows), hipGraph replay and the two half-batch streams as dn_ddim_sched_loop; flags:
 * DN_LOOP_GRAPH | DN_LOOP_SPLIT2.  The captured step is cached under the sampler, clip_denoised and the bits of eta besides what
 * every loop keys: it never serves the other sampler, another eta or another clip, nor another loop.  Workspace:
 * dn_gaussian_workspace_bytes (= dn_ddim_sched_workspace_bytes).  Unconditional model only; eta finite and >= 0; the latent width a
 * multiple of 4.  Every argument check precedes the first HIP call.  Returns the number of model evaluations (= n_steps) or a
 * negative error.
 * dn_gaussian_sched_step is the update alone on n (a multiple of 4) contiguous fp32 elements, x / eps / noise 16-byte aligned: row
 * *step_index (device int32) of table, z from `seed` (counter: element quad, step index) or the injected `noise` [n] of THIS step;
 * dn_gaussian_sched_step_keyed the keyed update alone on dense x / eps [B, T, Z] (Z a multiple of 4), for host-stepped chains.     */
size_t dn_gaussian_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t n_steps);
int dn_gaussian_loop(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* table,
                     int32_t n_steps, int32_t timesteps, int32_t sampler, int32_t clip_denoised, float eta, uint64_t seed,
                     const float* noise, int32_t flags, void* workspace, size_t workspace_bytes, void* stream);
int dn_gaussian_loop_keyed(DnEps* m, float* x, const int32_t* lengths, int32_t B, int32_t T, const int32_t* steps, const float* table,
                           int32_t n_steps, int32_t timesteps, int32_t sampler, int32_t clip_denoised, float eta, const uint64_t* keys,
                           int32_t flags, void* workspace, size_t workspace_bytes, void* stream);
int dn_gaussian_sched_step(float* x, const float* eps, int64_t n, const float* table, const int32_t* step_index, int32_t n_steps,
                           int32_t sampler, int32_t clip_denoised, float eta, uint64_t seed, const float* noise, void* stream);
int dn_gaussian_sched_step_keyed(float* x, const float* eps, const uint64_t* keys, int32_t B, int32_t T, int32_t Z, const float* table,
                                 const int32_t* steps, const int32_t* step_index, int32_t n_steps, int32_t sampler, int32_t clip_denoised,
                                 float eta, void* stream);

/* The prompted, classifier-free-guided chain over a timestep schedule, as a device loop: dn_ddim_sched_loop's chain -- steps, coef,
 * the level x enters at, the target of every update, eta_on / seed / noise [n_steps, B*T*latent] and the Philox key (seed, step
 * index, element quad of the B-row batch) are its arguments with its meaning, dn_ddim_sched_check validates the schedule's host
 * copy -- with the guided prediction of forward_with_cond_scale (latent_module.py:813-826) in place of the unconditional one:
 * cond_scale == 1: one conditioned pass over B rows; otherwise one pass over 2B rows [conditioned ; null] (the drop mask is per
 * sample, :843-859) combined as dn_cfg_combine combines them, null + (cond - null) * cond_scale.  prompt fp32 [B, Tp, dim_prompt],
 * prompt_lengths int32 [B]; needs a model created with cfg.dim_prompt > 0.
 * The entry owns, in the caller's workspace: the doubled lengths / prompt / prompt lengths and the drop mask [0..0 ; 1..1] of the
 * 2B-row pass, the 2B-row model input and prediction, a step-index vector and the loop's device counter (step indices, upwards),
 * copies of steps and coef, and a time table of n_steps rows (dn_eps_cond_time_table_steps: row i for e_i) -- all written at chain
 * start by device-to-device copies and kernels on the stream; no allocation, no synchronisation.  One step: fill the index vector
 * from the counter, dn_eps_forward_cond_ex (the chain's first step computes the prompt-only work, every later one passes
 * DN_COND_REUSE_PROMPT), ONE kernel that forms the guided eps, applies dn_ddim_sched_loop's update to x and writes the result to
 * both halves of the model's next input, and the counter's increment.  flags: DN_LOOP_GRAPH only (n_steps > 2: the first step runs
 * eagerly, the later form of the step is captured once and replayed; the graph is cached in a slot of its own, keyed by B, T, Tp,
 * n_steps, workspace, x, lengths, prompt, prompt_lengths, the bits of cond_scale, flags, eta_on, seed, the coefficient copy's
 * address and the run-time options' generation; an injected-noise chain is never cached).  DN_LOOP_SPLIT2 is refused: the
 * prompt-only state lives in one workspace and the guided pass already runs 2B rows.  Every argument check precedes the first HIP
 * call.  Workspace: dn_guided_ddim_workspace_bytes (guided = cond_scale != 1; the guided = 0 size is the smaller one and leaves
 * out every second half).  Returns the number of model evaluations (= n_steps) or a negative error.                            */
size_t dn_guided_ddim_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t Tp, int32_t n_steps, int32_t guided);
int dn_guided_ddim_loop(DnEps* m, float* x, const int32_t* lengths, const float* prompt, const int32_t* prompt_lengths, int32_t B, int32_t T,
                        int32_t Tp, float cond_scale, const int32_t* steps, const float* coef, int32_t n_steps, int32_t timesteps,
                        int32_t eta_on, uint64_t seed, const float* noise, int32_t flags, void* workspace, size_t workspace_bytes,
                        void* stream);

/* dn_guided_ddim_loop (latent_module.py:813-826, diffusion/gaussian_diffusion.py:513-560) with eta on and keyed per-step noise, as
 * dn_ddim_sched_loop_keyed draws it: stream 2 + e_i of keys[b] (device uint64 [B], 8-byte aligned) for the B-row latent, so a
 * scale-1 chain draws what dn_ddim_sched_loop_keyed draws.  `keys` stands where the twin takes eta_on, seed and noise; its address
 * is part of the guided slot's graph key (seed 0).  Null or misaligned keys and a latent width that is no multiple of 4 are refused
 * before anything is written; everything else as dn_guided_ddim_loop.                                                          */
int dn_guided_ddim_loop_keyed(DnEps* m, float* x, const int32_t* lengths, const float* prompt, const int32_t* prompt_lengths, int32_t B,
                              int32_t T, int32_t Tp, float cond_scale, const int32_t* steps, const float* coef, int32_t n_steps,
                              int32_t timesteps, const uint64_t* keys, int32_t flags, void* workspace, size_t workspace_bytes,
                              void* stream);

/* DPM-Solver++(2M) for the prompted, classifier-free-guided chain, as a device loop (Lu et al. 2022, "DPM-Solver++", the
 * data-prediction multistep solver, eq. 11-12 / algorithm 2): dn_guided_ddim_loop's chain -- the same steps, the level x enters at,
 * the target of every update, the guided prediction of forward_with_cond_scale (latent_module.py:813-826) over B or 2B rows, the
 * same workspace state and the same step sequence -- with dn_dpm_loop's second-order deterministic update in place of DDIM's.
 * coef: device fp32 [n_steps, DN_DPM_COLS], the rows of dn_dpm_loop (scheduler.dpm_schedule).  One step: fill the index vector from
 * the counter, dn_eps_forward_cond_ex, ONE kernel that forms the guided eps as dn_cfg_combine forms it, applies dn_dpm2m_step's
 * update statement for statement to x, keeps x0_i in `hist` and writes the result to both halves of the model's next input, and the
 * counter's increment.  hist (B T latent fp32) lives in the workspace and is read only by a second-order row; row 0 is first order, so
 * a chain never reads what an earlier call left there.  No noise is drawn: there is no eta, seed or noise argument.
 * flags: DN_LOOP_GRAPH only (n_steps > 2 on a non-null stream: the first step runs eagerly, the later form of the step is captured
 * once and replayed).  The graph shares dn_guided_ddim_loop's cache slot under a key bit of its own: a DDIM step is never replayed for
 * this loop nor the other way round, on whatever workspace, x, prompt and n_steps.  DN_LOOP_SPLIT2 is refused.  Every argument check
 * precedes the first HIP call; dn_ddim_sched_check validates a host copy of the steps.
 * Workspace: dn_guided_dpm_workspace_bytes = dn_guided_ddim_loop's layout with hist beside the prediction and DN_DPM_COLS columns in
 * the coefficient copy (>= dn_guided_ddim_workspace_bytes + B T latent fp32).  Returns the number of model evaluations (= n_steps) or
 * a negative error.                                                                                                              */
size_t dn_guided_dpm_workspace_bytes(const DnEps* m, int32_t B, int32_t T, int32_t Tp, int32_t n_steps, int32_t guided);
int dn_guided_dpm_loop(DnEps* m, float* x, const int32_t* lengths, const float* prompt, const int32_t* prompt_lengths, int32_t B, int32_t T,
                       int32_t Tp, float cond_scale, const int32_t* steps, const float* coef, int32_t n_steps, int32_t timesteps,
                       int32_t flags, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ VAE training step (BASELINE config 4) */
/* speech_vae_decoder_loss training (reference SpeechVAEEncoderDecoder.forward latent_module.py:1118-1142 + the criterion
 * fairseq/criterions/speech_vae_decoder_loss.py:45-95) on flat buffers in the PACKED parameter layout (csrc/engine.h: rows
 * padded to 128, K to 64, GEGLU interleave, conv taps as matrices; transformer tensors layer-major; zero pads stay zero under
 * Adam without weight decay):
 *   master fp32 [n]  what dn_adam_step updates          work [n] in cfg.dtype  (bf16: dn_adam_step's bf16 copy; f32: == master)
 *   grads  fp32 [n]  dn_vae_train_backward ADDS into it  aux  bytes            transposed matrices + summed skip biases,
 *                                                                              rebuilt by dn_vae_train_refresh after an update
 * diffnorm_amd/packing.py::pack_vae_train converts a state dict in the reference layout to / from this layout. */
typedef struct DnVaeTrain DnVaeTrain;
typedef struct {
  const float* feat;        /* [B, T, dim] fp32 target features (also the encoder input)                               */
  const int32_t* units;     /* [B, T] dictionary indices (unit + 4), 0 = pad                                           */
  const int32_t* lengths;   /* [B]                                                                                     */
  const float* noise;       /* [B, T, z] posterior noise (distributions.py:38-40 draws it on the CPU generator)        */
  int32_t B, T;
  int32_t ntokens;          /* sample["ntokens"] = sum of lengths                                                      */
  float w_lsce, w_mse, w_kl; /* criterion weights: 0.1, 10, 1e-4 (speech_vae_decoder_loss.py:80-83)                     */
  float label_smoothing;    /* 0.1                                                                                     */
  float loss_scale;         /* multiplies every gradient (1 normally)                                                   */
  float* stats;             /* fp32 [8] out: loss, nll_loss, mse_loss, kl_loss, acc, n_valid, lsce/ntokens, 0            */
  float* logits_out;        /* optional fp32 [B, T, vocab]                                                             */
  float* recon_out;         /* optional fp32 [B, T, dim]                                                               */
  const float* ext_dlogits; /* backward only, optional fp32 [B, T, vocab]: d loss / d logits supplied by the caller (a criterion
                               that differentiates the logits itself) instead of the fused LS-CE gradient; w_mse / w_kl are
                               then d loss / d mse_loss and d loss / d kl_loss                                          */
  float attn_dropout;       /* dropout on the attention probabilities (latent_module.py:338,668: 0.1 in train mode, 0 in eval) */
  uint32_t dropout_seed_lo, dropout_seed_hi; /* the mask is a counter hash of (seed, layer, batch, head, query, key): forward and
                               backward of one step must be given the same seed; change it every update                    */
  int32_t pad_;
} DnVaeTrainBatch;

int dn_vae_train_create(const DnVaeConfig* cfg, DnVaeTrain** out);
void dn_vae_train_destroy(DnVaeTrain* m);
int64_t dn_vae_train_param_count(const DnVaeTrain* m);   /* n: elements of master / work / grads                       */
size_t dn_vae_train_aux_bytes(const DnVaeTrain* m);
/* element offsets of the packed tensors in table order (2 * n_wave * 10 + 10 * depth + 4 entries); returns the count   */
int dn_vae_train_offsets(const DnVaeTrain* m, int64_t* offsets, int32_t capacity);
/* [offset, offset + count) of the gradient buffer that backward stage `stage` completes                               */
int dn_vae_train_stage_range(const DnVaeTrain* m, int32_t stage, int64_t* offset, int64_t* count);
int dn_vae_train_bind(DnVaeTrain* m, float* master, void* work, void* aux, float* grads);  /* 256-byte aligned buffers   */
int dn_vae_train_refresh(DnVaeTrain* m, void* stream);
size_t dn_vae_train_workspace_bytes(const DnVaeTrain* m, int32_t B, int32_t T);
/* forward + losses; every activation the backward needs stays in the workspace                                          */
int dn_vae_train_forward(DnVaeTrain* m, const DnVaeTrainBatch* batch, void* workspace, size_t workspace_bytes, void* stream);
/* backward stages first_stage .. last_stage of the step dn_vae_train_forward just ran on this workspace: 0 = loss gradients +
 * decoder_lm + to_pred, 1 .. depth = transformer layers depth-1 .. 0, depth+1 = decoder WaveNets + posterior, depth+2 =
 * encoder WaveNets.  Gradient ranges complete in reverse parameter order (dn_vae_train_stage_range), so the caller can start
 * the all-reduce of a finished range while later stages still run.                                                       */
int dn_vae_train_backward(DnVaeTrain* m, const DnVaeTrainBatch* batch, int32_t first_stage, int32_t last_stage, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ mask-predict update */
/* The per-iteration update of the CMLM decoder downstream of the normalised units (fairseq/models/nat/cmlm_transformer.py:88-134,
 * called from the loop of fairseq/iterative_refinement_generator.py:200-230): positions holding `unk` (the mask symbol) take
 * argmax / max of log_softmax(logits); `predicted` receives the tokens at that point; then, unless step + 1 == max_step, the
 * trunc((n_nonpad - 2) * (1 - (step + 1) / max_step)) lowest-scoring positions are re-masked (_skeptical_unmasking :19-25; equal
 * scores ordered by position).  logits fp32 [B, T, V]; tokens int32 [B, T] and scores fp32 [B, T] updated in place.  T <= 2048.  */
int dn_cmlm_step(const float* logits, int32_t* tokens, float* scores, int32_t* predicted, int32_t B, int32_t T, int32_t V, int32_t step,
                 int32_t max_step, int32_t unk, int32_t pad, void* stream);
/* The same update with the iteration index read from the DEVICE (int32 *step_dev): one refinement iteration of the loop of
 * fairseq/iterative_refinement_generator.py:200-230 -- dn_nar_decoder_forward + this -- can then be captured into a hipGraph once and
 * replayed while a device counter advances (diffnorm_amd/nar_decoder.py).                                                         */
int dn_cmlm_step_dev(const float* logits, int32_t* tokens, float* scores, int32_t* predicted, int32_t B, int32_t T, int32_t V,
                     const int32_t* step_dev, int32_t max_step, int32_t unk, int32_t pad, void* stream);

/* ------------------------------------------------------------------ diffusion training step */
/* LatentDiscreteModel.forward (latent_module.py:1514-1613; criterion fairseq/criterions/ddpm_discrete_loss.py:37-75) for the
 * eps-predictor `Model`, with the frozen VAE (diff_discrete.py:70-85) as a bound DnVaeTrain whose decoder only passes data
 * gradients.  Flat packed buffers / stages / refresh exactly as for the VAE engine above; the conditioning path (time MLP and
 * the FiLM / adaptive-norm projections) is stored and differentiated in fp32 in every mode.  The caller supplies what the
 * reference draws or looks up on the host: t, the posterior sample z of the frozen encoder (dn_vae_encode_params +
 * dn_posterior_sample), the beta_0 jitter, the target noise, the fp32 schedule tables and min(snr, 5) / snr per sample.   */
typedef struct DnEpsTrain DnEpsTrain;
typedef struct {
  const float* feat;        /* [B, T, dim_feat] target features (multitask reconstruction loss), may be NULL without multitask */
  const int32_t* units;     /* [B, T] dictionary indices, 0 = pad                                                         */
  const int32_t* lengths;   /* [B]                                                                                        */
  const float* z;           /* [B, T, latent] posterior sample of the frozen VAE encoder (:1530)                          */
  const float* jitter;      /* [B, T, latent]  x1 = z + jitter * beta0 (:1534-1536)                                       */
  const float* true_noise;  /* [B, T, latent]                                                                             */
  const int32_t* times;     /* [B] in [1, timesteps)                                                                      */
  const float* sqrt_ac;     /* fp32 [timesteps] sqrt(alphas_cumprod)                                                      */
  const float* sqrt_1mac;   /* fp32 [timesteps] sqrt(1 - alphas_cumprod)                                                  */
  const float* snr_weight;  /* fp32 [B]: min(snr_t, 5) / snr_t (:1565-1569)                                               */
  float beta0;
  int32_t B, T;
  int32_t n_units;          /* number of non-pad units (the LS-CE divisor, :1594)                                         */
  int32_t n_frames;         /* number of valid frames (the masked recon MSE counts n_frames * dim_feat elements)          */
  int32_t timesteps, multitask;
  float label_smoothing;    /* 0.1 */
  float recon_weight;       /* 50  */
  float loss_scale;
  float* stats;             /* fp32 [8] out: total_loss, nll_loss, recon_mse_loss, noise_loss, acc, n_units, 0, 0          */
  float* eps_out;           /* optional fp32 [B, T, latent]: the predicted noise                                          */
  float attn_dropout;       /* as in DnVaeTrainBatch; applies to the eps-predictor only: the frozen VAE runs in eval mode (:1530) */
  uint32_t dropout_seed_lo, dropout_seed_hi;
  int32_t pad_;
} DnEpsTrainBatch;

int dn_eps_train_create(const DnEpsConfig* cfg, DnEpsTrain** out);
void dn_eps_train_destroy(DnEpsTrain* m);
int64_t dn_eps_train_param_count(const DnEpsTrain* m);
size_t dn_eps_train_aux_bytes(const DnEpsTrain* m);
int dn_eps_train_offsets(const DnEpsTrain* m, int64_t* offsets, int32_t capacity);  /* 21 + 8 * depth entries */
int dn_eps_train_stage_range(const DnEpsTrain* m, int32_t stage, int64_t* offset, int64_t* count);
/* pos_table: fp32 [max_pos + 1, padk(dim)] sinusoidal table (row 0 zeros), a constant of the model                      */
int dn_eps_train_bind(DnEpsTrain* m, float* master, void* work, void* aux, float* grads, const float* pos_table);
int dn_eps_train_refresh(DnEpsTrain* m, void* stream);
size_t dn_eps_train_workspace_bytes(const DnEpsTrain* m, const DnVaeTrain* vae, int32_t B, int32_t T);
int dn_eps_train_forward(DnEpsTrain* m, DnVaeTrain* vae, const DnEpsTrainBatch* batch, void* workspace, size_t workspace_bytes, void* stream);
/* stages: 0 = loss gradients + frozen VAE decoder + final_proj + to_pred, 1 .. depth = transformer layers depth-1 .. 0,
 * depth+1 = WaveNet + init_conv, depth+2 = the conditioning path                                                         */
int dn_eps_train_backward(DnEpsTrain* m, DnVaeTrain* vae, const DnEpsTrainBatch* batch, int32_t first_stage, int32_t last_stage,
                          void* workspace, size_t workspace_bytes, void* stream);

const char* dn_last_error(void);
int dn_version(void);

/* Run-time options (process-wide; no reference counterpart: the reference has no such switches).  Each option starts from the
 * environment variable named beside it, read once when the library first looks, and is changed afterwards only through this entry
 * (the library never re-reads the environment per launch and callers never have to mutate it).  DN_OPTION_DEFAULT restores the
 * start value.  Names: "taps_inner" (DN_TAPS_INNER: K order of a causal conv's taps -- 0 term-outer everywhere, 1 tap-inner on
 * the 256-row tiles [default], 2 tap contractions routed to those tiles by SHAPE whatever the batch size: a batch and its shards
 * then agree bit for bit), "fuse_norm" (DN_FUSE_NORM), "no_split_norm" (DN_NO_SPLIT_NORM), "kblock" (DN_KBLOCK: 0 never / 1 always
 * K-blocked operands), "wgrad_stream", "wgrad_tn", "wgrad_groups" (DN_WGRAD_*: A/B switches of the weight-gradient path),
 * "wgrad_tn_x3" (DN_WGRAD_TN_X3: DN_BF16X3 weight gradients from the row-major split rows; "wgrad_tn" is the 2-byte modes only),
 * "ffn_fold" (DN_FFN_FOLD: sampling engines with folded weights attached -- 0 the FFN's causal conv and output projection as two
 * contractions [the default of DN_BF16 engines]; one folded contraction: 5 [the default otherwise] on the tile run_transformer's
 * route rule picks, 1 on the tile the route table chooses (term-outer; 128 x 128 at [32,512]), 2 / 3 / 4 forced to the 256 x 128 / 256 x 256 / 256 x 128 shared-row
 * tile (4 where that tile applies: 2-byte types, split norm, "taps_inner" not 0); like every option it is part of the captured-step cache keys through the option generation).
 * "nar_cg_fold" (DN_NAR_CG_FOLD: the guided NAR decoder pass -- 1 [default] the null half's encoder attention as the addition of
 * the constant row c_l, 0 evaluated literally; it changes the option generation like every option).
 * dn_get_option: *is_set = 0 when the option is neither set nor in the environment (the library's built-in choice applies). */
#define DN_OPTION_DEFAULT (-2147483647 - 1)
int dn_set_option(const char* name, int32_t value);
int dn_get_option(const char* name, int32_t* value, int32_t* is_set);

/* Classifier-free guidance (Model.forward_with_cond_scale, latent_module.py:813-826) over ONE pass of twice the batch: `both` fp32
 * [2, n] = the conditioned predictions followed by the null-conditioned ones -> out[i] = null + (cond - null) * scale.           */
int dn_cfg_combine(const float* both, float scale, int64_t n, float* out, void* stream);

/* ------------------------------------------------------------------ the model inside the mask-predict loop */
/* The DECODER side of the reference's NAR S2UT model NARS2UTTransformerModel (research/TranSpeech/nar_transformer.py:569-976; task
 * speech_to_speech_fasttranslate, fairseq/tasks/nat_s2s_task.py:107-127), which the research IterativeRefinementGenerator drives
 * (research/TranSpeech/iterative_refinement_generator.py:131-160).  The speech encoder is out of scope: its output is a given
 * tensor.  Packed tensors (diffnorm_amd/nar_decoder.py::pack_nar; matrices [rows -> 128][K] in cfg.dtype, biases / norms fp32):
 *   emb fp32 [V, D]   pos fp32 [max_pos, D] (sinusoidal, row `pad` zero)   len_W fp32 [256, D] (embed_length.weight)
 *   per layer, stacked: qkv_W [3D] + qkv_b (q ; k ; v of self_attn), so_W / so_b (out_proj), cq_W / cq_b (encoder_attn.q_proj),
 *   ckv_W [2D] / ckv_b (encoder_attn k ; v), co_W / co_b, fc1_W [F] / fc1_b, fc2_W / fc2_b, ln_g / ln_b [3, D] (self_attn_layer_norm,
 *   encoder_attn_layer_norm, final_layer_norm);  fin_g / fin_b (decoder.layer_norm);  out_W [V -> 128-row multiple, D].      */
typedef struct DnNar DnNar;
typedef struct {
  int32_t dim, ffn, layers, heads, vocab, max_pos, pad, dtype;
} DnNarConfig;
int dn_nar_create(const DnNarConfig* cfg, const void* const* weights, int32_t n_weights, DnNar** out);
void dn_nar_destroy(DnNar* m);
size_t dn_nar_workspace_bytes(const DnNar* m, int32_t B, int32_t T, int32_t S);
size_t dn_nar_cross_kv_bytes(const DnNar* m, int32_t B, int32_t S);
/* Keys / values of every layer's encoder attention (fairseq/modules/transformer_layer.py:455-470), which depend on the encoder
 * output only: enc_out fp32 [B, S, D] (batch-major) -> ckv [layers][B*S][k(D) ; v(D)] in cfg.dtype (fp32 for DN_BF16X3), computed
 * once per utterance batch and reused by every refinement iteration.                                                        */
int dn_nar_cross_kv(DnNar* m, const float* enc_out, int32_t B, int32_t S, void* ckv, void* workspace, size_t workspace_bytes, void* stream);
/* forward_length + forward_length_prediction (nar_transformer.py:436-480, no offset): masked mean of the encoder output over the
 * src_lengths[b] valid frames -> embed_length projection (fp32) -> arg-max.  lengths int32 [B].                              */
int dn_nar_predict_lengths(DnNar* m, const float* enc_out, const int32_t* src_lengths, int32_t B, int32_t S, int32_t* lengths,
                           void* workspace, size_t workspace_bytes, void* stream);
/* TransformerUnitDecoder.forward (nar_transformer.py:321-420, inference): tokens int32 [B, T] (`pad` after each row's tokens) ->
 * logits fp32 [B, T, vocab]; dn_cmlm_step turns them into the mask-predict update of forward_decoder (:791-842).            */
int dn_nar_decoder_forward(DnNar* m, const int32_t* tokens, const void* ckv, const int32_t* src_lengths, int32_t B, int32_t T, int32_t S,
                           float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ classifier-free guidance of the same decoder (nar_cg) */
/* The reference's `nar_cg` evaluation (scripts/s2ut/eval_cg.sh -> research/TranSpeech/nat_gen.py --cg_scale) runs the decoder twice
 * in every iteration of its mask-predict loop (nat_gen.py:196-236): TransformerUnitDecoder.forward on the speech encoder's output and
 * TransformerUnitDecoder.cg_forward (nar_transformer.py:123-183) on a "dropped" source -- every source position of every row replaced
 * by e_null = embed_tokens.weight[bos] (:144-149, the raw row: no sqrt(D) scale, no position) and the padding mask cleared
 * (:152-156).  All S keys / values of a layer are then equal, the softmax is uniform and the encoder attention of EVERY query is
 *   c_l = W_o,l (W_v,l e_null + b_v,l) + b_o,l          l = 0 .. layers - 1,
 * independent of the query, of S and of the batch: in the pre-norm layer (fairseq/modules/transformer_layer.py:447-470) the whole
 * block -- encoder_attn_layer_norm, q_proj, attention, out_proj -- is the broadcast addition of c_l.  Not in the reference; against
 * the literal evaluation it differs by the rounding of sum_S (1/S) v only.
 *
 * dn_nar_null_cross forms the fp32 [layers][dim] table of c_l on the device in the engine's arithmetic: emb[null_token] through the
 * packed ckv_W (v rows) / ckv_b and co_W / co_b with the operand roundings of dn_nar_cross_kv and of the attention output.  `buffer`
 * (256-byte aligned, dn_nar_null_cross_bytes) is the caller's, like the packed tensors: the engine keeps reading the table at its
 * start, so it stays allocated and untouched while guided passes run; the rest is scratch of this call.  Once per engine and token,
 * never per iteration.  dn_nar_null_table: the table's device address (NULL before the first call).                              */
size_t dn_nar_null_cross_bytes(const DnNar* m);
int dn_nar_null_cross(DnNar* m, int32_t null_token, void* buffer, size_t buffer_bytes, void* stream);
const float* dn_nar_null_table(const DnNar* m);
/* The two decoder passes of one iteration (nat_gen.py:209-222) as ONE pass over 2 B rows: embedding, self-attention, FFN, final
 * LayerNorm and output projection on all 2 B T rows; encoder attention on the first B T rows; the rows of the second half receive
 * + c_l.  tokens / ckv / src_lengths as dn_nar_decoder_forward -> logits2 fp32 [2, B, T, vocab], conditioned then null.  Refused
 * before dn_nar_null_cross.  Option "nar_cg_fold" (DN_NAR_CG_FOLD, default 1): 0 evaluates the null half's encoder attention
 * literally -- dn_nar_cross_kv on B S copies of e_null, every source length S, formed in the workspace by every pass -- the
 * on-device check of the fold and the A/B leg of tools/nar_cg_bench.py, not a tuned path.  No allocation, no synchronisation.     */
size_t dn_nar_guided_workspace_bytes(const DnNar* m, int32_t B, int32_t T, int32_t S);
int dn_nar_decoder_forward_guided(DnNar* m, const int32_t* tokens, const void* ckv, const int32_t* src_lengths, int32_t B, int32_t T, int32_t S,
                                  float* logits2, void* workspace, size_t workspace_bytes, void* stream);
/* The update of nat_gen.py:197-236 on logits2 fp32 [2, B, T, V] in one kernel.  Unlike forward_decoder's (dn_cmlm_step), the scores
 * START FROM ZERO in every iteration (:197; `scores` is written, never read); positions holding `unk` take arg-max / max of
 * log_softmax(cond + scale * (cond - null)) (:223-229); `predicted` receives the tokens at that point; unless step + 1 == max_step
 * the trunc((n_nonpad - 2) * (1 - (step + 1) / max_step)) lowest-scoring positions are re-masked and their scores zeroed (:230-236,
 * _skeptical_unmasking; equal scores ordered by position, as dn_cmlm_step).  Each logit row is read once; the scaled logits are never
 * written.  T <= 2048; scale <= 0 is refused (nat_gen.py:180,225: that loop is dn_cmlm_step over one pass, scores zeroed first).
 * _dev: the iteration index is read from the device, for a captured iteration.                                                */
int dn_cmlm_guided_step(const float* logits2, float scale, int32_t* tokens, float* scores, int32_t* predicted, int32_t B, int32_t T,
                        int32_t V, int32_t step, int32_t max_step, int32_t unk, int32_t pad, void* stream);
int dn_cmlm_guided_step_dev(const float* logits2, float scale, int32_t* tokens, float* scores, int32_t* predicted, int32_t B, int32_t T,
                            int32_t V, const int32_t* step_dev, int32_t max_step, int32_t unk, int32_t pad, void* stream);

/* ------------------------------------------------------------------ the speech encoder of the same model */
/* S2STransformerEncoder (research/TranSpeech/nar_transformer.py:40-76; no speaker embedding) = S2TTransformerEncoder._forward
 * (fairseq/models/speech_to_text/s2t_transformer.py:345-373): Conv1dSubsampler (two Conv1d(kernel, stride 2, padding kernel / 2) + GLU,
 * fairseq/models/speech_to_text/modules/convolution.py:13-57) -> sqrt(dim) scaling + sinusoidal positions of the padding mask -> `layers`
 * pre-norm TransformerEncoderLayers (fairseq/modules/transformer_layer.py:163-226) -> LayerNorm.  Packed tensors
 * (diffnorm_amd/nar_decoder.py::pack_nar_encoder; matrices [rows -> 128][K] in cfg.dtype, biases / norms / positions fp32):
 *   0 conv0_W [conv_channels][padk(kernel * input_dim)] (column j * input_dim + c = weight[o][c][j])   1 conv0_b
 *   2 conv1_W [2 dim][kernel * conv_channels / 2]   3 conv1_b   4 positions [max_pos][dim] (row `pad` zero)
 *   5 qkv_W [layers][3 dim][dim] (q ; k ; v)   6 qkv_b   7 so_W   8 so_b   9 fc1_W   10 fc1_b   11 fc2_W   12 fc2_b
 *   13 ln_g [layers][2][dim] (self_attn_layer_norm ; final_layer_norm)   14 ln_b   15 fin_g   16 fin_b                      */
typedef struct DnNarEnc DnNarEnc;
typedef struct {
  int32_t input_dim, conv_channels, kernel, dim, ffn, layers, heads, max_pos, pad, dtype;
} DnNarEncConfig;
int dn_nar_encoder_create(const DnNarEncConfig* cfg, const void* const* weights, int32_t n_weights, DnNarEnc** out);
void dn_nar_encoder_destroy(DnNarEnc* m);
int32_t dn_nar_encoder_out_frames(int32_t L); /* frames after the two stride-2 layers: floor((L - 1) / 2) + 1, twice */
size_t dn_nar_encoder_workspace_bytes(const DnNarEnc* m, int32_t B, int32_t L);
/* feats fp32 [B, L, input_dim] (zero-padded behind each utterance, as the collater leaves them; the whole padded batch is convolved,
 * like upstream), src_lengths int32 [B] -> enc_out fp32 [B, S, dim] (BATCH-major; upstream returns [S, B, dim]), out_lengths int32 [B]
 * (Conv1dSubsampler.get_out_seq_lens_tensor: the key-padding mask of the layers and of the decoder's encoder attention).          */
int dn_nar_encoder_forward(DnNarEnc* m, const float* feats, const int32_t* src_lengths, int32_t B, int32_t L, float* enc_out,
                           int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ the Conformer speech encoder of the recipe's model */
/* Key-masked multi-head self-attention with Transformer-XL relative positions, flash-style (csrc/rel_attention.hip).  Replaces
 * RelPositionMultiHeadedAttention.forward (fairseq/modules/espnet_multihead_attention.py:109-196; rel_shift :120-145, zero_triu False)
 * between linear_q / linear_k / linear_v / linear_pos and linear_out, and the [B, H, T, 2T - 1] matrix_bd it builds:
 *   score[i, j] = ((q_i + u_h) . k_j + (q_i + v_h) . pos[pos_zero_row + i - j]_h) * scale,  keys j >= lengths[b] masked,  out = softmax V.
 * q, k, v, out as DnAttnParams' (row m = b*T + t, head h at columns [h*dh, (h+1)*dh)); dtype is the element type of q, k, v, pos and
 * out, except DN_BF16X3: q, k, v, pos plain fp32 (what dn_conv_gemm stores beside its split rows), out in split rows, arithmetic
 * the fp32 form.  DN_F16 / DN_BF16: 2-byte MFMA operands, fp32 accumulation and softmax, q + u and q + v formed in fp32 and rounded
 * once.  dim_head 16, 32 or 64; T >= 1; every lengths[b] in [1, T] (an empty sequence has no softmax: callers refuse it).  No
 * buffer of size O(T^2) exists in any mode.  A sequence's result depends on nothing but its own rows, lengths[b] and T.        */
typedef struct {
  const void* q; const void* k; const void* v; void* out;
  int32_t ldq, ldk, ldv, ldo;
  int32_t B, T, heads, dim_head;
  int32_t dtype;
  int32_t ldp;             /* row stride of pos */
  const int32_t* lengths;  /* [B] or NULL (no mask) */
  float scale;             /* dim_head ** -0.5 */
  int32_t pos_zero_row;    /* the row of pos that holds offset 0: offset d = i - j is row pos_zero_row + d, so one table built for the
                              longest T serves every shorter batch; rows pos_zero_row - (T-1) .. pos_zero_row + (T-1) must exist
                              (refused otherwise, see pos_rows)                                                                   */
  const void* pos;         /* linear_pos(pe): one row per offset, head h at columns [h*dh, (h+1)*dh) */
  const float* bias_u;     /* pos_bias_u fp32 [heads, dim_head] */
  const float* bias_v;     /* pos_bias_v fp32 [heads, dim_head] */
  int32_t pos_rows;        /* rows of pos: pos_zero_row - (T-1) >= 0 and pos_zero_row + (T-1) < pos_rows are checked on the host */
  int32_t pad_;
} DnRelAttnParams;
int dn_rel_attention(const DnRelAttnParams* p, void* stream);

/* The middle of the Conformer convolution module in one pass (ConvolutionModule.forward, fairseq/modules/conformer_layer.py:77-99: glu,
 * depthwise_conv, batch_norm in eval mode, activation):
 *   out[b,t,c] = swish(sum_j w[c][j] * glu(x)[b, t + j - k/2, c] + shift[c]),   glu(x)[..,c] = x[..,c] * sigmoid(x[.., C + c]),
 * taps outside [0, S) zero; NO length mask, as upstream.  x [B*S, 2C] in `dtype` (fp32 in DN_BF16X3), w fp32 [C, k] and shift fp32 [C]
 * with the BatchNorm folded in by the host (w * gamma / sqrt(var + eps), beta - mean * gamma / sqrt(var + eps)); fp32 accumulation;
 * out [B*S, C] in `dtype` (split rows in DN_BF16X3).  k odd, <= 63; C a multiple of 64.                                          */
int dn_glu_dwconv(const void* x, const float* w, const float* shift, void* out, int32_t B, int32_t S, int32_t C, int32_t k, int32_t dtype,
                  void* stream);

/* S2SConformerEncoder (research/TranSpeech/nar_conformer.py:42-74; no speaker embedding) = S2TConformerEncoder._forward
 * (fairseq/models/speech_to_text/s2t_conformer.py:91-137), eval mode, attn_type espnet + pos_enc_type rel_pos: Conv1dSubsampler ->
 * sqrt(dim) scaling -> linear -> `layers` ConformerEncoderLayers (fairseq/modules/conformer_layer.py:229-284); no final LayerNorm.
 * Packed tensors (diffnorm_amd/nar_decoder.py::pack_conformer_encoder; matrices [rows -> 128][K] in cfg.dtype, the rest fp32):
 *   0 conv0_W  1 conv0_b  2 conv1_W  3 conv1_b (as dn_nar_encoder_create)   4 linear_W [dim][dim]  5 linear_b
 *   6 pe [2 max_frames - 1][dim] in cfg.dtype as an A operand (split rows in DN_BF16X3): RelPositionalEncoding's table
 *     (fairseq/modules/positional_encoding.py:94-112), offset d at row max_frames - 1 + d
 *   7 ffn1.w_1 [layers][ffn][dim]  8 its bias  9 0.5 * ffn1.w_2 [layers][dim][ffn]  10 0.5 * its bias   11-14 ffn2 likewise
 *   15 qkv_W [layers][3 dim][dim] (linear_q ; linear_k ; linear_v)  16 qkv_b  17 linear_pos_W [layers][dim][dim]
 *   18 linear_out_W  19 linear_out_b  20 pos_bias_u [layers][dim]  21 pos_bias_v
 *   22 pointwise_conv1_W [layers][2 dim][dim]  23 depthwise w [layers][dim][depthwise_kernel] and 24 shift [layers][dim], BatchNorm folded
 *   25 pointwise_conv2_W [layers][dim][dim]  26 ln_g [layers][5][dim] (ffn1 ; self_attn ; conv_module ; ffn2 ; final)  27 ln_b
 *   28 zeros [2 dim] (the bias of the bias-free projections)
 * linear_pos(pe) of a layer is formed inside the forward, in front of that layer's attention, into one workspace buffer.           */
typedef struct DnConformerEnc DnConformerEnc;
typedef struct {
  int32_t input_dim, conv_channels, kernel, dim, ffn, layers, heads, depthwise_kernel;
  int32_t max_frames; /* the longest S (frames after the subsampler) the packed position table serves */
  int32_t dtype;
} DnConformerEncConfig;
int dn_conformer_encoder_create(const DnConformerEncConfig* cfg, const void* const* weights, int32_t n_weights, DnConformerEnc** out);
void dn_conformer_encoder_destroy(DnConformerEnc* m);
size_t dn_conformer_encoder_workspace_bytes(const DnConformerEnc* m, int32_t B, int32_t L);
/* As dn_nar_encoder_forward: feats fp32 [B, L, input_dim], src_lengths int32 [B] -> enc_out fp32 [B, S, dim] batch-major (S =
 * dn_nar_encoder_out_frames(L)), out_lengths int32 [B].  Every one of the B * S rows is computed: the convolution module is not
 * masked upstream, so an utterance's output depends on how far its batch is padded, here as there; only attention keys are masked. */
int dn_conformer_encoder_forward(DnConformerEnc* m, const float* feats, const int32_t* src_lengths, int32_t B, int32_t L, float* enc_out,
                                 int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ CodeHiFiGAN unit vocoder: units -> waveform, batched */
/* CodeHiFiGANVocoder.forward (fairseq/models/text_to_speech/vocoder.py:214-235) = CodeGenerator (codehifigan.py) over the HiFiGAN
 * Generator (hifigan.py) with the duration predictor (fastspeech2.py:117-151), single-speaker, no f0.  Kernels: csrc/vocoder.hip.
 *
 * The conv operator.  Activations are channels-last fp32 [B, Lmax, C] with per-sequence lengths[B]:
 *   out[b,t,co] = post(bias[co] + sum_{j<k} sum_ci pre(x[b, t + (j - (k-1)/2) d, ci]) W[co,j,ci])      for t < lengths[b],
 * frames outside [0, lengths[b]) read as ZEROS (the reference's per-utterance zero padding), frames >= lengths[b] of `out` untouched.
 * pre = leaky ReLU of slope `slope` (1 = none, 0 = ReLU), computed in fp32 and rounded once to the operand type.  k odd, C_in a
 * multiple of 16 (of 128 beyond 128), (k - 1) / 2 * d <= 25 at 128 staged channels.  dtype DN_F32 or DN_F16 (half operands, fp32
 * accumulation); DN_BF16 / DN_BF16X3 are refused.  W: [ceil16(C_out)][row] in the operand type, a row holding per pass of
 * CK = min(C_in, 128) input channels the k * CK weights in (tap, channel) order, zero-padded to 32 elements in DN_F16
 * (diffnorm_amd/vocoder.py::pack_conv_weight; dn_voc_conv_weight_elems = the element count).  Tiles are counted from frame 0 of each
 * sequence: a frame's result does not depend on the batch, the row or Lmax.                                                     */
enum { DN_VOC_POST_NONE = 0, DN_VOC_POST_RES = 1, DN_VOC_POST_RES_ACC = 2, DN_VOC_POST_RELU = 3, DN_VOC_POST_TANH = 4 };
/* POST_RES: (acc + bias + res) / div.  POST_RES_ACC: (acc + bias + res + out's previous value) / div -- the sum over the ResBlocks
 * of a stage, div = their number on the last one and 1 before.  res may alias out.                                              */
typedef struct {
  const float* x;
  const void* W;
  const float* bias; /* fp32 [C_out] or NULL */
  const float* res;  /* fp32 [B, Lmax, ldr], POST_RES / POST_RES_ACC */
  float* out;        /* fp32 [B, Lmax, ldo] */
  const int32_t* lengths;
  int32_t B, Lmax, C_in, C_out, k, d, ldx, ldo, ldr, dtype, post;
  float slope, div;
} DnVocConvParams;
int dn_voc_conv(const DnVocConvParams* p, void* stream);
int dn_voc_conv_tile(int32_t dtype, int32_t C_in, int32_t C_out, int32_t k); /* frames per time tile, or DN_EINVAL */
int64_t dn_voc_conv_weight_elems(int32_t dtype, int32_t C_in, int32_t C_out, int32_t k); /* 0: unsupported shape */

#define DN_VOC_MAX_UPS 8
#define DN_VOC_MAX_KERNELS 4
typedef struct DnVoc DnVoc;
typedef struct {
  int32_t embedding_dim, num_embeddings, initial_channel, n_ups;
  int32_t up_rates[DN_VOC_MAX_UPS], up_kernels[DN_VOC_MAX_UPS];
  int32_t n_kernels, res_kernels[DN_VOC_MAX_KERNELS], res_dilations[DN_VOC_MAX_KERNELS][3];
  int32_t dur_hidden; /* var_pred_hidden_dim, 0 = no duration predictor */
  int32_t dtype;
} DnVocConfig;
/* Packed tensors (diffnorm_amd/vocoder.py::pack_vocoder; conv weights as above, biases / norms fp32):
 *   dict fp32 [V, E];  conv_pre W, b;  per stage: the transposed conv as a 3-tap conv C -> u * C / 2 (polyphase repack: output frame
 *   s u + r reads input frames s - 1, s, s + 1; needs k - u even and k <= 3 u, refused otherwise) W, b (repeated per phase), then per
 *   ResBlock and pair c1 W, b, c2 W, b;  conv_post W, b;  with a predictor (always DN_F32): conv1 W, b, ln1 g, b, conv2 W, b, ln2 g, b,
 *   proj w [H], b [1].                                                                                                        */
int dn_voc_create(const DnVocConfig* cfg, const void* const* weights, int32_t n_weights, DnVoc** out);
void dn_voc_destroy(DnVoc* m);
int32_t dn_voc_upsample(const DnVoc* m); /* samples per frame: the product of the rates */
size_t dn_voc_workspace_bytes(const DnVoc* m, int32_t B, int32_t Lmax0);
/* VariancePredictor in fp32 whatever the engine's dtype: codes int32 [B, Tmax] (valid: 0 <= code < V), lengths int32 [B] ->
 * durations int32 [B, Tmax] = max(round_half_even(exp(logd) - 1), 1) (0 behind a row's units) and sums int32 [B].  Workspace:
 * dn_voc_workspace_bytes(m, B, Tmax).                                                                                          */
int dn_voc_durations(DnVoc* m, const int32_t* codes, const int32_t* lengths, int32_t B, int32_t Tmax, int32_t* durations, int32_t* sums,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Units -> waveform.  durations NULL: one frame per unit.  Lmax0 = the longest row's frame count (the caller reads `sums` back once
 * per batch to size `wav`: the only synchronisation; a row with more frames is cut at Lmax0).  wav fp32 [B, Lmax0 * upsample],
 * wav_lengths int32 [B]; samples behind a row's length are not written.  Workspace: dn_voc_workspace_bytes(m, B, max(Lmax0, Tmax)). */
int dn_voc_forward(DnVoc* m, const int32_t* codes, const int32_t* lengths, const int32_t* durations, int32_t B, int32_t Tmax, int32_t Lmax0,
                   float* wav, int32_t* wav_lengths, void* workspace, size_t workspace_bytes, void* stream);
/* Stage timing of dn_voc_forward (tools/vocoder_bench.py): events recorded between the stages while switched on; dn_voc_stage_times
 * waits for the last profiled forward and returns n_ups + 2 values in ms: embedding + conv_pre, each stage, conv_post.            */
int dn_voc_set_profile(DnVoc* m, int32_t on);
int dn_voc_stage_times(DnVoc* m, float* ms, int32_t cap);

/* ------------------------------------------------------------------ mHuBERT front end: waveform -> layer features -> k-means units */
/* The reader of the recipe's feature dump (scripts/prepare/feature_dump.sh -> examples/textless_nlp/gslm/speech2unit/pretrained/
 * hubert_feature_reader.py): HubertModel.extract_features(source, padding_mask=None, mask=False, output_layer=k)
 * (fairseq/models/hubert/hubert.py:429-476, 529-545), eval mode, one utterance at a time.  A batch here gives every utterance what it
 * would get ALONE (the reader never batches; the reference's batched padding-mask path is not what this reproduces): a result depends
 * on the utterance's own samples and length only, not on B, the row or L.  Kernels and the pass: csrc/hubert.hip.  Supported form
 * (mHuBERT-base): extractor_mode "default", conv_bias False, layer_norm_first False, layer_type "transformer",
 * required_seq_len_multiple 1, task normalize False; every conv layer of the same width. The large form (wav2vec 2.0 / HuBERT
 * large, and the Wav2VecCtc recognisers of the recipe's ASR-BLEU) is the same engine with the DnHubertConfig fields behind
 * has_proj set; all of them zero is the base form, bit for bit.  The two forms are accepted as wholes (the ones released
 * checkpoints have and the goldens pin): extractor_ln and pre_norm go together, conv_bias and wave_norm only with them; any other
 * mix is refused at create.  required_seq_len_multiple needs no field: the frames it appends are masked keys that are cut off
 * again (wav2vec2.py:1027-1037, 1063-1065), so nothing is computed for it.
 *
 * Grouped Conv1d with 'same' zero padding of k / 2 frames in front and SamePad's trim behind (an even k drops the last frame;
 * make_conv_pos, fairseq/models/wav2vec/wav2vec2.py:899-915), then GELU and the residual add (TransformerEncoder.extract_features,
 * wav2vec2.py:1020-1022):
 *   out[b,t,g Cg + co] = x[b,t,g Cg + co] + gelu_erf(bias[g Cg + co] + sum_{j<k} sum_{ci<Cg} w[g][j][ci][co] x[b, t + j - k/2, g Cg + ci])
 * for t < lengths[b]; frames outside [0, lengths[b]) read as ZEROS (what a lone utterance's padding gives) and rows t >= lengths[b] of
 * out are written as zeros.  x, out fp32 [B, T, C]; w fp32 [groups][k][Cg][Cg] with the weight-norm folded in by the host; fp32 FMA
 * accumulation over (tap, channel) in that order whatever the engine's dtype.  One workgroup owns a frame tile of one group and stages
 * the tile's rows plus the k - 1 halo once in LDS for all taps; tiles are counted from frame 0 of each sequence.  Cg a multiple of 4,
 * <= 64; k <= 128.                                                                                                             */
int dn_grouped_conv1d(const float* x, const float* w, const float* bias, float* out, const int32_t* lengths, int32_t B, int32_t T, int32_t C,
                      int32_t groups, int32_t k, void* stream);

/* units[m] = argmax_j (x_m . c_j - |c_j|^2 / 2): the arg-min of |x|^2 - 2 x . c + |c|^2 of
 * examples/hubert/simple_kmeans/dump_km_label.py:38-53 (ApplyKmeans) and of the recipe's quantize_with_kmeans.py (sklearn predict);
 * ties go to the lowest index.  feats fp32 [M, D]; centroids: the packed fp32 matrix [n -> multiple of 128][D] (zero rows behind the
 * table) and half_norm fp32 [n -> multiple of 4] = -|c_j|^2 / 2 computed by the host in float64 (any value in the pad entries: they
 * are not compared).  Always the DN_F32 contraction (fp32 MFMA), whatever arithmetic the engine in front runs in: a unit is a
 * decision.  One contraction with half_norm as the bias, then dn_argmax_units' row arg-max.  D a multiple of 32; workspace:
 * dn_kmeans_workspace_bytes(M, n).                                                                                           */
size_t dn_kmeans_workspace_bytes(int32_t M, int32_t n_centroids);
int dn_kmeans_assign(const float* feats, const float* centroids, const float* half_norm, int32_t M, int32_t D, int32_t n_centroids,
                     int32_t* units, void* workspace, size_t workspace_bytes, void* stream);

/* Learning that codebook: one step of sklearn.cluster.MiniBatchKMeans (cluster_kmeans.py / learn_kmeans.py of the reference) is
 * dn_kmeans_assign -> dn_kmeans_accumulate -> dn_kmeans_update (diffnorm_amd/csrc/kmeans.hip).  D a multiple of 32 (<= 4096),
 * n <= 8192; feats, centers, sums 16-byte aligned; every workspace is dn_kmeans_workspace_bytes_train(M, n), 256-byte aligned.
 *
 * dn_kmeans_accumulate: sums[j][:] = sum of the rows with labels[m] == j (double [n, D]), counts[j] their number, inertia[0] =
 * sum_m |x_m - c_labels[m]|^2 from the differences, in double.  centers: the packed fp32 matrix dn_kmeans_assign reads (row stride D).
 * A stable counting sort of the row indices by label, then one wave per (cluster, 256 columns) adds that cluster's rows in ascending
 * row index: no floating-point atomics, the same bits on every call and for every M; an empty cluster gets count 0 and sums 0.  A
 * label outside [0, n) is never used as an index: its row is left out (callers check labels they did not get from dn_kmeans_assign).
 *
 * dn_kmeans_update: for every cluster with counts[j] > 0, c_j <- (c_j w_j + sums[j]) / (w_j + counts[j]) in double, rounded once to
 * fp32, w_j += counts[j] (weight_sums double [n]), half_norm[j] <- -|c_j|^2 / 2 of the rounded centre, in double, rounded once.  The
 * other clusters keep their bits.
 *
 * dn_kmeans_min_dist (k-means++ seeding): d2[m][j] = |x_m - cands[j]|^2 (differences, double accumulation, rounded once to fp32) for
 * k <= 16 candidates (cands fp32 [k, D]); pot[j] = sum_m min(mind2[m], d2[m][j]) in double, summed in a fixed order; commit >= 0
 * also stores mind2[m] <- min(mind2[m], d2[m][commit]) (commit -1: mind2 is only read).                                          */
size_t dn_kmeans_workspace_bytes_train(int32_t M, int32_t n_clusters);
int dn_kmeans_accumulate(const float* feats, const int32_t* labels, const float* centers, int32_t M, int32_t D, int32_t n_clusters, double* sums,
                         int32_t* counts, double* inertia, void* workspace, size_t workspace_bytes, void* stream);
int dn_kmeans_update(float* centers, float* half_norm, double* weight_sums, const double* sums, const int32_t* counts, int32_t n_clusters, int32_t D,
                     void* stream);
int dn_kmeans_min_dist(const float* feats, int32_t M, int32_t D, const float* cands, int32_t k, int32_t commit, float* mind2, double* pot,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Packed tensors (diffnorm_amd/hubert.py::pack_hubert; matrices [rows -> 128][K] in cfg.dtype, everything else fp32):
 *   0 conv0_w fp32 [16][C] (tap j of channel c at [j][c], zero rows behind the kernel)   1 GroupNorm gamma [C]   2 beta [C]
 *   3 .. n_conv + 1: conv layer i >= 1 as [C][k_i C], column j C + c = weight[o][c][j]
 *   then: layer_norm g, b [C] (HubertModel.layer_norm)   post_extract_proj W [dim][C], b
 *   pos_conv w fp32 [groups][k][Cg][Cg] (weight-norm folded: g v / |v| over dim 2, float64 on the host), bias [dim]
 *   encoder.layer_norm g, b   qkv_W [layers][3 dim][dim] (q ; k ; v), qkv_b   out_W, out_b   fc1_W, fc1_b   fc2_W, fc2_b
 *   ln_g [layers][2][dim] (self_attn_layer_norm ; final_layer_norm), ln_b   zeros [C] (the bias of the bias-free convs)
 *   extractor_ln: conv bias [n_conv][C] (read when conv_bias), conv LayerNorm g [n_conv][C], b [n_conv][C] (entries 1, 2 are not read)
 *   vocab > 0: proj W fp32 [vocab -> 128][dim], b [vocab -> multiple of 4]                                                                    */
#define DN_HUBERT_MAX_CONV 8
typedef struct DnHubert DnHubert;
typedef struct {
  int32_t n_conv, conv_dim;
  int32_t conv_kernel[DN_HUBERT_MAX_CONV], conv_stride[DN_HUBERT_MAX_CONV];
  int32_t dim, ffn, layers, heads, conv_pos, conv_pos_groups, dtype;
  int32_t has_proj; /* 0: no post_extract_proj (conv_dim == dim, hubert.py:264-268); its two table entries are then not read */
  int32_t wave_norm;    /* task normalize: F.layer_norm(wave, wave.shape) per utterance over its own samples (eps 1e-5), applied where
                           the first conv stages its samples: mean, then squared deviations from it, per-tile partials combined in order */
  int32_t extractor_ln; /* extractor_mode "layer_norm": Conv1d (+ bias) -> Fp32LayerNorm over the channels of a frame -> GELU behind
                           every conv (wav2vec2.py:849-859); conv_dim <= 512 */
  int32_t conv_bias;    /* with extractor_ln only (HuBERT large has none) */
  int32_t pre_norm;     /* layer_norm_first: x += attn(LN1(x)); x += fc2(gelu(fc1(LN2(x)))), no encoder.layer_norm in front; it follows
                           the last layer in dn_hubert_ctc_forward only (TransformerEncoder.forward, layer None, wav2vec2.py:1001-1007) */
  int32_t vocab;        /* > 0: the CTC head Linear(dim -> vocab) of Wav2VecEncoder (wav2vec2_asr.py:494-495); with pre_norm only */
} DnHubertConfig;
int dn_hubert_create(const DnHubertConfig* cfg, const void* const* weights, int32_t n_weights, DnHubert** out);
void dn_hubert_destroy(DnHubert* m);
/* frames of L samples behind the conv stack: floor((len - k) / stride) + 1 per layer (Wav2Vec2Model._get_feat_extract_output_lengths,
 * wav2vec2.py:564-579); 0 when L is too short for one frame                                                                  */
int32_t dn_hubert_out_frames(const DnHubert* m, int32_t L);
size_t dn_hubert_workspace_bytes(const DnHubert* m, int32_t B, int32_t L);
/* wave fp32 [B, L] (any finite values behind an utterance's samples), lengths int32 [B] (each long enough for one frame: the caller
 * checks; a shorter one yields no valid row) -> out fp32 [B, S, dim], S = dn_hubert_out_frames(m, L), the output of transformer layer
 * n_layers_run - 1 (output_layer = n_layers_run: TransformerEncoder.extract_features breaks at tgt_layer, wav2vec2.py:1045-1055);
 * rows at or past out_lengths[b] are written as zeros.  Refused before anything is launched: L shorter than one frame, n_layers_run
 * outside [1, layers], and any (B, L) for which a buffer would pass 2^31 - 1 elements (the kernels index rows in 32 bits).  No
 * allocation and no synchronisation inside.                                                                                  */
int dn_hubert_forward(DnHubert* m, const float* wave, const int32_t* lengths, int32_t B, int32_t L, int32_t n_layers_run, float* out,
                      int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream);
/* Stage timing of dn_hubert_forward (tools/hubert_bench.py): events recorded between the stages while switched on;
 * dn_hubert_stage_times waits for the last profiled forward and returns DN_HUBERT_STAGES values in ms: first conv + GroupNorm,
 * conv layers 1.., layer_norm + post_extract_proj + positional conv, the transformer layers, the masked copy of the output.    */
#define DN_HUBERT_STAGES 5
int dn_hubert_set_profile(DnHubert* m, int32_t on);
int dn_hubert_stage_times(DnHubert* m, float* ms, int32_t cap);

/* Wav2VecEncoder.forward in eval mode (wav2vec2_asr.py:473-501; research/TranSpeech/asr_bleu/utils.py:262-266): every layer,
 * encoder.layer_norm in the pre-norm form, then the head: emissions fp32 [B, S, vocab] = proj(x), rows at or past out_lengths[b]
 * zeros.  The head is always the DN_F32 contraction on the fp32 stream (a letter is a decision, as a unit is in
 * dn_kmeans_assign); it writes its pad columns (vocab -> multiple of 4) into the workspace; they never reach `emissions`.
 * Arguments, refusals and workspace as dn_hubert_forward; the engine must have been created with vocab > 0.  The fifth profiled
 * stage is then final norm + head + emission copy. */
int dn_hubert_ctc_forward(DnHubert* m, const float* wave, const int32_t* lengths, int32_t B, int32_t L, float* emissions, int32_t* out_lengths,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Best-path CTC decoding (what the recipe's beam-1, lexicon-free, LM-free decoder keeps): tok[t] = the arg-max of frame t (the lowest
 * index on ties); frame t is kept iff tok[t] != blank and (t == 0 or tok[t] != tok[t - 1]); the kept tokens in order ->
 * tokens_out[b, :counts_out[b]] (int32 [B, S]; entries behind the count are not written).  emissions fp32 [B, S, V]; frames at and
 * behind lengths[b] are never read.  One launch for the batch, a workgroup per utterance, any S.                              */
int dn_ctc_greedy(const float* emissions, const int32_t* lengths, int32_t B, int32_t S, int32_t V, int32_t blank, int32_t* tokens_out,
                  int32_t* counts_out, void* stream);

/* ------------------------------------------------------------------ Kaldi fbank + utterance CMVN: waveform -> S2UT source features */
/* The first box of the S2UT leg: get_fbank (fairseq/data/audio/audio_utils.py:242-277), i.e. torchaudio.compliance.kaldi.fbank(waveform,
 * num_mel_bins=80, sample_frequency=sr) at its defaults with dither 0 (the deterministic torchaudio form; pyKaldi's own default adds
 * random dither 1.0), then UtteranceCMVN.__call__ (fairseq/data/audio/feature_transforms/utterance_cmvn.py:30-41), which
 * examples/speech_to_speech/preprocessing/prep_s2ut_data.py:73 puts in every S2UT config.  Kernels: csrc/fbank.hip.
 *   frames    snip_edges: m = 1 + (n - frame_length) / frame_shift for n >= frame_length, else 0; frame i = x[i shift, i shift + length)
 *   per frame subtract the frame's mean (remove_dc_offset) -> f[j] -= preemphasis f[j - 1] with f[-1] := f[0] -> Povey window
 *             (0.5 - 0.5 cos(2 pi j / (length - 1)))^0.85 -> zero-pad to n_fft -> |rfft|^2 -> n_mels triangular filters in the mel
 *             domain (mel(f) = 1127 ln(1 + f / 700), n_mels + 2 equally spaced points from low_freq to high_freq, Nyquist bin weight 0)
 *             -> log(max(energy, FLT_EPSILON))
 *   CMVN      per utterance and column over its own frames: mean, var = E[x^2] - mean^2, y = (x - mean) / sqrt(max(var, 1e-10))
 * All arithmetic fp32 (the CMVN sums in double); a result depends on the utterance's own samples and length only, not on B, L, the row
 * or the neighbours, and no sample at or behind lengths[b] is read.  Refused (-1 with dn_last_error): n_fft other than 256 / 512 /
 * 1024 or below frame_length, frame_shift outside [1, frame_length], n_mels outside [1, 128], low_freq < 0, high_freq above Nyquist
 * or not above low_freq (0 = Nyquist).  The rest of torchaudio's signature (dither, use_energy, htk_compat, vtln, other windows,
 * snip_edges False, subtract_mean) has no field here: diffnorm_amd/fbank.py refuses it by name.                                 */
typedef struct DnFbank DnFbank;
typedef struct {
  float sample_rate;
  int32_t n_mels, frame_length, frame_shift, n_fft; /* the last three in samples; n_fft >= frame_length */
  float low_freq, high_freq;                        /* Hz; high_freq 0 = Nyquist */
  float preemphasis;
  int32_t remove_dc_offset;
  float input_scale;             /* samples are multiplied by it: 1.0 for int16-scale input (what the reference feeds), 32768.0 for [-1, 1] */
  int32_t norm_means, norm_vars; /* the two halves of UtteranceCMVN */
  int32_t cmvn;                  /* 0: the raw log-mel energies are the output */
} DnFbankConfig;
/* The one place the tables are computed (host code, no GPU needed), in double, rounded once: window fp32 [frame_length], mel fp32
 * [n_mels][n_fft / 2 + 1] (torchaudio's get_mel_banks with a zero Nyquist column; at most two non-zero weights per bin).          */
int dn_fbank_tables(const DnFbankConfig* cfg, float* window, float* mel);
/* tw fp32 [n_fft / 2][2] = (cos, -sin)(2 pi k / n_fft): the transform's twiddle factors, in double, rounded once (host code). */
int dn_fbank_twiddles(int32_t n_fft, float* tw);
/* tables: device pointers to { window, mel, twiddles }, each a verbatim copy of what the two functions above filled FOR THIS cfg (they
 * must outlive the handle).  The handle derives each filter's non-zero bin range from cfg by the code that fills the mel table and
 * never reads the tables on the host: a mel table from anywhere else is summed over the wrong bins -- it is not a way to bring
 * other filters.                                                                                                              */
int dn_fbank_create(const DnFbankConfig* cfg, const void* const* tables, int32_t n_tables, DnFbank** out);
void dn_fbank_destroy(DnFbank* m);
/* frames of L samples (0 when L < frame_length) */
int32_t dn_fbank_out_frames(const DnFbank* m, int32_t L);
size_t dn_fbank_workspace_bytes(const DnFbank* m, int32_t B, int32_t L);
/* wave fp32 [B, L] (anything, NaN included, at and behind an utterance's samples), lengths int32 [B] on the device (samples; clamped to
 * [0, L]) -> out fp32 [B, Lf, n_mels], Lf = dn_fbank_out_frames(m, L), out_lengths int32 [B]; rows at or behind out_lengths[b] are
 * written as zeros.  An utterance shorter than one frame (or empty) is a handled case: out_lengths[b] = 0, zero rows, return 0.
 * Stream-ordered, no allocation, no synchronisation with the host: it can be captured in a graph.  workspace: 256-byte aligned,
 * dn_fbank_workspace_bytes(m, B, L); every argument is checked before the first launch (a refused call has written nothing). */
int dn_fbank_forward(DnFbank* m, const float* wave, const int32_t* lengths, int32_t B, int32_t L, float* out, int32_t* out_lengths,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ sample-rate conversion in front of the three waveform front ends */
/* What the reference's loaders do before a model sees audio: torchaudio.functional.resample(waveform, sample_rate, 16000) in the ASR
 * loader (examples/speech_to_speech/asr_bleu/utils.py:231-237; research/TranSpeech/asr_bleu/utils.py:237) and the `to_mono` step of
 * convert_waveform (fairseq/data/audio/audio_utils.py:22-72: the mean over the channels).  The filter is torchaudio's windowed-sinc
 * polyphase bank, stated in diffnorm_amd/resample.py (resample_tables), which is where it is computed: in float64, rounded once.
 * With orig and new divided by their gcd, width = ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff)), K = 2 width + orig:
 *   out[b, i * new + p] = sum_{k < K} bank[p][k] * x_b[i * orig + k - width],  x_b = 0 outside [0, lengths[b]),
 * for i * new + p < out_length(lengths[b]) = ceil(new * lengths[b] / orig).  The sum runs over k in ascending order as fp32 FMAs from
 * zero on every path and in every tile: an utterance's output depends on its own samples and length only, not on B, L, the row or
 * the neighbours.  Kernel: csrc/resample.hip.                                                                                   */
#define DN_I16 16 /* a SAMPLE FORMAT of dn_resample_forward's input (16-bit PCM, scaled by 2^-15 in the load); no arithmetic mode */
typedef struct DnResample DnResample;
typedef struct {
  int32_t orig, new_;       /* the rates divided by their gcd, both >= 1 */
  int32_t width, K;         /* as above; K = 2 width + orig */
  int32_t force_global;     /* != 0: read the bank from global memory even where it fits in LDS (the two paths give identical bits) */
} DnResampleConfig;
/* tables: device pointers to { bank fp32 [new][K], the same bank transposed fp32 [K][new] } (they must outlive the handle).  The
 * bank is staged in LDS beside the input span when new * (K | 1) <= 8192 floats (32 KiB beside a span of at most 32 KiB); a larger
 * bank (441 : 160, 441 : 320) is read from the transposed copy in global memory, lanes on consecutive phases.  Refused: a
 * configuration whose one-frame span K (+ 1 / 32 skew) exceeds the 8192 staged floats.  (torchaudio.functional.resample's
 * _get_sinc_resample_kernel, which asr_bleu/utils.py:231-237 reaches, is the table's definition.)                                */
int dn_resample_create(const DnResampleConfig* cfg, const void* const* tables, int32_t n_tables, DnResample** out);
void dn_resample_destroy(DnResample* m);
/* ceil(new * L / orig) in 64-bit arithmetic (torchaudio's target_length, reached from asr_bleu/utils.py:231-237); 0 for L <= 0 */
int64_t dn_resample_out_length(const DnResample* m, int64_t L);
/* output samples per workgroup tile: frames_per_tile * new, about 1024 (the geometry the tests name their edges from; no reference
 * counterpart, the reference's resampler is one conv1d call)                                                                   */
int32_t dn_resample_tile(const DnResample* m);
/* 0: the forward needs no workspace; the entry exists for the engines' common calling pattern (asr_bleu/utils.py:231-237 has none) */
size_t dn_resample_workspace_bytes(const DnResample* m, int32_t B, int32_t L);
/* in: [B, L, channels] interleaved samples, in_dtype DN_F32 or DN_I16 (anything, NaN included, at and behind an utterance's samples:
 * they are never read); a sample is converted (int16 * 2^-15, exact) and the channels are summed in fp32 in channel order and divided
 * by their count as part of the load (convert_waveform's to_mono, audio_utils.py:49-50; channels 1: the sample itself).
 * lengths int32 [B] on the device (clamped to [0, L]) -> out fp32 [B, Lo], Lo = dn_resample_out_length(m, L), zeros at and behind
 * out_lengths[b] = dn_resample_out_length(m, lengths[b]), which is written on the device.  An empty utterance is a handled case.
 * Stream-ordered, no allocation, no synchronisation with the host.  Replaces torchaudio.functional.resample at
 * asr_bleu/utils.py:231-237.  Every argument is checked before the launch (a refused call has written nothing).                  */
int dn_resample_forward(DnResample* m, const void* in, int32_t in_dtype, int32_t channels, const int32_t* lengths, int32_t B, int32_t L, float* out,
                        int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ scores over integer sequences: edit distance, run-length reduction */
/* What says how good a result is: the share of units normalisation changed, and the word / character error rate of a vocoder -> ASR
 * loop.  Both are a unit-cost Levenshtein distance (substitution, insertion, deletion cost 1 each) over integer sequences; units are
 * compared after run-length de-duplication.  Replaces the `editdistance.eval(hyp_words, ref_words)` calls of fairseq's WER scorer
 * (fairseq/scoring/wer.py:50-58) and the reference's own one-thread-per-pair kernel's role (fairseq/clib/libnat_cuda), and the
 * per-utterance Python loop of diff_norm_synthesis.py:25-46 (reduce_token).  Kernels: csrc/metrics.hip, written for gfx950: one
 * wavefront per pair, the shorter sequence's columns in per-lane register strips, rows skewed one step per lane, the strip boundary
 * handed on by a DPP wave shift; pairs whose shorter side exceeds 2048 tokens are swept in panels of 2048 columns with the panel's
 * last column in the workspace.  Integer arithmetic, no atomics: bit-identical between calls and independent of B, of the pair's
 * position and of lda / ldb.                                                                                                      */
#define DN_EDIT_DISTANCE_MAX_LEN 8192
/* bytes dn_edit_distance needs for B pairs with rows of max_len_a / max_len_b tokens (0 for arguments it would refuse) */
size_t dn_edit_distance_workspace_bytes(int32_t B, int32_t max_len_a, int32_t max_len_b);
/* a int32 [B, lda], b int32 [B, ldb], a_len / b_len int32 [B] on the device (clamped to [0, lda] / [0, ldb]; elements at or behind a
 * length are never read) -> dist int32 [B]: dist[i] = Levenshtein(a[i, :a_len[i]], b[i, :b_len[i]]); an empty side gives the other
 * side's length.  lda, ldb in 1 .. DN_EDIT_DISTANCE_MAX_LEN (refused beyond).  panel_cols: 0 = the kernel's own (2048); otherwise a
 * multiple of 64 up to 2048: the columns of a panel, so that the workspace path can be run on short pairs (the results are the
 * same numbers).  workspace: 4-byte aligned, dn_edit_distance_workspace_bytes(B, lda, ldb).  Stream-ordered, no allocation, no
 * synchronisation with the host; every argument is checked before the launch.                                                   */
int dn_edit_distance(const int32_t* a, int32_t lda, const int32_t* a_len, const int32_t* b, int32_t ldb, const int32_t* b_len, int32_t B,
                     int32_t* dist, int32_t panel_cols, void* workspace, size_t workspace_bytes, void* stream);
/* Batched run-length de-duplication, the device form of reduce_token (diff_norm_synthesis.py:25-46): units int32 [B, ld], lengths
 * int32 [B] (clamped to [0, ld]) -> reduced int32 [B, ld]: row b holds its runs' values in order, zeros at and behind
 * reduced_len[b]; reduced_len int32 [B]; durations int32 [B, ld]: the runs' lengths; first int32 [B, ld]: the index of each run's
 * first frame (both zero behind reduced_len[b]; either may be null).  One pass, one wavefront per row, no atomics; the outputs must
 * not alias the input.                                                                                                            */
int dn_reduce_units(const int32_t* units, const int32_t* lengths, int32_t B, int32_t ld, int32_t* reduced, int32_t* reduced_len,
                    int32_t* durations, int32_t* first, void* stream);

/* ------------------------------------------------------------------ scores over integer sequences: BLEU's clipped n-gram statistics */
/* The two headline scores of the recipe are BLEU: of the decoded units (research/utils/unit_bleu.py:91,106) and of the re-transcribed
 * speech (research/TranSpeech/asr_bleu/compute_asr_bleu.py:153).  What belongs on the device are the per-pair statistics over integer
 * ids that fairseq's own scorer defines (fairseq/clib/libbleu/libbleu.cpp:73-109,138-156: bleu_addngram / bleu_add), the integers a
 * single-reference corpus BLEU sums: the two lengths and, for n = 1 .. DN_BLEU_ORDER,
 *   count_n = max(hyp_len - n + 1, 0)                                  the hypothesis's n-grams
 *   match_n = sum over distinct n-grams g of min(count_hyp(g), count_ref(g))   how many of them the reference covers (clipped)
 * The score over them (fairseq/scoring/bleu.py:132-151) is closed-form host arithmetic over the summed integers: diffnorm_amd/metrics.py.
 * Kernel: csrc/bleu.hip, one workgroup per pair: both rows in LDS, ONE bitonic sort of the hyp_len + ref_len start positions by their
 * 4-token key (full lexicographic comparison of the tokens as signed integers, a below-everything mark where a row has ended), after
 * which the equal n-grams of every order are contiguous; one pass of run boundaries and per-run hypothesis / reference counts serves
 * the four orders.  Exact for any int32 token values (only equality matters), no hash, no floating point, no atomics: bit-identical
 * between calls and independent of B, of the pair's position, of ld_hyp / ld_ref and of what lies behind the lengths.               */
#define DN_BLEU_ORDER 4
#define DN_BLEU_STATS 10 /* hyp_len, ref_len, match1, count1, ..., match4, count4 */
/* bytes dn_bleu_stats needs (0 for arguments it would refuse).  Every pair up to 8192 + 8192 tokens is sorted in LDS, so this is a
 * token size; the entry exists for the common calling pattern                                                                    */
size_t dn_bleu_stats_workspace_bytes(int32_t B, int32_t ld_hyp, int32_t ld_ref);
/* hyp int32 [B, ld_hyp], ref int32 [B, ld_ref], hyp_len / ref_len int32 [B] on the device (clamped to [0, ld_hyp] / [0, ld_ref];
 * elements at or behind a length are never read) -> stats int32 [B, DN_BLEU_STATS]: row i = the clamped hyp_len, ref_len, then
 * match_n, count_n for n = 1 .. 4 of the pair (hyp[i, :hyp_len[i]], ref[i, :ref_len[i]]); an empty side gives zero matches.
 * ld_hyp, ld_ref in 1 .. DN_EDIT_DISTANCE_MAX_LEN (refused beyond).  workspace: non-null, dn_bleu_stats_workspace_bytes(B, ld_hyp,
 * ld_ref) bytes, not touched.  Stream-ordered, no allocation, no synchronisation with the host; every argument is checked before the
 * launch.  Replaces bleu_add (libbleu.cpp:138-156) per pair, without its trimming of pad / eos and without its hash.               */
int dn_bleu_stats(const int32_t* hyp, int32_t ld_hyp, const int32_t* hyp_len, const int32_t* ref, int32_t ld_ref, const int32_t* ref_len, int32_t B,
                  int32_t* stats, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFNORM_HIP_H */
