// Host-side orchestration of the DiffNorm hot path on top of the op-level C ABI: sub-model
// descriptors (WaveNet, conditionable transformer), the workspace bump allocator and its check, the
// engines' stage timer, and the packed weight order shared with diffnorm_amd/packing.py.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/diffnorm_hip.h"
#include "common.h"

namespace dn {

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline int padk(int c) { return round_up(c, 64); }    // channel width as a K dimension / row stride
inline int padn(int c) { return round_up(c, 128); }   // packed weight rows

inline const void* eoff(const void* p, size_t elems, int es) { return static_cast<const char*>(p) + elems * es; }
inline void* eoff(void* p, size_t elems, int es) { return static_cast<char*>(p) + elems * es; }
inline int esize(int dtype) { return dtype == DN_BF16 || dtype == DN_F16 ? 2 : 4; }
// DN_BF16X3: tensors that are read by an epilogue or by the attention kernel rather than staged as a contraction operand stay
// plain fp32 (the WaveNet block's residual branch, q / k / v)
inline int side_dtype(int dtype) { return dtype == DN_BF16X3 ? DN_F32 : dtype; }
// blocks of 256 threads of a grid-stride element-wise kernel over n > 0 items
inline int ew_grid(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : b);
}

#define DN_TRY(expr)          \
  do {                        \
    int rc__ = (expr);        \
    if (rc__ != DN_OK) return rc__; \
  } while (0)

inline DnGemmParams gemm_base(int dtype, int M, int N, int K, int T, int32_t flags = 0) {
  DnGemmParams p;
  memset(&p, 0, sizeof(p));
  p.flags = flags;
  p.dtype = dtype;
  p.M = M; p.N = N; p.K = K; p.T = T;
  p.groups = 1;
  p.n_terms = 1;
  p.epilogue = DN_EPI_BIAS;
  p.out_dtype = dtype;
  p.res_dtype = dtype == DN_BF16X3 ? DN_F32 : dtype;  // (an epilogue's residual input is never split rows)
  return p;
}

struct Arena {  // bump allocator over the caller's workspace; base == nullptr only measures
  char* base;
  size_t off, cap;
  void* take(size_t bytes) {
    size_t a = (off + 255) & ~size_t(255);
    off = a + bytes;
    if (!base) return reinterpret_cast<void*>(a + 256);  // non-null dummy while measuring
    return off <= cap ? base + a : nullptr;
  }
};

// After the plan: the caller's workspace is aligned and holds what the plan took.  `hint` (the function that sizes the workspace)
// follows the message in brackets.
inline int check_workspace(const char* who, const void* workspace, size_t bytes, size_t required, const char* hint = nullptr) {
  DN_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  if (required > bytes) {
    if (hint) dn_set_error("%s: workspace %zu < required %zu (%s)", who, bytes, required, hint);
    else dn_set_error("%s: workspace %zu < required %zu", who, bytes, required);
    return DN_EWORKSPACE;
  }
  return DN_OK;
}

// Stage timing of an engine's forward (dn_voc_set_profile, dn_hubert_set_profile): events at the stage boundaries, created by the
// first enable(.., on), recorded by the forward's mark()s while switched on (`cursor` counts them from 0 in every forward), read back
// as the milliseconds between neighbours.
struct StageTimer {
  static constexpr int kMaxEvents = 16;
  hipEvent_t ev[kMaxEvents];
  int n_ev = 0, profile = 0;

  int enable(const char* who, int need, int on) {
    DN_CHECK_ARG(need >= 2 && need <= kMaxEvents, "%s: %d stage boundaries (2 .. %d)", who, need, kMaxEvents);
    if (on && !n_ev)
      for (int i = 0; i < need; ++i) {
        if (hipEventCreate(&ev[i]) != hipSuccess) {
          dn_set_error("%s: hipEventCreate failed", who);
          return DN_ELAUNCH;
        }
        n_ev = i + 1;
      }
    profile = on ? 1 : 0;
    return DN_OK;
  }
  void mark(int& cursor, hipStream_t s) {
    if (profile && cursor < n_ev) (void)hipEventRecord(ev[cursor++], s);
  }
  // waits for the last profiled forward; ms[i] = its stage i; returns the number of stages (n_ev - 1)
  int read(const char* who, float* ms, int cap) {
    DN_CHECK_ARG(ms && n_ev, "%s: profiling was not switched on (the engine's set_profile)", who);
    const int n = n_ev - 1;
    DN_CHECK_ARG(cap >= n, "%s: room for %d values needed", who, n);
    bool ok = hipEventSynchronize(ev[n]) == hipSuccess;
    for (int i = 0; i < n && ok; ++i) ok = hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) == hipSuccess;
    if (!ok) {
      dn_set_error("%s: no profiled forward has run", who);
      return DN_ELAUNCH;
    }
    return n;
  }
  void destroy() {
    for (int i = 0; i < n_ev; ++i) (void)hipEventDestroy(ev[i]);
    n_ev = profile = 0;
  }
};

// WaveNet / WavenetEncoder (latent_module.py:585-617, 1003-1032).  Packed tensors (packing.py):
//   init_W [3][padn(cout)][padk(cin)]   init_b [padk(cout)]
//   conv_W [S][L][3][padn(cout)][padk(cout)]   conv_b [S][L][padk(cout)]
//   res_W  [S][L][padn(cout)][padk(cout)]      res_b  [S][L][padk(cout)]
//   skip_W [L][padn(cout)][padk(cout)]         skip_b [padk(cout)]  (sum over the L blocks)
//   final_W [padn(cout)][padk(cout)]           final_b [padk(cout)]
//   conv_Wkb, res_Wkb: conv_W and res_W once more, K-blocked ([..][padk(cout)/32][padn(cout)][32], bf16; DN_LAYOUT_W_KBLOCKED)
//                      for the 256 x 256 tile, whose fill path moves whole cache lines; any pointer (unused) in f32 mode
struct WavenetW {
  int cin, cout, stacks, layers;
  const void *init_W, *conv_W, *res_W, *skip_W, *final_W, *conv_Wkb, *res_Wkb;
  const float *init_b, *conv_b, *res_b, *skip_b, *final_b;
};
constexpr int kWavenetTensors = 12;

// ConditionableTransformer (latent_module.py:642-706).  Packed tensors:
//   qkv_W [depth][padn(3*hd)][padk(D)]  (rows: to_q ; to_kv)       out_W [depth][padn(D)][padk(hd)]
//   ffin_W [depth][2*padk(inner)][padk(D)] GEGLU-interleaved        ffin_b [depth][2*padk(inner)]
//   ffconv_W [depth][3][padn(inner)][padk(inner)]                   ffconv_b [depth][padk(inner)]
//   ffconv_Wkb: the same weights K-blocked, [depth][3][padk(inner)/32][padn(inner)][32] (bf16; DN_LAYOUT_W_KBLOCKED) -- the
//               form the 256 x 352 tile stages as whole cache lines; any pointer (unused) in f32 mode
//   ffin_Wkb: ffin_W K-blocked, [depth][padk(D)/32][2*padk(inner)][32] (bf16) -- used when the GEGLU projection lands on the
//               256 x 256 tile: the split norm's producer then writes its activations K-blocked too (norm_split = 2)
//   qkv_Wkb: qkv_W K-blocked, [depth][padk(D)/32][padn(3*hd)][32] (bf16) -- layers >= 1 when the projection lands on the 256 x 256
//               tile: the previous layer's residual-closing contraction then writes the attention norm's row * gamma K-blocked
//   ffout_W [depth][padn(D)][padk(inner)]                           ffout_b [depth][padk(D)]
//   g1, g2 [depth][D] learned RMSNorm gammas (NULL when time-conditioned)
//   pred_gamma [D]   pred_W [padn(D)][padk(D)]
// Beside the table (dn_ffn_fold writes them, dn_eps_set_ffn_fold / dn_vae_set_ffn_fold attach them; NULL: the two-stage form):
//   fold_W [depth][3][padn(D)][padk(inner)] = ffout_W . ffconv_W tap by tap, in the operand format      fold_b [depth][padk(D)]
struct TransformerW {
  int dim, depth, heads, dim_head, inner;
  const void *qkv_W, *out_W, *ffin_W, *ffconv_W, *ffout_W, *pred_W, *ffconv_Wkb, *ffin_Wkb, *qkv_Wkb;
  const float *ffin_b, *ffconv_b, *ffout_b, *g1, *g2, *pred_gamma;
  const void* fold_W;
  const void* fold_Wkb;  // fold_W K-blocked, [depth][3][padk(inner)/32][padn(D)][32] (2-byte types; dn_ffn_fold_kblocked) or NULL
  const float* fold_b;
  int fold_default;  // option ffn_fold when unset: 5 (folded, routed by run_transformer), but 0 in DN_BF16 (the two-stage form there: DESIGN 11)
};
constexpr int kTransformerTensors = 15;

// grouped launch of the row-major weight gradient (wgrad_tn.hip): the blocks of a WaveNet stack in one launch
struct WgTnGroups {
  int groups;
  int64_t dy_gstride, x_gstride, grad_gstride;  // elements between the groups' dY / X / packed gradients
  int shift_by_group;                           // shifts scaled by 2^group
};
int wgrad_tn_launch(const void* dy, int lddy, int cout, const void* const* x, const int* ldx, const int* shift, int n_taps, int cin, int B, int T,
                    int slices, float* part, float* grad, void* stream, int tag, const WgTnGroups* grp);
constexpr int WGRAD_TN_X3_DEFAULT = 1;  // option wgrad_tn_x3 when unset (the x3 update 39.28 -> 37.35 ms, three alternating pairs)
// the same on DN_BF16X3 split rows (both operands [hi | lo]; ld, cin, cout and the group strides count 4-byte elements)
int wgrad_tn_x3_launch(const void* dy, int lddy, int cout, const void* const* x, const int* ldx, const int* shift, int n_taps, int cin, int B, int T,
                       int slices, float* part, float* grad, void* stream, int tag, const WgTnGroups* grp);

// One captured step of a device sampling loop.  The key is everything a captured kernel argument bakes in; it is memset to zero
// before it is filled (padding compares equal) and compared with memcmp.  A loop fills the fields it has and leaves the rest zero.
struct StepKey {
  const void *ws, *x, *len, *coef;  // (a scheduled chain: the workspace copy of its coefficients, an address that moves with n_steps)
  const void *prompt, *plen;        // guided loop
  const void* keys;                 // a keyed chain: the ADDRESS of its per-utterance keys (a replay reads keys[b] from memory, so new
                                    // contents at the same address give new draws; another address is a miss); else null
  uint64_t seed;                    // the Philox key of a seed-drawn chain (0 for a keyed one)
  int32_t B, T, Tp, n_steps;        // Tp, n_steps: guided loop (the unconditional slot serves any start_step / max_evals)
  int32_t flags;                    // DN_LOOP_* without DN_LOOP_KEEP_TABLE
  int32_t opt_gen;                  // dn::option_generation() at capture: the run-time options its routes were chosen under
  uint32_t scale_bits;              // guided loop: cond_scale
  uint32_t eta_bits;                // dn_gaussian_loop's DDIM update: the bits of eta, a kernel argument there (0 elsewhere)
  uint16_t ancestral, clip, scheduled, eta, dpm;  // which update the step applies
  uint16_t generic;                 // dn_gaussian_loop: the respaced GaussianDiffusion update (ancestral: p_sample, else ddim_sample)
  uint16_t injected;                // injected noise bakes its row base into the step: stored (it evicts), never served
  uint16_t reserved;                // zero
};
static_assert(sizeof(StepKey) == 7 * sizeof(void*) + 8 + 8 * 4 + 8 * 2, "StepKey has no padding: copies of a key compare equal too");
struct StepGraph {
  void* exec;  // hipGraphExec_t, null while empty
  StepKey key;
};

// ---- The update kernels of the device loops (pointwise.hip).
// Where a scheduled update takes its normals from: the utterances' keys (row_quads = T Z / 4 quads per utterance; noise and seed are
// not read), else the injected rows (noise_row floats apart; 0: `noise` is the row whatever the step index), else `seed`.
struct SchedNoise {
  const float* noise;
  int64_t noise_row;
  uint64_t seed;
  const uint64_t* keys;
  int64_t row_quads;
};
inline SchedNoise sched_noise(const float* noise, int64_t noise_row, uint64_t seed, const uint64_t* keys, int64_t row_quads) {
  return keys ? SchedNoise{nullptr, 0, 0, keys, row_quads} : SchedNoise{noise, noise_row, seed, nullptr, 0};
}
// One update of a chain over a timestep schedule, in place on elements [elem0, elem0 + n_elem) of the whole batch's x (both multiples
// of 4): row *counter of the rule's coefficients.  The descriptor is the kernel's argument as it stands.
enum SchedRule { SCHED_DDIM, SCHED_DPM2M, SCHED_GAUSSIAN };
struct SchedStep {
  int rule;
  float* x;
  int64_t elem0, n_elem;
  // eps source: `eps` at the element, or (guided; elem0 = 0) the conditioned rows eps[0:n_elem] combined at `scale` with the null rows
  // eps[n_elem:2 n_elem].  Sink: x, and xin[0:n_elem] (+ xin[n_elem:2 n_elem] when guided) unless xin is null or x itself.
  const float* eps;
  int guided;
  float scale;
  float* xin;
  // rule: coef [n_steps, DN_DDIM_SCHED_COLS | DN_DPM_COLS | DN_GD_COLS], steps (the rows' timesteps: DDIM always, else keyed only)
  const float* coef;
  const int32_t *steps, *counter;
  int eta_on;                      // SCHED_DDIM (keys imply it)
  float* hist;                     // SCHED_DPM2M: the previous data prediction, the whole batch's
  int n_steps, sampler, clip;      // SCHED_GAUSSIAN
  float eta;
  SchedNoise src;
};
// `who` names the loop in the messages ("<who>: the latent width must be a multiple of 4", "<who> step: <HIP error>")
int sched_step_launch(const char* who, const SchedStep& d, void* stream);

}  // namespace dn

// the ancestral update of dn_ddpm_loop[_keyed], and what the dn_gaussian_* entries check of the update's own arguments (pointwise.hip)
int dn_ddpm_step_launch(float* x, const float* eps, int M, int C, int T, const float* table, const int32_t* t, int clip, const float* noise,
                        int64_t noise_row, int t_top, uint64_t seed, const uint64_t* keys, int b0, void* stream);
int dn_gaussian_sched_args(const char* who, int32_t n_steps, int32_t sampler, float eta);

struct DnEps {
  DnEpsConfig cfg;
  // packed tensors in table order: w_freq, tc_W, tc_b, cond_W, cond_b, init_W, init_b,
  // <wavenet x10>, <transformer x12>, final_W, final_b, pos_table
  const float *w_freq, *tc_W, *tc_b, *cond_b, *init_b, *final_b, *pos_table;
  const void *cond_W, *init_W, *final_W;
  dn::WavenetW wn;
  dn::TransformerW tf;
  int n_cond;  // conditioning columns of a row: 2*padk(dim) per conditioned module
  int n_row;   // row stride of the conditioning table: n_cond, then (split RMSNorm) the depth x (3 hd + 2 padk(inner))
               // columns of beta . W^T for the adaptive norms' consumers
  // conditional variant (kEpsCondTensors; null when cfg.dim_prompt == 0)
  const float *tpc_W, *tpc_b, *null_pc, *lat_pos, *rffin_b, *rffout_b, *rnorm_g, *proj_b;
  const void *null_tok, *proj_W, *rq_W, *rkv_W, *rout_W, *rffin_W, *rffout_W, *cq_W, *ckv_W, *cout_W;
  // hipGraph caches of the device sampling loops: one slot for the four unconditional loops, one for dn_guided_ddim_loop and
  // dn_guided_dpm_loop (a guided loop neither serves nor evicts the unconditional ones; StepKey.dpm keeps the two guided loops apart)
  dn::StepGraph loop_graph, guided_graph;
  void *side_stream, *ev_fork, *ev_join;  // DN_LOOP_SPLIT2: second half-batch stream and its fork/join events
  // DN_LOOP_KEEP_TABLE: the conditioning table built by the previous dn_ddim_loop call on this workspace
  void *table_ws, *table_at;  // (table_at: where in the workspace it lies -- the plan in front of it moves with option ffn_fold)
  int table_B, table_T, table_split, table_rows;
};
constexpr int kEpsTensors = 7 + dn::kWavenetTensors + dn::kTransformerTensors + 3;
// conditional variant (cfg.dim_prompt > 0), appended to the table: tpc_W (fp32 [padn(C)][padk(P)]), tpc_b [C], null_prompt_cond [C],
// null_prompt_tokens [m][Dp], resampler proj_W [padn(D)][padk(P)], proj_b [Dp], latents + positions fp32 [m][Dp], per resampler layer
// (stacked) q_W [padn(hd)][Dp], kv_W [padn(2hd)][Dp], out_W [padn(D)][hd], ffin_W [2 ip][Dp] (GEGLU-interleaved), ffin_b [2 ip],
// ffout_W [padn(D)][ip], ffout_b [Dp], norm gamma [D]; per transformer layer (stacked) cross-attention q_W, kv_W, out_W.
constexpr int kEpsCondTensors = 18;

struct DnVae {
  DnVaeConfig cfg;
  int n_wave;
  dn::WavenetW enc[4], dec[4];
  dn::TransformerW tf;
  const void* lm_W;
  const float* lm_b;
};
