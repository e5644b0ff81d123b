// The mHuBERT front end of the recipe (scripts/prepare/feature_dump.sh -> examples/textless_nlp/gslm/speech2unit/pretrained/
// hubert_feature_reader.py; scripts/prepare/quantize_unit.sh -> quantize_with_kmeans.py): HubertModel.extract_features(source,
// padding_mask=None, mask=False, output_layer=k) (fairseq/models/hubert/hubert.py:429-476, 529-545), eval mode (the k-means
// assignment behind it is kmeans.hip's).  ConvFeatureExtractionModel (fairseq/models/wav2vec/wav2vec2.py:819-896, mode "default", no conv bias) ->
// LayerNorm -> post_extract_proj -> pos_conv + residual -> LayerNorm (TransformerEncoder.extract_features, :1009-1076,
// layer_norm_first False) -> post-norm TransformerSentenceEncoderLayers (:1258-1283).  The reader runs one utterance at a time, so a
// batch here gives every utterance what it gets alone: per-utterance GroupNorm statistics, zeros outside [0, len) in the positional
// conv, key lengths in the attention; every other stage is row-wise.
//   first conv + GroupNorm + GELU   conv0_stats_kernel / conv0_combine_kernel / conv0_apply_kernel (two passes over the waveform)
//   conv layers 1..                 a stride-s k-tap conv without padding as a contraction over gathered rows (strided_taps_kernel,
//                                   the subsampler's form in nar_common.h) on dn_conv_gemm; the GELU behind layer i is applied by the
//                                   gather of layer i + 1 (as the subsampler's GLU is), the last one by gelu_rows_kernel
//   positional conv                 dn_grouped_conv1d below
//   layers                          nar_common.h's LayerNorm and self_attention_block; dn_conv_gemm for the FFN
// The large form (wav2vec 2.0 / HuBERT large, and the Wav2VecCtc recognisers of the recipe's ASR-BLEU, research/TranSpeech/asr_bleu/
// utils.py:221-308) is the same pass with DnHubertConfig's appended fields set:
//   wave_norm                       wave_stats_kernel / wave_combine_kernel; applied by stage_wave
//   extractor_ln (+ conv_bias)      conv0_ln_kernel; layers 1..: the same contraction with the bias, then nar_common.h's LayerNorm + GELU
//   pre_norm                        the second layer loop of hubert_pass
//   vocab                           dn_hubert_ctc_forward: encoder.layer_norm, the fp32 head, emit_rows_kernel; dn_ctc_greedy decodes
#include <new>

#include "common.h"
#include "engine.h"
#include "nar_common.h"

using namespace dn;

namespace dn {
namespace {

constexpr int C0_KMAX = 16;   // taps of the first conv held in registers (zero weights behind the kernel)
constexpr int C0_SMAX = 8;    // its largest stride
constexpr int C0_TF = 256;    // frames per tile, counted from frame 0 of each utterance

__host__ __device__ __forceinline__ int conv_frames(int len, int k, int s) { return len >= k ? (len - k) / s + 1 : 0; }

// len1[b] = frames of utterance b behind the first conv; out_len[b] = behind the whole stack (at most S)
struct ConvGeom { int n, k[DN_HUBERT_MAX_CONV], s[DN_HUBERT_MAX_CONV]; };
__global__ void hubert_lengths_kernel(const int32_t* __restrict__ lengths, int B, int L, ConvGeom g, int S, int32_t* __restrict__ len1,
                                      int32_t* __restrict__ out_len) {
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    int l = lengths[b] < L ? lengths[b] : L;
    for (int i = 0; i < g.n; ++i) {
      l = conv_frames(l, g.k[i], g.s[i]);
      if (i == 0) len1[b] = l;
    }
    out_len[b] = l < S ? l : S;
  }
}

// The samples of a frame tile in LDS: ws[i] = wave[b][t0 * s + i], zeros at and behind the utterance's own length (whatever the
// caller left there never reaches a valid frame, not even through a zero weight)
// wstat (wave_norm): the utterance's (mean hi, mean lo, rstd) of wave_combine_kernel; the staged sample is then the normalised one,
// so no normalised copy of the waveform exists anywhere
__device__ __forceinline__ void stage_wave(float* ws, const float* __restrict__ wave, int64_t L, int b, int len, int t0, int s,
                                           const float4* __restrict__ wstat = nullptr) {
  const int n = C0_TF * s + C0_KMAX;
  const int64_t base = (int64_t)t0 * s;
  if (wstat) {
    const float4 st = wstat[b];
    for (int i = threadIdx.x; i < n; i += 256) ws[i] = base + i < len ? ((wave[(int64_t)b * L + base + i] - st.x) - st.y) * st.z : 0.f;
    return;
  }
  for (int i = threadIdx.x; i < n; i += 256) ws[i] = base + i < len ? wave[(int64_t)b * L + base + i] : 0.f;
}
__device__ __forceinline__ float conv0_at(const float* ws, const float (&w)[C0_KMAX]) {
  float a = 0.f;
#pragma unroll
  for (int j = 0; j < C0_KMAX; ++j) a = fmaf(w[j], ws[j], a);
  return a;
}

// Pass 1 of Fp32GroupNorm(C, C) behind Conv1d(1 -> C) (wav2vec2.py:860-866): per (utterance, tile, channel) the mean and the sum of
// squared deviations FROM THAT MEAN of the tile's valid frames (two sweeps over the staged samples: no E[x^2] - mean^2).
__global__ __launch_bounds__(256) void conv0_stats_kernel(const float* __restrict__ wave, const int32_t* __restrict__ lengths, const int32_t* __restrict__ len1,
                                                          int L, int C, int s, const float* __restrict__ w0, float2* __restrict__ part) {
  __shared__ float ws[C0_TF * C0_SMAX + C0_KMAX];
  const int tile = blockIdx.x, b = blockIdx.y, t0 = tile * C0_TF;
  int nv = len1[b] - t0;
  nv = nv < 0 ? 0 : nv > C0_TF ? C0_TF : nv;
  stage_wave(ws, wave, L, b, lengths[b] < L ? lengths[b] : L, t0, s);
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float w[C0_KMAX];
#pragma unroll
    for (int j = 0; j < C0_KMAX; ++j) w[j] = w0[j * C + c];
    float sum = 0.f;
    for (int f = 0; f < nv; ++f) sum += conv0_at(ws + f * s, w);
    const float mean = nv ? sum / (float)nv : 0.f;
    float m2 = 0.f;
    for (int f = 0; f < nv; ++f) {
      const float d = conv0_at(ws + f * s, w) - mean;
      m2 = fmaf(d, d, m2);
    }
    part[((int64_t)b * gridDim.x + tile) * C + c] = make_float2(mean, m2);
  }
}

// The tiles' (count, mean, M2) combined in tile order in double precision (Chan et al.): stat[b][c] = (mean hi, mean lo, rstd, 0)
__global__ __launch_bounds__(256) void conv0_combine_kernel(const float2* __restrict__ part, const int32_t* __restrict__ len1, int B, int C, int tiles,
                                                            float4* __restrict__ stat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  ChanAcc a;
  for (int t = 0; t < tiles; ++t) {
    int nb = len1[b] - t * C0_TF;
    if (nb <= 0) break;
    nb = nb > C0_TF ? C0_TF : nb;
    const float2 p = part[((int64_t)b * tiles + t) * C + c];
    a.add(nb, (double)p.x, (double)p.y);
  }
  float4 o = make_float4(0, 0, 0, 0);
  if (a.n > 0) {
    a.split(o.x, o.y);
    o.z = (float)(1.0 / sqrt(a.m2 / a.n + 1e-5));
  }
  stat[i] = o;
}

// Pass 2: the conv again, normalised, affine, GELU, stored once in the operand type: y[b][t][c], channels last
__global__ __launch_bounds__(256) void conv0_apply_kernel(const float* __restrict__ wave, const int32_t* __restrict__ lengths, int L, int T1, int C, int s,
                                                          const float* __restrict__ w0, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float4* __restrict__ stat, void* __restrict__ y, int dtype) {
  __shared__ float ws[C0_TF * C0_SMAX + C0_KMAX];
  const int b = blockIdx.y, t0 = blockIdx.x * C0_TF;
  const int nf = T1 - t0 < C0_TF ? T1 - t0 : C0_TF;
  stage_wave(ws, wave, L, b, lengths[b] < L ? lengths[b] : L, t0, s);
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float w[C0_KMAX];
#pragma unroll
    for (int j = 0; j < C0_KMAX; ++j) w[j] = w0[j * C + c];
    const float4 st = stat[b * C + c];
    const float sc = st.z * gamma[c], sh = beta[c];
    for (int f = 0; f < nf; ++f) {
      const float v = (conv0_at(ws + f * s, w) - st.x) - st.y;
      store_act(y, ((int64_t)b * T1 + t0 + f) * C + c, dtype, gelu_exact(fmaf(v, sc, sh)));
    }
  }
}

// Rows of the contraction that IS a Conv1d(k, stride s, no padding) over channels-last [B, Tin, C]:
// cols[b * Tout + t][j * C + c] = act(in[b][s t + j][c]); every source row exists (s (Tout - 1) + k - 1 <= Tin - 1).  GELU: `in` is the
// previous conv's fp32 pre-activation and the gathered value gelu(in); else `in` is in the operand type already.
template <bool GELU>
__global__ __launch_bounds__(256) void strided_taps_kernel(const void* __restrict__ in, int in_dtype, int B, int Tin, int Tout, int C, int k, int s,
                                                           void* __restrict__ cols, int dtype) {
  const int Kq = k * C / 4, Cq = C / 4;
  const int64_t n = (int64_t)B * Tout * Kq;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % Kq);
    const int64_t row = i / Kq;
    const int t = (int)(row % Tout), b = (int)(row / Tout), j = q / Cq, c = (q - j * Cq) * 4;
    float4 v = load4(in, ((int64_t)b * Tin + (int64_t)s * t + j) * C + c, in_dtype);
    if (GELU) v = make_float4(gelu_exact(v.x), gelu_exact(v.y), gelu_exact(v.z), gelu_exact(v.w));
    store4(cols, i * 4, dtype, v.x, v.y, v.z, v.w);
  }
}

// out = gelu(in) element-wise, fp32 -> out_dtype (in place when out_dtype is DN_F32 and out == in)
__global__ __launch_bounds__(256) void gelu_rows_kernel(const float* in, void* out, int out_dtype, int64_t nquad) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nquad; i += (int64_t)gridDim.x * 256) {
    const float4 v = *reinterpret_cast<const float4*>(in + i * 4);
    store4(out, i * 4, out_dtype, gelu_exact(v.x), gelu_exact(v.y), gelu_exact(v.z), gelu_exact(v.w));
  }
}

// out[b][t][:] = x[b][t][:] for t < len[b], zeros behind
__global__ __launch_bounds__(256) void masked_copy_kernel(const float* __restrict__ x, const int32_t* __restrict__ len, int B, int S, int D,
                                                          float* __restrict__ out) {
  const int Dq = D / 4;
  const int64_t n = (int64_t)B * S * Dq;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / Dq;
    const int t = (int)(row % S), b = (int)(row / S);
    reinterpret_cast<float4*>(out)[i] = t < len[b] ? reinterpret_cast<const float4*>(x)[i] : make_float4(0, 0, 0, 0);
  }
}

// ---- wave_norm: F.layer_norm(wave, wave.shape) of one utterance over its own samples (eps 1e-5, biased variance), taken as the
// GroupNorm pass above takes its statistics: per tile the mean, then the squared deviations FROM THAT MEAN (no E[x^2] - mean^2), the
// tiles combined in tile order.  The tile sums run in double (a fixed tree over the block), so a constant waveform has deviation 0.
constexpr int WN_PER = 16, WN_TILE = 256 * WN_PER;  // samples per thread / per tile
__device__ __forceinline__ double block_sum256(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
// part[b][tile] = (mean hi, mean lo, M2, 0) of the tile's valid samples
__global__ __launch_bounds__(256) void wave_stats_kernel(const float* __restrict__ wave, const int32_t* __restrict__ lengths, int L, float4* __restrict__ part) {
  __shared__ double red[256];
  const int tile = blockIdx.x, b = blockIdx.y, len = lengths[b] < L ? lengths[b] : L;
  int n = len - tile * WN_TILE;
  n = n < 0 ? 0 : n > WN_TILE ? WN_TILE : n;
  const float* w = wave + (int64_t)b * L + (int64_t)tile * WN_TILE;
  float x[WN_PER];
  double sum = 0;
#pragma unroll
  for (int k = 0; k < WN_PER; ++k) {
    const int i = threadIdx.x + 256 * k;
    x[k] = i < n ? w[i] : 0.f;
    sum += (double)x[k];
  }
  const double mean = n ? block_sum256(sum, red) / n : 0.0;
  const float mh = (float)mean, ml = (float)(mean - (double)mh);
  double q = 0;
#pragma unroll
  for (int k = 0; k < WN_PER; ++k)
    if ((int)threadIdx.x + 256 * k < n) {
      const float d = (x[k] - mh) - ml;
      q += (double)d * d;
    }
  const double m2 = block_sum256(q, red);
  if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + tile] = make_float4(mh, ml, (float)m2, 0.f);
}
// wstat[b] = (mean hi, mean lo, rstd, 0): Chan et al. over the tiles in order, in double
__global__ void wave_combine_kernel(const float4* __restrict__ part, const int32_t* __restrict__ lengths, int B, int L, int tiles, float4* __restrict__ wstat) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int len = lengths[b] < L ? lengths[b] : L;
  ChanAcc a;
  for (int t = 0; t < tiles; ++t) {
    int nb = len - t * WN_TILE;
    if (nb <= 0) break;
    nb = nb > WN_TILE ? WN_TILE : nb;
    const float4 p = part[(int64_t)b * tiles + t];
    a.add(nb, (double)p.x + (double)p.y, (double)p.z);
  }
  float4 o = make_float4(0, 0, 0, 0);
  if (a.n > 0) {
    a.split(o.x, o.y);
    o.z = (float)(1.0 / sqrt(a.m2 / a.n + 1e-5));
  }
  wstat[b] = o;
}

// ---- extractor_mode "layer_norm" (wav2vec2.py:849-859): Conv1d + bias -> Fp32LayerNorm over the C channels of each frame -> GELU.
// Layer 0 in one kernel: a wave per frame, lane -> channels lane + 64 i; the taps [16][C] and the tile's (normalised) samples lie in
// LDS; the norm is row-wise, so there are no cross-tile statistics.  C <= C0_LN_CMAX.
constexpr int C0_LN_CMAX = 512, C0_LN_NC = C0_LN_CMAX / 64;
__global__ __launch_bounds__(256) void conv0_ln_kernel(const float* __restrict__ wave, const int32_t* __restrict__ lengths, int L, int T1, int C, int s,
                                                       const float* __restrict__ w0, const float* __restrict__ bias, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float4* __restrict__ wstat, void* __restrict__ y, int dtype) {
  __shared__ float ws[C0_TF * C0_SMAX + C0_KMAX];
  __shared__ float wl[C0_KMAX * C0_LN_CMAX];
  const int b = blockIdx.y, t0 = blockIdx.x * C0_TF;
  const int nf = T1 - t0 < C0_TF ? T1 - t0 : C0_TF;
  stage_wave(ws, wave, L, b, lengths[b] < L ? lengths[b] : L, t0, s, wstat);
  for (int i = threadIdx.x; i < C0_KMAX * C; i += 256) wl[i] = w0[i];
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nc = C / 64;
  float bi[C0_LN_NC], g[C0_LN_NC], be[C0_LN_NC];
#pragma unroll
  for (int i = 0; i < C0_LN_NC; ++i) {
    const int c = lane + 64 * i;
    bi[i] = i < nc ? bias[c] : 0.f;
    g[i] = i < nc ? gamma[c] : 0.f;
    be[i] = i < nc ? beta[c] : 0.f;
  }
  for (int f = wv; f < nf; f += 4) {
    float xs[C0_KMAX], a[C0_LN_NC];
#pragma unroll
    for (int j = 0; j < C0_KMAX; ++j) xs[j] = ws[f * s + j];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < C0_LN_NC; ++i) {
      a[i] = 0.f;
      if (i < nc) {
        float acc = bi[i];
#pragma unroll
        for (int j = 0; j < C0_KMAX; ++j) acc = fmaf(wl[j * C + lane + 64 * i], xs[j], acc);
        a[i] = acc;
        sum += acc;
      }
    }
    const float mean = wave_sum(sum) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < C0_LN_NC; ++i)
      if (i < nc) q = fmaf(a[i] - mean, a[i] - mean, q);
    const float rstd = rsqrtf(wave_sum(q) / (float)C + 1e-5f);
    const int64_t row = ((int64_t)b * T1 + t0 + f) * C;
#pragma unroll
    for (int i = 0; i < C0_LN_NC; ++i)
      if (i < nc) store_act(y, row + lane + 64 * i, dtype, gelu_exact(fmaf((a[i] - mean) * rstd, g[i], be[i])));
  }
}

// The CTC head's output without its pad columns: out[b][t][v] = e[b S + t][v] for t < len[b], v < V; zero rows behind
__global__ __launch_bounds__(256) void emit_rows_kernel(const float* __restrict__ e, int ld, const int32_t* __restrict__ len, int B, int S, int V,
                                                        float* __restrict__ out) {
  const int64_t n = (int64_t)B * S * V;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int v = (int)(i % V);
    const int64_t row = i / V;
    const int t = (int)(row % S), b = (int)(row / S);
    out[i] = t < len[b] ? e[row * ld + v] : 0.f;
  }
}

// dn_ctc_greedy: a workgroup per utterance, 256 frames a round.  A thread takes its frame's arg-max (the first maximum: strict >),
// the frame is kept iff it is no blank and differs from the frame before it (toks[0] carries the last frame of the round before),
// and the kept tokens are compacted in order by a ballot prefix inside each wave and the waves' totals across the block.
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float* __restrict__ em, const int32_t* __restrict__ lengths, int S, int V, int blank,
                                                         int32_t* __restrict__ tokens, int32_t* __restrict__ counts) {
  __shared__ int toks[257], wtot[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int len = lengths[b];
  len = len < 0 ? 0 : len > S ? S : len;
  const float* e = em + (int64_t)b * S * V;
  int base = 0;
  for (int t0 = 0; t0 < len; t0 += 256) {
    const int t = t0 + tid;
    int tok = -1;
    if (t < len) {
      const float* row = e + (int64_t)t * V;
      float best = row[0];
      tok = 0;
      for (int v = 1; v < V; ++v) {
        const float x = row[v];
        if (x > best) { best = x; tok = v; }
      }
    }
    toks[tid + 1] = tok;
    __syncthreads();
    const bool keep = t < len && tok != blank && (t == 0 || tok != toks[tid]);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wtot[wv] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wv; ++w) off += wtot[w];
    if (keep) tokens[(int64_t)b * S + off + __popcll(mask & ((1ull << lane) - 1ull))] = tok;
    base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
    if (tid == 255) toks[0] = tok;
  }
  if (tid == 0) counts[b] = base;
}

// dn_grouped_conv1d.  A workgroup: GC_NF * (256 / Cg) frames of one group of one sequence; thread -> (output channel co, frame
// slot fr), GC_NF frames fr + FR i each.  The tile's rows and the k - 1 halo rows lie in LDS once for all taps; the weights stream
// from [g][tap][ci][co] (co fastest: one coalesced load per (tap, ci), reused for the GC_NF frames).
constexpr int GC_NF = 8, GC_CGMAX = 64, GC_KMAX = 128;
__global__ __launch_bounds__(256) void grouped_conv1d_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ out, const int32_t* __restrict__ lengths, int T, int C, int Cg, int k) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [TT + k - 1][Cg]
  const int tid = threadIdx.x, g = blockIdx.y, b = blockIdx.z, FR = 256 / Cg, TT = FR * GC_NF, t0 = blockIdx.x * TT, half = k / 2;
  const int len = lengths[b] < T ? lengths[b] : T;
  const int co = tid % Cg, fr = tid / Cg;
  const int64_t row0 = (int64_t)b * T;
  if (t0 >= len) {  // a tile behind the sequence: zeros
    if (fr < FR)
      for (int i = 0; i < GC_NF; ++i) {
        const int t = t0 + fr + FR * i;
        if (t < T) out[(row0 + t) * C + g * Cg + co] = 0.f;
      }
    return;
  }
  const int rows = TT + k - 1, Cq = Cg / 4;
  for (int i = tid; i < rows * Cq; i += 256) {
    const int r = i / Cq, c = (i - r * Cq) * 4, t = t0 + r - half;
    float4 v = make_float4(0, 0, 0, 0);
    if (t >= 0 && t < len) v = *reinterpret_cast<const float4*>(x + (row0 + t) * C + g * Cg + c);
    *reinterpret_cast<float4*>(xs + r * Cg + c) = v;
  }
  __syncthreads();
  if (fr >= FR) return;
  float acc[GC_NF];
#pragma unroll
  for (int i = 0; i < GC_NF; ++i) acc[i] = 0.f;
  const float* wg = w + (int64_t)g * k * Cg * Cg + co;
  for (int j = 0; j < k; ++j) {
    const float* wj = wg + (int64_t)j * Cg * Cg;
    const float* xj = xs + (fr + j) * Cg;
    for (int ci = 0; ci < Cg; ci += 4) {
      const float w0 = wj[ci * Cg], w1 = wj[(ci + 1) * Cg], w2 = wj[(ci + 2) * Cg], w3 = wj[(ci + 3) * Cg];
#pragma unroll
      for (int i = 0; i < GC_NF; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(xj + FR * i * Cg + ci);
        acc[i] = fmaf(w0, v.x, acc[i]);
        acc[i] = fmaf(w1, v.y, acc[i]);
        acc[i] = fmaf(w2, v.z, acc[i]);
        acc[i] = fmaf(w3, v.w, acc[i]);
      }
    }
  }
  const float bc = bias[g * Cg + co];
#pragma unroll
  for (int i = 0; i < GC_NF; ++i) {
    const int f = fr + FR * i, t = t0 + f;
    if (t >= T) continue;
    out[(row0 + t) * C + g * Cg + co] = t < len ? xs[(f + half) * Cg + co] + gelu_exact(acc[i] + bc) : 0.f;
  }
}

}  // namespace
}  // namespace dn

extern "C" int dn_grouped_conv1d(const float* x, const float* w, const float* bias, float* out, const int32_t* lengths, int32_t B, int32_t T, int32_t C,
                                 int32_t groups, int32_t k, void* stream) {
  DN_CHECK_ARG(x && w && bias && out && lengths && x != out, "dn_grouped_conv1d: null argument (or out aliases x)");
  DN_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && C > 0 && groups > 0 && groups <= 65535 && C % groups == 0, "dn_grouped_conv1d: B=%d T=%d C=%d groups=%d", B, T, C, groups);
  const int Cg = C / groups;
  DN_CHECK_ARG(Cg % 4 == 0 && Cg <= GC_CGMAX && k >= 1 && k <= GC_KMAX, "dn_grouped_conv1d: %d channels per group (a multiple of 4, <= %d), kernel %d (<= %d)", Cg,
               GC_CGMAX, k, GC_KMAX);
  DN_CHECK_ARG((int64_t)B * T * C < (int64_t)1 << 31, "dn_grouped_conv1d: B * T * C exceeds 2^31 elements");
  DN_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "dn_grouped_conv1d: x and out must be 16-byte aligned");
  const int TT = (256 / Cg) * GC_NF;
  const size_t lds = (size_t)(TT + k - 1) * Cg * sizeof(float);
  hipLaunchKernelGGL(grouped_conv1d_kernel, dim3((T + TT - 1) / TT, groups, B), dim3(256), lds, (hipStream_t)stream, x, w, bias, out, lengths, T, C, Cg, k);
  DN_CHECK_LAUNCH("dn_grouped_conv1d");
  return DN_OK;
}

struct DnHubert {
  DnHubertConfig cfg;
  const float *conv0_w, *gn_g, *gn_b, *ln_g, *ln_b, *proj_b, *pos_w, *pos_b, *enc_g, *enc_b, *qkv_b, *out_b, *fc1_b, *fc2_b, *lng, *lnb, *zeros;
  const void *conv_W[DN_HUBERT_MAX_CONV], *proj_W, *qkv_W, *out_W, *fc1_W, *fc2_W;
  const float *conv_b, *cln_g, *cln_b, *head_b;  // extractor_ln: [n_conv][C] each; vocab > 0: the CTC head
  const void* head_W;
  StageTimer timer;  // dn_hubert_set_profile: the DN_HUBERT_STAGES + 1 stage boundaries of the last profiled forward
};

extern "C" int dn_hubert_create(const DnHubertConfig* cfg, const void* const* w, int32_t n, DnHubert** out) {
  DN_CHECK_ARG(cfg && cfg->n_conv >= 2 && cfg->n_conv <= DN_HUBERT_MAX_CONV, "dn_hubert_create: 2 .. %d conv layers", DN_HUBERT_MAX_CONV);
  DN_TRY(check_create("dn_hubert_create", cfg, w, n, 21 + cfg->n_conv + (cfg->extractor_ln ? 3 : 0) + (cfg->vocab > 0 ? 2 : 0), out));
  const int C = cfg->conv_dim, dh = cfg->dim / cfg->heads;
  DN_CHECK_ARG(!cfg->extractor_ln || C <= C0_LN_CMAX, "dn_hubert_create: extractor_ln: conv width %d (<= %d)", C, C0_LN_CMAX);
  DN_CHECK_ARG(!cfg->extractor_ln == !cfg->pre_norm && (cfg->extractor_ln || (!cfg->conv_bias && !cfg->wave_norm)),
               "dn_hubert_create: the large form is one form: extractor_ln and pre_norm go together, conv_bias and wave_norm only with them");
  DN_CHECK_ARG(cfg->vocab >= 0 && cfg->vocab <= 4096 && (!cfg->vocab || cfg->pre_norm), "dn_hubert_create: vocab %d (0: no CTC head, <= 4096; the large form only)",
               cfg->vocab);
  DN_CHECK_ARG(C > 0 && C % 64 == 0 && C <= 1024, "dn_hubert_create: conv width %d must be a multiple of 64, <= 1024", C);
  DN_CHECK_ARG(cfg->conv_kernel[0] >= 1 && cfg->conv_kernel[0] <= C0_KMAX && cfg->conv_stride[0] >= 1 && cfg->conv_stride[0] <= C0_SMAX,
               "dn_hubert_create: first conv kernel %d (<= %d), stride %d (<= %d)", cfg->conv_kernel[0], C0_KMAX, cfg->conv_stride[0], C0_SMAX);
  for (int i = 1; i < cfg->n_conv; ++i)
    DN_CHECK_ARG(cfg->conv_kernel[i] >= 1 && cfg->conv_kernel[i] <= 8 && cfg->conv_stride[i] >= 1, "dn_hubert_create: conv layer %d: kernel %d stride %d", i,
                 cfg->conv_kernel[i], cfg->conv_stride[i]);
  DN_CHECK_ARG(cfg->has_proj || C == cfg->dim, "dn_hubert_create: no post_extract_proj needs conv width %d == embed width %d", C, cfg->dim);
  DN_CHECK_ARG(dh == 16 || dh == 32 || dh == 64, "dn_hubert_create: head width %d (16, 32 or 64)", dh);
  const int G = cfg->conv_pos_groups;
  DN_CHECK_ARG(G > 0 && cfg->dim % G == 0 && (cfg->dim / G) % 4 == 0 && cfg->dim / G <= GC_CGMAX && cfg->conv_pos >= 1 && cfg->conv_pos <= GC_KMAX,
               "dn_hubert_create: conv_pos %d (<= %d) with %d groups (channels per group a multiple of 4, <= %d)", cfg->conv_pos, GC_KMAX, G, GC_CGMAX);
  DnHubert* m = new (std::nothrow) DnHubert();
  DN_CHECK_ARG(m != nullptr, "dn_hubert_create: out of host memory");
  m->cfg = *cfg;
  TableCursor t{w, 0};
  m->conv0_w = t.next_vec(); m->gn_g = t.next_vec(); m->gn_b = t.next_vec();
  for (int i = 1; i < cfg->n_conv; ++i) m->conv_W[i] = t.next_mat();
  m->ln_g = t.next_vec(); m->ln_b = t.next_vec(); m->proj_W = t.next_mat(); m->proj_b = t.next_vec();
  m->pos_w = t.next_vec(); m->pos_b = t.next_vec(); m->enc_g = t.next_vec(); m->enc_b = t.next_vec();
  m->qkv_W = t.next_mat(); m->qkv_b = t.next_vec(); m->out_W = t.next_mat(); m->out_b = t.next_vec();
  m->fc1_W = t.next_mat(); m->fc1_b = t.next_vec(); m->fc2_W = t.next_mat(); m->fc2_b = t.next_vec();
  m->lng = t.next_vec(); m->lnb = t.next_vec(); m->zeros = t.next_vec();
  m->conv_b = m->cln_g = m->cln_b = m->head_b = nullptr;
  m->head_W = nullptr;
  if (cfg->extractor_ln) { m->conv_b = t.next_vec(); m->cln_g = t.next_vec(); m->cln_b = t.next_vec(); }
  if (cfg->vocab > 0) { m->head_W = t.next_mat(); m->head_b = t.next_vec(); }
  *out = m;
  return DN_OK;
}

extern "C" void dn_hubert_destroy(DnHubert* m) {
  if (!m) return;
  m->timer.destroy();
  delete m;
}

extern "C" int dn_hubert_set_profile(DnHubert* m, int32_t on) {
  DN_CHECK_ARG(m, "dn_hubert_set_profile: null engine");
  return m->timer.enable("dn_hubert_set_profile", DN_HUBERT_STAGES + 1, on);
}

extern "C" int dn_hubert_stage_times(DnHubert* m, float* ms, int32_t cap) {
  DN_CHECK_ARG(m && m->timer.n_ev == DN_HUBERT_STAGES + 1, "dn_hubert_stage_times: profiling was not switched on (dn_hubert_set_profile)");
  const int n = m->timer.read("dn_hubert_stage_times", ms, cap);
  return n < 0 ? n : DN_OK;
}

extern "C" int32_t dn_hubert_out_frames(const DnHubert* m, int32_t L) {
  if (!m) return 0;
  for (int i = 0; i < m->cfg.n_conv; ++i) L = conv_frames(L, m->cfg.conv_kernel[i], m->cfg.conv_stride[i]);
  return L;
}

namespace {
struct HubertBufs {
  int T[DN_HUBERT_MAX_CONV], tiles, wtiles;
  int64_t max_elems;  // the largest buffer, in elements
  float2* part; float4* stat; int32_t* len1;
  float4 *wpart, *wstat;  // wave_norm
  float* em;              // vocab > 0: the head's output with its pad columns [B S][vocab -> 4]
  void *y0, *cols, *xn, *qkv, *ao, *h;
  float *y, *x0, *xa, *xb, *hf;
};
HubertBufs plan_hubert(const DnHubert* m, int B, int L, Arena& ar) {
  const DnHubertConfig& c = m->cfg;
  const int es = esize(c.dtype), C = c.conv_dim, D = c.dim;
  HubertBufs b;
  int len = L;
  for (int i = 0; i < c.n_conv; ++i) b.T[i] = len = conv_frames(len, c.conv_kernel[i], c.conv_stride[i]);
  const int S = b.T[c.n_conv - 1];
  b.tiles = (b.T[0] + C0_TF - 1) / C0_TF;
  size_t cols = 0;
  for (int i = 1; i < c.n_conv; ++i) cols = std::max(cols, (size_t)b.T[i] * c.conv_kernel[i] * C);
  b.max_elems = (int64_t)B * std::max<int64_t>({(int64_t)b.T[0] * C, (int64_t)cols, (int64_t)S * c.ffn, (int64_t)S * 3 * D,
                                                      (int64_t)S * round_up(c.vocab, 4)});
  b.part = (float2*)ar.take((size_t)B * b.tiles * C * sizeof(float2));
  b.stat = (float4*)ar.take((size_t)B * C * sizeof(float4));
  b.len1 = (int32_t*)ar.take((size_t)B * sizeof(int32_t));
  b.y0 = ar.take((size_t)B * b.T[0] * C * es);
  b.cols = ar.take((size_t)B * cols * es);
  b.y = (float*)ar.take((size_t)B * b.T[1] * C * 4);
  b.x0 = (float*)ar.take((size_t)B * S * D * 4);
  b.xa = (float*)ar.take((size_t)B * S * D * 4);
  b.xb = (float*)ar.take((size_t)B * S * D * 4);
  b.xn = ar.take((size_t)B * S * std::max(C, D) * es);
  b.qkv = ar.take((size_t)B * S * 3 * D * es);
  b.ao = ar.take((size_t)B * S * D * es);
  b.hf = (float*)ar.take((size_t)B * S * c.ffn * 4);
  b.h = ar.take((size_t)B * S * c.ffn * es);
  b.wtiles = (L + WN_TILE - 1) / WN_TILE;
  b.wpart = b.wstat = nullptr;
  b.em = nullptr;
  if (c.wave_norm) {
    b.wpart = (float4*)ar.take((size_t)B * b.wtiles * sizeof(float4));
    b.wstat = (float4*)ar.take((size_t)B * sizeof(float4));
  }
  if (c.vocab > 0) b.em = (float*)ar.take((size_t)B * S * round_up(c.vocab, 4) * 4);
  return b;
}
}  // namespace

extern "C" size_t dn_hubert_workspace_bytes(const DnHubert* m, int32_t B, int32_t L) {
  if (!m || B <= 0 || dn_hubert_out_frames(m, L) < 1) return 0;
  Arena a{nullptr, 0, 0};
  (void)plan_hubert(m, B, L, a);
  return a.off + 512;
}

namespace {
// The pass behind both entries.  emissions == nullptr: `out` = the output of layer n_layers_run - 1 (dn_hubert_forward).  Else every
// layer runs, encoder.layer_norm follows in the pre-norm form (TransformerEncoder.forward with layer None, wav2vec2.py:1001-1007), and
// `out` = emissions fp32 [B, S, vocab] of the CTC head (dn_hubert_ctc_forward).
int hubert_pass(const char* who, DnHubert* m, const float* wave, const int32_t* lengths, int32_t B, int32_t L, int32_t n_layers_run, bool emissions, float* out,
                int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  const DnHubertConfig& c = m->cfg;
  const int S = dn_hubert_out_frames(m, L);
  DN_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && S >= 1, "%s: B=%d L=%d: the waveform is shorter than one frame of the conv stack", who, B, L);
  DN_CHECK_ARG(n_layers_run >= 1 && n_layers_run <= c.layers, "%s: output layer %d outside 1 .. %d", who, n_layers_run, c.layers);
  hipStream_t s = (hipStream_t)stream;
  Arena ar{(char*)workspace, 0, workspace_bytes};
  const HubertBufs b = plan_hubert(m, B, L, ar);
  DN_CHECK_ARG(b.max_elems < (int64_t)1 << 31, "%s: B=%d L=%d: a buffer of %lld elements exceeds 2^31 (rows are indexed in 32 bits): split the batch", who,
               B, L, (long long)b.max_elems);
  DN_TRY(check_workspace(who, workspace, workspace_bytes, ar.off));
  const int dtype = c.dtype, es = esize(dtype), C = c.conv_dim, D = c.dim, F = c.ffn, H = c.heads, dh = D / H;
  ConvGeom g;
  g.n = c.n_conv;
  for (int i = 0; i < DN_HUBERT_MAX_CONV; ++i) { g.k[i] = c.conv_kernel[i]; g.s[i] = c.conv_stride[i]; }
  int ei = 0;
  auto mark = [&]() { m->timer.mark(ei, s); };
  // LayerNorm of x into the fp32 stream `y32` and, as the next contraction's A operand, into xn; in DN_F32 the two are one
  const void* xn = b.xn;
  auto norm_both = [&](const Rows& rr, const float* x, const float* gm, const float* bt, float* y32) {
    layernorm(rr, x, gm, bt, y32, DN_F32);
    if (dtype == DN_F32) xn = y32;
    else { layernorm(rr, x, gm, bt, b.xn, dtype); xn = b.xn; }
  };
  mark();
  // (out_lengths is written first; a failed launch anywhere in the pass is reported by the DN_CHECK_LAUNCH at its end)
  hipLaunchKernelGGL(hubert_lengths_kernel, dim3(1), dim3(256), 0, s, lengths, B, L, g, S, b.len1, out_lengths);
  // ---- conv layer 0 + Fp32GroupNorm + GELU (wav2vec2.py:860-866), statistics per utterance over its own frames
  const int T1 = b.T[0], s0 = c.conv_stride[0];
  if (c.wave_norm) {  // the utterance's own mean and rstd; applied where the first conv stages its samples
    hipLaunchKernelGGL(wave_stats_kernel, dim3(b.wtiles, B), dim3(256), 0, s, wave, lengths, L, b.wpart);
    hipLaunchKernelGGL(wave_combine_kernel, dim3((B + 63) / 64), dim3(64), 0, s, b.wpart, lengths, B, L, b.wtiles, b.wstat);
  }
  if (c.extractor_ln) {  // conv + bias + Fp32LayerNorm over the channels + GELU, one kernel (wav2vec2.py:849-859)
    hipLaunchKernelGGL(conv0_ln_kernel, dim3(b.tiles, B), dim3(256), 0, s, wave, lengths, L, T1, C, s0, m->conv0_w, c.conv_bias ? m->conv_b : m->zeros, m->cln_g,
                       m->cln_b, b.wstat, b.y0, dtype);
  } else {
    hipLaunchKernelGGL(conv0_stats_kernel, dim3(b.tiles, B), dim3(256), 0, s, wave, lengths, b.len1, L, C, s0, m->conv0_w, b.part);
    hipLaunchKernelGGL(conv0_combine_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, b.part, b.len1, B, C, b.tiles, b.stat);
    hipLaunchKernelGGL(conv0_apply_kernel, dim3(b.tiles, B), dim3(256), 0, s, wave, lengths, L, T1, C, s0, m->conv0_w, m->gn_g, m->gn_b, b.stat, b.y0, dtype);
  }
  mark();
  // ---- conv layers 1.. + GELU (:867-868): gathered rows, one contraction each; y holds layer i's pre-activation
  for (int i = 1; i < c.n_conv; ++i) {
    const int k = c.conv_kernel[i], st = c.conv_stride[i], Tin = b.T[i - 1], Tout = b.T[i];
    const int grid = ew_grid((int64_t)B * Tout * k * C / 4);
    if (i == 1 || c.extractor_ln)
      hipLaunchKernelGGL((strided_taps_kernel<false>), dim3(grid), dim3(256), 0, s, b.y0, dtype, B, Tin, Tout, C, k, st, b.cols, dtype);
    else
      hipLaunchKernelGGL((strided_taps_kernel<true>), dim3(grid), dim3(256), 0, s, b.y, DN_F32, B, Tin, Tout, C, k, st, b.cols, dtype);
    DN_TRY(linear(Rows{dtype, B * Tout, Tout, 0, s}, b.cols, k * C, m->conv_W[i], c.conv_bias ? m->conv_b + (size_t)i * C : m->zeros, C, DN_EPI_BIAS, b.y,
                  DN_F32));
    if (c.extractor_ln) {  // the norm sits between the conv and the GELU: one row kernel, into the next gather's input (the last: fp32, in place)
      const bool last = i + 1 == c.n_conv;
      layernorm_gelu(Rows{dtype, B * Tout, Tout, C, s}, b.y, m->cln_g + (size_t)i * C, m->cln_b + (size_t)i * C, last ? (void*)b.y : b.y0, last ? DN_F32 : dtype);
    }
  }
  const Rows rc{dtype, B * S, S, C, s}, r{dtype, B * S, S, D, s};
  if (!c.extractor_ln)
    hipLaunchKernelGGL(gelu_rows_kernel, dim3(ew_grid((int64_t)rc.M * C / 4)), dim3(256), 0, s, b.y, b.y, DN_F32, (int64_t)rc.M * C / 4);
  mark();
  // ---- layer_norm, post_extract_proj (hubert.py:445-453)
  if (c.has_proj) {
    layernorm(rc, b.y, m->ln_g, m->ln_b, b.xn, dtype);
    DN_TRY(linear(rc, b.xn, C, m->proj_W, m->proj_b, D, DN_EPI_BIAS, b.x0, DN_F32));
  } else {
    layernorm(rc, b.y, m->ln_g, m->ln_b, b.x0, DN_F32);
  }
  // ---- x + gelu(SamePad(pos_conv(x))), encoder.layer_norm (wav2vec2.py:1020-1025); frames outside the utterance are zeros
  DN_TRY(dn_grouped_conv1d(b.x0, m->pos_w, m->pos_b, b.xa, out_lengths, B, S, D, c.conv_pos_groups, c.conv_pos, s));
  mark();
  float *cur = b.xa, *other = b.xb;
  // the two halves of layer l, on the normalised rows `in` and the residual stream x: x += out_proj(attention(qkv(in))) over the
  // utterance's own frames, and x += fc2(gelu(fc1(in))) (fc1 lands in fp32, the GELU rounds it to the operand type)
  auto self_attn = [&](int l, const void* in, float* x) {
    return self_attention_block(r, H, dh, in, layer_mat(m->qkv_W, l, 3 * D, D, es), m->qkv_b + (size_t)l * 3 * D, layer_mat(m->out_W, l, D, D, es),
                                m->out_b + (size_t)l * D, b.qkv, b.ao, out_lengths, x);
  };
  auto ffn = [&](int l, const void* in, float* x) {
    DN_TRY(linear(r, in, D, layer_mat(m->fc1_W, l, F, D, es), m->fc1_b + (size_t)l * F, F, DN_EPI_BIAS, b.hf, DN_F32));
    hipLaunchKernelGGL(gelu_rows_kernel, dim3(ew_grid((int64_t)r.M * F / 4)), dim3(256), 0, s, b.hf, b.h, dtype, (int64_t)r.M * F / 4);
    return linear_resadd(r, b.h, F, layer_mat(m->fc2_W, l, D, F, es), m->fc2_b + (size_t)l * D, x);
  };
  if (c.pre_norm) {  // no encoder.layer_norm in front of pre-norm layers (:1024): the stream stays in b.xa
    for (int l = 0; l < n_layers_run; ++l) {  // layer_norm_first True (:1235-1257): x += attn(LN1(x)); x += fc2(gelu(fc1(LN2(x))))
      const float* lg = m->lng + (size_t)l * 2 * D;
      const float* lb = m->lnb + (size_t)l * 2 * D;
      layernorm(r, cur, lg, lb, b.xn, dtype);
      DN_TRY(self_attn(l, b.xn, cur));
      layernorm(r, cur, lg + D, lb + D, b.xn, dtype);
      DN_TRY(ffn(l, b.xn, cur));
    }
  } else {
    std::swap(cur, other);
    norm_both(r, b.xa, m->enc_g, m->enc_b, cur);
    for (int l = 0; l < n_layers_run; ++l) {  // TransformerSentenceEncoderLayer.forward, layer_norm_first False (:1258-1283)
      const float* lg = m->lng + (size_t)l * 2 * D;
      const float* lb = m->lnb + (size_t)l * 2 * D;
      DN_TRY(self_attn(l, xn, cur));
      norm_both(r, cur, lg, lb, other);  // self_attn_layer_norm BEHIND the residual
      std::swap(cur, other);
      DN_TRY(ffn(l, xn, cur));
      if (l + 1 < n_layers_run) norm_both(r, cur, lg + D, lb + D, other);  // final_layer_norm
      else layernorm(r, cur, lg + D, lb + D, other, DN_F32);
      std::swap(cur, other);
    }
  }
  mark();
  if (emissions) {  // encoder.layer_norm (the head exists in the pre-norm form only) -> proj (wav2vec2_asr.py:494-495); the pad columns stay
    // in the workspace.  Always the DN_F32 contraction on the fp32 stream, whatever the engine's arithmetic, as dn_kmeans_assign's: a
    // letter is a decision
    const int V = c.vocab, Vp = round_up(V, 4);
    layernorm(r, cur, m->enc_g, m->enc_b, b.xb, DN_F32);
    DN_TRY(linear(Rows{DN_F32, r.M, S, D, s}, b.xb, D, m->head_W, m->head_b, Vp, DN_EPI_BIAS, b.em, DN_F32));
    hipLaunchKernelGGL(emit_rows_kernel, dim3(ew_grid((int64_t)r.M * V)), dim3(256), 0, s, b.em, Vp, out_lengths, B, S, V, out);
  } else {
    hipLaunchKernelGGL(masked_copy_kernel, dim3(ew_grid((int64_t)r.M * D / 4)), dim3(256), 0, s, cur, out_lengths, B, S, D, out);
  }
  mark();
  DN_CHECK_LAUNCH(who);
  return DN_OK;
}
}  // namespace

extern "C" int dn_hubert_forward(DnHubert* m, const float* wave, const int32_t* lengths, int32_t B, int32_t L, int32_t n_layers_run, float* out,
                                 int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && wave && lengths && out && out_lengths && workspace, "dn_hubert_forward: null argument");
  return hubert_pass("dn_hubert_forward", m, wave, lengths, B, L, n_layers_run, false, out, out_lengths, workspace, workspace_bytes, stream);
}

extern "C" int dn_hubert_ctc_forward(DnHubert* m, const float* wave, const int32_t* lengths, int32_t B, int32_t L, float* emissions, int32_t* out_lengths,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && wave && lengths && emissions && out_lengths && workspace, "dn_hubert_ctc_forward: null argument");
  DN_CHECK_ARG(m->cfg.vocab > 0, "dn_hubert_ctc_forward: the engine was created without a CTC head (vocab 0)");
  return hubert_pass("dn_hubert_ctc_forward", m, wave, lengths, B, L, m->cfg.layers, true, emissions, out_lengths, workspace, workspace_bytes, stream);
}

extern "C" int dn_ctc_greedy(const float* emissions, const int32_t* lengths, int32_t B, int32_t S, int32_t V, int32_t blank, int32_t* tokens_out,
                             int32_t* counts_out, void* stream) {
  DN_CHECK_ARG(emissions && lengths && tokens_out && counts_out, "dn_ctc_greedy: null argument");
  DN_CHECK_ARG(B > 0 && S > 0 && V > 0 && blank >= 0 && blank < V, "dn_ctc_greedy: B=%d S=%d V=%d blank=%d (inside the vocabulary)", B, S, V, blank);
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, emissions, lengths, S, V, blank, tokens_out, counts_out);
  DN_CHECK_LAUNCH("dn_ctc_greedy");
  return DN_OK;
}
