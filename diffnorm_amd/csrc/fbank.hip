// Kaldi-compliant log-mel filterbank features + utterance CMVN, waveform -> [B, Lf, n_mels]: the first box of the S2UT leg, what the
// reference computes on the CPU one utterance at a time with get_fbank (fairseq/data/audio/audio_utils.py:242-277 ->
// torchaudio.compliance.kaldi.fbank at its defaults, dither 0) and UtteranceCMVN (fairseq/data/audio/feature_transforms/
// utterance_cmvn.py:30-41).  The definition is written out in include/diffnorm_hip.h.
//   fbank_lengths_kernel   out_lengths[b] = frames of min(lengths[b], L) samples
//   fbank_frames_kernel    a workgroup = FB_POINTS / n_fft consecutive frames of ONE utterance, counted from its frame 0: their samples
//                          staged in LDS once, then per frame DC removal, pre-emphasis, window, an n_fft / 2-point complex transform of
//                          the even / odd samples (radix-2 Stockham, ping-pong in LDS, natural order in and out), the real-input
//                          post-pass, power, the mel filters over their own bins only, log
//   cmvn_stats_kernel / cmvn_combine_kernel / cmvn_apply_kernel
//                          per (utterance, FB_CHUNK-frame chunk counted from frame 0, column) the chunk mean and the sum of squared
//                          deviations from it in double; the chunks combined in chunk order (Chan et al.); the normalisation in place
// A frame's values depend on its own samples only (every sum runs in a fixed order set by the configuration), a column's statistics
// on the utterance's own frame count only: a ragged batch gives every utterance what it gets alone, bit for bit.  No atomics.
#include <float.h>
#include <math.h>

#include <new>
#include <vector>

#include "common.h"
#include "engine.h"

using namespace dn;

// The phases of fbank_frames_kernel are plain functions of (thread index, LDS image).  tools/fbank_phases_host.hip defines
// DN_FB_PHASE as `__host__ __device__ inline`, includes this file and steps them on the CPU one thread at a time, built with the host
// sanitizers (tests/test_fbank_host.py runs it against the float64 restatement).
#ifndef DN_FB_PHASE
#define DN_FB_PHASE __device__ __forceinline__
#endif

namespace dn {
namespace {

constexpr int FB_NT = 256;         // threads of a frames workgroup
constexpr int FB_POINTS = 4096;    // frames per workgroup x n_fft: 16 / 8 / 4 frames at n_fft 256 / 512 / 1024
constexpr int FB_MAX_FFT = 1024;
constexpr int FB_MAX_MELS = 128;
constexpr int FB_CHUNK = 64;       // frames per CMVN statistics chunk

struct FbGeom {
  int W, S, N, H, lgH, M, F, T;  // window, shift, n_fft, H = N / 2 complex points, n_mels, F frames per workgroup, T = FB_NT / F threads per frame
  float scale, preemph, log_floor;  // log_floor = log(FLT_EPSILON) rounded once from double (the device logf may sit an ulp beside it)
  int remove_dc;
};
struct FbRanges { uint16_t lo[FB_MAX_MELS], hi[FB_MAX_MELS]; };  // filter m is non-zero on the bins [lo, hi)

// a, b: the transform's ping-pong buffers, frame f at [f N, (f + 1) N) as re[H] | im[H].  The staged samples (W + S (F - 1) <= F N
// floats, S <= W <= N) live in b until the window phase has read them.  Every butterfly stage READS at unit stride (t and t + H / 2)
// and writes runs of `s` elements 2 s apart: at s < 32 a 2-way bank conflict of 4-byte LDS stores, which costs no extra cycle (the
// store's issue takes as long), so the power-of-two strides need no padding in this form; the post-pass reads k and H - k, both unit
// stride.
struct FbLds {
  float a[FB_POINTS], b[FB_POINTS];
  float2 tw[FB_MAX_FFT / 2];  // (cos, -sin)(2 pi k / N), k < H
  float part[FB_NT];
};

// b[i] = scale * wave[f0 S + i] for the samples the utterance owns, zeros behind them (never a read at or past its length)
DN_FB_PHASE void fb_stage(int tid, FbLds& l, const FbGeom& g, const float* __restrict__ row, int avail, const float2* __restrict__ tw) {
  const int n = g.W + g.S * (g.F - 1);
  for (int i = tid; i < n; i += FB_NT) l.b[i] = i < avail ? row[i] * g.scale : 0.f;
  for (int i = tid; i < g.H; i += FB_NT) l.tw[i] = tw[i];
}

// thread (f, t): the sum of samples t, t + T, .. of frame f
DN_FB_PHASE void fb_partial_sums(int tid, FbLds& l, const FbGeom& g) {
  const int f = tid / g.T, t = tid - f * g.T;
  float s = 0.f;
  for (int j = t; j < g.W; j += g.T) s += l.b[f * g.S + j];
  l.part[tid] = s;
}

// z[n] = x[2 n] + i x[2 n + 1] of the frame: mean removed, pre-emphasised (f[-1] := f[0]), windowed, zero-padded
DN_FB_PHASE void fb_window(int tid, FbLds& l, const FbGeom& g, const float* __restrict__ window) {
  const int f = tid / g.T, t = tid - f * g.T;
  float mean = 0.f;
  if (g.remove_dc) {
    float s = 0.f;
    for (int i = 0; i < g.T; ++i) s += l.part[f * g.T + i];
    mean = s / (float)g.W;
  }
  const float* x = l.b + f * g.S;
  float* z = l.a + f * g.N;
  for (int j = t; j < g.N; j += g.T) {
    float v = 0.f;
    if (j < g.W) v = fmaf(-g.preemph, x[j ? j - 1 : 0] - mean, x[j] - mean) * window[j];
    z[(j & 1) * g.H + (j >> 1)] = v;
  }
}

// One radix-2 Stockham stage at stride s = 2^lgs over every frame: butterfly t = p s + q reads x[t], x[t + H / 2] and writes
// y[2 p s + q] = a + b, y[2 p s + q + s] = (a - b) exp(-2 pi i p s / H)
DN_FB_PHASE void fb_butterflies(int tid, const float* src, float* dst, const FbLds& l, const FbGeom& g, int lgs) {
  const int hh = g.H >> 1, s = 1 << lgs;
  for (int u = tid; u < g.F * hh; u += FB_NT) {
    const int f = u >> (g.lgH - 1), t = u & (hh - 1), p = t >> lgs, q = t & (s - 1);
    const float *xr = src + f * g.N, *xi = xr + g.H;
    float *yr = dst + f * g.N, *yi = yr + g.H;
    const float ar = xr[t], ai = xi[t], br = xr[t + hh], bi = xi[t + hh];
    const float2 w = l.tw[(2 * p) << lgs];
    const int o = ((2 * p) << lgs) + q;
    yr[o] = ar + br;
    yi[o] = ai + bi;
    const float dr = ar - br, di = ai - bi;
    yr[o + s] = fmaf(dr, w.x, -(di * w.y));
    yi[o + s] = fmaf(dr, w.y, di * w.x);
  }
}

// X[k] = E[k] + exp(-2 pi i k / N) O[k], k = 0 .. H, with E = (Z[k] + conj Z[H - k]) / 2 and O = (Z[k] - conj Z[H - k]) / (2 i) the
// transforms of the even and the odd samples (Z[H] := Z[0]); dst[f N + k] = |X[k]|^2
DN_FB_PHASE void fb_power(int tid, const float* src, float* dst, const FbLds& l, const FbGeom& g) {
  const int n = g.H + 1;
  for (int u = tid; u < g.F * n; u += FB_NT) {
    const int f = u / n, k = u - f * n, k0 = k & (g.H - 1), k1 = (g.H - k) & (g.H - 1);
    const float *zr = src + f * g.N, *zi = zr + g.H;
    const float ar = zr[k0], ai = zi[k0], br = zr[k1], bi = -zi[k1];
    const float er = 0.5f * (ar + br), ei = 0.5f * (ai + bi);
    const float orr = 0.5f * (ai - bi), oi = -0.5f * (ar - br);
    const float2 w = k < g.H ? l.tw[k] : make_float2(-1.f, 0.f);
    const float xr = er + fmaf(orr, w.x, -(oi * w.y)), xi = ei + fmaf(orr, w.y, oi * w.x);
    dst[f * g.N + k] = fmaf(xr, xr, xi * xi);
  }
}

// rows[f][m] = log(max(sum_k mel[m][k] P[f][k], FLT_EPSILON)) over filter m's own bins, in bin order; zeros for the frames the
// utterance does not have (f >= nf) among the nrows rows of the output this workgroup owns
DN_FB_PHASE void fb_mel(int tid, const float* pw, const FbGeom& g, const float* __restrict__ mel, const FbRanges& r, float* __restrict__ rows, int nf,
                        int nrows) {
  for (int u = tid; u < nrows * g.M; u += FB_NT) {
    const int f = u / g.M, m = u - f * g.M;
    float v = 0.f;
    if (f < nf) {
      const float* p = pw + f * g.N;
      const float* wm = mel + (size_t)m * (g.H + 1);
      float e = 0.f;
      for (int k = r.lo[m]; k < r.hi[m]; ++k) e = fmaf(wm[k], p[k], e);
      v = e > FLT_EPSILON ? logf(e) : g.log_floor;
    }
    rows[u] = v;
  }
}

__host__ __device__ __forceinline__ int fb_frames(int n, int W, int S) { return n >= W ? 1 + (n - W) / S : 0; }
__host__ __device__ __forceinline__ int fb_clamp_len(int len, int L) { return len < 0 ? 0 : len > L ? L : len; }

__global__ void fbank_lengths_kernel(const int32_t* __restrict__ lengths, int B, int L, int W, int S, int32_t* __restrict__ out_len) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) out_len[b] = fb_frames(fb_clamp_len(lengths[b], L), W, S);
}

__global__ __launch_bounds__(FB_NT) void fbank_frames_kernel(const float* __restrict__ wave, const int32_t* __restrict__ lengths,
                                                             const int32_t* __restrict__ out_len, int L, int Lf, FbGeom g, FbRanges r,
                                                             const float* __restrict__ window, const float2* __restrict__ tw,
                                                             const float* __restrict__ mel, float* __restrict__ out) {
  __shared__ FbLds l;
  const int tid = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * g.F;
  const int nrows = Lf - f0 < g.F ? Lf - f0 : g.F;
  const int nf = out_len[b] - f0 < nrows ? out_len[b] - f0 : nrows;
  float* rows = out + ((int64_t)b * Lf + f0) * g.M;
  if (nf <= 0) {  // the whole tile lies behind the utterance
    for (int i = tid; i < nrows * g.M; i += FB_NT) rows[i] = 0.f;
    return;
  }
  fb_stage(tid, l, g, wave + (int64_t)b * L + (int64_t)f0 * g.S, fb_clamp_len(lengths[b], L) - f0 * g.S, tw);
  __syncthreads();
  fb_partial_sums(tid, l, g);
  __syncthreads();
  fb_window(tid, l, g, window);
  __syncthreads();
  float *src = l.a, *dst = l.b;
  for (int lgs = 0; lgs < g.lgH; ++lgs) {
    fb_butterflies(tid, src, dst, l, g, lgs);
    __syncthreads();
    float* t = src; src = dst; dst = t;
  }
  fb_power(tid, src, dst, l, g);
  __syncthreads();
  fb_mel(tid, dst, g, mel, r, rows, nf, nrows);
}

// per (utterance, chunk, column): the chunk's mean and its sum of squared deviations from that mean, in double (a column of equal
// values has exactly that value as its mean and M2 = 0)
__global__ __launch_bounds__(FB_MAX_MELS) void cmvn_stats_kernel(const float* __restrict__ x, const int32_t* __restrict__ out_len, int Lf, int M,
                                                                 double2* __restrict__ part) {
  const int c = blockIdx.x, b = blockIdx.y, m = threadIdx.x;
  int n = out_len[b] - c * FB_CHUNK;
  n = n > FB_CHUNK ? FB_CHUNK : n;
  if (m >= M || n <= 0) return;
  const float* col = x + ((int64_t)b * Lf + (int64_t)c * FB_CHUNK) * M + m;
  double sum = 0;
  for (int f = 0; f < n; ++f) sum += (double)col[(int64_t)f * M];
  const double mean = sum / n;
  double m2 = 0;
  for (int f = 0; f < n; ++f) {
    const double d = (double)col[(int64_t)f * M] - mean;
    m2 = fma(d, d, m2);
  }
  part[((int64_t)b * gridDim.x + c) * M + m] = make_double2(mean, m2);
}

// the chunks' (count, mean, M2) combined in chunk order: stat[b][m] = (mean hi, mean lo, std, 0), var = M2 / n = E[x^2] - mean^2,
// std = sqrt(max(var, 1e-10)) (utterance_cmvn.py:37-38)
__global__ __launch_bounds__(256) void cmvn_combine_kernel(const double2* __restrict__ part, const int32_t* __restrict__ out_len, int B, int M, int chunks,
                                                           float4* __restrict__ stat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * M) return;
  const int b = i / M, m = i - b * M;
  ChanAcc a;
  for (int c = 0; c < chunks; ++c) {
    int nb = out_len[b] - c * FB_CHUNK;
    if (nb <= 0) break;
    nb = nb > FB_CHUNK ? FB_CHUNK : nb;
    const double2 p = part[((int64_t)b * chunks + c) * M + m];
    a.add(nb, p.x, p.y);
  }
  float4 o = make_float4(0.f, 0.f, 1.f, 0.f);
  if (a.n > 0) {
    const double var = a.m2 / a.n;
    a.split(o.x, o.y);
    o.z = (float)sqrt(var > 1e-10 ? var : 1e-10);
  }
  stat[i] = o;
}

// x = x - mean (norm_means), x = x / std (norm_vars) on the utterance's own rows (:34-39); the zero rows behind them stay
__global__ __launch_bounds__(256) void cmvn_apply_kernel(float* __restrict__ x, const int32_t* __restrict__ out_len, const float4* __restrict__ stat, int B,
                                                         int Lf, int M, int norm_means, int norm_vars) {
  const int64_t n = (int64_t)B * Lf * M;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i % M);
    const int64_t row = i / M;
    const int t = (int)(row % Lf), b = (int)(row / Lf);
    if (t >= out_len[b]) continue;
    const float4 st = stat[b * M + m];
    float v = x[i];
    if (norm_means) v = (v - st.x) - st.y;
    if (norm_vars) v = v / st.z;
    x[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
double fb_mel_of(double hz) { return 1127.0 * log(1.0 + hz / 700.0); }

int fb_check(const char* who, const DnFbankConfig* c) {
  DN_CHECK_ARG(c != nullptr, "%s: null configuration", who);
  DN_CHECK_ARG(c->sample_rate > 0.f, "%s: sample rate %g", who, (double)c->sample_rate);
  DN_CHECK_ARG(c->n_fft == 256 || c->n_fft == 512 || c->n_fft == 1024, "%s: n_fft %d (the transform is built for 256, 512 and 1024 points)", who, c->n_fft);
  DN_CHECK_ARG(c->frame_length >= 2 && c->frame_length <= c->n_fft, "%s: frame length %d samples outside [2, n_fft = %d]", who, c->frame_length, c->n_fft);
  DN_CHECK_ARG(c->frame_shift >= 1 && c->frame_shift <= c->frame_length, "%s: frame shift %d samples outside [1, frame length = %d]", who, c->frame_shift,
               c->frame_length);
  DN_CHECK_ARG(c->n_mels >= 1 && c->n_mels <= FB_MAX_MELS, "%s: %d mel bins outside [1, %d]", who, c->n_mels, FB_MAX_MELS);
  const double nyq = 0.5 * (double)c->sample_rate, hi = c->high_freq == 0.f ? nyq : (double)c->high_freq;
  DN_CHECK_ARG(c->low_freq >= 0.f && hi <= nyq && (double)c->low_freq < hi, "%s: mel band [%g, %g] Hz must satisfy 0 <= low < high <= Nyquist = %g (high 0 = Nyquist)", who,
               (double)c->low_freq, (double)c->high_freq, nyq);
  DN_CHECK_ARG(isfinite(c->preemphasis) && isfinite(c->input_scale) && c->input_scale != 0.f, "%s: pre-emphasis %g, input scale %g", who, (double)c->preemphasis,
               (double)c->input_scale);
  return DN_OK;
}

// weight of FFT bin k in filter m (torchaudio.compliance.kaldi.get_mel_banks without vtln), in double
double fb_mel_weight(const DnFbankConfig& c, int m, int k) {
  if (k >= c.n_fft / 2) return 0.0;  // the Nyquist column
  const double nyq = 0.5 * (double)c.sample_rate, hi = c.high_freq == 0.f ? nyq : (double)c.high_freq;
  const double mlo = fb_mel_of((double)c.low_freq), mhi = fb_mel_of(hi), delta = (mhi - mlo) / (c.n_mels + 1);
  const double left = mlo + m * delta, centre = mlo + (m + 1) * delta, right = mlo + (m + 2) * delta;
  const double mel = fb_mel_of((double)k * (double)c.sample_rate / (double)c.n_fft);
  const double up = (mel - left) / (centre - left), down = (right - mel) / (right - centre);
  const double w = up < down ? up : down;
  return w > 0.0 ? w : 0.0;
}

int fb_lg2(int n) {
  int l = 0;
  while ((1 << l) < n) ++l;
  return l;
}

}  // namespace
}  // namespace dn

extern "C" int dn_fbank_tables(const DnFbankConfig* cfg, float* window, float* mel) {
  DN_TRY(fb_check("dn_fbank_tables", cfg));
  DN_CHECK_ARG(window && mel, "dn_fbank_tables: null table");
  const int W = cfg->frame_length, nb = cfg->n_fft / 2 + 1;
  for (int j = 0; j < W; ++j) window[j] = (float)pow(0.5 - 0.5 * cos(2.0 * M_PI * j / (W - 1)), 0.85);
  for (int m = 0; m < cfg->n_mels; ++m)
    for (int k = 0; k < nb; ++k) mel[(size_t)m * nb + k] = (float)fb_mel_weight(*cfg, m, k);
  return DN_OK;
}

extern "C" int dn_fbank_twiddles(int32_t n_fft, float* tw) {
  DN_CHECK_ARG(tw && (n_fft == 256 || n_fft == 512 || n_fft == 1024), "dn_fbank_twiddles: n_fft %d (256, 512 or 1024)", n_fft);
  for (int k = 0; k < n_fft / 2; ++k) {
    const double a = 2.0 * M_PI * k / n_fft;
    tw[2 * k] = (float)cos(a);
    tw[2 * k + 1] = (float)-sin(a);
  }
  return DN_OK;
}

struct DnFbank {
  DnFbankConfig cfg;
  FbGeom g;
  FbRanges r;
  const float *window, *mel;
  const float2* tw;
};

extern "C" int dn_fbank_create(const DnFbankConfig* cfg, const void* const* tables, int32_t n_tables, DnFbank** out) {
  DN_TRY(fb_check("dn_fbank_create", cfg));
  DN_CHECK_ARG(tables && out && n_tables == 3 && tables[0] && tables[1] && tables[2], "dn_fbank_create: three tables (window, mel, twiddles) expected");
  DnFbank* m = new (std::nothrow) DnFbank();
  DN_CHECK_ARG(m != nullptr, "dn_fbank_create: out of host memory");
  m->cfg = *cfg;
  FbGeom& g = m->g;
  g.W = cfg->frame_length; g.S = cfg->frame_shift; g.N = cfg->n_fft; g.H = g.N / 2; g.lgH = fb_lg2(g.H); g.M = cfg->n_mels;
  g.F = FB_POINTS / g.N; g.T = FB_NT / g.F;
  g.scale = cfg->input_scale; g.preemph = cfg->preemphasis; g.log_floor = (float)log((double)FLT_EPSILON); g.remove_dc = cfg->remove_dc_offset != 0;
  for (int f = 0; f < FB_MAX_MELS; ++f) m->r.lo[f] = m->r.hi[f] = 0;
  // The bins of filter f that carry weight AS ROUNDED in dn_fbank_tables' table: [lo, hi).  The tables live on the device and are
  // not read here, so the ranges come from the same function that filled them: the mel table MUST be dn_fbank_tables' for this cfg.
  for (int f = 0; f < g.M; ++f) {
    int lo = g.H + 1, hi = 0;
    for (int k = 0; k <= g.H; ++k)
      if ((float)fb_mel_weight(*cfg, f, k) != 0.f) { lo = k < lo ? k : lo; hi = k + 1; }
    m->r.lo[f] = (uint16_t)(hi ? lo : 0);
    m->r.hi[f] = (uint16_t)hi;
  }
  m->window = (const float*)tables[0]; m->mel = (const float*)tables[1]; m->tw = (const float2*)tables[2];
  *out = m;
  return DN_OK;
}

extern "C" void dn_fbank_destroy(DnFbank* m) { delete m; }

extern "C" int32_t dn_fbank_out_frames(const DnFbank* m, int32_t L) { return m ? fb_frames(L, m->g.W, m->g.S) : 0; }

namespace {
struct FbBufs { double2* part; float4* stat; int chunks; };
FbBufs plan_fbank(const DnFbank* m, int B, int Lf, Arena& ar) {
  FbBufs b;
  b.chunks = (Lf + FB_CHUNK - 1) / FB_CHUNK;
  b.part = (double2*)ar.take((size_t)B * b.chunks * m->g.M * sizeof(double2));
  b.stat = (float4*)ar.take((size_t)B * m->g.M * sizeof(float4));
  return b;
}
}  // namespace

extern "C" size_t dn_fbank_workspace_bytes(const DnFbank* m, int32_t B, int32_t L) {
  if (!m || B <= 0) return 0;
  Arena a{nullptr, 0, 0};
  if (m->cfg.cmvn) (void)plan_fbank(m, B, dn_fbank_out_frames(m, L), a);
  return a.off + 512;
}

extern "C" int dn_fbank_forward(DnFbank* m, const float* wave, const int32_t* lengths, int32_t B, int32_t L, float* out, int32_t* out_lengths,
                                void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && wave && lengths && out_lengths, "dn_fbank_forward: null argument");
  DN_CHECK_ARG(B > 0 && B <= 65535 && L > 0, "dn_fbank_forward: B=%d (1 .. 65535) L=%d", B, L);
  const FbGeom& g = m->g;
  const int Lf = dn_fbank_out_frames(m, L);
  hipStream_t s = (hipStream_t)stream;
  const bool cmvn = Lf > 0 && m->cfg.cmvn && (m->cfg.norm_means || m->cfg.norm_vars);
  // every argument is checked before the first launch: a refused call has written nothing
  DN_CHECK_ARG(Lf == 0 || out != nullptr, "dn_fbank_forward: null output");
  FbBufs b{nullptr, nullptr, 0};
  if (cmvn) {
    DN_CHECK_ARG(workspace, "dn_fbank_forward: null workspace (CMVN needs one)");
    Arena ar{(char*)workspace, 0, workspace_bytes};
    b = plan_fbank(m, B, Lf, ar);
    DN_TRY(check_workspace("dn_fbank_forward", workspace, workspace_bytes, ar.off));
  }
  hipLaunchKernelGGL(fbank_lengths_kernel, dim3((B + 255) / 256), dim3(256), 0, s, lengths, B, L, g.W, g.S, out_lengths);
  if (Lf > 0)
    hipLaunchKernelGGL(fbank_frames_kernel, dim3((Lf + g.F - 1) / g.F, B), dim3(FB_NT), 0, s, wave, lengths, out_lengths, L, Lf, g, m->r, m->window, m->tw, m->mel,
                       out);
  if (cmvn) {
    hipLaunchKernelGGL(cmvn_stats_kernel, dim3(b.chunks, B), dim3(FB_MAX_MELS), 0, s, out, out_lengths, Lf, g.M, b.part);
    hipLaunchKernelGGL(cmvn_combine_kernel, dim3((B * g.M + 255) / 256), dim3(256), 0, s, b.part, out_lengths, B, g.M, b.chunks, b.stat);
    hipLaunchKernelGGL(cmvn_apply_kernel, dim3(ew_grid((int64_t)B * Lf * g.M)), dim3(256), 0, s, out, out_lengths, b.stat, B, Lf, g.M, m->cfg.norm_means,
                       m->cfg.norm_vars);
  }
  DN_CHECK_LAUNCH("dn_fbank_forward");
  return DN_OK;
}
