// Sample-rate conversion in front of the three waveform front ends, [B, L, C] samples -> [B, Lo] mono fp32: what the reference's
// loaders do with torchaudio.functional.resample (examples/speech_to_speech/asr_bleu/utils.py:231-237) and convert_waveform's
// to_mono (fairseq/data/audio/audio_utils.py:49-50).  The definition is written out in include/diffnorm_hip.h; the filter bank is
// computed in diffnorm_amd/resample.py.
//   resample_kernel   a workgroup = one tile of Tt = F * new consecutive output samples of ONE utterance, counted from its output 0:
//                     the F * orig + K - orig input samples the tile needs are staged in LDS once -- converted, down-mixed, zeros
//                     outside [0, len) -- then output i * new + p = sum_k bank[p][k] * x[i * orig + k], k ascending, fp32 FMAs.
//                     The bank comes from LDS (rows K | 1 floats apart) or, when it does not fit, from its transposed copy in
//                     global memory (lanes on consecutive phases read consecutive floats); the products and their order are the
//                     same, so the two paths give identical bits.
// LDS banking (ds_read_b32: 32 banks, conflicts per 32-lane half): lane o reads x[(o / new) * orig + k].  An odd orig is a
// conflict-free stride as it is; an even one (2 : 1, 2 : 3, 4 : 1) puts lanes l and l + 16 on one bank, so for even orig sample a
// lives at a + a / 32, which moves every 32-float row one bank on.  Bank rows of an odd length keep the `new` phases of a half-wave
// (2 : 3 reads three of them at once) on different banks.  Global loads and stores are one coalesced dword per lane: neither the
// input span (it starts width samples before a multiple of orig, times the channel count) nor an output row ([B, Lo] with any Lo) has
// an alignment a wider access could rely on.
// A tile's values depend on the utterance's own samples and length only: a ragged batch gives every utterance what it gets alone,
// bit for bit.  No atomics.
#include <new>

#include "common.h"
#include "engine.h"

using namespace dn;

namespace dn {
namespace {

constexpr int RS_NT = 256;         // threads of a workgroup
constexpr int RS_TILE = 1024;      // output samples a tile aims at: F = max(1, RS_TILE / new) frames, Tt = F * new
constexpr int RS_X_MAX = 8192;     // floats of the staged input span, skew included (32 KiB)
constexpr int RS_TAB_MAX = 8192;   // floats of a bank that is staged in LDS beside the span (32 KiB): new * (K | 1) <= RS_TAB_MAX

struct RsGeom {
  int orig, nw, width, K, KS;  // KS = K | 1: floats between the bank's rows in LDS
  int F, Tt, span;             // frames per tile, outputs per tile, staged samples of a full tile = F * orig + K - orig
  int sh;                      // sample a of the span lives at a + (a >> sh): 5 for even orig, 31 (no skew) for odd
  int xs_floats;               // floats of the span's LDS image
};

__host__ __device__ __forceinline__ int rs_clamp_len(int len, int L) { return len < 0 ? 0 : len > L ? L : len; }
__host__ __device__ __forceinline__ int64_t rs_out_len(int64_t n, int orig, int nw) { return n <= 0 ? 0 : ((int64_t)nw * n + orig - 1) / orig; }

// sample `pos` of utterance row `row` ([L][C] interleaved): converted, the channels summed in channel order and divided by their count
template <typename T>
__device__ __forceinline__ float rs_load(const T* __restrict__ row, int64_t pos, int C) {
  const T* p = row + pos * C;
  constexpr float scale = sizeof(T) == 2 ? 1.f / 32768.f : 1.f;
  float s = (float)p[0] * scale;
  if (C == 1) return s;
  for (int c = 1; c < C; ++c) s += (float)p[c] * scale;
  return s / (float)C;
}

template <bool TAB_LDS, typename T>
__global__ __launch_bounds__(RS_NT) void resample_kernel(const T* __restrict__ in, int C, const int32_t* __restrict__ lengths, int L, int Lo, RsGeom g,
                                                         const float* __restrict__ bank, const float* __restrict__ bankT, float* __restrict__ out,
                                                         int32_t* __restrict__ out_len) {
  extern __shared__ float rs_lds[];
  float* xs = rs_lds;
  float* ts = rs_lds + g.xs_floats;
  const int tid = threadIdx.x, b = blockIdx.y;
  const int t0 = blockIdx.x * g.Tt;  // < Lo
  const int len = rs_clamp_len(lengths[b], L);
  const int olen = (int)rs_out_len(len, g.orig, g.nw);  // <= Lo, which the host has checked to fit an int
  if (blockIdx.x == 0 && tid == 0) out_len[b] = olen;
  const int nout = Lo - t0 < g.Tt ? Lo - t0 : g.Tt;
  const int nvalid = olen - t0 < nout ? olen - t0 : nout;
  float* row = out + (int64_t)b * Lo + t0;
  if (nvalid <= 0) {  // the whole tile lies behind the utterance
    for (int o = tid; o < nout; o += RS_NT) row[o] = 0.f;
    return;
  }
  // the samples of the frames that carry a valid output: (frames - 1) * orig + K <= g.span
  const int frames = (nvalid + g.nw - 1) / g.nw;
  const int nspan = (frames - 1) * g.orig + g.K;
  const int64_t start = (int64_t)blockIdx.x * g.F * g.orig - g.width;
  const T* src = in + (int64_t)b * L * C;
  for (int j = tid; j < nspan; j += RS_NT) {
    const int64_t pos = start + j;
    xs[j + (j >> g.sh)] = pos >= 0 && pos < len ? rs_load(src, pos, C) : 0.f;
  }
  if (TAB_LDS) {
    for (int p = 0; p < g.nw; ++p)
      for (int k = tid; k < g.K; k += RS_NT) ts[p * g.KS + k] = bank[p * g.K + k];
  }
  __syncthreads();
  for (int o = tid; o < nout; o += RS_NT) {
    float acc = 0.f;
    if (o < nvalid) {
      const int i = o / g.nw, p = o - i * g.nw;
      const int a0 = i * g.orig;
      if (TAB_LDS) {
        const float* w = ts + p * g.KS;
        for (int k = 0; k < g.K; ++k) {
          const int a = a0 + k;
          acc = fmaf(w[k], xs[a + (a >> g.sh)], acc);
        }
      } else {
        const float* w = bankT + p;
        for (int k = 0; k < g.K; ++k) {
          const int a = a0 + k;
          acc = fmaf(w[(int64_t)k * g.nw], xs[a + (a >> g.sh)], acc);
        }
      }
    }
    row[o] = acc;
  }
}

}  // namespace
}  // namespace dn

struct DnResample {
  DnResampleConfig cfg;
  RsGeom g;
  bool tab_lds;
  size_t lds_bytes;
  const float *bank, *bankT;
};

extern "C" int dn_resample_create(const DnResampleConfig* cfg, const void* const* tables, int32_t n_tables, DnResample** out) {
  DN_CHECK_ARG(cfg != nullptr && out != nullptr, "dn_resample_create: null argument");
  DN_CHECK_ARG(cfg->orig >= 1 && cfg->new_ >= 1 && cfg->width >= 1, "dn_resample_create: orig %d, new %d, width %d (each at least 1)", cfg->orig, cfg->new_,
               cfg->width);
  DN_CHECK_ARG((int64_t)cfg->K == 2 * (int64_t)cfg->width + cfg->orig, "dn_resample_create: K %d is not 2 width + orig = 2 * %d + %d", cfg->K, cfg->width, cfg->orig);
  DN_CHECK_ARG(tables && n_tables == 2 && tables[0] && tables[1], "dn_resample_create: two tables (bank [new][K], its transpose [K][new]) expected");
  RsGeom g;
  g.orig = cfg->orig; g.nw = cfg->new_; g.width = cfg->width; g.K = cfg->K; g.KS = cfg->K | 1;
  g.sh = (g.orig & 1) ? 31 : 5;
  const auto image = [&](int64_t span) { return span + (g.sh == 5 ? span / 32 + 1 : 0); };
  int64_t F = RS_TILE / g.nw;
  F = F < 1 ? 1 : F;
  while (F > 1 && image(F * g.orig + g.K - g.orig) > RS_X_MAX) --F;
  const int64_t span = F * g.orig + g.K - g.orig;
  DN_CHECK_ARG(image(span) <= RS_X_MAX && F * g.nw <= (1 << 20), "dn_resample_create: %d : %d with %d taps needs %lld staged samples per frame, more than %d",
               g.orig, g.nw, g.K, (long long)span, RS_X_MAX);
  g.F = (int)F; g.Tt = (int)(F * g.nw); g.span = (int)span; g.xs_floats = (int)image(span);
  DnResample* m = new (std::nothrow) DnResample();
  DN_CHECK_ARG(m != nullptr, "dn_resample_create: out of host memory");
  m->cfg = *cfg;
  m->g = g;
  m->tab_lds = !cfg->force_global && (int64_t)g.nw * g.KS <= RS_TAB_MAX;
  m->lds_bytes = sizeof(float) * ((size_t)g.xs_floats + (m->tab_lds ? (size_t)g.nw * g.KS : 0));  // <= 64 KiB
  m->bank = (const float*)tables[0]; m->bankT = (const float*)tables[1];
  *out = m;
  return DN_OK;
}

extern "C" void dn_resample_destroy(DnResample* m) { delete m; }

extern "C" int64_t dn_resample_out_length(const DnResample* m, int64_t L) { return m ? rs_out_len(L, m->g.orig, m->g.nw) : 0; }

extern "C" int32_t dn_resample_tile(const DnResample* m) { return m ? m->g.Tt : 0; }

extern "C" size_t dn_resample_workspace_bytes(const DnResample* m, int32_t B, int32_t L) { return 0; }

namespace {
template <typename T>
void rs_launch(const DnResample* m, const T* in, int C, const int32_t* lengths, int B, int L, int Lo, float* out, int32_t* out_lengths, hipStream_t s) {
  const dim3 grid((Lo + m->g.Tt - 1) / m->g.Tt, B), block(RS_NT);
  if (m->tab_lds)
    hipLaunchKernelGGL((resample_kernel<true, T>), grid, block, m->lds_bytes, s, in, C, lengths, L, Lo, m->g, m->bank, m->bankT, out, out_lengths);
  else
    hipLaunchKernelGGL((resample_kernel<false, T>), grid, block, m->lds_bytes, s, in, C, lengths, L, Lo, m->g, m->bank, m->bankT, out, out_lengths);
}
}  // namespace

extern "C" int dn_resample_forward(DnResample* m, const void* in, int32_t in_dtype, int32_t channels, const int32_t* lengths, int32_t B, int32_t L, float* out,
                                   int32_t* out_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && in && lengths && out && out_lengths, "dn_resample_forward: null argument");
  DN_CHECK_ARG(in_dtype == DN_F32 || in_dtype == DN_I16, "dn_resample_forward: input dtype %d (DN_F32 or DN_I16)", in_dtype);
  DN_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && channels >= 1 && channels <= 64, "dn_resample_forward: B=%d (1 .. 65535) L=%d channels=%d (1 .. 64)", B, L, channels);
  const int64_t Lo = dn_resample_out_length(m, L);
  DN_CHECK_ARG(Lo <= 2147483647 - m->g.Tt, "dn_resample_forward: %d samples give %lld output samples, more than an int32 counts", L, (long long)Lo);
  hipStream_t s = (hipStream_t)stream;
  if (in_dtype == DN_I16)
    rs_launch(m, (const int16_t*)in, channels, lengths, B, L, (int)Lo, out, out_lengths, s);
  else
    rs_launch(m, (const float*)in, channels, lengths, B, L, (int)Lo, out, out_lengths, s);
  DN_CHECK_LAUNCH("dn_resample_forward");
  return DN_OK;
}
