// CodeHiFiGAN unit vocoder (fairseq/models/text_to_speech/codehifigan.py, hifigan.py, vocoder.py:214-235): units -> waveform.
//
// One conv operator serves every layer: a centred, dilated conv over channels-last fp32 activations [B, Lmax, C] with per-sequence
// lengths, as an implicit GEMM  M = the 64 frames of one sequence's time tile, N = C_out, K = k * C_in.  The transposed convs of the
// upsampling stages are the same operator on polyphase-repacked weights (diffnorm_amd/vocoder.py::polyphase).  Frames outside
// [0, length) are read as zeros by every layer -- the reference's per-utterance zero padding -- so a padded batch computes, frame by
// frame, what each utterance computes alone; tiles are counted from frame 0 of each sequence, so the summation order of a frame does
// not depend on the batch, the row or Lmax either, and batched results equal single ones bit for bit.
//
// Arithmetic: DN_F32 (v_mfma_f32_16x16x4_f32) and DN_F16 (v_mfma_f32_16x16x32_f16: half operands, fp32 accumulate).  Activations
// are stored fp32 in both; the `pre` activation is applied in fp32 to the stored value and rounded once to the operand type while
// the tile is staged in LDS.
#include <algorithm>
#include <vector>

#include "common.h"
#include "engine.h"

namespace dn {
namespace voc {

constexpr int TILE_T = 64;        // frames per workgroup (4 MFMA row fragments)
constexpr int CK_MAX = 128;       // input channels staged per pass
constexpr int LDS_MAX = 64 * 1024;
constexpr int THREADS = 256;

struct ConvArgs {
  const float* x;
  const void* W;
  const float* bias;
  const float* res;
  float* out;
  const int32_t* lengths;
  int64_t x_bstride, out_bstride, res_bstride;  // elements between batch rows
  int ldx, ldo, ldr;                            // elements between frames
  int C_in, C_out, Cout_pad, k, d;
  int CK, nchunk, ksteps, Ktot;                 // channels per pass, passes, k-steps per pass, elements per packed weight row
  int len_mul, Lmax;                            // a sequence has min(lengths[b] * len_mul, Lmax) frames
  int post;
  float slope, div;
};

__host__ __device__ inline int kstep_elems(int dtype) { return dtype == DN_F16 ? 32 : 16; }

// Elements of one packed weight row: per pass of CK input channels the k * CK products in (tap, channel) order, padded with zeros to
// the MFMA k-step (nothing to pad in DN_F32; 16 elements in DN_F16 when k * CK is an odd multiple of 16).
inline int pass_channels(int C_in) { return C_in <= CK_MAX ? C_in : CK_MAX; }
inline int pass_ksteps(int dtype, int C_in, int k) {
  const int ks = kstep_elems(dtype);
  return (k * pass_channels(C_in) + ks - 1) / ks;
}
inline int weight_row_elems(int dtype, int C_in, int k) { return (C_in / pass_channels(C_in)) * pass_ksteps(dtype, C_in, k) * kstep_elems(dtype); }

// MF x NF accumulator fragments per wave.  SPLIT_N: the four waves share the tile's 64 frames and take 16 output channels each
// (C_out >= 64); otherwise each wave owns 16 frames and all (<= 48) output channels, so C_out = 16 and C_out = 1 waste no MFMA.
template <typename E, int MF, int NF, bool SPLIT_N>
__global__ __launch_bounds__(THREADS) void conv_kernel(const ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int ES = Elem<E>::bytes;
  constexpr int EPL = 16 / ES;    // consecutive k a lane holds of a k-step
  constexpr int KSTEP = 64 / ES;  // k per k-step
  if constexpr (IsHalf<E>::value) f16_saturate();
  const int b = blockIdx.z, t0 = blockIdx.x * TILE_T;
  const int len = min(a.lengths[b] * a.len_mul, a.Lmax);
  if (t0 >= len) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int half = (a.k - 1) / 2, halo = half * a.d;
  const int rows = TILE_T + 2 * halo;
  const int rstride = a.CK * ES + 16;  // + 16 bytes: the 16 rows of a fragment read fall on distinct banks
  const int m0 = SPLIT_N ? 0 : wave * 16;
  const int n0 = SPLIT_N ? blockIdx.y * 64 + wave * 16 : 0;
  const bool active = n0 < a.Cout_pad;

  f32x4 acc[MF][NF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float* xb = a.x + (int64_t)b * a.x_bstride;
  const char* wlane = reinterpret_cast<const char*>(a.W) + ((int64_t)(active ? n0 + r : 0) * a.Ktot + q * EPL) * ES;
  const int vec_per_row = a.CK >> 2;
  for (int c = 0; c < a.nchunk; ++c) {
    if (c) __syncthreads();
    for (int i = tid; i < rows * vec_per_row; i += THREADS) {
      const int row = i / vec_per_row, v = i - row * vec_per_row;
      const int t = t0 - halo + row;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t >= 0 && t < len) val = *reinterpret_cast<const float4*>(xb + (int64_t)t * a.ldx + c * a.CK + 4 * v);
      val.x = val.x > 0.f ? val.x : val.x * a.slope;
      val.y = val.y > 0.f ? val.y : val.y * a.slope;
      val.z = val.z > 0.f ? val.z : val.z * a.slope;
      val.w = val.w > 0.f ? val.w : val.w * a.slope;
      char* dst = lds + row * rstride + v * 4 * ES;
      if constexpr (ES == 2) *reinterpret_cast<uint2*>(dst) = make_uint2(pack_f16x2(val.x, val.y), pack_f16x2(val.z, val.w));
      else *reinterpret_cast<float4*>(dst) = val;
    }
    __syncthreads();
    if (active) {
      const char* wp = wlane + (int64_t)c * a.ksteps * KSTEP * ES;
      int j = 0, cc = q * EPL;  // this lane's (tap, channel) of the current k-step
      while (cc >= a.CK) { cc -= a.CK; ++j; }
      for (int s = 0; s < a.ksteps; ++s) {
        uint4 bf[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) bf[nf] = *reinterpret_cast<const uint4*>(wp + ((int64_t)nf * 16 * a.Ktot + s * KSTEP) * ES);
        const bool tap = j < a.k;  // beyond the last tap: the zero padding of the weight row
        const char* ap = lds + (m0 + r + halo + (tap ? j - half : 0) * a.d) * rstride + cc * ES;
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          uint4 af = *reinterpret_cast<const uint4*>(ap + mf * 16 * rstride);
          if (!tap) af = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) mma_kstep<E>(acc[mf][nf], af, bf[nf]);
        }
        cc += KSTEP;
        while (cc >= a.CK) { cc -= a.CK; ++j; }
      }
    }
  }
  if (!active) return;
  float* ob = a.out + (int64_t)b * a.out_bstride;
  const float* rb = a.res ? a.res + (int64_t)b * a.res_bstride : nullptr;
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const int co = n0 + nf * 16 + r;
    if (co >= a.C_out) continue;
    const float bias = a.bias ? a.bias[co] : 0.f;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = t0 + m0 + mf * 16 + 4 * q + e;
        if (t >= len) continue;
        float v = acc[mf][nf][e] + bias;
        float* o = ob + (int64_t)t * a.ldo + co;
        if (a.post == DN_VOC_POST_RES || a.post == DN_VOC_POST_RES_ACC) {
          v += rb[(int64_t)t * a.ldr + co];
          if (a.post == DN_VOC_POST_RES_ACC) v += *o;
          if (a.div != 1.f) v = v / a.div;
        } else if (a.post == DN_VOC_POST_RELU) {
          v = fmaxf(v, 0.f);
        } else if (a.post == DN_VOC_POST_TANH) {
          v = tanhf(v);
        }
        *o = v;
      }
    }
  }
}

template <typename E>
static void launch_conv_e(const ConvArgs& a, dim3 grid, size_t lds_bytes, hipStream_t st) {
  if (a.Cout_pad >= 64) {
    grid.y = (a.Cout_pad + 63) / 64;
    conv_kernel<E, 4, 1, true><<<grid, THREADS, lds_bytes, st>>>(a);
  } else if (a.Cout_pad == 48) {
    conv_kernel<E, 1, 3, false><<<grid, THREADS, lds_bytes, st>>>(a);
  } else if (a.Cout_pad == 32) {
    conv_kernel<E, 1, 2, false><<<grid, THREADS, lds_bytes, st>>>(a);
  } else {
    conv_kernel<E, 1, 1, false><<<grid, THREADS, lds_bytes, st>>>(a);
  }
}

// shape checks shared by dn_voc_conv and the engine (which has checked its layers at create time)
static const char* conv_shape_error(int dtype, int C_in, int C_out, int k, int d) {
  if (dtype == DN_BF16 || dtype == DN_BF16X3) return "the vocoder runs in DN_F32 or DN_F16: eight significand bits are no audio arithmetic";
  if (dtype != DN_F32 && dtype != DN_F16) return "unknown dtype";
  if (C_in < 16 || C_in % 16 || (C_in > CK_MAX && C_in % CK_MAX)) return "C_in must be a multiple of 16, and of 128 beyond 128";
  if (C_out < 1) return "C_out < 1";
  if (k < 1 || !(k & 1) || d < 1) return "k must be odd and d >= 1";
  const int rows = TILE_T + (k - 1) * d, rstride = pass_channels(C_in) * (dtype == DN_F16 ? 2 : 4) + 16;
  if ((int64_t)rows * rstride > LDS_MAX) return "tile + halo does not fit in LDS ((k - 1) / 2 * d <= 25)";
  return nullptr;
}

static int launch_conv(int dtype, ConvArgs a, int B, hipStream_t st) {
  a.Cout_pad = (a.C_out + 15) / 16 * 16;
  a.CK = pass_channels(a.C_in);
  a.nchunk = a.C_in / a.CK;
  a.ksteps = pass_ksteps(dtype, a.C_in, a.k);
  a.Ktot = weight_row_elems(dtype, a.C_in, a.k);
  if (B <= 0 || a.Lmax <= 0) return DN_OK;
  const int rows = TILE_T + (a.k - 1) * a.d, rstride = a.CK * (dtype == DN_F16 ? 2 : 4) + 16;
  dim3 grid((a.Lmax + TILE_T - 1) / TILE_T, 1, B);
  if (dtype == DN_F16) launch_conv_e<F16>(a, grid, (size_t)rows * rstride, st);
  else launch_conv_e<F32>(a, grid, (size_t)rows * rstride, st);
  DN_CHECK_LAUNCH("dn_voc_conv");
  return DN_OK;
}

// ------------------------------------------------------------------------------------------------ the small kernels
// Exclusive scan of a row's durations (all 1 when dur == nullptr): cum[b][0 .. T], frames[b] = min(total, Lmax0), and the
// waveform length frames * up.  One wave per row.  Summed in 64 bits and saturated at INT32_MAX, so no set of durations wraps a
// sum: the host refuses a row whose frames * up does not fit an int32 (dn_voc_forward), which a saturated sum never does.
__device__ __forceinline__ int32_t sat31(long long v) { return (int32_t)(v < 0x7fffffffLL ? v : 0x7fffffffLL); }

__global__ __launch_bounds__(64) void scan_kernel(const int32_t* dur, const int32_t* lengths, int Tmax, int Lmax0, int up, int32_t* cum,
                                                  int32_t* frames, int32_t* sums, int32_t* wav_lengths) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = min(max(lengths[b], 0), Tmax);
  long long carry = 0;
  int32_t* c = cum ? cum + (int64_t)b * (Tmax + 1) : nullptr;
  for (int base = 0; base < T; base += 64) {
    const int i = base + lane;
    const int v = i < T ? (dur ? max(dur[(int64_t)b * Tmax + i], 0) : 1) : 0;
    long long s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(s, o);
      if (lane >= o) s += u;
    }
    if (c && i < T) c[i] = sat31(carry + s - v);
    carry += __shfl(s, 63);
  }
  if (lane == 0) {
    const int total = sat31(carry);
    if (c) c[T] = total;
    if (sums) sums[b] = total;
    const int f = min(total, Lmax0);
    if (frames) frames[b] = f;
    if (wav_lengths) wav_lengths[b] = f * up;
  }
}

// Embedding lookup fused with repeat_interleave: frame f of row b takes dict[code[b][i]], cum[b][i] <= f < cum[b][i + 1].
__global__ __launch_bounds__(256) void embed_kernel(const float* dict, const int32_t* codes, const int32_t* lengths, const int32_t* cum,
                                                    const int32_t* frames, int B, int Tmax, int Lmax0, int E, int V, float* out) {
  const int vec = E >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * Lmax0 * vec) return;
  const int v = (int)(i % vec);
  const int64_t bf = i / vec;
  const int f = (int)(bf % Lmax0), b = (int)(bf / Lmax0);
  if (f >= frames[b]) return;
  const int32_t* c = cum + (int64_t)b * (Tmax + 1);
  int lo = 0, hi = min(max(lengths[b], 0), Tmax);  // the answer lies in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c[mid] <= f) lo = mid; else hi = mid;
  }
  const int code = min(max(codes[(int64_t)b * Tmax + lo], 0), V - 1);
  *reinterpret_cast<float4*>(out + bf * E + 4 * v) = *reinterpret_cast<const float4*>(dict + (int64_t)code * E + 4 * v);
}

// LayerNorm over the channels of every valid frame, in place (eps 1e-5, biased variance).  One wave per frame.
__global__ __launch_bounds__(256) void layernorm_kernel(float* x, const int32_t* lengths, int B, int Tmax, int H, const float* g, const float* bta) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B * Tmax) return;
  const int b = row / Tmax, t = row - b * Tmax;
  if (t >= lengths[b]) return;
  float* p = x + (int64_t)row * H;
  float s = 0.f;
  for (int i = lane; i < H; i += 64) s += p[i];
  const float mean = wave_sum(s) / (float)H;
  float ss = 0.f;
  for (int i = lane; i < H; i += 64) { const float dlt = p[i] - mean; ss += dlt * dlt; }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)H + 1e-5f);
  for (int i = lane; i < H; i += 64) p[i] = (p[i] - mean) * rstd * g[i] + bta[i];
}

// proj (H -> 1) and the duration rule clamp(round(exp(v) - 1), min = 1); rintf = half-to-even like torch.round.  A duration is capped
// at DUR_MAX frames (11 minutes of one unit at 50 frames / s; the inf of a diverged predictor lands there, its NaN on 1).
constexpr float DUR_MAX = 32767.f;
__global__ __launch_bounds__(256) void duration_kernel(const float* x, const int32_t* lengths, int B, int Tmax, int H, const float* w, const float* bias,
                                                       int32_t* dur, float* logd) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B * Tmax) return;
  const int b = row / Tmax, t = row - b * Tmax;
  if (t >= lengths[b]) {
    if (lane == 0) dur[row] = 0;
    return;
  }
  const float* p = x + (int64_t)row * H;
  float s = 0.f;
  for (int i = lane; i < H; i += 64) s += p[i] * w[i];
  const float v = wave_sum(s) + bias[0];
  if (lane == 0) {
    dur[row] = (int32_t)fminf(fmaxf(rintf(expf(v) - 1.0f), 1.0f), DUR_MAX);
    if (logd) logd[row] = v;
  }
}

}  // namespace voc
}  // namespace dn

using namespace dn::voc;

// ------------------------------------------------------------------------------------------------ the engine
struct DnVocLayer {
  const void* W;
  const float* b;
  int C_in, C_out, k, d;
};

struct DnVoc {
  DnVocConfig cfg;
  const float* dict;
  DnVocLayer pre, post;
  std::vector<DnVocLayer> ups;                 // polyphase form: k = 3, C_out = rate * channels
  std::vector<DnVocLayer> res;                 // [stage][kernel][pair][c1, c2]
  DnVocLayer p1, p2;                           // duration predictor convs (always DN_F32)
  const float *ln1g, *ln1b, *ln2g, *ln2b, *pw, *pb;
  int up_total;
  int64_t max_elems_per_frame;                 // widest activation per input frame: max over layers of (frames per input frame) * C
  dn::StageTimer timer;                        // dn_voc_set_profile: the stage boundaries of the last profiled forward
};

extern "C" int dn_voc_conv_tile(int32_t dtype, int32_t C_in, int32_t C_out, int32_t k) {
  const char* e = conv_shape_error(dtype, C_in, C_out, k, 1);
  DN_CHECK_ARG(!e, "dn_voc_conv_tile: %s", e);
  return TILE_T;
}

extern "C" int64_t dn_voc_conv_weight_elems(int32_t dtype, int32_t C_in, int32_t C_out, int32_t k) {
  if (conv_shape_error(dtype, C_in, C_out, k, 1)) return 0;
  return (int64_t)((C_out + 15) / 16 * 16) * weight_row_elems(dtype, C_in, k);
}

extern "C" int dn_voc_conv(const DnVocConvParams* p, void* stream) {
  DN_CHECK_ARG(p, "dn_voc_conv: null parameters");
  const char* e = conv_shape_error(p->dtype, p->C_in, p->C_out, p->k, p->d);
  DN_CHECK_ARG(!e, "dn_voc_conv: %s", e);
  DN_CHECK_ARG(p->x && p->W && p->out && p->lengths, "dn_voc_conv: x, W, out and lengths are required");
  DN_CHECK_ARG(p->B >= 1 && p->Lmax >= 1, "dn_voc_conv: B = %d, Lmax = %d", p->B, p->Lmax);
  DN_CHECK_ARG(p->ldx >= p->C_in && p->ldx % 4 == 0 && p->ldo >= p->C_out, "dn_voc_conv: ldx = %d (C_in %d, multiple of 4), ldo = %d (C_out %d)", p->ldx,
               p->C_in, p->ldo, p->C_out);
  DN_CHECK_ARG(((uintptr_t)p->x & 15) == 0 && ((uintptr_t)p->W & 15) == 0, "dn_voc_conv: x and W must be 16-byte aligned");
  DN_CHECK_ARG(p->post >= DN_VOC_POST_NONE && p->post <= DN_VOC_POST_TANH, "dn_voc_conv: post = %d", p->post);
  const bool needs_res = p->post == DN_VOC_POST_RES || p->post == DN_VOC_POST_RES_ACC;
  DN_CHECK_ARG(!needs_res || (p->res && p->ldr >= p->C_out), "dn_voc_conv: post %d needs res (ldr >= C_out)", p->post);
  DN_CHECK_ARG(p->div != 0.f, "dn_voc_conv: div = 0 (1 = none)");
  ConvArgs a = {};
  a.x = p->x; a.W = p->W; a.bias = p->bias; a.res = needs_res ? p->res : nullptr; a.out = p->out; a.lengths = p->lengths;
  a.ldx = p->ldx; a.ldo = p->ldo; a.ldr = p->ldr;
  a.x_bstride = (int64_t)p->Lmax * p->ldx; a.out_bstride = (int64_t)p->Lmax * p->ldo; a.res_bstride = (int64_t)p->Lmax * p->ldr;
  a.C_in = p->C_in; a.C_out = p->C_out; a.k = p->k; a.d = p->d;
  a.len_mul = 1; a.Lmax = p->Lmax; a.post = p->post; a.slope = p->slope; a.div = needs_res ? p->div : 1.f;
  return launch_conv(p->dtype, a, p->B, (hipStream_t)stream);
}

extern "C" int dn_voc_create(const DnVocConfig* c, const void* const* weights, int32_t n_weights, DnVoc** out) {
  DN_CHECK_ARG(c && weights && out, "dn_voc_create: null argument");
  DN_CHECK_ARG(c->dtype != DN_BF16 && c->dtype != DN_BF16X3, "dn_voc_create: the vocoder runs in DN_F32 or DN_F16 (bf16 / bf16x3 are refused: eight significand bits are no audio arithmetic)");
  DN_CHECK_ARG(c->dtype == DN_F32 || c->dtype == DN_F16, "dn_voc_create: dtype %d", c->dtype);
  DN_CHECK_ARG(c->n_ups >= 1 && c->n_ups <= DN_VOC_MAX_UPS && c->n_kernels >= 1 && c->n_kernels <= DN_VOC_MAX_KERNELS, "dn_voc_create: %d stages, %d resblock kernels",
               c->n_ups, c->n_kernels);
  DN_CHECK_ARG(c->num_embeddings >= 1 && c->embedding_dim >= 16, "dn_voc_create: dictionary %d x %d", c->num_embeddings, c->embedding_dim);
  DN_CHECK_ARG(c->initial_channel % (16 << c->n_ups) == 0, "dn_voc_create: upsample_initial_channel %d must leave a multiple of 16 channels after %d halvings",
               c->initial_channel, c->n_ups);
  const int n_expected = 3 + 2 * c->n_ups + 12 * c->n_ups * c->n_kernels + 2 + (c->dur_hidden ? 10 : 0);
  DN_CHECK_ARG(n_weights == n_expected, "dn_voc_create: %d packed tensors, expected %d", n_weights, n_expected);
  for (int i = 0; i < n_weights; ++i) DN_CHECK_ARG(weights[i] && ((uintptr_t)weights[i] & 15) == 0, "dn_voc_create: packed tensor %d is null or not 16-byte aligned", i);
  DnVoc* m = new DnVoc();
  m->cfg = *c;
  int wi = 0;
  const char* err = nullptr;
  auto layer = [&](int dtype, int C_in, int C_out, int k, int d) {
    DnVocLayer l = {weights[wi], reinterpret_cast<const float*>(weights[wi + 1]), C_in, C_out, k, d};
    wi += 2;
    if (!err) err = conv_shape_error(dtype, C_in, C_out, k, d);
    return l;
  };
  m->dict = reinterpret_cast<const float*>(weights[wi++]);
  m->pre = layer(c->dtype, c->embedding_dim, c->initial_channel, 7, 1);
  int ch = c->initial_channel;
  int64_t fpf = 1;  // frames per input frame
  m->up_total = 1;
  m->max_elems_per_frame = std::max<int64_t>(c->embedding_dim, ch);
  for (int i = 0; i < c->n_ups && !err; ++i) {
    const int u = c->up_rates[i], k = c->up_kernels[i];
    if (u < 1 || k < u || (k - u) % 2) { err = "a transposed conv needs k >= u and k - u even (its output is then exactly L * u frames)"; break; }
    if (k > 3 * u) { err = "a transposed conv with k > 3 u reaches beyond the neighbouring input frames"; break; }
    m->ups.push_back(layer(c->dtype, ch, u * (ch / 2), 3, 1));
    ch /= 2;
    fpf *= u;
    m->up_total *= u;
    m->max_elems_per_frame = std::max(m->max_elems_per_frame, fpf * ch);
    for (int j = 0; j < c->n_kernels; ++j)
      for (int pr = 0; pr < 3; ++pr) {
        m->res.push_back(layer(c->dtype, ch, ch, c->res_kernels[j], c->res_dilations[j][pr]));
        m->res.push_back(layer(c->dtype, ch, ch, c->res_kernels[j], 1));
      }
  }
  if (!err) m->post = layer(c->dtype, ch, 1, 7, 1);
  if (!err && c->dur_hidden) {
    if (c->dur_hidden % 16) err = "var_pred_hidden_dim must be a multiple of 16";
    m->p1 = layer(DN_F32, c->embedding_dim, c->dur_hidden, 3, 1);
    m->ln1g = reinterpret_cast<const float*>(weights[wi++]); m->ln1b = reinterpret_cast<const float*>(weights[wi++]);
    m->p2 = layer(DN_F32, c->dur_hidden, c->dur_hidden, 3, 1);
    m->ln2g = reinterpret_cast<const float*>(weights[wi++]); m->ln2b = reinterpret_cast<const float*>(weights[wi++]);
    m->pw = reinterpret_cast<const float*>(weights[wi++]); m->pb = reinterpret_cast<const float*>(weights[wi++]);
    m->max_elems_per_frame = std::max<int64_t>(m->max_elems_per_frame, c->dur_hidden);
  }
  if (err) {
    dn_set_error("dn_voc_create: %s", err);
    delete m;
    return DN_EINVAL;
  }
  *out = m;
  return DN_OK;
}

extern "C" void dn_voc_destroy(DnVoc* m) {
  if (!m) return;
  m->timer.destroy();
  delete m;
}

extern "C" int32_t dn_voc_upsample(const DnVoc* m) { return m ? m->up_total : 0; }

namespace {
// five activation buffers of the widest layer, the scan [B][Lmax + 1] and the per-row frame counts
struct VocBufs {
  float* buf[5];
  int32_t *cum, *frames;
};
VocBufs plan_voc(const DnVoc* m, int B, int Lmax, dn::Arena& ar) {
  VocBufs w;
  for (int i = 0; i < 5; ++i) w.buf[i] = (float*)ar.take((size_t)B * Lmax * m->max_elems_per_frame * sizeof(float));
  w.cum = (int32_t*)ar.take((size_t)B * (Lmax + 1) * sizeof(int32_t));
  w.frames = (int32_t*)ar.take((size_t)B * sizeof(int32_t));
  return w;
}
// The plan over the caller's workspace.  A pass takes exactly dn_voc_workspace_bytes: one byte less is refused, and with
// DN_EINVAL, as a bad workspace of the vocoder's always has been.
int plan_voc_checked(const char* who, const DnVoc* m, int B, int Lmax, void* ws, size_t ws_bytes, VocBufs& w) {
  DN_CHECK_ARG(ws, "%s: null workspace", who);
  dn::Arena ar{(char*)ws, 0, ws_bytes};
  w = plan_voc(m, B, Lmax, ar);
  return dn::check_workspace(who, ws, ws_bytes, ar.off) == DN_OK ? DN_OK : DN_EINVAL;
}
int run_layer(int dtype, const DnVocLayer& l, const float* x, float* out, int ldo, const float* res, const int32_t* lengths, int len_mul, int Lmax, int B,
              float slope, int post, float div, hipStream_t st) {
  ConvArgs a = {};
  a.x = x; a.W = l.W; a.bias = l.b; a.res = res; a.out = out; a.lengths = lengths;
  a.ldx = l.C_in; a.ldo = ldo; a.ldr = l.C_out;
  a.x_bstride = (int64_t)Lmax * l.C_in; a.out_bstride = (int64_t)Lmax * ldo; a.res_bstride = (int64_t)Lmax * l.C_out;
  a.C_in = l.C_in; a.C_out = l.C_out; a.k = l.k; a.d = l.d;
  a.len_mul = len_mul; a.Lmax = Lmax; a.post = post; a.slope = slope; a.div = div;
  return launch_conv(dtype, a, B, st);
}
}  // namespace

extern "C" size_t dn_voc_workspace_bytes(const DnVoc* m, int32_t B, int32_t Lmax0) {
  if (!m || B < 1 || Lmax0 < 1) return 0;
  dn::Arena a{nullptr, 0, 0};
  (void)plan_voc(m, B, Lmax0, a);
  return a.off;
}

extern "C" int dn_voc_durations(DnVoc* m, const int32_t* codes, const int32_t* lengths, int32_t B, int32_t Tmax, int32_t* durations, int32_t* sums,
                                void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && codes && lengths && durations && sums, "dn_voc_durations: null argument");
  DN_CHECK_ARG(m->cfg.dur_hidden > 0, "dn_voc_durations: the model has no duration predictor (dur_predictor_params)");
  DN_CHECK_ARG(B >= 1 && Tmax >= 1, "dn_voc_durations: B = %d, Tmax = %d", B, Tmax);
  VocBufs w;
  DN_TRY(plan_voc_checked("dn_voc_durations", m, B, Tmax, workspace, workspace_bytes, w));
  hipStream_t st = (hipStream_t)stream;
  const int E = m->cfg.embedding_dim, H = m->cfg.dur_hidden;
  scan_kernel<<<B, 64, 0, st>>>(nullptr, lengths, Tmax, Tmax, 1, w.cum, w.frames, nullptr, nullptr);
  const int64_t nvec = (int64_t)B * Tmax * (E / 4);
  embed_kernel<<<(unsigned)((nvec + 255) / 256), 256, 0, st>>>(m->dict, codes, lengths, w.cum, w.frames, B, Tmax, Tmax, E, m->cfg.num_embeddings, w.buf[0]);
  DN_CHECK_LAUNCH("dn_voc_durations: embedding");
  const unsigned row_blocks = (unsigned)((B * Tmax + 3) / 4);
  DN_TRY(run_layer(DN_F32, m->p1, w.buf[0], w.buf[1], H, nullptr, w.frames, 1, Tmax, B, 1.f, DN_VOC_POST_RELU, 1.f, st));
  layernorm_kernel<<<row_blocks, 256, 0, st>>>(w.buf[1], w.frames, B, Tmax, H, m->ln1g, m->ln1b);
  DN_TRY(run_layer(DN_F32, m->p2, w.buf[1], w.buf[2], H, nullptr, w.frames, 1, Tmax, B, 1.f, DN_VOC_POST_RELU, 1.f, st));
  layernorm_kernel<<<row_blocks, 256, 0, st>>>(w.buf[2], w.frames, B, Tmax, H, m->ln2g, m->ln2b);
  duration_kernel<<<row_blocks, 256, 0, st>>>(w.buf[2], w.frames, B, Tmax, H, m->pw, m->pb, durations, nullptr);
  scan_kernel<<<B, 64, 0, st>>>(durations, lengths, Tmax, 0x7fffffff, 1, nullptr, nullptr, sums, nullptr);
  DN_CHECK_LAUNCH("dn_voc_durations");
  return DN_OK;
}

extern "C" int dn_voc_set_profile(DnVoc* m, int32_t on) {
  DN_CHECK_ARG(m, "dn_voc_set_profile: null engine");
  return m->timer.enable("dn_voc_set_profile", m->cfg.n_ups + 3, on);
}

extern "C" int dn_voc_stage_times(DnVoc* m, float* ms, int32_t cap) {
  DN_CHECK_ARG(m, "dn_voc_stage_times: null engine");
  return m->timer.read("dn_voc_stage_times", ms, cap);
}

extern "C" int dn_voc_forward(DnVoc* m, const int32_t* codes, const int32_t* lengths, const int32_t* durations, int32_t B, int32_t Tmax, int32_t Lmax0,
                              float* wav, int32_t* wav_lengths, void* workspace, size_t workspace_bytes, void* stream) {
  DN_CHECK_ARG(m && codes && lengths && wav && wav_lengths, "dn_voc_forward: null argument");
  DN_CHECK_ARG(B >= 1 && Tmax >= 1 && Lmax0 >= 1, "dn_voc_forward: B = %d, Tmax = %d, Lmax0 = %d", B, Tmax, Lmax0);
  DN_CHECK_ARG(durations || Lmax0 >= Tmax, "dn_voc_forward: without durations every unit is one frame: Lmax0 = %d < Tmax = %d", Lmax0, Tmax);
  DN_CHECK_ARG((int64_t)Lmax0 * m->up_total < (int64_t)1 << 31, "dn_voc_forward: %d frames x %d samples overflow a row's int32 indices", Lmax0, m->up_total);
  VocBufs w;
  DN_TRY(plan_voc_checked("dn_voc_forward", m, B, std::max(Lmax0, Tmax), workspace, workspace_bytes, w));
  // the scan is [B][Tmax + 1]; the plan sized it for max(Lmax0, Tmax) + 1 per row
  hipStream_t st = (hipStream_t)stream;
  const DnVocConfig& c = m->cfg;
  const int dt = c.dtype, E = c.embedding_dim;
  int ei = 0;
  auto mark = [&]() { m->timer.mark(ei, st); };
  mark();
  scan_kernel<<<B, 64, 0, st>>>(durations, lengths, Tmax, Lmax0, m->up_total, w.cum, w.frames, nullptr, wav_lengths);
  const int64_t nvec = (int64_t)B * Lmax0 * (E / 4);
  embed_kernel<<<(unsigned)((nvec + 255) / 256), 256, 0, st>>>(m->dict, codes, lengths, w.cum, w.frames, B, Tmax, Lmax0, E, c.num_embeddings, w.buf[1]);
  DN_CHECK_LAUNCH("dn_voc_forward: embedding");
  DN_TRY(run_layer(dt, m->pre, w.buf[1], w.buf[0], m->pre.C_out, nullptr, w.frames, 1, Lmax0, B, 1.f, DN_VOC_POST_NONE, 1.f, st));
  mark();
  float *cur = w.buf[0], *X = w.buf[1], *T = w.buf[2], *H = w.buf[3], *S = w.buf[4];
  int mul = 1, L = Lmax0, ri = 0;
  for (int i = 0; i < c.n_ups; ++i) {
    const DnVocLayer& up = m->ups[i];
    // [L, u * C] rows of the polyphase conv are the [L * u, C] activation in memory
    DN_TRY(run_layer(dt, up, cur, X, up.C_out, nullptr, w.frames, mul, L, B, 0.1f, DN_VOC_POST_NONE, 1.f, st));
    mul *= c.up_rates[i];
    L *= c.up_rates[i];
    const int ch = up.C_in / 2;
    for (int j = 0; j < c.n_kernels; ++j) {
      const float* h = X;
      for (int pr = 0; pr < 3; ++pr, ri += 2) {
        DN_TRY(run_layer(dt, m->res[ri], h, T, ch, nullptr, w.frames, mul, L, B, 0.1f, DN_VOC_POST_NONE, 1.f, st));
        if (pr < 2) {
          DN_TRY(run_layer(dt, m->res[ri + 1], T, H, ch, h, w.frames, mul, L, B, 0.1f, DN_VOC_POST_RES, 1.f, st));
          h = H;
        } else {  // the block's output joins the stage's sum; the last one divides by the number of blocks, once
          DN_TRY(run_layer(dt, m->res[ri + 1], T, S, ch, h, w.frames, mul, L, B, 0.1f, j ? DN_VOC_POST_RES_ACC : DN_VOC_POST_RES,
                               j == c.n_kernels - 1 ? (float)c.n_kernels : 1.f, st));
        }
      }
    }
    std::swap(cur, S);
    mark();
  }
  DN_TRY(run_layer(dt, m->post, cur, wav, 1, nullptr, w.frames, mul, L, B, 0.01f, DN_VOC_POST_TANH, 1.f, st));
  mark();
  return DN_OK;
}
