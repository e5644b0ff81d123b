// HBM-bound kernels of the path: norms, timestep conditioning, scheduler updates, posterior sampling,
// argmax, Philox normal fill, row conversion.  All are one pass over their operands with 16-byte
// accesses where the layout allows; reductions are wave-level (64 lanes) with DPP-free shuffles.
#include "common.h"
#include "engine.h"

namespace dn {

// ------------------------------------------------------------------------------------------ RMSNorm
// one wave per row; D <= 1024 keeps the row in registers (4 float4 per lane), larger D re-reads.
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, int ldx, void* __restrict__ y, int ldy,
                                                      int out_dtype, int M, int D, int T, const float* __restrict__ gamma,
                                                      const float* __restrict__ gb, int gb_ld, int gb_half) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* xr = x + (int64_t)row * ldx;
  float4 v[4];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = c < D ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0, 0, 0, 0);
    ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
  }
  for (int c = (256 + lane) * 4; c < D; c += 256) {
    const float4 u = *reinterpret_cast<const float4*>(xr + c);
    ss += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
  }
  ss = wave_sum(ss);
  const float denom = fmaxf(sqrtf(ss), 1e-12f);
  const float scale = sqrtf((float)D);
  const float* gbr = gb ? gb + (int64_t)(row / T) * gb_ld : nullptr;
  auto emit = [&](int c, float4 u) {
    float o[4] = {u.x / denom * scale, u.y / denom * scale, u.z / denom * scale, u.w / denom * scale};
    if (gamma) {
      const float4 ga = *reinterpret_cast<const float4*>(gamma + c);
      o[0] *= ga.x; o[1] *= ga.y; o[2] *= ga.z; o[3] *= ga.w;
    }
    if (gbr) {
      const float4 ga = *reinterpret_cast<const float4*>(gbr + c);
      const float4 be = *reinterpret_cast<const float4*>(gbr + gb_half + c);
      o[0] = o[0] * ga.x + be.x; o[1] = o[1] * ga.y + be.y; o[2] = o[2] * ga.z + be.z; o[3] = o[3] * ga.w + be.w;
    }
    store4(y, (int64_t)row * ldy + c, out_dtype, o[0], o[1], o[2], o[3]);
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < D) emit(c, v[i]);
  }
  for (int c = (256 + lane) * 4; c < D; c += 256) emit(c, *reinterpret_cast<const float4*>(xr + c));
  // zero the pad columns [D, ldy) so the row can feed a K-padded contraction
  for (int c = D + lane * 4; c < ldy; c += 256) store4(y, (int64_t)row * ldy + c, out_dtype, 0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------ time cond
// block = (16 outputs, one sample): the 2*half+1 Fourier features go to LDS once, then each wave does
// 4 dot products of length 2*half+1.  The angle is formed exactly as the reference forms it in fp32:
// fl(fl(fl(t*w)*2)*pi_f32) -- t up to 999 and w ~ N(0,1) give arguments of 1e3..1e4 rad, so sinf/cosf
// (full range reduction) are used, never the fast intrinsics.
__global__ __launch_bounds__(256) void time_cond_kernel(const int32_t* __restrict__ times, const float* __restrict__ wf, int half,
                                                        const float* __restrict__ W, const float* __restrict__ bias, int C,
                                                        float* __restrict__ out, void* __restrict__ out_act, int act_dtype, int ldo) {
  extern __shared__ float feat[];
  const int b = blockIdx.y;
  const int nfeat = 2 * half + 1;
  const float tf = (float)times[b];
  for (int k = threadIdx.x; k < nfeat; k += 256) {
    float f;
    if (k == 0) {
      f = tf;
    } else {
      const int j = k <= half ? k - 1 : k - 1 - half;
      float ang = __fmul_rn(__fmul_rn(__fmul_rn(tf, wf[j]), 2.0f), 3.14159265358979323846f);
      f = k <= half ? sinf(ang) : cosf(ang);
    }
    feat[k] = f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = blockIdx.x * 16 + wave * 4 + i;
    if (c >= C) break;
    const float* wr = W + (int64_t)c * nfeat;
    float s = 0.f;
    for (int k = lane; k < nfeat; k += 64) s += feat[k] * wr[k];
    s = wave_sum(s);
    if (lane == 0) {
      const float v = silu(s + bias[c]);
      out[(int64_t)b * ldo + c] = v;
      if (out_act) {
        if (act_dtype == DN_BF16X3)
          store1_split(out_act, (int64_t)b * ldo + c, v);
        else if (dn_is16(act_dtype))
          reinterpret_cast<uint16_t*>(out_act)[(int64_t)b * ldo + c] = to_h16(act_dtype, v);
        else
          reinterpret_cast<float*>(out_act)[(int64_t)b * ldo + c] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ scheduler
__global__ __launch_bounds__(256) void ddim_step_kernel(const float* x, const float* __restrict__ eps, float* xo,
                                                        void* __restrict__ xact, int act_dtype, int ld_act, int M, int C, int ld,
                                                        int T, const float* __restrict__ coef, const int32_t* __restrict__ t) {
  const int64_t n = (int64_t)M * C;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i / C), c = (int)(i - (int64_t)m * C);
    const float* cf = coef + 4 * t[m / T];
    const float sa = cf[0], s1 = cf[1];
    const int64_t o = (int64_t)m * ld + c;
    const float xv = x[o], ev = eps[o];
    // x1_hat = safe_div(x - s1*eps, sa); pred_noise = safe_div(x - sa*x1_hat, s1); mean = x1_hat*sqrt(abp) + sqrt(1-abp)*pn
    const float x1 = __fdiv_rn(__fsub_rn(xv, __fmul_rn(s1, ev)), fmaxf(sa, 1e-10f));
    const float pn = __fdiv_rn(__fsub_rn(xv, __fmul_rn(sa, x1)), fmaxf(s1, 1e-10f));
    const float r = __fadd_rn(__fmul_rn(x1, cf[2]), __fmul_rn(cf[3], pn));
    xo[o] = r;
    if (xact) store_act(xact, (int64_t)m * ld_act + c, act_dtype, r);
  }
}

__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x, const float* __restrict__ noise, float* __restrict__ out,
                                                       void* __restrict__ oact, int act_dtype, int ld_act, int M, int C, int ld, int T,
                                                       const float* __restrict__ ca, const float* __restrict__ cb,
                                                       const int32_t* __restrict__ t) {
  const int64_t n = (int64_t)M * C;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i / C), c = (int)(i - (int64_t)m * C);
    const int tb = t[m / T];
    const int64_t o = (int64_t)m * ld + c;
    const float r = __fadd_rn(__fmul_rn(ca[tb], x[o]), __fmul_rn(cb[tb], noise[o]));
    out[o] = r;
    if (oact) store_act(oact, (int64_t)m * ld_act + c, act_dtype, r);
  }
}

// ------------------------------------------------------------------------------------------ posterior
__global__ __launch_bounds__(256) void posterior_kernel(const float* __restrict__ params, int ldp, const float* __restrict__ noise, int ldn,
                                                        float* __restrict__ z, void* __restrict__ zact, int act_dtype, int ldz, int M,
                                                        int Z, int T, const int32_t* __restrict__ lengths, float* __restrict__ kl_rows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* pr = params + (int64_t)row * ldp;
  float kl = 0.f;
  for (int c = lane; c < Z; c += 64) {
    const float mean = pr[c];
    const float lv = fminf(fmaxf(pr[Z + c], -30.0f), 20.0f);
    const float sd = expf(0.5f * lv);
    const float v = __fadd_rn(mean, __fmul_rn(sd, noise[(int64_t)row * ldn + c]));
    z[(int64_t)row * ldz + c] = v;
    if (zact) store_act(zact, (int64_t)row * ldz + c, act_dtype, v);
    kl += mean * mean + expf(lv) - 1.0f - lv;
  }
  for (int c = Z + lane; c < ldz; c += 64) {
    z[(int64_t)row * ldz + c] = 0.f;
    if (zact) store_act(zact, (int64_t)row * ldz + c, act_dtype, 0.f);
  }
  if (kl_rows) {
    kl = wave_sum(kl);
    const int b = row / T, t = row - b * T;
    const bool valid = lengths ? t < lengths[b] : true;
    if (lane == 0) kl_rows[row] = valid ? 0.5f * kl : 0.f;
  }
}

// ------------------------------------------------------------------------------------------ argmax
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, int ld, int M, int V, int offset,
                                                     int32_t* __restrict__ units) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* lr = logits + (int64_t)row * ld;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < V; c += 64) {
    const float v = lr[c];
    if (v > best || (v == best && c < bi)) {  // first maximum wins, like torch.argmax
      best = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) units[row] = bi - offset;
}

// ------------------------------------------------------------------------------------------ Philox randn
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (uint32_t)p1;
  c[3] = (uint32_t)p0;
  c[0] = n0;
  c[2] = n2;
}

// Box-Muller on the four output words of one Philox call: two 24-bit uniforms in (0,1] per pair (16777215 + 0.5 ties to 2^24), the
// one definition every generator below ends in
__device__ __forceinline__ void box_muller4(const uint32_t (&c)[4], float (&r)[4]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.28318530717958647692f * u2, &sn, &cs);
    r[2 * h] = rad * cs;
    r[2 * h + 1] = rad * sn;
  }
}

__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset) {
  const int64_t nquad = (n + 3) >> 2;
  for (int64_t q = blockIdx.x * 256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
    const uint64_t ctr = offset + (uint64_t)q;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      philox_round(c, k0, k1);
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    float r[4];
    box_muller4(c, r);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q * 4 + j < n) out[q * 4 + j] = r[j];
  }
}

// ------------------------------------------------------------------------------------------ ancestral (DDPM) step of the device loop
// p_sample (diffusion/gaussian_diffusion.py:376-417) with a fixed variance, the arithmetic of gaussian_step_kernel's sampler 0 as
// compiled -- every product of x0 and of the posterior mean rounded before its sum, the final + sd z fused -- written under
// contract(off) so that the compiler cannot fuse it otherwise (it used to: one product of each sum went unrounded into an fma, a
// last-bit difference from dn_gaussian_step; dn_gaussian_loop's p_sample over the same table is tested bit-equal to this loop);
// the noise is injected (`noise`, the row of this step) or drawn here: Philox4x32-10, key = seed, counter = (element quad, t) --
// t comes from the per-sample step vector the loop fills from its device counter, so graph replays draw fresh noise.
// kKeyed (dn_ddpm_loop_keyed): drawn from the utterance's key instead (step_noise_keyed4 below) -- x, eps and t are the launch's (a
// half batch's), keys the WHOLE batch's and quad0 the launch's first quad in it, so both halves draw under the keys alone.
__device__ __forceinline__ void philox_normal4(uint64_t seed, uint64_t ctr_lo, uint32_t ctr_hi, float (&r)[4]);
__device__ __forceinline__ void step_noise_keyed4(const uint64_t* __restrict__ keys, int64_t Q, int64_t row_quads, int t, float (&z)[4]);
template <bool kKeyed>
__global__ __launch_bounds__(256) void ddpm_step_kernel(float* x, const float* __restrict__ eps, int M, int C, int T,
                                                        const float* __restrict__ table, const int32_t* __restrict__ t,
                                                        int clip, const float* __restrict__ noise, int64_t noise_row, int t_top,
                                                        uint64_t seed, const uint64_t* __restrict__ keys, int64_t quad0, int64_t row_quads) {
  const int64_t nquad = ((int64_t)M * C) >> 2;  // C is a multiple of 4: a quad stays inside one row
  for (int64_t q = blockIdx.x * 256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
    const int64_t i = q << 2;
    const int m = (int)(i / C);
    const int tn = t[m / T];
    const float* tb = table + (int64_t)tn * DN_GD_COLS;
    const float4 xv = *reinterpret_cast<const float4*>(x + i), ev = *reinterpret_cast<const float4*>(eps + i);
    float z[4];
    if (kKeyed) {
      step_noise_keyed4(keys, quad0 + q, row_quads, tn, z);
    } else if (noise) {
      const float4 nv = *reinterpret_cast<const float4*>(noise + (int64_t)(t_top - tn) * noise_row + i);
      z[0] = nv.x; z[1] = nv.y; z[2] = nv.z; z[3] = nv.w;
    } else {
      philox_normal4(seed, (uint64_t)q, (uint32_t)tn, z);
    }
    const float sd = tn != 0 ? expf(__fmul_rn(0.5f, tb[4])) : 0.0f;
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, es[4] = {ev.x, ev.y, ev.z, ev.w};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
      float x0 = tb[0] * xs[j] - tb[1] * es[j];
      if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
      const float mean = tb[2] * x0 + tb[3] * xs[j];
      o[j] = fmaf(sd, z[j], mean);
    }
    *reinterpret_cast<float4*>(x + i) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

__device__ __forceinline__ void philox_normal4(uint64_t seed, uint64_t ctr_lo, uint32_t ctr_hi, float (&r)[4]) {
  uint32_t c[4] = {(uint32_t)ctr_lo, (uint32_t)(ctr_lo >> 32), ctr_hi, 0x44504d50u};  // ("DPMP": a stream apart from dn_randn's)
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  box_muller4(c, r);
}

// ------------------------------------------------------------------------------------------ keyed chain-start noise
// One noise stream per utterance: Philox4x32-10 under key = keys[b] (low, high), counter = (q low, q high, stream_id, "STRT"),
// q = frame * (Z / 4) + channel quad WITHIN the utterance -- a draw depends on the key, the frame and the channel only, not on the
// row b, the batch size, the padded length or the launch.  stream_id 0: posterior noise, 1: chain-start noise, 2 + t: the noise of the
// update that leaves timestep t (the keyed update kernels: step_noise_keyed4).  The fourth word keeps the stream apart from dn_randn's
// (0) and the seed-drawn update kernels' ("DPMP").
__device__ __forceinline__ void philox_keyed4(uint64_t key, uint64_t q, uint32_t stream_id, float (&r)[4]) {
  uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), stream_id, 0x53545254u};
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  box_muller4(c, r);
}

// The per-step noise of a keyed chain, shared by the three update kernels: quad Q of the WHOLE batch [B, T, Z] (row_quads = T Z / 4
// quads per utterance) at timestep t -> keys[b]'s stream 2 + t at the quad within the utterance, which is what dn_randn_keyed
// materialises for stream_id = 2 + t.  The timestep, not the step index, is the stream: a draw does not depend on the schedule's
// other members.  One 64-bit division per quad, as chain_start_kernel pays.
__device__ __forceinline__ void step_noise_keyed4(const uint64_t* __restrict__ keys, int64_t Q, int64_t row_quads, int t, float (&z)[4]) {
  const int64_t b = Q / row_quads;
  philox_keyed4(keys[b], (uint64_t)(Q - b * row_quads), 2u + (uint32_t)t, z);
}

// out [B, T, Z] dense; one thread per quad of channels (Z is a multiple of 4: a quad stays inside one frame)
__global__ __launch_bounds__(256) void randn_keyed_kernel(float* __restrict__ out, const uint64_t* __restrict__ keys, int64_t nquad,
                                                          int64_t row_quads, uint32_t stream_id) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < nquad; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / row_quads;
    float r[4];
    philox_keyed4(keys[b], (uint64_t)(i - b * row_quads), stream_id, r);
    *reinterpret_cast<float4*>(out + (i << 2)) = make_float4(r[0], r[1], r[2], r[3]);
  }
}

// Posterior sample + q_sample in one pass (distributions.py:24-41, latent_module.py:1405-1409): posterior_kernel's and
// q_sample_kernel's statements in their order on the keyed draws n0 (stream 0) and n1 (stream 1); params [B*T, ldp] = [mean ; logvar],
// x and z (optional) dense [B*T, Z].  Pad frames are drawn like any other.
__global__ __launch_bounds__(256) void chain_start_kernel(const float* __restrict__ params, int ldp, const uint64_t* __restrict__ keys,
                                                          int64_t nquad, int64_t row_quads, int Z, const float* __restrict__ ca,
                                                          const float* __restrict__ cb, const int32_t* __restrict__ t,
                                                          float* __restrict__ x, float* __restrict__ z_out) {
  const int zq = Z >> 2;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < nquad; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / row_quads, m = i / zq;
    const int c = (int)(i - m * zq) << 2;
    const float* pr = params + m * ldp + c;
    const float4 mv = *reinterpret_cast<const float4*>(pr), lv4 = *reinterpret_cast<const float4*>(pr + Z);
    const uint64_t key = keys[b], q = (uint64_t)(i - b * row_quads);
    float n0[4], n1[4];
    philox_keyed4(key, q, 0u, n0);
    philox_keyed4(key, q, 1u, n1);
    const int tb = t[b];
    const float a = ca[tb], s = cb[tb];
    const float mean[4] = {mv.x, mv.y, mv.z, mv.w}, logvar[4] = {lv4.x, lv4.y, lv4.z, lv4.w};
    float zs[4], xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lv = fminf(fmaxf(logvar[j], -30.0f), 20.0f);
      const float sd = expf(0.5f * lv);
      // z = __fadd_rn(mean, __fmul_rn(sd, n0)), x = __fadd_rn(__fmul_rn(a, z), __fmul_rn(s, n1)) as the compiler builds them in
      // posterior_kernel and q_sample_kernel (sd n0 contracted into its sum; a z onto the rounded s n1), spelled out so that this
      // kernel cannot be contracted differently (as sched_update does for ddim_step_kernel)
      zs[j] = fmaf(sd, n0[j], mean[j]);
      xs[j] = fmaf(a, zs[j], __fmul_rn(s, n1[j]));
    }
    *reinterpret_cast<float4*>(x + (i << 2)) = make_float4(xs[0], xs[1], xs[2], xs[3]);
    if (z_out) *reinterpret_cast<float4*>(z_out + (i << 2)) = make_float4(zs[0], zs[1], zs[2], zs[3]);
  }
}

// ------------------------------------------------------------------------------------------ convert rows
__global__ __launch_bounds__(256) void convert_rows_kernel(const void* __restrict__ src, int sdt, int lds, void* __restrict__ dst, int ddt,
                                                           int ldd, int M, int C) {
  const int64_t n = (int64_t)M * ldd;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i / ldd), c = (int)(i - (int64_t)m * ldd);
    float v = 0.f;
    if (c < C) {
      const int64_t so = (int64_t)m * lds + c;
      v = sdt == DN_BF16X3 ? load1_split(src, so) : dn_is16(sdt) ? from_h16(sdt, reinterpret_cast<const uint16_t*>(src)[so]) : reinterpret_cast<const float*>(src)[so];
    }
    store_act(dst, i, ddt, v);
  }
}


// ------------------------------------------------------------------------------------------ generic Gaussian step
// One reverse step of the OpenAI-style scheduler for an eps-predicting model: pred_xstart (optionally clipped),
// posterior mean, fixed / learned-range variance, then either the ancestral sample (p_sample) or the DDIM update.
// table: fp32 [T, DN_GD_COLS] = {sqrt_recip_abar, sqrt_recipm1_abar, post_coef1, post_coef2, fixed_log_var,
// min_log, max_log, abar, abar_prev} -- the fp32 casts of the float64 schedule, as _extract_into_tensor makes.
__global__ __launch_bounds__(256) void gaussian_step_kernel(const DnGaussianStep p) {
  const int64_t total = (int64_t)p.N * p.inner;
  const int cmul = p.learned_range ? 2 : 1;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i / p.inner);
    const int64_t rem = i - (int64_t)n * p.inner;
    const int tn = p.t[n];
    const float* tb = p.table + (int64_t)tn * DN_GD_COLS;
    const float xv = p.x[i];
    const float eps = p.model_out[(int64_t)n * p.inner * cmul + rem];
    float x0 = p.predict_xstart ? eps : __fsub_rn(__fmul_rn(tb[0], xv), __fmul_rn(tb[1], eps));  // START_X: the output is x_0 (:317-318)
    if (p.clip_denoised) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    float logvar = tb[4], var = tb[11];
    if (p.learned_range) {
      const float v = p.model_out[(int64_t)n * p.inner * 2 + p.inner + rem];
      const float frac = __fdiv_rn(__fadd_rn(v, 1.0f), 2.0f);
      logvar = __fadd_rn(__fmul_rn(frac, tb[6]), __fmul_rn(__fsub_rn(1.0f, frac), tb[5]));
      var = expf(logvar);
    }
    const float nz = tn != 0 ? 1.0f : 0.0f;
    const float nv = p.noise ? p.noise[i] : 0.0f;
    float out;
    if (p.sampler == 0) {  // p_sample: mean + 1[t != 0] * exp(0.5 * log_variance) * noise
      float mean = __fadd_rn(__fmul_rn(tb[2], x0), __fmul_rn(tb[3], xv));
      if (p.cond_grad) mean = __fadd_rn(mean, __fmul_rn(var, p.cond_grad[i]));  // condition_mean (:346-358)
      out = __fadd_rn(mean, __fmul_rn(__fmul_rn(nz, expf(__fmul_rn(0.5f, logvar))), nv));
    } else {  // ddim_sample
      if (p.cond_grad) {  // condition_score (:360-374): shift eps by the conditional score, re-derive the x_0 prediction (not re-clipped)
        float ec = __fdiv_rn(__fsub_rn(__fmul_rn(tb[0], xv), x0), tb[1]);
        ec = __fsub_rn(ec, __fmul_rn(sqrtf(__fsub_rn(1.0f, tb[7])), p.cond_grad[i]));
        x0 = __fsub_rn(__fmul_rn(tb[0], xv), __fmul_rn(tb[1], ec));
      }
      const float e2 = __fdiv_rn(__fsub_rn(__fmul_rn(tb[0], xv), x0), tb[1]);
      const float ab = tb[7], abp = tb[8];
      const float sigma = __fmul_rn(__fmul_rn(p.eta, sqrtf(__fdiv_rn(__fsub_rn(1.0f, abp), __fsub_rn(1.0f, ab)))),
                                    sqrtf(__fsub_rn(1.0f, __fdiv_rn(ab, abp))));
      const float mean = __fadd_rn(__fmul_rn(x0, sqrtf(abp)),
                                   __fmul_rn(sqrtf(__fsub_rn(__fsub_rn(1.0f, abp), __fmul_rn(sigma, sigma))), e2));
      out = __fadd_rn(mean, __fmul_rn(__fmul_rn(nz, sigma), nv));
    }
    p.sample[i] = out;
    if (p.pred_xstart) p.pred_xstart[i] = x0;
  }
}

// ------------------------------------------------------------------------------------------ scheduled updates of the device loops
// One update of a chain over a timestep schedule, in place on the float4 quads [q0, q0 + nquad) of the whole batch (engine.h: SchedStep),
// under row i = *counter of the rule's coefficients, uniform over the launch.  sched_step_kernel assembles it from an eps source, a
// rule and a sink, and every scheduled loop runs that one kernel: seeded, injected or keyed, whole batch or half, unconditional or
// guided.  So eager, graph replay, the two half-batch streams and the guided chain at scale 1 apply the same statements, each of
// which exists once below with every product and sum spelled out (or under contract(off)): no two chains can be contracted differently.
// HBM-bound: 2 reads (+ the null row, the history, an injected noise row) and 1 write (+ the history, one or two model inputs) of 16
// bytes per quad; grid-stride, no LDS.

// ---- eps source: the buffer's quad, or (kCfg) its conditioned row combined with the null row n elements further on.
// forward_with_cond_scale's combination (latent_module.py:813-826), three rounded operations; cfg_combine_kernel applies it too
__device__ __forceinline__ float cfg_combine(float c, float u, float scale) { return __fadd_rn(u, __fmul_rn(__fsub_rn(c, u), scale)); }
template <bool kCfg>
__device__ __forceinline__ void eps_quad(const float* __restrict__ eps, int64_t i, int64_t n, float scale, float (&es)[4]) {
  const float4 cv = *reinterpret_cast<const float4*>(eps + i);
  es[0] = cv.x; es[1] = cv.y; es[2] = cv.z; es[3] = cv.w;
  if (kCfg) {
    const float4 uv = *reinterpret_cast<const float4*>(eps + n + i);
    const float us[4] = {uv.x, uv.y, uv.z, uv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) es[j] = cfg_combine(es[j], us[j], scale);
  }
}

// ---- noise (engine.h: SchedNoise): the Philox counter is the element quad OF THE WHOLE BATCH and the step index -- a half-batch
// launch starts at its first quad, and the guided chain's B-row latent is the whole batch -- so eager, graph replay, the two half-batch
// streams and a scale-1 guided chain draw the same numbers.  kKeyed: the utterance's stream 2 + steps[i] (step_noise_keyed4): the
// timestep, the frame and the channel, not the row, B, the padded T or the step index.
// the four normals of quad q (elements i .. i+3) of the whole batch at `step` (timestep t): kKeyed: the utterance's stream 2 + t; else
// the injected row, or Philox keyed by (q, step)
template <bool kKeyed>
__device__ __forceinline__ void sched_normal4(const SchedNoise& s, int64_t q, int64_t i, int step, int t, float (&z)[4]) {
  const float* __restrict__ noise = s.noise;
  const int64_t noise_row = s.noise_row;
  const uint64_t seed = s.seed;
  if (kKeyed) {
    step_noise_keyed4(s.keys, q, s.row_quads, t, z);
  } else if (noise) {
    const float4 nv = *reinterpret_cast<const float4*>(noise + (int64_t)step * noise_row + i);
    z[0] = nv.x; z[1] = nv.y; z[2] = nv.z; z[3] = nv.w;
  } else {
    philox_normal4(seed, (uint64_t)q, (uint32_t)step, z);
  }
}

// ---- rules.  A rule reads row `step` of its coefficients once per thread, says whether the row draws, and maps a quad (x, eps, z) to
// the new x.
// DDIM (dn_ddim_sched_loop, dn_guided_ddim_loop): coef [n, DN_DDIM_SCHED_COLS] = {sqrt abar_e, sqrt(1-abar_e), sqrt abar_tgt,
// sqrt(1-abar_tgt-sigma^2), sigma}.  !kEta: the statements of ddim_step_kernel, product for product (as compiled: see sched_update).
// kEta: + 1[e_i != 0] sigma z (diffusion/gaussian_diffusion.py:513-560).
struct SchedCoef {
  float sa, s1, ct, cd, sg;
};
// row `step` of `coef`, with sigma masked to 0 without eta and at timestep 0
__device__ __forceinline__ SchedCoef sched_coef(const float* __restrict__ coef, const int32_t* __restrict__ steps, int step, bool eta_on) {
  const float* cf = coef + (int64_t)step * DN_DDIM_SCHED_COLS;
  return {cf[0], cf[1], cf[2], cf[3], (eta_on && steps[step] != 0) ? cf[4] : 0.0f};
}
// ddim_step_kernel's statements as the compiler builds them (products contracted into the sums that take them: x - s1 eps,
// x - sa x1, and x1 c2 onto the rounded c3 pn), spelled out so that no two kernels can be contracted differently
__device__ __forceinline__ float sched_update(const SchedCoef& c, float x, float e, float z, bool eta_on) {
  const float x1 = __fdiv_rn(fmaf(-c.s1, e, x), fmaxf(c.sa, 1e-10f));
  const float pn = __fdiv_rn(fmaf(-c.sa, x1, x), fmaxf(c.s1, 1e-10f));
  const float r = fmaf(c.ct, x1, __fmul_rn(c.cd, pn));
  return eta_on ? fmaf(c.sg, z, r) : r;
}
template <bool kEta>
struct DdimRule {
  SchedCoef c;
  __device__ DdimRule(const SchedStep& d, int step, bool) : c(sched_coef(d.coef, d.steps, step, kEta)) {}
  __device__ bool draws() const { return kEta; }
  __device__ void quad(const SchedStep&, int64_t, const float (&xs)[4], const float (&es)[4], const float (&z)[4], float (&o)[4]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = sched_update(c, xs[j], es[j], z[j], kEta);
  }
};

// DPM-Solver++(2M) (dn_dpm_loop, dn_guided_dpm_loop; Lu et al. 2022, data-prediction multistep form): coef [n, DN_DPM_COLS] =
// {alpha_s, sigma_s, a, b, c1, c0}:
//   x0_i = (x - sigma_s eps) / max(alpha_s, 1e-10);  x <- a x + b (c1 x0_i + c0 x0_{i-1});  hist <- x0_i.
// hist holds x0_{i-1} of the whole batch and is read only by a second-order row (c0 != 0: uniform over the launch), so the first row of
// a chain never reads what an earlier chain left there.  Deterministic: no draws.
struct Dpm2mRule {
  float as, ss, a, b, c1, c0;
  __device__ Dpm2mRule(const SchedStep& d, int step, bool) {
    const float* cf = d.coef + (int64_t)step * DN_DPM_COLS;
    as = fmaxf(cf[0], 1e-10f), ss = cf[1], a = cf[2], b = cf[3], c1 = cf[4], c0 = cf[5];
  }
  __device__ bool draws() const { return false; }
  __device__ void quad(const SchedStep& s, int64_t i, const float (&xs)[4], const float (&es)[4], const float (&)[4], float (&o)[4]) const {
    const bool two = c0 != 0.0f;
    float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (two) hv = *reinterpret_cast<const float4*>(s.hist + i);
    const float hs[4] = {hv.x, hv.y, hv.z, hv.w};
    float p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      p[j] = __fdiv_rn(fmaf(-ss, es[j], xs[j]), as);
      float d = __fmul_rn(c1, p[j]);
      if (two) d = fmaf(c0, hs[j], d);
      o[j] = fmaf(a, xs[j], __fmul_rn(b, d));
    }
    *reinterpret_cast<float4*>(s.hist + i) = make_float4(p[0], p[1], p[2], p[3]);
  }
};

// Generic Gaussian (dn_gaussian_loop, dn_gaussian_sched_step): a respaced p_sample / ddim_sample chain, gaussian_step_kernel's
// eps-predicting, fixed-variance branch under table [n_steps, DN_GD_COLS] given in chain order.  What depends on the row alone (the
// standard deviation, DDIM's sigma and its two square roots) is formed once per thread.  The noise switch is the RESPACED index,
// n_steps-1-i: the last row adds none, whatever original timestep steps[i] it has.  Nothing is drawn where nothing is added (the last
// row; DDIM at eta == 0), but an injected row is read as the host chain reads it.
// The arithmetic is gaussian_step_kernel's AS COMPILED, spelled out under contract(off) so that this kernel cannot be contracted
// differently (as sched_update does for ddim_step_kernel): there the products of x0, of the posterior mean and of DDIM's mean are
// rounded (packed multiplies) before their sums, DDIM's numerator is the rounded c0 x minus x0, and two sums take their product
// unrounded: 1 - abar_prev - sigma^2 and the final + sdev z.  A host-stepped chain over dn_gaussian_step is tested bit-equal.
struct GdRow {
  float c0, c1, c2, c3;  // sqrt_recip_abar, sqrt_recipm1_abar, posterior_mean_coef1, posterior_mean_coef2
  float sdev;            // the factor of z: 1[not the last row] exp(0.5 log_var) (p_sample) or sigma (ddim_sample)
  float sq_abp, sq_dir;  // ddim_sample: sqrt(abar_prev), sqrt(1 - abar_prev - sigma^2)
};
__device__ __forceinline__ GdRow gd_row(const float* __restrict__ tb, float nz, int sampler, float eta) {
#pragma clang fp contract(off)
  GdRow r = {tb[0], tb[1], tb[2], tb[3], 0.0f, 0.0f, 0.0f};
  if (sampler == 0) {
    r.sdev = nz * expf(0.5f * tb[4]);
  } else {
    const float ab = tb[7], abp = tb[8];
    const float sigma = (eta * sqrtf((1.0f - abp) / (1.0f - ab))) * sqrtf(1.0f - ab / abp);
    r.sq_abp = sqrtf(abp);
    r.sq_dir = sqrtf(fmaf(-sigma, sigma, 1.0f - abp));
    r.sdev = nz * sigma;
  }
  return r;
}
__device__ __forceinline__ float gd_update(const GdRow& r, float x, float e, float z, int sampler, int clip) {
#pragma clang fp contract(off)
  const float cx = r.c0 * x;
  float x0 = cx - r.c1 * e;
  if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  float mean;
  if (sampler == 0) {
    mean = r.c2 * x0 + r.c3 * x;
  } else {  // eps re-derived from the (clipped) x_0 prediction (:539)
    const float e2 = (cx - x0) / r.c1;
    mean = x0 * r.sq_abp + r.sq_dir * e2;
  }
  return fmaf(r.sdev, z, mean);
}
struct GaussRule {
  GdRow r;
  bool noisy;
  __device__ GaussRule(const SchedStep& d, int step, bool keyed) {
    const float nz = step != d.n_steps - 1 ? 1.0f : 0.0f;
    r = gd_row(d.coef + (int64_t)step * DN_GD_COLS, nz, d.sampler, d.eta);
    noisy = (nz != 0.0f && (d.sampler == 0 || d.eta != 0.0f)) || (!keyed && d.src.noise);
  }
  __device__ bool draws() const { return noisy; }
  __device__ void quad(const SchedStep& d, int64_t, const float (&xs)[4], const float (&es)[4], const float (&z)[4], float (&o)[4]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = gd_update(r, xs[j], es[j], z[j], d.sampler, d.clip);
  }
};

// ---- the kernel.  Sink: x, and the model's next input where it is another buffer -- xin[0:n] and (kCfg: the 2B-row pass) xin[n:2n],
// one pass where a host-driven guided chain copies x twice, combines, updates and decrements.  !kCfg: nothing past n is touched.
template <class Rule, bool kCfg, bool kKeyed>
__global__ __launch_bounds__(256) void sched_step_kernel(const SchedStep d) {
  const int step = *d.counter;
  const Rule rule(d, step, kKeyed);
  const int t = kKeyed ? d.steps[step] : 0;
  const bool draws = rule.draws();
  const int64_t q0 = d.elem0 >> 2, nquad = d.n_elem >> 2, n = d.n_elem;
  for (int64_t q = q0 + blockIdx.x * 256 + threadIdx.x; q < q0 + nquad; q += (int64_t)gridDim.x * 256) {
    const int64_t i = q << 2;
    const float4 xv = *reinterpret_cast<const float4*>(d.x + i);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
    float es[4], z[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    if (draws) sched_normal4<kKeyed>(d.src, q, i, step, t, z);  // (before eps is loaded: four registers fewer live across the Philox rounds)
    eps_quad<kCfg>(d.eps, i, n, d.scale, es);
    rule.quad(d, i, xs, es, z, o);
    const float4 ov = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(d.x + i) = ov;
    if (kCfg) {
      *reinterpret_cast<float4*>(d.xin + i) = ov;
      *reinterpret_cast<float4*>(d.xin + n + i) = ov;
    } else if (d.xin != d.x) {
      *reinterpret_cast<float4*>(d.xin + i) = ov;
    }
  }
}

// p_mean_variance / q_posterior_mean_variance / ddim_reverse_sample / the VB term, one thread per element (header: DnGaussianMoments)
__global__ __launch_bounds__(256) void gaussian_moments_kernel(const DnGaussianMoments p) {
  const int64_t total = (int64_t)p.N * p.inner;
  const int cmul = p.learned_range ? 2 : 1;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i / p.inner);
    const int64_t rem = i - (int64_t)n * p.inner;
    const int tn = p.t[n];
    const float* tb = p.table + (int64_t)tn * DN_GD_COLS;
    const float xv = p.x[i];
    if (!p.model_out) {  // q(x_{t-1} | x_t, x_0)
      const float xs = p.x_start[i];
      if (p.mean) p.mean[i] = __fadd_rn(__fmul_rn(tb[2], xs), __fmul_rn(tb[3], xv));
      if (p.variance) p.variance[i] = tb[10];
      if (p.log_variance) p.log_variance[i] = tb[5];
      continue;
    }
    const float eps = p.model_out[(int64_t)n * p.inner * cmul + rem];
    float x0 = p.predict_xstart ? eps : __fsub_rn(__fmul_rn(tb[0], xv), __fmul_rn(tb[1], eps));
    if (p.clip_denoised) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    float logvar = tb[4], var = tb[11];
    if (p.learned_range) {
      const float v = p.model_out[(int64_t)n * p.inner * 2 + p.inner + rem];
      const float frac = __fdiv_rn(__fadd_rn(v, 1.0f), 2.0f);
      logvar = __fadd_rn(__fmul_rn(frac, tb[6]), __fmul_rn(__fsub_rn(1.0f, frac), tb[5]));
      var = expf(logvar);
    }
    const float mean = __fadd_rn(__fmul_rn(tb[2], x0), __fmul_rn(tb[3], xv));
    if (p.mean) p.mean[i] = mean;
    if (p.variance) p.variance[i] = var;
    if (p.log_variance) p.log_variance[i] = logvar;
    if (p.pred_xstart) p.pred_xstart[i] = x0;
    if (p.reverse_sample) {  // (:583-596)
      const float e2 = __fdiv_rn(__fsub_rn(__fmul_rn(tb[0], xv), x0), tb[1]);
      const float abn = tb[9];
      p.reverse_sample[i] = __fadd_rn(__fmul_rn(x0, sqrtf(abn)), __fmul_rn(sqrtf(__fsub_rn(1.0f, abn)), e2));
    }
    if (p.vb && p.x_start) {
      const float xs = p.x_start[i];
      float v;
      if (tn != 0) {  // normal_kl(true_mean, true_log_variance_clipped, mean, log_variance), diffusion_utils.py:10-34
        const float tm = __fadd_rn(__fmul_rn(tb[2], xs), __fmul_rn(tb[3], xv));
        const float lv1 = tb[5], d = tm - mean;
        v = 0.5f * (-1.0f + logvar - lv1 + expf(lv1 - logvar) + d * d * expf(-logvar));
      } else {  // -discretized_gaussian_log_likelihood(x_start, means = mean, log_scales = 0.5 * log_variance)
        const float c = xs - mean, inv = expf(-0.5f * logvar);
        auto cdf = [](float z) { return 0.5f * (1.0f + tanhf(0.79788456080286535588f * (z + 0.044715f * z * z * z))); };
        const float cp = cdf(inv * (c + 1.0f / 255.0f)), cm = cdf(inv * (c - 1.0f / 255.0f));
        const float lp = xs < -0.999f ? logf(fmaxf(cp, 1e-12f)) : (xs > 0.999f ? logf(fmaxf(1.0f - cm, 1e-12f)) : logf(fmaxf(cp - cm, 1e-12f)));
        v = -lp;
      }
      p.vb[i] = v * 1.44269504088896340736f;  // / ln 2: bits
    }
  }
}

// ------------------------------------------------------------------------------------------ CMLM mask-predict update (f4)
// One workgroup per sequence (T <= 2048).  Phase 1: every position holding `unk` (the mask symbol) takes argmax / max of the
// log-softmax of its logit row (one wave per position; the two scorings below).  Phase 2 (not on the last iteration): the boundary
// lowest-scoring positions -- boundary = trunc((n_nonpad - 2) * p), scores ascending, ties by position -- are re-masked (token = unk,
// score = 0).
// step_dev != nullptr: the iteration index is read from the device (a captured refinement iteration is replayed while a device
// counter advances: nothing of the iteration is baked into the graph) and p / remask are derived here exactly as the host derives them.

// Unguided scoring (forward_decoder): arg-max / max of log_softmax(lr[0:V]), the maximum first and the sum in a second pass.
__device__ __forceinline__ void cmlm_score(const float* __restrict__ lr, int V, int lane, int32_t& tok, float& sc) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < V; c += 64) {
    const float v = lr[c];
    if (v > best) { best = v; bi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  float se = 0.f;
  for (int c = lane; c < V; c += 64) se += expf(lr[c] - best);
  se = wave_sum(se);
  tok = bi;
  sc = -logf(se);  // max - logsumexp = -(log sum exp(x - max))
}

// Guided scoring (research/TranSpeech/nat_gen.py:223-226; classifier-free guidance, --cg_scale): arg-max / max of
// log_softmax(cond + scale * (cond - null)).  The combination, the log-softmax and the arg-max are one pass over the two logit rows
// (running maximum and rescaled sum per lane, merged across the wave): each row is read once and the scaled logits are never written.
// The three roundings of the combination are torch's (no contraction into an FMA).
__device__ __forceinline__ void cmlm_score_guided(const float* __restrict__ lc, const float* __restrict__ ln, float scale, int V, int lane,
                                                  int32_t& tok, float& sc) {
  float best = -INFINITY, se = 0.f;
  int bi = 0x7fffffff;
  for (int c = lane; c < V; c += 64) {
    const float cv = lc[c];
    const float v = __fadd_rn(cv, __fmul_rn(scale, __fsub_rn(cv, ln[c])));
    if (v > best) {
      se = se * expf(best - v) + 1.0f;  // (first element: 0 * exp(-inf) + 1)
      best = v; bi = c;
    } else {
      se += expf(v - best);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64), os = __shfl_xor(se, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const float mx = fmaxf(best, ov);
    const float sa = best == -INFINITY ? 0.f : se * expf(best - mx), sb = ov == -INFINITY ? 0.f : os * expf(ov - mx);
    se = sa + sb;  // (commutative: both lanes of a pair hold the same sum)
    if (ov > best || (ov == best && oi < bi)) bi = oi;
    best = mx;
  }
  tok = bi;
  sc = -logf(se);  // max - logsumexp
}

// kGuided: logits = [cond rows ; null rows] of one 2B-row pass (the grid is the B sequences), and the scores START FROM ZERO in every
// iteration (nat_gen.py:197, output_scores = new_full(shape, 0.0)); else a kept position keeps its earlier score (forward_decoder).
template <bool kGuided>
__global__ __launch_bounds__(256) void cmlm_step_kernel(const float* __restrict__ logits, float scale, int32_t* __restrict__ tokens,
                                                        float* __restrict__ scores, int32_t* __restrict__ predicted, int T, int V, float p,
                                                        int remask, int unk, int pad, const int32_t* __restrict__ step_dev, int max_step) {
  if (step_dev) {
    const int step = *step_dev;
    remask = (step + 1) < max_step;
    p = (float)(1.0 - (double)(step + 1) / (double)max_step);  // the Python float of the reference, cast to the scores' fp32
  }
  __shared__ float s_sc[2048];
  __shared__ int32_t s_tok[2048];
  __shared__ int s_n;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t half = (int64_t)gridDim.x * T * V;
  if (threadIdx.x == 0) s_n = 0;
  for (int t = wave; t < T; t += 4) {
    int32_t tok = tokens[(int64_t)b * T + t];
    float sc = kGuided ? 0.f : scores[(int64_t)b * T + t];
    if (tok == unk) {  // wave-uniform
      const float* lr = logits + ((int64_t)b * T + t) * V;
      if (kGuided)
        cmlm_score_guided(lr, lr + half, scale, V, lane, tok, sc);
      else
        cmlm_score(lr, V, lane, tok, sc);
    }
    if (lane == 0) {
      s_tok[t] = tok;
      s_sc[t] = sc;
      predicted[(int64_t)b * T + t] = tok;
    }
  }
  __syncthreads();
  if (remask) {
    int cnt = 0;
    for (int t = threadIdx.x; t < T; t += 256) cnt += s_tok[t] != pad;
    if (cnt) atomicAdd(&s_n, cnt);  // integer count within the workgroup: order-independent
    __syncthreads();
    const long long boundary = (long long)((float)(s_n - 2) * p);
    for (int i = threadIdx.x; i < T; i += 256) {
      const float si = s_sc[i];
      int rank = 0;
      for (int j = 0; j < T; ++j) {
        const float sj = s_sc[j];
        rank += (sj < si) || (sj == si && j < i);
      }
      int32_t tok = s_tok[i];
      float sc = si;
      if ((long long)rank < boundary) { tok = unk; sc = 0.f; }
      tokens[(int64_t)b * T + i] = tok;
      scores[(int64_t)b * T + i] = sc;
    }
  } else {
    for (int i = threadIdx.x; i < T; i += 256) {
      tokens[(int64_t)b * T + i] = s_tok[i];
      scores[(int64_t)b * T + i] = s_sc[i];
    }
  }
}

// blocks of this file's grid-stride kernels: at least one, at most kPointwiseGridCap (engine.h's ew_grid stops at 4096)
constexpr int kPointwiseGridCap = 2048;
static inline int pw_grid(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > kPointwiseGridCap ? kPointwiseGridCap : b));
}

}  // namespace dn

using namespace dn;

extern "C" int dn_rmsnorm(const float* x, int32_t ldx, void* y, int32_t ldy, int32_t out_dtype, int32_t M, int32_t D, int32_t T,
                          const float* gamma, const float* gamma_beta, int32_t gb_ld, int32_t gb_half, void* stream) {
  DN_CHECK_ARG(x && y && M > 0 && D > 0 && T > 0, "dn_rmsnorm: bad args");
  DN_CHECK_ARG(D % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldy >= D && ldx >= D, "dn_rmsnorm: D=%d ldx=%d ldy=%d must be multiples of 4", D, ldx, ldy);
  DN_CHECK_ARG(!gamma_beta || (gb_ld % 4 == 0 && gb_half % 4 == 0), "dn_rmsnorm: gamma_beta strides must be multiples of 4");
  hipLaunchKernelGGL(rmsnorm_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, out_dtype, M, D, T, gamma,
                     gamma_beta, gb_ld, gb_half);
  DN_CHECK_LAUNCH("dn_rmsnorm");
  return DN_OK;
}

extern "C" int dn_time_cond(const int32_t* times, int32_t B, const float* w_freq, int32_t half, const float* W, const float* bias,
                            int32_t C, float* out, void* out_act, int32_t act_dtype, int32_t ldo, void* stream) {
  DN_CHECK_ARG(times && w_freq && W && bias && out && B > 0 && half > 0 && C > 0 && ldo >= C, "dn_time_cond: bad args");
  hipLaunchKernelGGL(time_cond_kernel, dim3((C + 15) / 16, B), dim3(256), (2 * half + 1) * sizeof(float), (hipStream_t)stream, times,
                     w_freq, half, W, bias, C, out, out_act, act_dtype, ldo);
  DN_CHECK_LAUNCH("dn_time_cond");
  return DN_OK;
}

extern "C" int dn_ddim_step(const float* x, const float* eps, float* x_out, void* x_act, int32_t act_dtype, int32_t ld_act, int32_t M,
                            int32_t C, int32_t ld, int32_t T, const float* coef, const int32_t* t, void* stream) {
  DN_CHECK_ARG(x && eps && x_out && coef && t && M > 0 && C > 0 && ld >= C && T > 0, "dn_ddim_step: bad args");
  hipLaunchKernelGGL(ddim_step_kernel, dim3(pw_grid((int64_t)M * C)), dim3(256), 0, (hipStream_t)stream, x, eps, x_out, x_act, act_dtype,
                     ld_act, M, C, ld, T, coef, t);
  DN_CHECK_LAUNCH("dn_ddim_step");
  return DN_OK;
}

// forward_with_cond_scale's combination (latent_module.py:813-826): out = null + (cond - null) * scale over the two halves of one
// 2B-batch pass ([cond rows ; null rows])
__global__ __launch_bounds__(256) void cfg_combine_kernel(const float* __restrict__ both, float scale, int64_t n, float* __restrict__ out) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    out[i] = cfg_combine(both[i], both[n + i], scale);
  }
}
extern "C" int dn_cfg_combine(const float* both, float scale, int64_t n, float* out, void* stream) {
  DN_CHECK_ARG(both && out && n > 0, "dn_cfg_combine: bad argument");
  hipLaunchKernelGGL(cfg_combine_kernel, dim3(pw_grid(n)), dim3(256), 0, (hipStream_t)stream, both, scale, n, out);
  DN_CHECK_LAUNCH("dn_cfg_combine");
  return DN_OK;
}

// (engine.h: the ancestral update of dn_ddpm_loop)
// keys != NULL (dn_ddpm_loop_keyed): the whole batch's keys and the launch's first batch row b0; noise and seed are not read
int dn_ddpm_step_launch(float* x, const float* eps, int M, int C, int T, const float* table, const int32_t* t, int clip, const float* noise,
                        int64_t noise_row, int t_top, uint64_t seed, const uint64_t* keys, int b0, void* stream_) {
  DN_CHECK_ARG(C % 4 == 0, "dn_ddpm_loop: the latent width must be a multiple of 4");
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(pw_grid(((int64_t)M * C) >> 2)), block(256);
  const int64_t row_quads = (int64_t)T * (C >> 2);
  if (keys)
    hipLaunchKernelGGL(ddpm_step_kernel<true>, grid, block, 0, stream, x, eps, M, C, T, table, t, clip, nullptr, 0, t_top, 0, keys,
                       (int64_t)b0 * row_quads, row_quads);
  else
    hipLaunchKernelGGL(ddpm_step_kernel<false>, grid, block, 0, stream, x, eps, M, C, T, table, t, clip, noise, noise_row, t_top, seed, nullptr,
                       0, 0);
  DN_CHECK_LAUNCH("dn_ddpm_loop step");
  return DN_OK;
}

// (engine.h) the one launcher of the scheduled updates: the instantiation a descriptor names
template <class Rule, bool kCfg, bool kKeyed>
static void sched_launch(const SchedStep& d, hipStream_t stream) {
  hipLaunchKernelGGL((sched_step_kernel<Rule, kCfg, kKeyed>), dim3(pw_grid(d.n_elem >> 2)), dim3(256), 0, stream, d);
}
template <class Rule, bool kKeyed>
static void sched_launch_source(const SchedStep& d, hipStream_t stream) {
  d.guided ? sched_launch<Rule, true, kKeyed>(d, stream) : sched_launch<Rule, false, kKeyed>(d, stream);
}
int dn::sched_step_launch(const char* who, const SchedStep& desc, void* stream_) {
  DN_CHECK_ARG(desc.elem0 % 4 == 0 && desc.n_elem % 4 == 0 && desc.n_elem > 0, "%s: the latent width must be a multiple of 4", who);
  DN_CHECK_ARG(!desc.guided || (desc.rule != SCHED_GAUSSIAN && desc.elem0 == 0), "%s: no guided form of this update", who);
  SchedStep d = desc;
  if (!d.xin) d.xin = d.x;  // (the kernel writes xin where it is not x)
  hipStream_t stream = (hipStream_t)stream_;
  const bool keyed = d.src.keys != nullptr;
  if (d.rule == SCHED_DPM2M)
    sched_launch_source<Dpm2mRule, false>(d, stream);
  else if (d.rule == SCHED_GAUSSIAN)
    keyed ? sched_launch<GaussRule, false, true>(d, stream) : sched_launch<GaussRule, false, false>(d, stream);
  else if (keyed)
    sched_launch_source<DdimRule<true>, true>(d, stream);
  else
    d.eta_on ? sched_launch_source<DdimRule<true>, false>(d, stream) : sched_launch_source<DdimRule<false>, false>(d, stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    dn_set_error("%s step: %s", who, hipGetErrorString(e));
    return DN_ELAUNCH;
  }
  return DN_OK;
}

extern "C" int dn_dpm2m_step(float* x, const float* eps, float* hist, int64_t n, const float* coef, const int32_t* step_index, void* stream) {
  DN_CHECK_ARG(x && eps && hist && coef && step_index, "dn_dpm2m_step: null argument");
  DN_CHECK_ARG(n > 0 && n % 4 == 0, "dn_dpm2m_step: n=%lld must be a positive multiple of 4", (long long)n);
  DN_CHECK_ARG((((uintptr_t)x | (uintptr_t)eps | (uintptr_t)hist) & 15) == 0, "dn_dpm2m_step: x, eps and hist must be 16-byte aligned");
  SchedStep u = {SCHED_DPM2M, x, 0, n, eps};
  u.coef = coef; u.counter = step_index; u.hist = hist;
  return sched_step_launch("dn_dpm_loop", u, stream);
}

extern "C" int dn_ddim_sched_step(float* x, const float* eps, int64_t n, const float* coef, const int32_t* steps, const int32_t* step_index,
                                  int32_t eta_on, uint64_t seed, const float* noise, void* stream) {
  DN_CHECK_ARG(x && eps && coef && steps && step_index, "dn_ddim_sched_step: null argument");
  DN_CHECK_ARG(n > 0 && n % 4 == 0, "dn_ddim_sched_step: n=%lld must be a positive multiple of 4", (long long)n);
  DN_CHECK_ARG((((uintptr_t)x | (uintptr_t)eps | (uintptr_t)noise) & 15) == 0, "dn_ddim_sched_step: x, eps and noise must be 16-byte aligned");
  DN_CHECK_ARG(eta_on || !noise, "dn_ddim_sched_step: injected noise needs eta_on (eta = 0 draws none)");
  SchedStep u = {SCHED_DDIM, x, 0, n, eps};
  u.coef = coef; u.steps = steps; u.counter = step_index; u.eta_on = eta_on != 0;
  u.src = sched_noise(noise, 0, eta_on ? seed : 0, nullptr, 0);  // (row stride 0: `noise` is this step's row whatever the step index)
  return sched_step_launch("dn_ddim_sched_loop", u, stream);
}

extern "C" int dn_ddim_sched_step_keyed(float* x, const float* eps, const uint64_t* keys, int32_t B, int32_t T, int32_t Z, const float* coef,
                                        const int32_t* steps, const int32_t* step_index, void* stream) {
  DN_CHECK_ARG(x && eps && keys && coef && steps && step_index, "dn_ddim_sched_step_keyed: null argument");
  DN_CHECK_ARG(B > 0 && T > 0 && Z > 0 && Z % 4 == 0, "dn_ddim_sched_step_keyed: B=%d T=%d must be positive, Z=%d a positive multiple of 4", B, T,
               Z);
  DN_CHECK_ARG((((uintptr_t)x | (uintptr_t)eps) & 15) == 0 && ((uintptr_t)keys & 7) == 0,
               "dn_ddim_sched_step_keyed: x and eps must be 16-byte, keys 8-byte aligned");
  const int64_t row_quads = (int64_t)T * (Z >> 2);
  SchedStep u = {SCHED_DDIM, x, 0, (int64_t)B * row_quads * 4, eps};
  u.coef = coef; u.steps = steps; u.counter = step_index; u.eta_on = 1;
  u.src = sched_noise(nullptr, 0, 0, keys, row_quads);
  return sched_step_launch("dn_ddim_sched_loop", u, stream);
}

// what the four dn_gaussian_* entries check of the update's own arguments
int dn_gaussian_sched_args(const char* who, int32_t n_steps, int32_t sampler, float eta) {
  DN_CHECK_ARG(n_steps >= 1, "%s: n_steps=%d must be positive", who, n_steps);
  DN_CHECK_ARG(sampler == 0 || sampler == 1, "%s: sampler=%d (0 = p_sample, 1 = ddim_sample)", who, sampler);
  DN_CHECK_ARG(eta >= 0.0f && eta <= 1e30f, "%s: eta=%g must be finite and not negative", who, (double)eta);
  return DN_OK;
}

extern "C" int dn_gaussian_sched_step(float* x, const float* eps, int64_t n, const float* table, const int32_t* step_index, int32_t n_steps,
                                      int32_t sampler, int32_t clip_denoised, float eta, uint64_t seed, const float* noise, void* stream) {
  DN_CHECK_ARG(x && eps && table && step_index, "dn_gaussian_sched_step: null argument");
  DN_CHECK_ARG(n > 0 && n % 4 == 0, "dn_gaussian_sched_step: n=%lld must be a positive multiple of 4", (long long)n);
  DN_CHECK_ARG((((uintptr_t)x | (uintptr_t)eps | (uintptr_t)noise) & 15) == 0, "dn_gaussian_sched_step: x, eps and noise must be 16-byte aligned");
  if (const int rc = dn_gaussian_sched_args("dn_gaussian_sched_step", n_steps, sampler, eta)) return rc;
  SchedStep u = {SCHED_GAUSSIAN, x, 0, n, eps};
  u.coef = table; u.counter = step_index; u.n_steps = n_steps; u.sampler = sampler; u.clip = clip_denoised != 0; u.eta = eta;
  u.src = sched_noise(noise, 0, seed, nullptr, 0);  // (row stride 0: `noise` is this step's row whatever the step index)
  return sched_step_launch("dn_gaussian_loop", u, stream);
}

extern "C" int dn_gaussian_sched_step_keyed(float* x, const float* eps, const uint64_t* keys, int32_t B, int32_t T, int32_t Z, const float* table,
                                            const int32_t* steps, const int32_t* step_index, int32_t n_steps, int32_t sampler,
                                            int32_t clip_denoised, float eta, void* stream) {
  DN_CHECK_ARG(x && eps && keys && table && steps && step_index, "dn_gaussian_sched_step_keyed: null argument");
  DN_CHECK_ARG(B > 0 && T > 0 && Z > 0 && Z % 4 == 0, "dn_gaussian_sched_step_keyed: B=%d T=%d must be positive, Z=%d a positive multiple of 4", B,
               T, Z);
  DN_CHECK_ARG((((uintptr_t)x | (uintptr_t)eps) & 15) == 0 && ((uintptr_t)keys & 7) == 0,
               "dn_gaussian_sched_step_keyed: x and eps must be 16-byte, keys 8-byte aligned");
  if (const int rc = dn_gaussian_sched_args("dn_gaussian_sched_step_keyed", n_steps, sampler, eta)) return rc;
  const int64_t row_quads = (int64_t)T * (Z >> 2);
  SchedStep u = {SCHED_GAUSSIAN, x, 0, (int64_t)B * row_quads * 4, eps};
  u.coef = table; u.steps = steps; u.counter = step_index; u.n_steps = n_steps; u.sampler = sampler; u.clip = clip_denoised != 0; u.eta = eta;
  u.src = sched_noise(nullptr, 0, 0, keys, row_quads);
  return sched_step_launch("dn_gaussian_loop", u, stream);
}

extern "C" int dn_q_sample(const float* x, const float* noise, float* out, void* out_act, int32_t act_dtype, int32_t ld_act, int32_t M,
                           int32_t C, int32_t ld, int32_t T, const float* coef_a, const float* coef_b, const int32_t* t, void* stream) {
  DN_CHECK_ARG(x && noise && out && coef_a && coef_b && t && M > 0 && C > 0 && ld >= C && T > 0, "dn_q_sample: bad args");
  hipLaunchKernelGGL(q_sample_kernel, dim3(pw_grid((int64_t)M * C)), dim3(256), 0, (hipStream_t)stream, x, noise, out, out_act, act_dtype,
                     ld_act, M, C, ld, T, coef_a, coef_b, t);
  DN_CHECK_LAUNCH("dn_q_sample");
  return DN_OK;
}

extern "C" int dn_posterior_sample(const float* params, int32_t ldp, const float* noise, int32_t ldn, float* z, void* z_act,
                                   int32_t act_dtype, int32_t ldz, int32_t M, int32_t Z, int32_t T, const int32_t* lengths,
                                   float* kl_rows, void* stream) {
  DN_CHECK_ARG(params && noise && z && M > 0 && Z > 0 && ldp >= 2 * Z && ldn >= Z && ldz >= Z && T > 0, "dn_posterior_sample: bad args");
  hipLaunchKernelGGL(posterior_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, params, ldp, noise, ldn, z, z_act, act_dtype,
                     ldz, M, Z, T, lengths, kl_rows);
  DN_CHECK_LAUNCH("dn_posterior_sample");
  return DN_OK;
}

extern "C" int dn_argmax_units(const float* logits, int32_t ld, int32_t M, int32_t V, int32_t offset, int32_t* units, void* stream) {
  DN_CHECK_ARG(logits && units && M > 0 && V > 0 && ld >= V, "dn_argmax_units: bad args");
  hipLaunchKernelGGL(argmax_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, M, V, offset, units);
  DN_CHECK_LAUNCH("dn_argmax_units");
  return DN_OK;
}

extern "C" int dn_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
  DN_CHECK_ARG(out && n > 0, "dn_randn: bad args");
  hipLaunchKernelGGL(randn_kernel, dim3(pw_grid((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n, seed, offset);
  DN_CHECK_LAUNCH("dn_randn");
  return DN_OK;
}

extern "C" int dn_randn_keyed(float* out, const uint64_t* keys, int32_t B, int32_t T, int32_t Z, uint32_t stream_id, void* stream) {
  DN_CHECK_ARG(out && keys, "dn_randn_keyed: null argument");
  DN_CHECK_ARG(B > 0 && T > 0 && Z > 0 && Z % 4 == 0, "dn_randn_keyed: B=%d T=%d must be positive, Z=%d a positive multiple of 4", B, T, Z);
  DN_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)keys & 7) == 0, "dn_randn_keyed: out must be 16-byte, keys 8-byte aligned");
  const int64_t row_quads = (int64_t)T * (Z >> 2), nquad = (int64_t)B * row_quads;
  hipLaunchKernelGGL(randn_keyed_kernel, dim3(pw_grid(nquad)), dim3(256), 0, (hipStream_t)stream, out, keys, nquad, row_quads, stream_id);
  DN_CHECK_LAUNCH("dn_randn_keyed");
  return DN_OK;
}

extern "C" int dn_chain_start(const float* params, int32_t ldp, const uint64_t* keys, int32_t B, int32_t T, int32_t Z, const float* coef_a,
                              const float* coef_b, const int32_t* t, float* x, float* z_out, void* stream) {
  DN_CHECK_ARG(params && keys && coef_a && coef_b && t && x, "dn_chain_start: null argument");
  DN_CHECK_ARG(B > 0 && T > 0 && Z > 0 && Z % 4 == 0, "dn_chain_start: B=%d T=%d must be positive, Z=%d a positive multiple of 4", B, T, Z);
  DN_CHECK_ARG(ldp >= 2 * Z && ldp % 4 == 0, "dn_chain_start: ldp=%d must be a multiple of 4 and at least 2 Z = %d", ldp, 2 * Z);
  DN_CHECK_ARG((((uintptr_t)params | (uintptr_t)x | (uintptr_t)z_out) & 15) == 0 && ((uintptr_t)keys & 7) == 0,
               "dn_chain_start: params, x and z_out must be 16-byte, keys 8-byte aligned");
  const int64_t row_quads = (int64_t)T * (Z >> 2), nquad = (int64_t)B * row_quads;
  hipLaunchKernelGGL(chain_start_kernel, dim3(pw_grid(nquad)), dim3(256), 0, (hipStream_t)stream, params, ldp, keys, nquad, row_quads, Z,
                     coef_a, coef_b, t, x, z_out);
  DN_CHECK_LAUNCH("dn_chain_start");
  return DN_OK;
}

extern "C" int dn_convert_rows(const void* src, int32_t src_dtype, int32_t lds, void* dst, int32_t dst_dtype, int32_t ldd, int32_t M,
                               int32_t C, void* stream) {
  DN_CHECK_ARG(src && dst && M > 0 && C > 0 && lds >= C && ldd >= C, "dn_convert_rows: bad args");
  hipLaunchKernelGGL(convert_rows_kernel, dim3(pw_grid((int64_t)M * ldd)), dim3(256), 0, (hipStream_t)stream, src, src_dtype, lds, dst,
                     dst_dtype, ldd, M, C);
  DN_CHECK_LAUNCH("dn_convert_rows");
  return DN_OK;
}

extern "C" int dn_gaussian_step(const DnGaussianStep* p, void* stream) {
  DN_CHECK_ARG(p && p->x && p->model_out && p->sample && p->t && p->table, "dn_gaussian_step: null argument");
  DN_CHECK_ARG(p->N > 0 && p->inner > 0 && (p->sampler == 0 || p->sampler == 1), "dn_gaussian_step: bad shape / sampler");
  hipLaunchKernelGGL(gaussian_step_kernel, dim3(pw_grid((int64_t)p->N * p->inner)), dim3(256), 0, (hipStream_t)stream, *p);
  DN_CHECK_LAUNCH("dn_gaussian_step");
  return DN_OK;
}

extern "C" int dn_gaussian_moments(const DnGaussianMoments* p, void* stream) {
  DN_CHECK_ARG(p && p->x && p->t && p->table && (p->model_out || p->x_start), "dn_gaussian_moments: null argument");
  DN_CHECK_ARG(p->N > 0 && p->inner > 0, "dn_gaussian_moments: bad shape");
  hipLaunchKernelGGL(gaussian_moments_kernel, dim3(pw_grid((int64_t)p->N * p->inner)), dim3(256), 0, (hipStream_t)stream, *p);
  DN_CHECK_LAUNCH("dn_gaussian_moments");
  return DN_OK;
}

extern "C" int dn_cmlm_step(const float* logits, int32_t* tokens, float* scores, int32_t* predicted, int32_t B, int32_t T, int32_t V,
                            int32_t step, int32_t max_step, int32_t unk, int32_t pad, void* stream) {
  DN_CHECK_ARG(logits && tokens && scores && predicted && B > 0 && T > 0 && T <= 2048 && V > 1 && max_step > 0 && step >= 0,
               "dn_cmlm_step: bad args (T=%d must be <= 2048)", T);
  const int remask = (step + 1) < max_step;
  const float p = (float)(1.0 - (double)(step + 1) / (double)max_step);  // the Python float of the reference, cast to the scores' fp32
  hipLaunchKernelGGL(cmlm_step_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, 0.f, tokens, scores, predicted, T, V, p, remask, unk,
                     pad, (const int32_t*)nullptr, max_step);
  DN_CHECK_LAUNCH("dn_cmlm_step");
  return DN_OK;
}

extern "C" int dn_cmlm_step_dev(const float* logits, int32_t* tokens, float* scores, int32_t* predicted, int32_t B, int32_t T, int32_t V,
                                const int32_t* step_dev, int32_t max_step, int32_t unk, int32_t pad, void* stream) {
  DN_CHECK_ARG(logits && tokens && scores && predicted && step_dev && B > 0 && T > 0 && T <= 2048 && V > 1 && max_step > 0,
               "dn_cmlm_step_dev: bad args (T=%d must be <= 2048)", T);
  hipLaunchKernelGGL(cmlm_step_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, 0.f, tokens, scores, predicted, T, V, 0.f, 0, unk,
                     pad, step_dev, max_step);
  DN_CHECK_LAUNCH("dn_cmlm_step_dev");
  return DN_OK;
}

extern "C" int dn_cmlm_guided_step(const float* logits2, float scale, int32_t* tokens, float* scores, int32_t* predicted, int32_t B, int32_t T,
                                   int32_t V, int32_t step, int32_t max_step, int32_t unk, int32_t pad, void* stream) {
  DN_CHECK_ARG(logits2 && tokens && scores && predicted && B > 0 && T > 0 && T <= 2048 && V > 1 && max_step > 0 && step >= 0,
               "dn_cmlm_guided_step: bad args (T=%d must be <= 2048)", T);
  DN_CHECK_ARG(scale > 0.f, "dn_cmlm_guided_step: guidance scale %g must be > 0 (nat_gen.py:180: without it the loop runs dn_cmlm_step on one pass)", (double)scale);
  const int remask = (step + 1) < max_step;
  const float p = (float)(1.0 - (double)(step + 1) / (double)max_step);
  hipLaunchKernelGGL(cmlm_step_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, logits2, scale, tokens, scores, predicted, T, V, p, remask, unk,
                     pad, (const int32_t*)nullptr, max_step);
  DN_CHECK_LAUNCH("dn_cmlm_guided_step");
  return DN_OK;
}

extern "C" int dn_cmlm_guided_step_dev(const float* logits2, float scale, int32_t* tokens, float* scores, int32_t* predicted, int32_t B, int32_t T,
                                       int32_t V, const int32_t* step_dev, int32_t max_step, int32_t unk, int32_t pad, void* stream) {
  DN_CHECK_ARG(logits2 && tokens && scores && predicted && step_dev && B > 0 && T > 0 && T <= 2048 && V > 1 && max_step > 0,
               "dn_cmlm_guided_step_dev: bad args (T=%d must be <= 2048)", T);
  DN_CHECK_ARG(scale > 0.f, "dn_cmlm_guided_step_dev: guidance scale %g must be > 0", (double)scale);
  hipLaunchKernelGGL(cmlm_step_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, logits2, scale, tokens, scores, predicted, T, V, 0.f, 0, unk,
                     pad, step_dev, max_step);
  DN_CHECK_LAUNCH("dn_cmlm_guided_step_dev");
  return DN_OK;
}
