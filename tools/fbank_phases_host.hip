// Steps the phases of fbank_frames_kernel (diffnorm_amd/csrc/fbank.hip) on the CPU, one thread at a time and one phase after the
// other, exactly as the workgroup barriers order them on the device: the same index arithmetic, table code and fp32 operations,
// checked by the host sanitizers.  No GPU is involved.  Every tile stages its samples from an exact-size copy of the utterance,
// so a read at or past the utterance's length is a heap overflow the sanitizer reports.
// Build: hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I diffnorm_amd/csrc
//        tools/fbank_phases_host.hip -o fbank_phases_host
// Usage: fbank_phases_host <sample_rate> <n_mels> <frame_length> <frame_shift> <n_fft> <wave.f32> <out.f32>
//        reads the utterance's samples as raw fp32 (int16 scale), writes the raw log-mel rows [frames][n_mels] as raw fp32.
#define DN_FB_PHASE __host__ __device__ inline
#include "fbank.hip"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

void dn_set_error(const char* fmt, ...) { (void)fmt; }  // capi.hip's, which is not linked here

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: %s sample_rate n_mels frame_length frame_shift n_fft wave.f32 out.f32\n", argv[0]);
    return 2;
  }
  DnFbankConfig c{};
  c.sample_rate = (float)atof(argv[1]); c.n_mels = atoi(argv[2]); c.frame_length = atoi(argv[3]); c.frame_shift = atoi(argv[4]); c.n_fft = atoi(argv[5]);
  c.low_freq = 20.f; c.high_freq = 0.f; c.preemphasis = 0.97f; c.remove_dc_offset = 1; c.input_scale = 1.f; c.cmvn = 0;
  FILE* f = fopen(argv[6], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const int n = (int)(ftell(f) / 4);
  fseek(f, 0, SEEK_SET);
  std::vector<float> wave(n);
  if (n && fread(wave.data(), 4, n, f) != (size_t)n) return 3;
  fclose(f);
  if (c.n_fft < 2 || c.n_fft > 4096 || c.frame_length < 1 || c.n_mels < 1 || c.n_mels > 4096) return 4;
  std::vector<float> win(c.frame_length), mel((size_t)c.n_mels * (c.n_fft / 2 + 1)), tw(c.n_fft);
  if (dn_fbank_tables(&c, win.data(), mel.data()) != DN_OK || dn_fbank_twiddles(c.n_fft, tw.data()) != DN_OK) return 4;
  const void* tabs[3] = {win.data(), mel.data(), tw.data()};
  DnFbank* m = nullptr;
  if (dn_fbank_create(&c, tabs, 3, &m) != DN_OK) return 4;
  const FbGeom g = m->g;
  const int Lf = dn_fbank_out_frames(m, n);
  std::vector<float> out((size_t)Lf * g.M, -1.f);
  std::unique_ptr<FbLds> l(new FbLds());
  for (int f0 = 0; f0 < Lf; f0 += g.F) {
    const int nrows = Lf - f0 < g.F ? Lf - f0 : g.F;
    const std::vector<float> own(wave.begin() + (size_t)f0 * g.S, wave.end());  // exactly the samples the utterance has from here on
    for (int t = 0; t < FB_NT; ++t) fb_stage(t, *l, g, own.data(), n - f0 * g.S, (const float2*)tw.data());
    for (int t = 0; t < FB_NT; ++t) fb_partial_sums(t, *l, g);
    for (int t = 0; t < FB_NT; ++t) fb_window(t, *l, g, win.data());
    float *src = l->a, *dst = l->b;
    for (int lgs = 0; lgs < g.lgH; ++lgs) {
      for (int t = 0; t < FB_NT; ++t) fb_butterflies(t, src, dst, *l, g, lgs);
      float* x = src; src = dst; dst = x;
    }
    for (int t = 0; t < FB_NT; ++t) fb_power(t, src, dst, *l, g);
    for (int t = 0; t < FB_NT; ++t) fb_mel(t, dst, g, mel.data(), m->r, out.data() + (size_t)f0 * g.M, nrows, nrows);
  }
  dn_fbank_destroy(m);
  f = fopen(argv[7], "wb");
  if (!f || (out.size() && fwrite(out.data(), 4, out.size(), f) != out.size())) return 5;
  fclose(f);
  printf("frames %d, %d per tile, %d threads per frame\n", Lf, g.F, g.T);
  return 0;
}
