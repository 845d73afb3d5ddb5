// The in-LDS forward FFT of the STFT kernels (stft.hip, mix.hip): one wavefront transforms N = 256 / 512 / 1024 complex points held in LDS
// with radix-8 / radix-4 Stockham passes whose butterflies live in registers.
#pragma once
#include "common.h"

#define STFT_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
// forward DFTs (kernel exp(-2 pi i r q / R)) of R points held in registers, in place
__device__ __forceinline__ void dft4(float2& a0, float2& a1, float2& a2, float2& a3) {
  const float2 s0 = cadd(a0, a2), d0 = csub(a0, a2), s1 = cadd(a1, a3), d1 = csub(a1, a3);
  a0 = cadd(s0, s1);
  a2 = csub(s0, s1);
  a1 = make_float2(d0.x + d1.y, d0.y - d1.x);      // d0 - i d1
  a3 = make_float2(d0.x - d1.y, d0.y + d1.x);      // d0 + i d1
}
template <int R>
__device__ __forceinline__ void dft_r(float2 (&a)[R]) {
  if constexpr (R == 4) {
    dft4(a[0], a[1], a[2], a[3]);
  } else {
    static_assert(R == 8, "radix 4 or 8");
    float2 e0 = a[0], e1 = a[2], e2 = a[4], e3 = a[6], o0 = a[1], o1 = a[3], o2 = a[5], o3 = a[7];
    dft4(e0, e1, e2, e3);
    dft4(o0, o1, o2, o3);
    constexpr float kS = 0.70710678118654752f;
    const float2 t1 = make_float2((o1.x + o1.y) * kS, (o1.y - o1.x) * kS);      // o1 (1 - i) / sqrt 2
    const float2 t2 = make_float2(o2.y, -o2.x);                                 // -i o2
    const float2 t3 = make_float2((o3.y - o3.x) * kS, -(o3.x + o3.y) * kS);     // o3 (-1 - i) / sqrt 2
    a[0] = cadd(e0, o0); a[4] = csub(e0, o0);
    a[1] = cadd(e1, t1); a[5] = csub(e1, t1);
    a[2] = cadd(e2, t2); a[6] = csub(e2, t2);
    a[3] = cadd(e3, t3); a[7] = csub(e3, t3);
  }
}
// One radix-R Stockham pass over N points (P = product of the radices of the earlier passes): butterfly i takes in[i + r N / R], multiplies by
// exp(-2 pi i r k / (R P)), k = i mod P, transforms, and writes out[(i - k) R + k + q P].  tw = the FULL table exp(-2 pi i q / N), q < N.
// When a pass is ONE butterfly per lane (N / R = 64) `out` may be `in`: the wave's reads are all issued before its first write and the LDS
// serves one wave's operations in issue order.
template <int N, int R, int P>
__device__ __forceinline__ void fft_pass(const float2* in, float2* out, const float2* __restrict__ tw, int lane) {
  constexpr int NB = N / R;
#pragma unroll
  for (int i0 = 0; i0 < NB; i0 += 64) {
    const int i = i0 + lane;
    if (NB < 64 && i >= NB) break;
    const int k = i & (P - 1);
    float2 a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = in[i + r * NB];
    if constexpr (P > 1) {
#pragma unroll
      for (int r = 1; r < R; ++r) a[r] = cmul(a[r], tw[r * k * (N / (R * P))]);
    }
    dft_r<R>(a);
    const int j = (i - k) * R + k;
#pragma unroll
    for (int q = 0; q < R; ++q) out[j + q * P] = a[q];
  }
}
// the whole transform.  512 and 256 points: every pass is one butterfly per lane -> IN PLACE in b0 (b1 unused: half the LDS, twice the
// workgroups per CU); 1024 points ping-pongs.  Returns the index (0 / 1) of the buffer that holds the result.
template <int N>
__device__ __forceinline__ int fft_forward(float2* b0, float2* b1, const float2* tw, int lane) {
  if constexpr (N == 512) {
    fft_pass<512, 8, 1>(b0, b0, tw, lane); STFT_WAVE_SYNC();
    fft_pass<512, 8, 8>(b0, b0, tw, lane); STFT_WAVE_SYNC();
    fft_pass<512, 8, 64>(b0, b0, tw, lane); STFT_WAVE_SYNC();
    return 0;
  } else if constexpr (N == 256) {
    fft_pass<256, 4, 1>(b0, b0, tw, lane); STFT_WAVE_SYNC();
    fft_pass<256, 4, 4>(b0, b0, tw, lane); STFT_WAVE_SYNC();
    fft_pass<256, 4, 16>(b0, b0, tw, lane); STFT_WAVE_SYNC();
    fft_pass<256, 4, 64>(b0, b0, tw, lane); STFT_WAVE_SYNC();
    return 0;
  } else {
    static_assert(N == 1024, "n_fft 256, 512 or 1024");
    fft_pass<1024, 8, 1>(b0, b1, tw, lane); STFT_WAVE_SYNC();
    fft_pass<1024, 8, 8>(b1, b0, tw, lane); STFT_WAVE_SYNC();
    fft_pass<1024, 4, 64>(b0, b1, tw, lane); STFT_WAVE_SYNC();
    fft_pass<1024, 4, 256>(b1, b0, tw, lane); STFT_WAVE_SYNC();
    return 0;
  }
}
