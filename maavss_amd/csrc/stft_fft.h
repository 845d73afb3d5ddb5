// What stft_kernel (stft.hip) and stft_mix_kernel (mix.hip) share: the in-LDS forward FFT (one wavefront transforms N = 256 / 512 / 1024 complex
// points with radix-8 / radix-4 Stockham passes whose butterflies live in registers), the framing of two real frames into one complex frame, the
// split of their spectra, the noise of x, and on the host the frame refusals and the n_fft -> kernel ladder.
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

// Round 3: (1) the waves of a workgroup are independent, so the FFT stages are ordered by the wave's own LDS queue (LDS operations of
// one wave complete in issue order) and a compiler-level wave barrier (STFT_WAVE_SYNC) instead of ten workgroup barriers per frame; (2) a
// workgroup builds its twiddle table once and walks a grid-stride list of frame PAIRS; (3) two real frames share one complex FFT
// (z = a + i b, A[k] = (Z[k] + conj Z[N-k]) / 2, B[k] = (Z[k] - conj Z[N-k]) / 2i): half the butterflies and LDS passes per frame; (4) one
// Philox block serves two bins (its four normals: re / im of bins f and f + 64) instead of one.  profiles/r3_stft_bench.json.
// Round 4: the Stockham FFT runs in radix-8 / radix-4 passes (512 = 8.8.8, 256 = 4.4.4.4, 1024 = 8.8.4.4) with the butterflies in registers:
// three LDS round trips per frame pair instead of nine, 69 LDS instructions per lane instead of 180, ~270 vector instructions instead of ~900
// (the kernel is bound by its vector work, not by HBM: DESIGN.md); Box-Muller takes its angle through v_sin_f32 / v_cos_f32, whose argument
// is in revolutions -- exactly the uniform deviate -- instead of sincospif's software range reduction.  profiles/r4_stft_bench.json.
template <int NFFT> constexpr int STFT_NBUF = NFFT == 1024 ? 2 : 1;     // LDS buffers per wave: 512 / 256 points transform in place
// tw[q] = exp(-2 pi i q / N) for q < N (the radix-8 / radix-4 passes index up to 7 k N / (8 P) < N); ends with the workgroup barrier
template <int NFFT>
__device__ __forceinline__ void stft_twiddles(float2* tw) {
  for (int q = threadIdx.x; q < NFFT; q += blockDim.x) {
    float s, c;
    sincospif(-2.0f * (float)q / (float)NFFT, &s, &c);
    tw[q] = make_float2(c, s);
  }
  __syncthreads();
}
// dst[n] = window[n] * (frame t0 of sample0, frame t1 of sample1), n < NFFT: frame t is centred on sample t * hop and reflected at both ends
// of its clip; sampleX(j) returns sample j of that clip.  Without a second frame the imaginary part is 0 and sample1 is not called.
__device__ __forceinline__ int stft_reflect(int j, int length) { j = j < 0 ? -j : j; return j >= length ? 2 * (length - 1) - j : j; }
template <int NFFT, class Sample0, class Sample1>
__device__ __forceinline__ void stft_load_pair(float2* dst, const float* __restrict__ window, int lane, int t0, int t1, int hop, int length,
                                               bool two_frames, Sample0 sample0, Sample1 sample1) {
  for (int n = lane; n < NFFT; n += 64) {
    const int j0 = stft_reflect(t0 * hop + n - NFFT / 2, length), j1 = stft_reflect(t1 * hop + n - NFFT / 2, length);
    const float wn = window[n];
    dst[n] = make_float2(sample0(j0) * wn, two_frames ? sample1(j1) * wn : 0.f);
  }
}
// bin f of frame `fr` (0 / 1) of the pair whose transform is z
template <int NFFT>
__device__ __forceinline__ float2 stft_split(const float2* z, int f, int fr) {
  const float2 a = z[f], b = z[(NFFT - f) & (NFFT - 1)];
  return fr == 0 ? make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y)) : make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
}

// ---- the noise of x.  Counter layout (a Philox4x32-10 block = four normals), frames numbered fid = b * n_frames + t:
// block stft_ctr_pair(fid, jp, lane) = re / im of bins f0 = lane + 128 jp and f0 + 64 of frame fid, for the bins below n_fft / 2; the LAST
// bin (n_fft / 2, present when n_bins_out = n_fft / 2 + 1) of both frames of the pair (fid0 even, fid0 + 1) takes block stft_ctr_last(fid0)
// = (re, im) of frame fid0, (re, im) of frame fid0 + 1: jp = 7, lane 0, which no paired bin uses (jp <= 3).  With normalize_output_fft the
// noise is added by (or as by) stft_normalise_kernel from one block per bin, stft_ctr_bin: normal 0 = re, 1 = im.
__device__ __forceinline__ uint64_t stft_ctr_pair(uint64_t fid, int jp, int lane) { return (fid * 8 + jp) * 64 + lane; }
__device__ __forceinline__ uint64_t stft_ctr_last(uint64_t fid0) { return (fid0 * 8 + 7) * 64; }
__device__ __forceinline__ uint64_t stft_ctr_bin(uint64_t fid, int n_bins_out, int64_t f) { return fid * n_bins_out + f; }
// g = the given noise of bins f0 (re, im) and f0 + 64 (re, im; 0 without it) of a frame, o0 = offset of its bin f0 in the re plane: what a
// block stft_ctr_pair holds when the noise is generated.  `noise` is NOT __restrict__ here (the kernels' own parameter is): with it stft_kernel<512, 4>
// took 6 % longer from B = 256 up (profiles/stft_shared_ab.txt)
__device__ __forceinline__ void stft_noise_given(float (&g)[4], const float* noise, int64_t o0, int64_t plane, bool two) {
  g[0] = noise[o0];
  g[1] = noise[o0 + plane];
  g[2] = two ? noise[o0 + 64] : 0.f;
  g[3] = two ? noise[o0 + 64 + plane] : 0.f;
}
// (re, im) = the noise of one bin on the per-bin layout
__device__ __forceinline__ void stft_noise_bin(float& re, float& im, uint64_t seed, uint64_t ctr) {
  float h[4];
  philox_normal4(seed, ctr, h);
  re = h[0], im = h[1];
}
// every x both kernels and stft_normalise_kernel write goes through this one expression, so that -ffp-contract contracts them alike: the
// mixer's x of a clip without a partner is the plain call's bit for bit (tests/test_mixer_gpu.py)
__device__ __forceinline__ float stft_add_noise(float v, float sigma, float g) { return v + sigma * g; }

// ---- host side
#define STFT_CHECK_N_FFT(who, n_fft) MAAVSS_CHECK_ARG(n_fft == 256 || n_fft == 512 || n_fft == 1024, "%s: n_fft must be 256, 512 or 1024 (got %d)", who, n_fft)
// the refusals of a frame grid, with the entry point's name in front
static inline int stft_check_frames(const char* who, int n_fft, int hop, int n_frames, int n_bins_out, int64_t length) {
  STFT_CHECK_N_FFT(who, n_fft);
  MAAVSS_CHECK_ARG(hop > 0 && n_frames > 0, "%s: empty problem", who);
  MAAVSS_CHECK_ARG(n_bins_out >= 1 && n_bins_out <= n_fft / 2 + 1, "%s: n_bins_out out of range", who);
  MAAVSS_CHECK_ARG(length > n_fft / 2, "%s: reflect padding needs length > n_fft/2", who);
  MAAVSS_CHECK_ARG((int64_t)(n_frames - 1) * hop + n_fft / 2 - 1 < 2 * length - 1, "%s: frames run past the reflected signal", who);
  return MAAVSS_OK;
}
// an admitted n_fft -> LAUNCH(N, FPB): the kernel instance and its wavefronts (frame pairs; frames for the inverse) per workgroup
#define STFT_DISPATCH(n_fft, LAUNCH) \
  do { if ((n_fft) == 256) LAUNCH(256, 4); else if ((n_fft) == 512) LAUNCH(512, 4); else LAUNCH(1024, 2); } while (0)
// grid-stride over the frame pairs: at most 8 workgroups per CU worth of blocks (the twiddle table is built once per workgroup)
static inline int stft_pair_grid(int npairs, int fpb) { return cdiv(npairs, fpb) < 2048 ? cdiv(npairs, fpb) : 2048; }
