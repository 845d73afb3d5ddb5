// Mixer: mix-and-separate training examples at a chosen signal-to-interferer ratio -- extends AV_Dataset.add_noise /
// gen_stft_example (reference av_dataset.py:217-220, 335-342), whose only corruption is white noise on the STFT coefficients.
//
//   s_b[n] = sum_k pool[partners[b][k]][n]        (slots with -1 are empty; f32, summed in k order, everywhere it is formed)
//   g_b    = snr_factor_b * sqrt(sum_n audio_b[n]^2 / sum_n s_b[n]^2),   snr_factor_b = 10^(-snr_db_b / 20) from the host;
//            g_b = 0 when the clip has no partner or either sum is 0     (the 1/L of the two mean powers cancels)
//            and when the quotient or the product leaves float's range (a near-silent interferer): never inf or NaN
//   x      = y + (g_b c_b) STFT(s_b) + sigma noise,   y = what maavss_stft_fwd [+ maavss_stft_normalise] wrote, READ here
//   mix_b  = audio_b + g_b s_b
//
// Three kernels: (1) one workgroup per clip reduces the two sums of squares in a fixed order and writes g_b; (2) the STFT of s_b with
// the framing, window, Stockham passes and two-frames-per-FFT packing of stft.hip (stft_fft.h), the gather-sum done while the frame
// is loaded and the mix done in the epilogue; (3) the mixture waveform.  The clean spectrum never shares an FFT with an interferer:
// y stays bit for bit the plain call's, and the interferer's rounding noise never reaches it.
#include "common.h"
#include "stft_fft.h"

#define MIX_MAX_K 4
#define MIX_THREADS 256

// the pool rows of clip b's partners, in slot order; empty (-1) and out-of-range entries -> null.  Uniform over the workgroup / wave.
__device__ __forceinline__ bool mix_rows(const float* __restrict__ pool, int64_t pool_stride, int n_pool, const int* __restrict__ partners,
                                         int k_slots, int64_t b, const float* (&rows)[MIX_MAX_K]) {
  bool any = false;
#pragma unroll
  for (int k = 0; k < MIX_MAX_K; ++k) {
    const int p = k < k_slots ? partners[b * k_slots + k] : -1;
    const bool ok = p >= 0 && p < n_pool;
    rows[k] = ok ? pool + (int64_t)p * pool_stride : nullptr;
    any |= ok;
  }
  return any;
}
__device__ __forceinline__ float mix_gather(const float* const (&rows)[MIX_MAX_K], int n) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MIX_MAX_K; ++k)
    if (rows[k] != nullptr) s += rows[k][n];
  return s;
}

// (1) thread i accumulates samples i, i + 256, ... (ceil(L / 256) sequential fused multiply-adds, one rounding each), then a binary tree
// over the 256 partials in LDS: no atomics, the order is fixed by L alone, so g_b does not depend on the launch it is part of.
__global__ __launch_bounds__(MIX_THREADS) void mix_gains_kernel(const float* __restrict__ audio, int64_t audio_stride,
                                                                const float* __restrict__ pool, int64_t pool_stride, int n_pool,
                                                                const int* __restrict__ partners, int k_slots, int length,
                                                                const float* __restrict__ snr_factor, float* __restrict__ gain) {
  __shared__ float red[2][MIX_THREADS];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* rows[MIX_MAX_K];
  const bool any = mix_rows(pool, pool_stride, n_pool, partners, k_slots, b, rows);
  const float* a = audio + b * audio_stride;
  float sc = 0.f, si = 0.f;
  for (int n = tid; n < length; n += MIX_THREADS) {
    const float v = a[n], s = mix_gather(rows, n);
    sc = fmaf(v, v, sc);
    si = fmaf(s, s, si);
  }
  red[0][tid] = sc;
  red[1][tid] = si;
  __syncthreads();
  for (int w = MIX_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float pc = red[0][0], pi = red[1][0];
    // a near-silent interferer (pi tiny or denormal) can push pc / pi or the product past float's range: such a clip stays unmixed
    // (g = 0) rather than carry inf into x and the mixture
    const float g = (any && pc > 0.f && pi > 0.f) ? snr_factor[b] * sqrtf(pc / pi) : 0.f;
    gain[b] = isfinite(g) ? g : 0.f;
  }
}

// (3) mixture[b][n] = audio[b][n] + g_b s_b[n]; one workgroup per 1024 samples of a clip
__global__ __launch_bounds__(MIX_THREADS) void mix_wave_kernel(const float* __restrict__ audio, int64_t audio_stride,
                                                               const float* __restrict__ pool, int64_t pool_stride, int n_pool,
                                                               const int* __restrict__ partners, int k_slots, int length, int chunks,
                                                               const float* __restrict__ gain, float* __restrict__ mixture,
                                                               int64_t mixture_stride) {
  const int64_t b = blockIdx.x / chunks;
  const int n0 = (blockIdx.x % chunks) * (4 * MIX_THREADS) + threadIdx.x;
  const float* rows[MIX_MAX_K];
  mix_rows(pool, pool_stride, n_pool, partners, k_slots, b, rows);
  const float g = gain[b];
  const float* a = audio + b * audio_stride;
  float* m = mixture + b * mixture_stride;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int n = n0 + u * MIX_THREADS;
    if (n < length) m[n] = g != 0.f ? fmaf(g, mix_gather(rows, n), a[n]) : a[n];
  }
}

// (2) one wavefront per PAIR of frames of one clip (frames 2p and 2p + 1; the last pair of an odd frame count is half empty): unlike
// stft_kernel no pair crosses a clip, so both frames share g_b, c_b and the partner rows, and a clip's result does not depend on its
// neighbours in the launch.  A clip with g_b c_b = 0 skips the transform and copies y.
// x0 = y + (g c) I, x = x0 + sigma * noise; sigma = 0 writes x0 itself, so x(sigma) - x(0) is the noise term to one rounding.
// Noise counters (stft_fft.h), fid = b * n_frames + t: clip_absmax == null -> those of stft_kernel, the last bin's taken per frame (block
// stft_ctr_last of the launch's even frame, normals 2 (fid & 1) and 2 (fid & 1) + 1); clip_absmax != null -> those of stft_normalise_kernel.
template <int NFFT, int FPB>
__global__ __launch_bounds__(64 * FPB) void stft_mix_kernel(
    const float* __restrict__ pool, int64_t pool_stride, int n_pool, const int* __restrict__ partners, int k_slots, int length,
    const float* __restrict__ window, int hop, int n_frames, int n_bins_out, int batch, const float* __restrict__ y, float* __restrict__ x,
    const float* __restrict__ noise, float sigma, uint64_t seed, const float* __restrict__ gain, const float* __restrict__ clip_absmax) {
  __shared__ float2 buf[STFT_NBUF<NFFT>][FPB][NFFT];
  __shared__ float2 tw[NFFT];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  stft_twiddles<NFFT>(tw);
  const int64_t plane = (int64_t)n_frames * n_bins_out;
  const int ppc = (n_frames + 1) / 2;                                   // pairs per clip
  const int npairs = batch * ppc;
  const int n_low = n_bins_out < NFFT / 2 ? n_bins_out : NFFT / 2;
  const bool last_bin = n_bins_out > NFFT / 2;
  const bool normalised = clip_absmax != nullptr;
  const bool gen = noise == nullptr && sigma != 0.f;
  const bool add_noise = sigma != 0.f;
  for (int pid = blockIdx.x * FPB + wv; pid < npairs; pid += gridDim.x * FPB) {
    const int b = pid / ppc, t0 = 2 * (pid - b * ppc), t1 = t0 + 1;
    const bool two_frames = t1 < n_frames;
    const float gc = gain[b] * (normalised ? 1.0f / (clip_absmax[b] + 1e-7f) : 1.0f);
    const bool mix = gc != 0.f && isfinite(gc);                          // g c past float's range (both clips near-silent): x = y
    int cur = 0;
    if (mix) {
      const float* rows[MIX_MAX_K];
      mix_rows(pool, pool_stride, n_pool, partners, k_slots, b, rows);
      auto sample = [&](int j) { return mix_gather(rows, j); };
      stft_load_pair<NFFT>(&buf[0][wv][0], window, lane, t0, t1, hop, length, two_frames, sample, sample);
      STFT_WAVE_SYNC();
      cur = fft_forward<NFFT>(&buf[0][wv][0], &buf[STFT_NBUF<NFFT> - 1][wv][0], tw, lane);
    }
#pragma unroll
    for (int fr = 0; fr < 2; ++fr) {
      if (fr == 1 && !two_frames) break;
      const int t = fr ? t1 : t0;
      const int64_t fid = (int64_t)b * n_frames + t;
      const int64_t row = ((int64_t)b * 2) * plane + (int64_t)t * n_bins_out;
      auto bin = [&](int f) __attribute__((always_inline)) { return mix ? stft_split<NFFT>(&buf[cur][wv][0], f, fr) : make_float2(0.f, 0.f); };
      auto put = [&](int64_t o, float2 v, float nre, float nim) __attribute__((always_inline)) {
        const float yre = y[o], yim = y[o + plane];
        const float re = mix ? yre + gc * v.x : yre, im = mix ? yim + gc * v.y : yim;
        x[o] = add_noise ? stft_add_noise(re, sigma, nre) : re;
        x[o + plane] = add_noise ? stft_add_noise(im, sigma, nim) : im;
      };
      for (int f0 = lane, jp = 0; f0 < n_low; f0 += 128, ++jp) {
        const int f1 = f0 + 64;
        const bool two = f1 < n_low;
        const int64_t o0 = row + f0;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (noise != nullptr) {
          stft_noise_given(g, noise, o0, plane, two);
        } else if (gen && !normalised) {
          philox_normal4(seed, stft_ctr_pair(fid, jp, lane), g);
        } else if (gen) {
          stft_noise_bin(g[0], g[1], seed, stft_ctr_bin(fid, n_bins_out, f0));
          if (two) stft_noise_bin(g[2], g[3], seed, stft_ctr_bin(fid, n_bins_out, f1));
        }
        put(o0, bin(f0), g[0], g[1]);
        if (two) put(o0 + 64, bin(f1), g[2], g[3]);
      }
      if (last_bin && lane == 0) {
        const int64_t o = row + NFFT / 2;
        float nre = 0.f, nim = 0.f;
        if (noise != nullptr) {
          nre = noise[o];
          nim = noise[o + plane];
        } else if (gen && !normalised) {
          float h[4];
          philox_normal4(seed, stft_ctr_last(fid & ~(int64_t)1), h);
          nre = (fid & 1) ? h[2] : h[0];
          nim = (fid & 1) ? h[3] : h[1];
        } else if (gen) {
          stft_noise_bin(nre, nim, seed, stft_ctr_bin(fid, n_bins_out, NFFT / 2));
        }
        put(o, bin(NFFT / 2), nre, nim);
      }
    }
    STFT_WAVE_SYNC();      // the next pair overwrites buf[0][wv]
  }
}

static int mix_check_common(const char* who, const void* pool, int64_t pool_stride, int64_t n_pool, const void* partners, int k_slots,
                            int64_t batch, int64_t length) {
  MAAVSS_CHECK_ARG(pool && partners, "%s: null pointer", who);
  MAAVSS_CHECK_ARG(k_slots >= 1 && k_slots <= MIX_MAX_K, "%s: 1 to %d partner slots (got %d)", who, MIX_MAX_K, k_slots);
  MAAVSS_CHECK_ARG(batch > 0 && batch < (1 << 20) && length > 0 && length < (1 << 30), "%s: batch must be in [1, 2^20) and length in [1, 2^30)", who);
  MAAVSS_CHECK_ARG(n_pool > 0 && n_pool <= INT32_MAX, "%s: empty pool", who);
  MAAVSS_CHECK_ARG(pool_stride >= 0, "%s: negative pool_stride", who);
  return MAAVSS_OK;
}

// do the element ranges [a, a + a_n) and [b, b + b_n) share a float?
static bool mix_overlap(const float* a, int64_t a_n, const float* b, int64_t b_n) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uint64_t)b_n * sizeof(float) && b0 < a0 + (uint64_t)a_n * sizeof(float);
}
static int64_t mix_extent(int64_t rows, int64_t stride, int64_t length) { return (rows - 1) * stride + length; }

extern "C" int maavss_mix_gains(const float* audio, int64_t batch, int64_t length, int64_t audio_stride, const float* pool,
                                int64_t n_pool, int64_t pool_stride, const int* partners, int k_slots, const float* snr_factor,
                                float* gain, void* stream) {
  if (int rc = mix_check_common("mix_gains", pool, pool_stride, n_pool, partners, k_slots, batch, length)) return rc;
  MAAVSS_CHECK_ARG(audio && snr_factor && gain, "mix_gains: null pointer");
  MAAVSS_CHECK_ARG(audio_stride >= 0, "mix_gains: negative audio_stride");
  hipLaunchKernelGGL(mix_gains_kernel, dim3((unsigned)batch), dim3(MIX_THREADS), 0, (hipStream_t)stream, audio, audio_stride, pool,
                     pool_stride, (int)n_pool, partners, k_slots, (int)length, snr_factor, gain);
  MAAVSS_LAUNCH_CHECK("mix_gains_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_mix_wave(const float* audio, int64_t batch, int64_t length, int64_t audio_stride, const float* pool,
                               int64_t n_pool, int64_t pool_stride, const int* partners, int k_slots, const float* gain,
                               float* mixture, int64_t mixture_stride, void* stream) {
  if (int rc = mix_check_common("mix_wave", pool, pool_stride, n_pool, partners, k_slots, batch, length)) return rc;
  MAAVSS_CHECK_ARG(audio && gain && mixture, "mix_wave: null pointer");
  MAAVSS_CHECK_ARG(audio_stride >= 0, "mix_wave: negative audio_stride");
  MAAVSS_CHECK_ARG(mixture_stride >= length || batch == 1, "mix_wave: mixture_stride smaller than length (rows would overlap)");
  MAAVSS_CHECK_ARG(!mix_overlap(mixture, mix_extent(batch, mixture_stride, length), audio, mix_extent(batch, audio_stride, length)) &&
                       !mix_overlap(mixture, mix_extent(batch, mixture_stride, length), pool, mix_extent(n_pool, pool_stride, length)),
                   "mix_wave: mixture overlaps audio or pool (other workgroups still read those rows)");
  const int chunks = cdiv(length, 4 * MIX_THREADS);
  MAAVSS_CHECK_ARG(batch * chunks <= INT32_MAX, "mix_wave: too many samples for one launch");
  hipLaunchKernelGGL(mix_wave_kernel, dim3((unsigned)(batch * chunks)), dim3(MIX_THREADS), 0, (hipStream_t)stream, audio, audio_stride,
                     pool, pool_stride, (int)n_pool, partners, k_slots, (int)length, chunks, gain, mixture, mixture_stride);
  MAAVSS_LAUNCH_CHECK("mix_wave_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_stft_mix_fwd(const float* pool, int64_t n_pool, int64_t length, int64_t pool_stride, const int* partners,
                                   int k_slots, int64_t batch, const float* window, int n_fft, int hop, int n_frames, int n_bins_out,
                                   const float* y, float* x, const float* noise, float sigma, uint64_t seed, const float* gain,
                                   const float* clip_absmax, void* stream) {
  if (int rc = mix_check_common("stft_mix", pool, pool_stride, n_pool, partners, k_slots, batch, length)) return rc;
  MAAVSS_CHECK_ARG(window && y && x && gain, "stft_mix: null pointer");
  if (int rc = stft_check_frames("stft_mix", n_fft, hop, n_frames, n_bins_out, length)) return rc;
  const int64_t spec = batch * 2 * n_frames * n_bins_out;
  MAAVSS_CHECK_ARG(!mix_overlap(x, spec, y, spec) && !mix_overlap(x, spec, pool, mix_extent(n_pool, pool_stride, length)) &&
                       (noise == nullptr || !mix_overlap(x, spec, noise, spec)),
                   "stft_mix: x overlaps y, noise or pool (they are read while x is written)");
  MAAVSS_CHECK_ARG(batch * ((int64_t)n_frames + 1) < INT32_MAX, "stft_mix: too many frames for one launch");
  const int npairs = (int)(batch * ((n_frames + 1) / 2));
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(N, FPB)                                                                                                                      \
  hipLaunchKernelGGL((stft_mix_kernel<N, FPB>), dim3(stft_pair_grid(npairs, FPB)), dim3(64 * FPB), 0, st, pool, pool_stride, (int)n_pool, \
                     partners, k_slots, (int)length, window, hop, n_frames, n_bins_out, (int)batch, y, x, noise, sigma, seed, gain,        \
                     clip_absmax)
  STFT_DISPATCH(n_fft, LAUNCH);
#undef LAUNCH
  MAAVSS_LAUNCH_CHECK("stft_mix_kernel");
  return MAAVSS_OK;
}
