// K17: audio STFT (+ noise) -- replaces AV_Dataset.stft / gen_stft_example / add_noise
// (reference av_dataset.py:157-174, 217-220, 335-342).
//
// One wavefront per PAIR of consecutive frames of the launch's frame list (a pair may straddle two clips), on a grid-stride list of pairs:
// reflect-padded framing + (pre-scaled) periodic Hamming window are applied while the two frames are loaded into LDS as one complex frame,
// a radix-8 / radix-4 Stockham FFT runs in LDS with its butterflies in registers (twiddles from an LDS table), and the two one-sided
// spectra are separated and written straight into the [B, 2, T_a, F] (re/im plane, frame, bin) layout the model consumes, together with the
// noisy copy x = y + sigma * N(0,1) and each clip's max|y|.  4*L bytes in, 2 * 2*T_a*F*4 bytes out per clip.
// Framing, transform, split and noise counters are stft_fft.h's, shared with mix.hip; why they are built this way is told there.
#include "common.h"
#include "stft_fft.h"

// The last bin's noise: a wave evaluates block stft_ctr_last for its next 64 pairs in one call (lane k = the pair of iteration k) and hands the values out by
// v_readlane -- round 4: as a third pass of the bin loop the one extra bin cost a whole wave-wide Philox call per frame, a third of the kernel's generator work.
template <int NFFT, int STFT_FPB>
__global__ __launch_bounds__(64 * STFT_FPB) void stft_kernel(
    const float* __restrict__ audio, int64_t audio_stride, int length, const float* __restrict__ window, int hop,
    int n_frames, int n_bins_out, int total_frames, float* __restrict__ y, float* __restrict__ x,
    const float* __restrict__ noise, float sigma, uint64_t seed, float* __restrict__ clip_absmax) {
  __shared__ float2 buf[STFT_NBUF<NFFT>][STFT_FPB][NFFT];
  __shared__ float2 tw[NFFT];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  stft_twiddles<NFFT>(tw);
  const int64_t plane = (int64_t)n_frames * n_bins_out;
  const int npairs = (total_frames + 1) / 2;
  const int n_low = n_bins_out < NFFT / 2 ? n_bins_out : NFFT / 2;      // bins served by the paired blocks
  const bool last_bin = n_bins_out > NFFT / 2;
  const bool gen_last = last_bin && x != nullptr && noise == nullptr;
  const int pid_step = gridDim.x * STFT_FPB;
  float nyq[4] = {0.f, 0.f, 0.f, 0.f};
  int it = 0;
  for (int pid = blockIdx.x * STFT_FPB + wv; pid < npairs; pid += pid_step, ++it) {
    if (gen_last && (it & 63) == 0) {
      const int64_t pk = (int64_t)pid + (int64_t)lane * pid_step;       // the pair of iteration it + lane
      philox_normal4(seed, stft_ctr_last(2 * pk), nyq);
    }
    const int fid0 = 2 * pid, fid1 = fid0 + 1;
    const bool two_frames = fid1 < total_frames;
    const int b0 = fid0 / n_frames, t0 = fid0 % n_frames;
    const int b1 = two_frames ? fid1 / n_frames : b0, t1 = two_frames ? fid1 % n_frames : t0;
    const float* a0 = audio + (int64_t)b0 * audio_stride;
    const float* a1 = audio + (int64_t)b1 * audio_stride;
    stft_load_pair<NFFT>(&buf[0][wv][0], window, lane, t0, t1, hop, length, two_frames, [&](int j) { return a0[j]; }, [&](int j) { return a1[j]; });
    STFT_WAVE_SYNC();
    const int cur = fft_forward<NFFT>(&buf[0][wv][0], &buf[STFT_NBUF<NFFT> - 1][wv][0], tw, lane);
    // ---- separate the two spectra and write them (+ the noisy copies); `fr` = 0 / 1 selects the frame of the pair
#pragma unroll
    for (int fr = 0; fr < 2; ++fr) {
      if (fr == 1 && !two_frames) break;
      const int fid = fr ? fid1 : fid0, b = fr ? b1 : b0, t = fr ? t1 : t0;
      const int64_t row = ((int64_t)b * 2) * plane + (int64_t)t * n_bins_out;
      float* yre = y + row;
      float* yim = yre + plane;
      float amax = 0.f;
      auto bin = [&](int f) __attribute__((always_inline)) { return stft_split<NFFT>(&buf[cur][wv][0], f, fr); };
      // bins in pairs (f, f + 64): one Philox block = four normals = the noise of both
      for (int f0 = lane, jp = 0; f0 < n_low; f0 += 128, ++jp) {
        const int f1 = f0 + 64;
        const bool two = f1 < n_low;
        const float2 v0 = bin(f0), v1 = two ? bin(f1) : make_float2(0.f, 0.f);
        yre[f0] = v0.x;
        yim[f0] = v0.y;
        if (two) { yre[f1] = v1.x; yim[f1] = v1.y; }
        amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v0.x), fabsf(v0.y)), fmaxf(fabsf(v1.x), fabsf(v1.y))));
        if (x != nullptr) {
          const int64_t o0 = row + f0;
          float g[4];
          if (noise != nullptr) stft_noise_given(g, noise, o0, plane, two);
          else philox_normal4(seed, stft_ctr_pair(fid, jp, lane), g);
          x[o0] = stft_add_noise(v0.x, sigma, g[0]);
          x[o0 + plane] = stft_add_noise(v0.y, sigma, g[1]);
          if (two) {
            x[o0 + 64] = stft_add_noise(v1.x, sigma, g[2]);
            x[o0 + 64 + plane] = stft_add_noise(v1.y, sigma, g[3]);
          }
        }
      }
      if (last_bin) {
        // the values of this pair sit in lane (it & 63) of the block evaluated above
        const float gre = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nyq[2 * fr]), it & 63));
        const float gim = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nyq[2 * fr + 1]), it & 63));
        if (lane == 0) {
          const float2 v = bin(NFFT / 2);
          const int64_t o = row + NFFT / 2;
          yre[NFFT / 2] = v.x;
          yim[NFFT / 2] = v.y;
          amax = fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y)));
          if (x != nullptr) {
            x[o] = stft_add_noise(v.x, sigma, noise != nullptr ? noise[o] : gre);
            x[o + plane] = stft_add_noise(v.y, sigma, noise != nullptr ? noise[o + plane] : gim);
          }
        }
      }
      if (clip_absmax != nullptr) {
        amax = wave_max(amax);
        if (lane == 0) atomicMax((unsigned int*)(clip_absmax + b), __float_as_uint(amax));  // amax >= 0
      }
    }
    STFT_WAVE_SYNC();      // the next pair overwrites buf[0][wv]
  }
}

// normalize_output_fft path (av_dataset.py:339-341): y *= 1/(max|y| + 1e-7) per clip, then x = y + sigma*N.
__global__ void stft_normalise_kernel(float* __restrict__ y, float* __restrict__ x, const float* __restrict__ noise,
                                      const float* __restrict__ clip_absmax, int64_t per_clip, int64_t total,
                                      int n_frames, int n_bins_out, float sigma, uint64_t seed) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per_clip;
    const float s = 1.0f / (clip_absmax[b] + 1e-7f);
    const float v = y[i] * s;
    y[i] = v;
    if (x != nullptr) {
      float nz;
      if (noise != nullptr) {
        nz = noise[i];
      } else {
        const int64_t r = i - b * per_clip;
        const int64_t plane = (int64_t)n_frames * n_bins_out;
        const int pl = (int)(r / plane);
        const int64_t tf = r - pl * plane;  // t * n_bins + f: the clip's first frame below, the counter is linear in both
        float g[4];
        philox_normal4(seed, stft_ctr_bin(b * n_frames, n_bins_out, tf), g);
        nz = g[pl];
      }
      x[i] = stft_add_noise(v, sigma, nz);
    }
  }
}

extern "C" int maavss_stft_fwd(const float* audio, int64_t batch, int64_t length, int64_t audio_stride,
                               const float* window, int n_fft, int hop, int n_frames, int n_bins_out, float* y,
                               float* x, const float* noise, float sigma, uint64_t seed, float* clip_absmax,
                               void* stream) {
  MAAVSS_CHECK_ARG(audio && window && y, "stft: null pointer");
  MAAVSS_CHECK_ARG(batch > 0, "stft: empty problem");
  if (int rc = stft_check_frames("stft", n_fft, hop, n_frames, n_bins_out, length)) return rc;
  const int total = (int)(batch * n_frames);
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(N, FPB)                                                                                                                 \
  hipLaunchKernelGGL((stft_kernel<N, FPB>), dim3(stft_pair_grid(cdiv(total, 2), FPB)), dim3(64 * FPB), 0, st, audio, audio_stride, \
                     (int)length, window, hop, n_frames, n_bins_out, total, y, x, noise, sigma, seed, clip_absmax)
  STFT_DISPATCH(n_fft, LAUNCH);
#undef LAUNCH
  MAAVSS_LAUNCH_CHECK("stft_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_stft_normalise(float* y, float* x, const float* noise, const float* clip_absmax, int64_t batch,
                                     int n_frames, int n_bins_out, float sigma, uint64_t seed, void* stream) {
  MAAVSS_CHECK_ARG(y && clip_absmax, "stft_normalise: null pointer");
  const int64_t per_clip = 2LL * n_frames * n_bins_out, total = per_clip * batch;
  int grid = cdiv(total, 256);
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(stft_normalise_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, y, x, noise, clip_absmax,
                     per_clip, total, n_frames, n_bins_out, sigma, seed);
  MAAVSS_LAUNCH_CHECK("stft_normalise_kernel");
  return MAAVSS_OK;
}

// ---- inverse STFT (AV_Dataset.istft, av_dataset.py:181-201: torch.istft(n_fft, hop, win_length = n_fft, window,
// normalized, onesided, center)) -- the audio side of SURVEY.md 8 row f2 (mask / autoencoder output -> waveform).
// Pass 1, one wavefront per frame: the one-sided bins of the [B,2,T,F] tensor are mirrored into the Hermitian
// spectrum in LDS (imaginary parts of DC and Nyquist dropped as irfft does; a trimmed Nyquist bin reads as zero, the
// reference pads it), the same Stockham FFT runs with conjugated twiddles, and the real part, scaled by
// (normalized ? sqrt(N) : 1) / N and multiplied by the synthesis window, goes to frames[B][T][N].
// Pass 2, one thread per output sample: overlap-add of the <= ceil(N / hop) frames that cover it, divided by the
// window-square envelope, with the N/2 samples of centre padding cut off (length hop * (T - 1)).
template <int NFFT, int FPB>
__global__ __launch_bounds__(64 * FPB) void istft_frames_kernel(const float* __restrict__ spec, const float* __restrict__ window,
                                                                int n_frames, int n_bins_in, int total_frames, float scale,
                                                                float* __restrict__ frames) {
  constexpr int LOG2N = NFFT == 256 ? 8 : (NFFT == 512 ? 9 : 10);
  __shared__ float2 buf[2][FPB][NFFT];
  __shared__ float2 tw[NFFT / 2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int q = threadIdx.x; q < NFFT / 2; q += blockDim.x) {
    float s, c;
    sincospif(2.0f * (float)q / (float)NFFT, &s, &c);   // conjugate twiddles: inverse transform
    tw[q] = make_float2(c, s);
  }
  const int fid = blockIdx.x * FPB + wv;
  const bool active = fid < total_frames;
  const int b = active ? fid / n_frames : 0, t = active ? fid % n_frames : 0;
  const int64_t plane = (int64_t)n_frames * n_bins_in;
  const float* re = spec + ((int64_t)b * 2) * plane + (int64_t)t * n_bins_in;
  const float* im = re + plane;
  for (int k = lane; k <= NFFT / 2; k += 64) {
    float2 v = make_float2(0.f, 0.f);
    if (active && k < n_bins_in) v = make_float2(re[k], (k == 0 || k == NFFT / 2) ? 0.f : im[k]);
    buf[0][wv][k] = v;
    if (k > 0 && k < NFFT / 2) buf[0][wv][NFFT - k] = make_float2(v.x, -v.y);
  }
  __syncthreads();
  int cur = 0;
#pragma unroll
  for (int s = 0; s < LOG2N; ++s) {
    const int p = 1 << s;
    for (int i = lane; i < NFFT / 2; i += 64) {
      const int k = i & (p - 1);
      float2 u0 = buf[cur][wv][i];
      float2 u1 = buf[cur][wv][i + NFFT / 2];
      float2 w = tw[k * (NFFT / (2 * p))];
      float2 v = make_float2(u1.x * w.x - u1.y * w.y, u1.x * w.y + u1.y * w.x);
      const int j = ((i - k) << 1) + k;
      buf[cur ^ 1][wv][j] = make_float2(u0.x + v.x, u0.y + v.y);
      buf[cur ^ 1][wv][j + p] = make_float2(u0.x - v.x, u0.y - v.y);
    }
    __syncthreads();
    cur ^= 1;
  }
  if (!active) return;
  float* out = frames + (int64_t)fid * NFFT;
  for (int n = lane; n < NFFT; n += 64) out[n] = buf[cur][wv][n].x * scale * window[n];
}

__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ window,
                                                        int n_fft, int hop, int n_frames, int out_len, int64_t out_stride,
                                                        int64_t total, float* __restrict__ audio) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / out_len), n = (int)(i % out_len);
    const int pos = n + n_fft / 2;                       // position in the centre-padded signal
    int t_hi = pos / hop;
    if (t_hi > n_frames - 1) t_hi = n_frames - 1;
    int t_lo = (pos - n_fft + hop) / hop;                // smallest t with t*hop + n_fft > pos
    if (pos - n_fft + 1 <= 0) t_lo = 0;
    float num = 0.f, den = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
      const int j = pos - t * hop;
      if (j < 0 || j >= n_fft) continue;
      num += frames[((int64_t)b * n_frames + t) * n_fft + j];
      den += window[j] * window[j];
    }
    audio[(int64_t)b * out_stride + n] = num / den;
  }
}

extern "C" int maavss_istft(const float* spec, int64_t batch, int n_frames, int n_bins_in, const float* window, int n_fft,
                            int hop, int normalized, float* frames_ws, float* audio, int64_t audio_stride, void* stream) {
  STFT_CHECK_N_FFT("istft", n_fft);
  MAAVSS_CHECK_ARG(spec && window && frames_ws && audio, "istft: null pointer");
  MAAVSS_CHECK_ARG(batch > 0 && hop > 0 && n_frames > 1, "istft: needs at least two frames");
  MAAVSS_CHECK_ARG(n_bins_in == n_fft / 2 || n_bins_in == n_fft / 2 + 1, "istft: n_bins must be n_fft/2 (trimmed) or n_fft/2+1");
  MAAVSS_CHECK_ARG(hop <= n_fft, "istft: hop larger than the window leaves gaps (window envelope would be zero)");
  const int out_len = hop * (n_frames - 1);
  MAAVSS_CHECK_ARG(audio_stride >= out_len, "istft: audio_stride smaller than hop*(n_frames-1)");
  MAAVSS_CHECK_ARG((int64_t)(n_frames - 1) * hop + n_fft >= out_len + n_fft / 2, "istft: frames do not cover the output");
  const int total = (int)(batch * n_frames);
  const float scale = (normalized ? sqrtf((float)n_fft) : 1.f) / (float)n_fft;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH(N, FPB)                                                                                                   \
  hipLaunchKernelGGL((istft_frames_kernel<N, FPB>), dim3(cdiv(total, FPB)), dim3(64 * FPB), 0, st, spec, window, n_frames, \
                     n_bins_in, total, scale, frames_ws)
  STFT_DISPATCH(n_fft, LAUNCH);
#undef LAUNCH
  MAAVSS_LAUNCH_CHECK("istft_frames_kernel");
  const int64_t n_out = batch * out_len;
  int grid = cdiv(n_out, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(istft_ola_kernel, dim3(grid), dim3(256), 0, st, frames_ws, window, n_fft, hop, n_frames, out_len, audio_stride,
                     n_out, audio);
  MAAVSS_LAUNCH_CHECK("istft_ola_kernel");
  return MAAVSS_OK;
}
