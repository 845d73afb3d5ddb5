// Audio transform of the data path: AV_Dataset.audio_transforms (av_dataset.py:203-215) -- channel downmix, the optional `normalize`,
// torchaudio's sinc_interp_hann Resample and the optional contrast -- from the demuxer's PCM ([B][C][L0], f32 or int16) to the mono f32
// [B][L] clips the STFT reads.
//   pass 0 (audio_transform_absmax_kernel, normalize only): one block per clip, max |downmixed sample| into ws[b].  One block and no
//           atomics: nothing to zero first, and the maximum is order-independent anyway.
//   pass 1 (audio_transform_kernel): a block owns AT_RUN consecutive output samples of one clip.  Output n = j * new + p reads the S live
//           taps of phase p against x[j * orig - width + first_tap[p] + k]; first_tap grows with p by orig / new per phase, so the block's
//           outputs read one contiguous input span of about AT_RUN * orig / new + S samples.  The block loads that span ONCE, coalesced
//           (consecutive lanes, consecutive samples, per channel), downmixing, scaling int16 and applying the clip scale on the way into
//           LDS; samples outside [0, L0) are the zero padding.  Then every lane forms its output from LDS.  Taps are stored tap-major
//           ([S][new]) so that the lanes of a wave, consecutive phases, read one coalesced row per tap; the table is at most 16 MiB and
//           usually a few KiB, i.e. served from L2 / L1 after the first block (with new == 1 every lane reads the same tap).
//           orig == new is the pass-through: the downmixed sample itself, no LDS.  The contrast epilogue sits behind both.
// Traffic: the input once plus S / (AT_RUN * orig / new) of overlap between neighbouring blocks, and 4 * B * L bytes written.
// Every LDS offset is clamped into the staged span and every global index is tested against [0, L0): a malformed tap table gives wrong
// samples, never an access out of bounds.
#include <climits>

#include "common.h"

namespace {

constexpr int AT_RUN = 256;                 // output samples per block (one per thread)
constexpr int64_t AT_MAX_LDS = 64 * 1024;   // bytes of the staged input span

template <typename T>
__device__ __forceinline__ float at_sample(const T* p);
template <>
__device__ __forceinline__ float at_sample<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float at_sample<int16_t>(const int16_t* p) { return (float)*p * (1.0f / 32768.0f); }   // exact

// the reference's `audio /= C; audio.sum(dim=0)`: every channel divided first, then summed in channel order
template <typename T>
__device__ __forceinline__ float at_downmix(const T* __restrict__ clip, int64_t stride_c, int C, float fC, int64_t g) {
  float v = at_sample(clip + g);
  if (C == 1) return v;
  v = __fdiv_rn(v, fC);
  for (int c = 1; c < C; ++c) v += __fdiv_rn(at_sample(clip + c * stride_c + g), fC);
  return v;
}

// torchaudio.functional.contrast(x, 75): sin(x pi/2 + 0.1 sin(4 x pi/2)), with the library sinf
__device__ __forceinline__ float at_contrast(float x) {
  const float t = x * 1.57079632679489661923f;
  return sinf(t + 0.1f * sinf(t * 4.0f));
}

// input samples a block stages: the first taps of outputs n0 and n0 + AT_RUN - 1 lie at most ceil((AT_RUN - 1) orig / new) + 1 apart
// (first_tap[p] = floor(a + p orig / new) + 1 for one real a), plus the S taps of the last output and one sample of slack
inline int64_t at_span(int orig, int new_rate, int S) { return ((int64_t)(AT_RUN - 1) * orig + new_rate - 1) / new_rate + 2 + S; }

template <typename T>
__global__ __launch_bounds__(1024) void audio_transform_absmax_kernel(const T* __restrict__ src, int64_t stride_b, int64_t stride_c, int C,
                                                                      int64_t L0, float* __restrict__ scale) {
  const T* clip = src + blockIdx.x * stride_b;
  const float fC = (float)C;
  float m = 0.f;
  for (int64_t g = threadIdx.x; g < L0; g += 1024) m = fmaxf(m, fabsf(at_downmix(clip, stride_c, C, fC, g)));
  __shared__ float red[16][1];
  m = wg_reduce<WG_THREAD0, WG_MAX>(wave_max(m), red, threadIdx.x >> 6, threadIdx.x & 63);
  if (threadIdx.x == 0) scale[blockIdx.x] = m;
}

// grid (blocks_per_clip * B), block AT_RUN, dynamic LDS span * 4 bytes (RESAMPLE only)
template <typename T, bool RESAMPLE>
__global__ __launch_bounds__(AT_RUN) void audio_transform_kernel(const T* __restrict__ src, int64_t stride_b, int64_t stride_c, int C,
                                                                 int64_t L0, const float* __restrict__ taps,
                                                                 const int32_t* __restrict__ first_tap, int orig, int new_rate, int S,
                                                                 int width, int span, const float* __restrict__ scale, int contrast,
                                                                 float* __restrict__ out, int64_t L, int64_t ld_out, int blocks_per_clip) {
  extern __shared__ float xs[];
  const int64_t b = blockIdx.x / blocks_per_clip;
  const int64_t n0 = (int64_t)(blockIdx.x % blocks_per_clip) * AT_RUN;
  const int64_t n = n0 + threadIdx.x;
  const T* clip = src + b * stride_b;
  const float fC = (float)C;
  const float m = scale ? scale[b] : 1.0f;
  float v;
  if constexpr (!RESAMPLE) {
    if (n >= L) return;
    v = at_downmix(clip, stride_c, C, fC, n);            // L <= L0, checked by the host
    if (scale) v *= m;
  } else {
    const int64_t j0 = n0 / new_rate;
    const int64_t lo = j0 * orig - width + first_tap[n0 - j0 * new_rate];
    for (int e = threadIdx.x; e < span; e += AT_RUN) {
      const int64_t g = lo + e;
      float x = 0.f;                                     // the zero padding of both ends
      if (g >= 0 && g < L0) {
        x = at_downmix(clip, stride_c, C, fC, g);
        if (scale) x *= m;
      }
      xs[e] = x;
    }
    __syncthreads();
    if (n >= L) return;
    const int64_t j = n / new_rate;
    const int p = (int)(n - j * new_rate);
    const int64_t start = j * orig - width + first_tap[p];
    const int off = (int)min(max(start - lo, (int64_t)0), (int64_t)(span - S));
    const float* tp = taps + p;
    const float* xp = xs + off;
    v = 0.f;
    for (int k = 0; k < S; ++k) v = fmaf(tp[(int64_t)k * new_rate], xp[k], v);
  }
  if (contrast) v = at_contrast(v);
  out[b * ld_out + n] = v;
}

bool at_shape_ok(int64_t B, int C, int64_t L0) {
  return B > 0 && B <= INT_MAX && C >= 1 && C <= 1024 && L0 >= 1 && L0 <= ((int64_t)1 << 40);
}

template <typename T>
int at_launch(const T* src, int64_t B, int C, int64_t L0, int64_t stride_b, int64_t stride_c, const float* taps, const int32_t* first_tap,
              int orig, int new_rate, int S, int width, int normalize, int contrast, float* out, int64_t L, int64_t ld_out, float* scale,
              hipStream_t st) {
  if (normalize) {
    hipLaunchKernelGGL(audio_transform_absmax_kernel<T>, dim3((unsigned)B), dim3(1024), 0, st, src, stride_b, stride_c, C, L0, scale);
    MAAVSS_LAUNCH_CHECK("audio_transform_absmax_kernel");
  }
  const int bpc = cdiv(L, AT_RUN);
  const unsigned grid = (unsigned)(bpc * B);
  if (orig == new_rate) {
    hipLaunchKernelGGL((audio_transform_kernel<T, false>), dim3(grid), dim3(AT_RUN), 0, st, src, stride_b, stride_c, C, L0, taps, first_tap,
                       orig, new_rate, S, width, 0, (const float*)scale, contrast, out, L, ld_out, bpc);
  } else {
    const int span = (int)at_span(orig, new_rate, S);
    hipLaunchKernelGGL((audio_transform_kernel<T, true>), dim3(grid), dim3(AT_RUN), (size_t)span * 4, st, src, stride_b, stride_c, C, L0, taps,
                       first_tap, orig, new_rate, S, width, span, (const float*)scale, contrast, out, L, ld_out, bpc);
  }
  MAAVSS_LAUNCH_CHECK("audio_transform_kernel");
  return MAAVSS_OK;
}

}  // namespace

extern "C" int64_t maavss_audio_transform_ws_bytes(int64_t B, int C, int64_t L0, int normalize) {
  if (!at_shape_ok(B, C, L0)) return -1;
  return normalize ? align256(B * 4) : 0;
}

extern "C" int maavss_audio_transform(const void* src, int src_dtype, int64_t B, int C, int64_t L0, int64_t stride_b, int64_t stride_c,
                                      const float* taps, const int32_t* first_tap, int orig_rate, int new_rate, int S, int width,
                                      int normalize, int contrast, float* out, int64_t L, int64_t ld_out, void* ws, int64_t ws_bytes,
                                      void* stream) {
  MAAVSS_CHECK_ARG(src && out, "audio_transform: null pointer");
  MAAVSS_CHECK_ARG(src_dtype == 0 || src_dtype == 1, "audio_transform: src_dtype %d (0 = f32, 1 = int16)", src_dtype);
  MAAVSS_CHECK_ARG(at_shape_ok(B, C, L0), "audio_transform: bad shape B = %lld, C = %d, L0 = %lld", (long long)B, C, (long long)L0);
  MAAVSS_CHECK_ARG(stride_b >= 0 && stride_c >= 0, "audio_transform: negative stride (%lld, %lld)", (long long)stride_b, (long long)stride_c);
  MAAVSS_CHECK_ARG(((uintptr_t)src & (src_dtype == 0 ? 3 : 1)) == 0 && ((uintptr_t)out & 3) == 0, "audio_transform: misaligned src or out");
  MAAVSS_CHECK_ARG(orig_rate >= 1 && new_rate >= 1, "audio_transform: rates %d -> %d must be positive", orig_rate, new_rate);
  MAAVSS_CHECK_ARG(L >= 1 && ld_out >= L, "audio_transform: L = %lld, ld_out = %lld", (long long)L, (long long)ld_out);
  if (orig_rate == new_rate) {
    MAAVSS_CHECK_ARG(L <= L0, "audio_transform: L = %lld exceeds the %lld input samples", (long long)L, (long long)L0);
  } else {
    MAAVSS_CHECK_ARG(taps && first_tap, "audio_transform: resampling %d -> %d needs the tap table", orig_rate, new_rate);
    MAAVSS_CHECK_ARG(S >= 1 && width >= 0 && (int64_t)new_rate * S <= ((int64_t)1 << 22),
                     "audio_transform: bad tap table (S = %d, width = %d, new = %d; at most 2^22 taps)", S, width, new_rate);
    const int64_t full = (L0 * new_rate + orig_rate - 1) / orig_rate;
    MAAVSS_CHECK_ARG(L <= full, "audio_transform: L = %lld exceeds the %lld samples %lld inputs resample to", (long long)L, (long long)full,
                     (long long)L0);
    MAAVSS_CHECK_ARG(at_span(orig_rate, new_rate, S) * 4 <= AT_MAX_LDS,
                     "audio_transform: %d -> %d with %d taps needs a staged span of %lld samples, the limit is %lld (rate ratio too large)",
                     orig_rate, new_rate, S, (long long)at_span(orig_rate, new_rate, S), (long long)(AT_MAX_LDS / 4));
  }
  MAAVSS_CHECK_ARG((int64_t)cdiv(L, AT_RUN) * B < ((int64_t)1 << 31), "audio_transform: grid too large");
  float* scale = nullptr;
  if (normalize) {
    const int64_t need = maavss_audio_transform_ws_bytes(B, C, L0, 1);
    MAAVSS_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0 && ws_bytes >= need, "audio_transform: workspace of %lld bytes, needs %lld",
                     (long long)ws_bytes, (long long)need);
    scale = (float*)ws;
  }
  hipStream_t st = (hipStream_t)stream;
  if (src_dtype == 0)
    return at_launch((const float*)src, B, C, L0, stride_b, stride_c, taps, first_tap, orig_rate, new_rate, S, width, normalize, contrast != 0,
                     out, L, ld_out, scale, st);
  return at_launch((const int16_t*)src, B, C, L0, stride_b, stride_c, taps, first_tap, orig_rate, new_rate, S, width, normalize,
                   contrast != 0, out, L, ld_out, scale, st);
}
