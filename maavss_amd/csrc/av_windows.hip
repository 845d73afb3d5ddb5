// Whole-recording inference (maavss_amd.Enhancer): the window batches of the reference's num_seq loop (train_avse_frames.py:
// 150-176) cut from per-frame attention maps and from one batched STFT of overlapping clips, and the stitch of the model's outputs
// into one STFT that a single inverse turns into a waveform.  Every pass is a memory-bound copy, grid-stride, float4 where the
// run lengths allow it; every index taken from a table is clamped, and the entry points validate their arguments.
//   av_clip_scale     per clip c: 1 / m_c with m_c the clip max of av_dataset.py:328 -- over the fmax of pass 1 (maavss_vit_attn_maps_pass1)
//                     of the clip's frames, or over the clip's map values; with attn_diff over the zero-padded temporal difference
//                     (av_dataset.py:323-326, vit_maps_diff_kernel: the maximum starts at 0).  Reads T_c * frame_elems * 4 B per clip
//                     (T_c * 4 B with fmax), writes 4 B.
//   av_attn_windows   [n_win][n][H][W]: window w = c * num_seq + j, frame t = clip frame j + t = recording frame clip_start[c] + j + t,
//                     value map * (1 / m_c) (with attn_diff: (map_k - map_{k-1}) * (1 / m_c), frame 0 of the clip 0 * (1 / m_c)) --
//                     the arithmetic of vit_maps_pass2_kernel, so the result is bit-identical to attention_frames(clip, clip_frames = T_c).
//                     upsample = 1: maps are pass-1 maps [frames][H/8][W/8], nearest x8, zero outside the patch grid; 0: full-resolution
//                     maps [frames][H][W].  Writes n_win * n * H * W * 4 B; the maps are read from L2 (a frame is shared by up to n windows).
//   av_stft_windows   [n_win][2][a n][F] = STFT frames [a j, a (j + n)) of clip c (train_avse_frames.py:159-163).
//                     Reads and writes n_win * 2 * a * n * F * 4 B.
//   av_stitch         out [2][a * n_clips * num_seq][F], rows a w .. a w + a - 1 = pred[w - w0] * g_c with g_c = clip_absmax[c] + 1e-7
//                     (the divisor of maavss_stft_normalise; 1 without clip_absmax) -- output_stft of train_avse_frames.py:172-174
//                     over all clips.  Reads and writes n_win * 2 * a * F * 4 B.
#include "common.h"

namespace {

__device__ __forceinline__ int64_t av_clip_first_frame(const int32_t* clip_start, int64_t c, int64_t n_frames, int clip_frames) {
  const int64_t f0 = clip_start[c];
  return f0 < 0 ? 0 : (f0 > n_frames - clip_frames ? n_frames - clip_frames : f0);
}

__global__ __launch_bounds__(256) void av_clip_scale_kernel(const float* __restrict__ maps, const float* __restrict__ fmax,
                                                            const int32_t* __restrict__ clip_start, int64_t n_frames, int clip_frames,
                                                            int64_t frame_elems, int attn_diff, float* __restrict__ clip_rcp) {
  __shared__ float red[4][1];
  const int64_t c = blockIdx.x;
  const int64_t f0 = av_clip_first_frame(clip_start, c, n_frames, clip_frames);
  const float* mp = maps + f0 * frame_elems;
  float mx;
  if (attn_diff) {
    mx = 0.f;
    for (int64_t e = threadIdx.x; e < frame_elems; e += 256)
      for (int t = 1; t < clip_frames; ++t) mx = fmaxf(mx, mp[t * frame_elems + e] - mp[(t - 1) * frame_elems + e]);
  } else if (fmax != nullptr) {
    mx = -1e30f;
    for (int t = threadIdx.x; t < clip_frames; t += 256) mx = fmaxf(mx, fmax[f0 + t]);
  } else {
    mx = -1e30f;
    const int64_t n = (int64_t)clip_frames * frame_elems;
    for (int64_t e = threadIdx.x; e < n; e += 256) mx = fmaxf(mx, mp[e]);
  }
  mx = wg_reduce<WG_THREAD0, WG_MAX>(wave_max(mx), red, threadIdx.x >> 6, threadIdx.x & 63);
  if (threadIdx.x == 0) clip_rcp[c] = 1.f / mx;
}

__global__ __launch_bounds__(256) void av_attn_windows_kernel(const float* __restrict__ maps, const float* __restrict__ clip_rcp,
                                                              const int32_t* __restrict__ clip_start, int64_t n_clips, int64_t n_frames,
                                                              int clip_frames, int num_seq, int win_frames, int64_t w0, int H, int W,
                                                              int upsample, int attn_diff, float* __restrict__ out, int64_t total4) {
  const int W4 = W / 4, hp = H / 8, wp = W / 8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int x4 = (int)(i % W4), y = (int)((i / W4) % H);
    const int64_t q = i / ((int64_t)W4 * H);                // window-local frame row: iw * win_frames + t
    const int t = (int)(q % win_frames);
    const int64_t w = w0 + q / win_frames;
    int64_t c = w / num_seq;
    c = c < n_clips ? c : n_clips - 1;
    int k = (int)(w % num_seq) + t;                          // frame of the clip
    k = k < clip_frames ? k : clip_frames - 1;
    const int64_t f = av_clip_first_frame(clip_start, c, n_frames, clip_frames) + k;
    const float r = clip_rcp[c];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (upsample) {
      const int py = y >> 3, px = (x4 * 4) >> 3;            // 4 consecutive pixels never straddle an 8-pixel patch
      if (py < hp && px < wp) {
        const int64_t n = (int64_t)hp * wp;
        const float* sp = maps + f * n + py * wp + px;
        const float v = (attn_diff ? (k == 0 ? 0.f : sp[0] - sp[-n]) : sp[0]) * r;
        o = make_float4(v, v, v, v);
      }
    } else {
      const int64_t n = (int64_t)H * W;
      const float4* sp = reinterpret_cast<const float4*>(maps + f * n + (int64_t)y * W) + x4;
      float4 a = sp[0];
      if (attn_diff) {
        if (k == 0) {
          a = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(sp) - n);
          a = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
        }
      }
      o = make_float4(a.x * r, a.y * r, a.z * r, a.w * r);
    }
    reinterpret_cast<float4*>(out)[i] = o;
  }
}

template <int V>
struct VecT;
template <>
struct VecT<1> { using T = float; };
template <>
struct VecT<4> { using T = float4; };

template <int V>
__global__ __launch_bounds__(256) void av_stft_windows_kernel(const float* __restrict__ y, int64_t n_clips, int clip_rows, int n_bins,
                                                              int a, int num_seq, int win_frames, int64_t w0, float* __restrict__ out,
                                                              int64_t total_v) {
  using T = typename VecT<V>::T;
  const int64_t run_v = (int64_t)a * win_frames * n_bins / V;          // vectors per window and plane
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_v; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i % run_v, q = i / run_v;                         // q = iw * 2 + plane
    const int p = (int)(q & 1);
    const int64_t w = w0 + (q >> 1);
    int64_t c = w / num_seq;
    c = c < n_clips ? c : n_clips - 1;
    const int j = (int)(w % num_seq);
    const float* src = y + ((c * 2 + p) * clip_rows + (int64_t)a * j) * n_bins;
    reinterpret_cast<T*>(out)[i] = reinterpret_cast<const T*>(src)[r];
  }
}

template <int V>
__global__ __launch_bounds__(256) void av_stitch_kernel(const float* __restrict__ pred, const float* __restrict__ clip_absmax,
                                                        int64_t n_clips, int num_seq, int a, int n_bins, int64_t w0,
                                                        float* __restrict__ out, int64_t total_v) {
  using T = typename VecT<V>::T;
  const int64_t run_v = (int64_t)a * n_bins / V;
  const int64_t out_rows = (int64_t)a * n_clips * num_seq;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_v; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i % run_v, q = i / run_v;                         // q = iw * 2 + plane
    const int p = (int)(q & 1);
    const int64_t w = w0 + (q >> 1);
    int64_t c = w / num_seq;
    c = c < n_clips ? c : n_clips - 1;
    const float g = clip_absmax != nullptr ? clip_absmax[c] + 1e-7f : 1.f;
    T v = reinterpret_cast<const T*>(pred)[i];
    if constexpr (V == 4) {
      v.x *= g; v.y *= g; v.z *= g; v.w *= g;
    } else {
      v *= g;
    }
    reinterpret_cast<T*>(out + (p * out_rows + (int64_t)a * w) * n_bins)[r] = v;
  }
}

inline bool av_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline unsigned av_grid(int64_t items) {
  const int64_t g = (items + 255) / 256;
  return (unsigned)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int maavss_av_clip_scale(const float* maps, const float* fmax, const int32_t* clip_start, int64_t n_clips, int64_t n_frames,
                                    int clip_frames, int64_t frame_elems, int attn_diff, float* clip_rcp, void* stream) {
  MAAVSS_CHECK_ARG(maps && clip_start && clip_rcp, "av_clip_scale: null pointer");
  MAAVSS_CHECK_ARG(n_clips > 0 && clip_frames > 0 && frame_elems > 0, "av_clip_scale: empty problem");
  MAAVSS_CHECK_ARG(n_frames >= clip_frames, "av_clip_scale: %lld frames hold no clip of %d frames", (long long)n_frames, clip_frames);
  MAAVSS_CHECK_ARG(n_clips <= 0x7fffffff, "av_clip_scale: too many clips");
  hipLaunchKernelGGL(av_clip_scale_kernel, dim3((unsigned)n_clips), dim3(256), 0, (hipStream_t)stream, maps, fmax, clip_start, n_frames,
                     clip_frames, frame_elems, attn_diff ? 1 : 0, clip_rcp);
  MAAVSS_LAUNCH_CHECK("av_clip_scale_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_av_attn_windows(const float* maps, const float* clip_rcp, const int32_t* clip_start, int64_t n_clips,
                                      int64_t n_frames, int clip_frames, int num_seq, int win_frames, int64_t w0, int64_t n_win, int H, int W,
                                      int upsample, int attn_diff, float* out, void* stream) {
  MAAVSS_CHECK_ARG(maps && clip_rcp && clip_start && out, "av_attn_windows: null pointer");
  MAAVSS_CHECK_ARG(n_clips > 0 && num_seq > 0 && win_frames > 0 && n_win > 0 && w0 >= 0, "av_attn_windows: empty problem");
  MAAVSS_CHECK_ARG(w0 + n_win <= n_clips * num_seq, "av_attn_windows: windows %lld..%lld past the %lld of %lld clips", (long long)w0,
                   (long long)(w0 + n_win), (long long)(n_clips * num_seq), (long long)n_clips);
  MAAVSS_CHECK_ARG(num_seq - 1 + win_frames <= clip_frames, "av_attn_windows: windows of %d frames at %d offsets exceed a %d-frame clip",
                   win_frames, num_seq, clip_frames);
  MAAVSS_CHECK_ARG(n_frames >= clip_frames, "av_attn_windows: %lld frames hold no clip of %d frames", (long long)n_frames, clip_frames);
  MAAVSS_CHECK_ARG(H >= 8 && W >= 8 && W % 4 == 0, "av_attn_windows: frames must be at least 8x8 with W a multiple of 4");
  MAAVSS_CHECK_ARG(av_aligned16(out) && (upsample || av_aligned16(maps)), "av_attn_windows: out (and full-resolution maps) must be 16-byte aligned");
  const int64_t total4 = n_win * win_frames * H * (W / 4);
  hipLaunchKernelGGL(av_attn_windows_kernel, dim3(av_grid(total4)), dim3(256), 0, (hipStream_t)stream, maps, clip_rcp, clip_start, n_clips,
                     n_frames, clip_frames, num_seq, win_frames, w0, H, W, upsample ? 1 : 0, attn_diff ? 1 : 0, out, total4);
  MAAVSS_LAUNCH_CHECK("av_attn_windows_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_av_stft_windows(const float* y, int64_t n_clips, int clip_rows, int n_bins, int hops_per_frame, int num_seq,
                                      int win_frames, int64_t w0, int64_t n_win, float* out, void* stream) {
  MAAVSS_CHECK_ARG(y && out, "av_stft_windows: null pointer");
  MAAVSS_CHECK_ARG(n_clips > 0 && n_bins > 0 && hops_per_frame > 0 && num_seq > 0 && win_frames > 0 && n_win > 0 && w0 >= 0,
                   "av_stft_windows: empty problem");
  MAAVSS_CHECK_ARG(w0 + n_win <= n_clips * num_seq, "av_stft_windows: windows %lld..%lld past the %lld of %lld clips", (long long)w0,
                   (long long)(w0 + n_win), (long long)(n_clips * num_seq), (long long)n_clips);
  MAAVSS_CHECK_ARG((int64_t)hops_per_frame * (num_seq - 1 + win_frames) <= clip_rows,
                   "av_stft_windows: windows of %d x %d STFT frames at %d offsets exceed a clip of %d frames", win_frames, hops_per_frame,
                   num_seq, clip_rows);
  const int64_t run = (int64_t)hops_per_frame * win_frames * n_bins;
  hipStream_t st = (hipStream_t)stream;
  // float4 runs start at ((c * 2 + p) * clip_rows + a j) * n_bins floats of y: every plane and every hop offset must be a multiple of 4
  if (((int64_t)hops_per_frame * n_bins) % 4 == 0 && ((int64_t)clip_rows * n_bins) % 4 == 0 && av_aligned16(y) && av_aligned16(out)) {
    const int64_t total = n_win * 2 * run / 4;
    hipLaunchKernelGGL(av_stft_windows_kernel<4>, dim3(av_grid(total)), dim3(256), 0, st, y, n_clips, clip_rows, n_bins, hops_per_frame,
                       num_seq, win_frames, w0, out, total);
  } else {
    const int64_t total = n_win * 2 * run;
    hipLaunchKernelGGL(av_stft_windows_kernel<1>, dim3(av_grid(total)), dim3(256), 0, st, y, n_clips, clip_rows, n_bins, hops_per_frame,
                       num_seq, win_frames, w0, out, total);
  }
  MAAVSS_LAUNCH_CHECK("av_stft_windows_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_av_stitch(const float* pred, const float* clip_absmax, int64_t n_clips, int num_seq, int hops_per_frame, int n_bins,
                                int64_t w0, int64_t n_win, float* out, void* stream) {
  MAAVSS_CHECK_ARG(pred && out, "av_stitch: null pointer");
  MAAVSS_CHECK_ARG(n_clips > 0 && num_seq > 0 && hops_per_frame > 0 && n_bins > 0 && n_win > 0 && w0 >= 0, "av_stitch: empty problem");
  MAAVSS_CHECK_ARG(w0 + n_win <= n_clips * num_seq, "av_stitch: windows %lld..%lld past the %lld of %lld clips", (long long)w0,
                   (long long)(w0 + n_win), (long long)(n_clips * num_seq), (long long)n_clips);
  const int64_t run = (int64_t)hops_per_frame * n_bins;
  hipStream_t st = (hipStream_t)stream;
  if (run % 4 == 0 && av_aligned16(pred) && av_aligned16(out)) {
    const int64_t total = n_win * 2 * run / 4;
    hipLaunchKernelGGL(av_stitch_kernel<4>, dim3(av_grid(total)), dim3(256), 0, st, pred, clip_absmax, n_clips, num_seq, hops_per_frame,
                       n_bins, w0, out, total);
  } else {
    const int64_t total = n_win * 2 * run;
    hipLaunchKernelGGL(av_stitch_kernel<1>, dim3(av_grid(total)), dim3(256), 0, st, pred, clip_absmax, n_clips, num_seq, hops_per_frame,
                       n_bins, w0, out, total);
  }
  MAAVSS_LAUNCH_CHECK("av_stitch_kernel");
  return MAAVSS_OK;
}
