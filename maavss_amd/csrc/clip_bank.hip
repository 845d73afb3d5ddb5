// Device-resident clip bank (maavss_amd.ClipBank): the reference's attention-frame cache and audio memmap (av_dataset.py:251-268,
// 285-294) held in HBM -- per-frame attention maps at patch resolution (what maavss_vit_attn_maps_pass1 writes, 4 B or 2 B a value)
// and one f32 buffer of every recording's samples -- and a training batch cut from them by two tables of start positions.
// Every pass is a memory-bound copy; every index taken from a table is clamped, and the entry points validate their arguments.
//   bank_pack_u16     q = rint(min(max(v, 0), 1) * 65535): one f32 product, rounded half to even; NaN packs to 0.
//                     Reads 4 n B, writes 2 n B.
//   bank_unpack_u16   v = q / 65535, the correctly rounded f32 quotient (65535 gives exactly 1; a product with the rounded reciprocal
//                     does not).  Reads 2 n B, writes 4 n B.
//   bank_clip_scale   per clip b: 1 / m_b with m_b the clip max of av_dataset.py:328 over the clip's (dequantised) map values, with
//                     attn_diff over the zero-padded temporal difference (av_dataset.py:323-326: the maximum starts at 0) -- the
//                     arithmetic of av_clip_scale_kernel (av_windows.hip).  Reads clip_frames * n * {4, 2} B per clip, writes 4 B.
//   bank_attn_clips   out [B][clip_frames][H][W]: frame t of clip b = bank frame start[b] + t, nearest x8, zero outside the patch grid,
//                     value map * (1 / m_b) (attn_diff: (map_t - map_{t-1}) * (1 / m_b), frame 0 of the clip 0 * (1 / m_b): the frame
//                     in front of a clip, which may belong to another recording, is never read) -- the arithmetic of
//                     av_attn_windows_kernel with num_seq = 1, win_frames = clip_frames, so an f32 bank gives attention_frames(clip,
//                     clip_frames) bit for bit.  One thread per (frame, patch row, 4-pixel column): one map value read (and
//                     dequantised) from L2, eight 16-byte stores, a wave's store instruction covering 1 KiB of consecutive float4 of a
//                     pixel row (and the start of the next patch row's).
//                     Writes B * clip_frames * H * W * 4 B; reads an eighth of a map value per store.
//   bank_audio_clips  out[b][0 .. L) = bank[start[b] .. start[b] + L): starts are arbitrary, so the source rows are not 16-byte
//                     aligned -- four dword loads (a wave's are contiguous) and one 16-byte store per thread where out allows,
//                     element stores otherwise and in a row's last L % 4 samples.  Offsets are 64-bit.  Reads and writes B * L * 4 B.
// One body serves both storages: the kernels are templates over the stored type and differ in bank_load alone.
#include "common.h"
#include "bank_load.h"      // bank_load (both storages), bank_clamp

namespace {

__global__ __launch_bounds__(256) void bank_pack_u16_kernel(const float* __restrict__ maps, uint16_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = (uint16_t)(int)rintf(fminf(fmaxf(maps[i], 0.f), 1.f) * 65535.f);      // fmaxf(NaN, 0) = 0
}

__global__ __launch_bounds__(256) void bank_unpack_u16_kernel(const uint16_t* __restrict__ q, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = bank_load(q, i);
}

template <typename T>
__global__ __launch_bounds__(256) void bank_clip_scale_kernel(const T* __restrict__ maps, const int32_t* __restrict__ start,
                                                              int64_t n_frames, int clip_frames, int frame_elems, int attn_diff,
                                                              float* __restrict__ clip_rcp) {
  __shared__ float red[4][1];
  const int64_t f0 = bank_clamp(start[blockIdx.x], n_frames - clip_frames);
  const T* mp = maps + f0 * frame_elems;
  float mx;
  if (attn_diff) {
    mx = 0.f;
    for (int e = threadIdx.x; e < frame_elems; e += 256) {
      float prev = bank_load(mp, e);
      for (int t = 1; t < clip_frames; ++t) {
        const float cur = bank_load(mp, (int64_t)t * frame_elems + e);
        mx = fmaxf(mx, cur - prev);
        prev = cur;
      }
    }
  } else {
    mx = -1e30f;
    const int64_t n = (int64_t)clip_frames * frame_elems;
    for (int64_t e = threadIdx.x; e < n; e += 256) mx = fmaxf(mx, bank_load(mp, e));
  }
  mx = wg_reduce<WG_THREAD0, WG_MAX>(wave_max(mx), red, threadIdx.x >> 6, threadIdx.x & 63);
  if (threadIdx.x == 0) clip_rcp[blockIdx.x] = 1.f / mx;
}

// item i = ((b * clip_frames + t) * hpc + py) * W4 + x4, hpc = ceil(H / 8) patch rows (the last one may lie outside the patch grid)
template <typename T>
__global__ __launch_bounds__(256) void bank_attn_clips_kernel(const T* __restrict__ maps, const float* __restrict__ clip_rcp,
                                                              const int32_t* __restrict__ start, int64_t n_frames, int clip_frames,
                                                              int H, int W, int attn_diff, float* __restrict__ out, uint32_t total) {
  const uint32_t W4 = W / 4, hpc = (H + 7) / 8;
  const int hp = H / 8, wp = W / 8, n = hp * wp;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t x4 = i % W4, r = i / W4;
    const uint32_t py = r % hpc, q = r / hpc;                 // q = b * clip_frames + t
    const uint32_t b = q / (uint32_t)clip_frames, t = q % (uint32_t)clip_frames;
    const int px = (int)(x4 * 4) >> 3;                        // 4 consecutive pixels never straddle an 8-pixel patch
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((int)py < hp && px < wp) {
      const int64_t f = bank_clamp(start[b], n_frames - clip_frames) + t;
      const int64_t at = f * n + (int)py * wp + px;
      const float v = (attn_diff ? (t == 0 ? 0.f : bank_load(maps, at) - bank_load(maps, at - n)) : bank_load(maps, at)) * clip_rcp[b];
      o = make_float4(v, v, v, v);
    }
    const int y0 = (int)py * 8, rows = H - y0 < 8 ? H - y0 : 8;
    float4* op = reinterpret_cast<float4*>(out) + ((int64_t)q * H + y0) * W4 + x4;
    for (int y = 0; y < rows; ++y) op[(int64_t)y * W4] = o;
  }
}

template <int V>
__global__ __launch_bounds__(256) void bank_audio_clips_kernel(const float* __restrict__ bank, const int64_t* __restrict__ start,
                                                               int64_t n_samples, int64_t L, float* __restrict__ out, int64_t ld_out,
                                                               int64_t total) {
  const int64_t per_row = (L + V - 1) / V;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / per_row, j = (i % per_row) * V;
    const float* sp = bank + bank_clamp(start[b], n_samples - L) + j;
    float* op = out + b * ld_out + j;
    if (V == 4 && j + 4 <= L) {
      *reinterpret_cast<float4*>(op) = make_float4(sp[0], sp[1], sp[2], sp[3]);
    } else {
      for (int64_t k = 0; k < V && j + k < L; ++k) op[k] = sp[k];
    }
  }
}

inline bool bank_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline unsigned bank_grid(int64_t items) {
  const int64_t g = (items + 255) / 256;
  return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

template <typename T>
int bank_attn_clips_launch(const T* maps, const int32_t* start, int64_t n_clips, int64_t n_frames, int clip_frames, int H, int W,
                           int attn_diff, float* clip_rcp, float* out, hipStream_t st) {
  hipLaunchKernelGGL(bank_clip_scale_kernel<T>, dim3((unsigned)n_clips), dim3(256), 0, st, maps, start, n_frames, clip_frames,
                     (H / 8) * (W / 8), attn_diff, clip_rcp);
  MAAVSS_LAUNCH_CHECK("bank_clip_scale_kernel");
  const int64_t total = n_clips * clip_frames * ((H + 7) / 8) * (W / 4);
  hipLaunchKernelGGL(bank_attn_clips_kernel<T>, dim3(bank_grid(total)), dim3(256), 0, st, maps, clip_rcp, start, n_frames, clip_frames,
                     H, W, attn_diff, out, (uint32_t)total);
  MAAVSS_LAUNCH_CHECK("bank_attn_clips_kernel");
  return MAAVSS_OK;
}

}  // namespace

extern "C" int maavss_bank_pack_u16(const float* maps, void* out, int64_t n, void* stream) {
  MAAVSS_CHECK_ARG(maps && out, "bank_pack_u16: null pointer");
  MAAVSS_CHECK_ARG(n > 0, "bank_pack_u16: empty problem");
  MAAVSS_CHECK_ARG(bank_aligned(out, 2), "bank_pack_u16: out must be 2-byte aligned");
  hipLaunchKernelGGL(bank_pack_u16_kernel, dim3(bank_grid(n)), dim3(256), 0, (hipStream_t)stream, maps, (uint16_t*)out, n);
  MAAVSS_LAUNCH_CHECK("bank_pack_u16_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_bank_unpack_u16(const void* q, float* out, int64_t n, void* stream) {
  MAAVSS_CHECK_ARG(q && out, "bank_unpack_u16: null pointer");
  MAAVSS_CHECK_ARG(n > 0, "bank_unpack_u16: empty problem");
  MAAVSS_CHECK_ARG(bank_aligned(q, 2), "bank_unpack_u16: q must be 2-byte aligned");
  hipLaunchKernelGGL(bank_unpack_u16_kernel, dim3(bank_grid(n)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)q, out, n);
  MAAVSS_LAUNCH_CHECK("bank_unpack_u16_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_bank_attn_clips(const void* maps, int storage, const int32_t* clip_start, int64_t n_clips, int64_t n_frames_total,
                                      int clip_frames, int H, int W, int attn_diff, float* clip_rcp, float* out, void* stream) {
  MAAVSS_CHECK_ARG(maps && clip_start && clip_rcp && out, "bank_attn_clips: null pointer");
  MAAVSS_CHECK_ARG(storage == 0 || storage == 1, "bank_attn_clips: storage must be 0 (f32) or 1 (u16), got %d", storage);
  MAAVSS_CHECK_ARG(n_clips > 0 && clip_frames > 0, "bank_attn_clips: empty problem");
  MAAVSS_CHECK_ARG(n_frames_total >= clip_frames, "bank_attn_clips: %lld frames hold no clip of %d frames", (long long)n_frames_total,
                   clip_frames);
  MAAVSS_CHECK_ARG(H >= 8 && W >= 8 && W % 4 == 0, "bank_attn_clips: frames must be at least 8x8 with W a multiple of 4");
  MAAVSS_CHECK_ARG(bank_aligned(out, 16) && bank_aligned(maps, storage ? 2 : 4), "bank_attn_clips: out must be 16-byte aligned, maps to their element");
  MAAVSS_CHECK_ARG(n_clips <= 0x7fffffff && n_clips * clip_frames * ((H + 7) / 8) * (W / 4) <= 0x7fffffff,
                   "bank_attn_clips: %lld clips of %d frames exceed the kernel's 32-bit item index", (long long)n_clips, clip_frames);
  hipStream_t st = (hipStream_t)stream;
  const int d = attn_diff ? 1 : 0;
  return storage ? bank_attn_clips_launch((const uint16_t*)maps, clip_start, n_clips, n_frames_total, clip_frames, H, W, d, clip_rcp, out, st)
                 : bank_attn_clips_launch((const float*)maps, clip_start, n_clips, n_frames_total, clip_frames, H, W, d, clip_rcp, out, st);
}

extern "C" int maavss_bank_audio_clips(const float* bank, int64_t n_samples, const int64_t* clip_start, int64_t n_clips, int64_t L,
                                       float* out, int64_t ld_out, void* stream) {
  MAAVSS_CHECK_ARG(bank && clip_start && out, "bank_audio_clips: null pointer");
  MAAVSS_CHECK_ARG(n_clips > 0 && L > 0, "bank_audio_clips: empty problem");
  MAAVSS_CHECK_ARG(n_samples >= L, "bank_audio_clips: %lld samples hold no clip of %lld", (long long)n_samples, (long long)L);
  MAAVSS_CHECK_ARG(ld_out >= L, "bank_audio_clips: ld_out = %lld is shorter than a clip of %lld samples", (long long)ld_out, (long long)L);
  MAAVSS_CHECK_ARG(bank_aligned(clip_start, 8), "bank_audio_clips: clip_start must be 8-byte aligned");
  MAAVSS_CHECK_ARG(out + n_clips * ld_out <= bank || bank + n_samples <= out, "bank_audio_clips: out overlaps the bank");
  hipStream_t st = (hipStream_t)stream;
  if (bank_aligned(out, 16) && ld_out % 4 == 0) {
    const int64_t total = n_clips * ((L + 3) / 4);
    hipLaunchKernelGGL(bank_audio_clips_kernel<4>, dim3(bank_grid(total)), dim3(256), 0, st, bank, clip_start, n_samples, L, out, ld_out, total);
  } else {
    const int64_t total = n_clips * L;
    hipLaunchKernelGGL(bank_audio_clips_kernel<1>, dim3(bank_grid(total)), dim3(256), 0, st, bank, clip_start, n_samples, L, out, ld_out, total);
  }
  MAAVSS_LAUNCH_CHECK("bank_audio_clips_kernel");
  return MAAVSS_OK;
}
