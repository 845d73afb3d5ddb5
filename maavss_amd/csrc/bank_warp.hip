// Per-clip random resized crop and flip of the clip bank's stored maps (maavss_amd.ClipBank.batch(boxes=, flip=), warp_maps): the
// geometric part of the frames-fed path's RandomResizedCrop (av_dataset.py:108-112), applied at patch resolution to the tensor the
// fusion network reads, without the ViT.  include/maavss.h states the definition operation for operation; tests/bank_warp_twin.py
// restates it.  This file is compiled with -ffp-contract=off: every f64 operation below is rounded on its own.
//   bank_warp_maps    out [B * T][n] f32, n = (S / 8)^2: frame t of clip b = bank frame start[b] + t resampled bilinearly
//                     (align_corners = False, clamped to the patches the box touches) from the clip's box, mirrored when the clip is
//                     flipped, then divided by the frame's own maximum as pass 1 of the extractor does (frame_norm).  One workgroup
//                     per (clip, frame); a thread owns the patches tid, tid + 256, ...: four taps through bank_load (the frame is a
//                     few KB and stays in L2), one store, the frame maximum through reduce.h, then the thread rescales what it wrote.
//                     Index and weight numerators are integers; no atomics.  Reads at most 4 n * {4, 2} B, writes n * 4 B per frame.
#include "common.h"
#include "bank_load.h"      // bank_load (both storages), bank_clamp

namespace {

// One axis of the resampling: output patch i of hp reads source patches a and b with weight w on b.  The centre of the output patch
// in source-patch units is (off + (i + 0.5) * len / hp) / 8 - 0.5 = N / D with the integers below.  off + len <= S = 8 hp and
// i < hp give -8 hp < N < 2 hp S = S^2 / 4, so with S <= 32768 (the entry point refuses more) everything fits 32 bits -- a 64-bit
// division is a subroutine of its own on this hardware.
__device__ __forceinline__ void warp_axis(int i, int hp, int off, int len, int& a, int& b, double& w) {
  const int D = 16 * hp;
  const int N = 2 * off * hp + (2 * i + 1) * len - 8 * hp;
  const int y0 = N < 0 ? -1 : N / D;                      // floor: N > -D
  const int r = N - y0 * D;                               // in [0, D)
  w = (double)r / (double)D;
  const int lo = off / 8, hi = (off + len - 1) / 8;
  a = y0 < lo ? lo : (y0 > hi ? hi : y0);
  b = y0 + 1 < lo ? lo : (y0 + 1 > hi ? hi : y0 + 1);
}

template <typename T>
__global__ __launch_bounds__(256) void bank_warp_maps_kernel(const T* __restrict__ maps, const int32_t* __restrict__ start,
                                                             const int32_t* __restrict__ boxes, const uint8_t* __restrict__ flips,
                                                             int64_t n_frames, int clip_frames, int S, int frame_norm,
                                                             float* __restrict__ out) {
  __shared__ float red[4][1];
  const int hp = S / 8, n = hp * hp;
  const uint32_t q = blockIdx.x, b = q / (uint32_t)clip_frames, t = q % (uint32_t)clip_frames;
  const T* mp = maps + (bank_clamp(start[b], n_frames - clip_frames) + t) * n;
  // the box was checked on the host copy; the device copy is clamped into the frame like every other table
  const int top = (int)bank_clamp(boxes[4 * b], S - 1), left = (int)bank_clamp(boxes[4 * b + 1], S - 1);
  const int height = (int)bank_clamp(boxes[4 * b + 2] - 1, S - top - 1) + 1, width = (int)bank_clamp(boxes[4 * b + 3] - 1, S - left - 1) + 1;
  const bool flip = flips != nullptr && flips[b] != 0;
  float* op = out + (int64_t)q * n;
  float mx = -1e30f;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int i = e / hp, j = e % hp;
    int ya, yb, xc, xd;
    double wy, wx;
    warp_axis(i, hp, top, height, ya, yb, wy);
    warp_axis(j, hp, left, width, xc, xd, wx);
    const double mac = (double)bank_load(mp, ya * hp + xc), mad = (double)bank_load(mp, ya * hp + xd);
    const double mbc = (double)bank_load(mp, yb * hp + xc), mbd = (double)bank_load(mp, yb * hp + xd);
    const double r0 = (1.0 - wx) * mac + wx * mad;
    const double r1 = (1.0 - wx) * mbc + wx * mbd;
    const float v = (float)((1.0 - wy) * r0 + wy * r1);
    op[i * hp + (flip ? hp - 1 - j : j)] = v;
    mx = fmaxf(mx, v);
  }
  if (!frame_norm) return;                                // uniform over the workgroup
  mx = wg_reduce<WG_ALL, WG_MAX>(wave_max(mx), red, threadIdx.x >> 6, threadIdx.x & 63);
  const float rcp = 1.f / mx;                             // no guard, as in vit_maps_pass1_kernel: an all-zero frame gives 0 * inf
  for (int e = threadIdx.x; e < n; e += 256) {            // the elements this thread wrote above
    const int i = e / hp, j = e % hp, at = i * hp + (flip ? hp - 1 - j : j);
    op[at] = op[at] * rcp;
  }
}

}  // namespace

extern "C" int maavss_bank_warp_maps(const void* maps, int storage, const int32_t* clip_start, const int32_t* boxes, const void* flips,
                                     int64_t n_clips, int64_t n_frames_total, int clip_frames, int S, int frame_norm, float* out,
                                     void* stream) {
  MAAVSS_CHECK_ARG(maps && clip_start && boxes && out, "bank_warp_maps: null pointer");
  MAAVSS_CHECK_ARG(storage == 0 || storage == 1, "bank_warp_maps: storage must be 0 (f32) or 1 (u16), got %d", storage);
  MAAVSS_CHECK_ARG(n_clips > 0 && clip_frames > 0, "bank_warp_maps: empty problem");
  MAAVSS_CHECK_ARG(n_frames_total >= clip_frames, "bank_warp_maps: %lld frames hold no clip of %d frames", (long long)n_frames_total,
                   clip_frames);
  MAAVSS_CHECK_ARG(S >= 8 && S % 8 == 0 && S <= 32768, "bank_warp_maps: S = %d must be a multiple of 8 in [8, 32768]", S);
  MAAVSS_CHECK_ARG(((uintptr_t)maps & (storage ? 1 : 3)) == 0 && ((uintptr_t)out & 3) == 0, "bank_warp_maps: maps and out must be aligned to their element");
  MAAVSS_CHECK_ARG(n_clips <= 0x7fffffff / clip_frames, "bank_warp_maps: %lld clips of %d frames exceed the 32-bit workgroup index",
                   (long long)n_clips, clip_frames);
  const dim3 grid((unsigned)(n_clips * clip_frames));
  hipStream_t st = (hipStream_t)stream;
  const int fn = frame_norm ? 1 : 0;
  if (storage)
    hipLaunchKernelGGL(bank_warp_maps_kernel<uint16_t>, grid, dim3(256), 0, st, (const uint16_t*)maps, clip_start, boxes,
                       (const uint8_t*)flips, n_frames_total, clip_frames, S, fn, out);
  else
    hipLaunchKernelGGL(bank_warp_maps_kernel<float>, grid, dim3(256), 0, st, (const float*)maps, clip_start, boxes,
                       (const uint8_t*)flips, n_frames_total, clip_frames, S, fn, out);
  MAAVSS_LAUNCH_CHECK("bank_warp_maps_kernel");
  return MAAVSS_OK;
}
