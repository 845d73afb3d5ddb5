// Frame transform of the data path: AV_Dataset's RandomResizedCrop(framesize, scale=(0.6, 1.0)) + Normalize (av_dataset.py:108-112,
// applied at :315-319 / :346-350 after permute(0,3,1,2).float() / 255) and the optional torchvision autocontrast behind it, from the
// decoder's uint8 HWC frames to the f32 [F][3][S][S] frames the ViT extractor reads.
//   pass 1 (video_transform_tables_kernel): per clip and axis, the tap table of every output coordinate -- first source index,
//           tap count and weights -- exactly as torch's bilinear resize derives them (align_corners=False; antialias = the
//           separable triangle filter whose support is max(1, in / S) input pixels).  Weights are stored tap-major ([tap][S]) so
//           that the 64 lanes of a wave, 64 consecutive output columns, read one coalesced row per tap.
//   pass 2 (video_transform_kernel): one thread per output pixel and 4 rows, all three channels: a horizontal sum over the x taps
//           of every source row the y taps name, then the vertical sum -- torch's separable order -- and one affine step
//           x * (1 / (255 std_c)) - mean_c / std_c that folds /255 and Normalize.  With autocontrast the block's per-channel
//           min / max go to [F][3] by integer atomicMin / atomicMax on order-preserving keys (order-independent: deterministic).
//   pass 3 (autocontrast only): (x - min) * 1 / (max - min) clamped to [0, 1] in place, float4.
// Traffic: the crop's bytes once (taps re-read from L2 / L1) and 4 * 3 * S^2 bytes written per frame (autocontrast: the output is read
// and written once more).  Every source index is clamped to the crop and every crop to the frame, so no box can read out of bounds.
#include <algorithm>
#include <climits>

#include "common.h"

namespace {

constexpr int VT_BX = 64;      // output columns per block (one wave per row)
constexpr int VT_BY = 4;       // waves per block
constexpr int VT_ROWS = 4;     // output rows per thread: a block covers 64 x 16 output pixels

struct VtLayout {              // byte offsets inside the workspace
  int64_t ranges, wy, wx, keys, total;
  int ty, tx;                  // taps per output coordinate (y, x)
};

__host__ __device__ inline int vt_taps(int in, int S, int antialias) {
  // antialias: support = max(1, in / S) <= ceil(in / S) source pixels each side -> at most 2 ceil(in / S) + 1 taps (+2 margin)
  return antialias ? 2 * (int)((in + S - 1) / S) + 3 : 2;
}

inline VtLayout vt_layout(int64_t F, int clip_frames, int H0, int W0, int S, int antialias, int autocontrast) {
  VtLayout L;
  const int64_t nclips = F / clip_frames;
  L.ty = vt_taps(H0, S, antialias);
  L.tx = vt_taps(W0, S, antialias);
  L.ranges = 0;                                                           // int32 [clip][2 axes][S][2] (start, count)
  L.wy = align256(nclips * 2 * S * 2 * 4);                                // f32 [clip][ty][S]
  L.wx = L.wy + align256(nclips * (int64_t)L.ty * S * 4);                 // f32 [clip][tx][S]
  L.keys = L.wx + align256(nclips * (int64_t)L.tx * S * 4);               // int32 [F][3][2] (min key, max key)
  L.total = L.keys + (autocontrast ? align256(F * 6 * 4) : 0);
  return L;
}

// the box of a clip, clamped to the frame (the host has validated it; this only makes a bad device copy harmless)
__device__ __forceinline__ void vt_box(const int32_t* __restrict__ boxes, int clip, int H0, int W0, int& top, int& left, int& h, int& w) {
  h = min(max(boxes[clip * 4 + 2], 1), H0);
  w = min(max(boxes[clip * 4 + 3], 1), W0);
  top = min(max(boxes[clip * 4 + 0], 0), H0 - h);
  left = min(max(boxes[clip * 4 + 1], 0), W0 - w);
}

// float -> int key with the float's order (signed compare); and back
__device__ __forceinline__ int vt_key(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float vt_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

// grid (cdiv(S, 256), nclips, 2): one thread per (clip, axis, output coordinate)
__global__ __launch_bounds__(256) void video_transform_tables_kernel(const int32_t* __restrict__ boxes, int32_t* __restrict__ ranges,
                                                                     float* __restrict__ wy, float* __restrict__ wx, int H0, int W0, int S,
                                                                     int ty, int tx, int antialias) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int clip = blockIdx.y, axis = blockIdx.z;
  if (o >= S) return;
  int top, left, h, w;
  vt_box(boxes, clip, H0, W0, top, left, h, w);
  const int in = axis == 0 ? h : w;
  const int taps = axis == 0 ? ty : tx;
  float* wt = (axis == 0 ? wy + (int64_t)clip * ty * S : wx + (int64_t)clip * tx * S) + o;
  const float scale = (float)in / (float)S;           // area_pixel_compute_scale (align_corners=False)
  int start, count;
  if (antialias) {
    // torch's antialiased weights (upsample "_aa"): the float / double mix of the expressions is torch's own
    const float support = scale >= 1.0f ? (float)(1.0 * (double)scale) : 1.0f;
    const float invscale = scale >= 1.0f ? (float)(1.0 / (double)scale) : 1.0f;
    const float center = (float)((double)scale * ((double)o + 0.5));
    start = max((int)((double)center - (double)support + 0.5), 0);
    count = min((int)((double)center + (double)support + 0.5), in) - start;
    count = min(max(count, 0), taps);
    float tot = 0.f;
    for (int j = 0; j < count; ++j) {
      const float x = fabsf((float)(((double)(j + start) - (double)center + 0.5) * (double)invscale));
      const float v = x < 1.0f ? 1.0f - x : 0.0f;
      wt[(int64_t)j * S] = v;
      tot += v;
    }
    if (tot != 0.f)
      for (int j = 0; j < count; ++j) wt[(int64_t)j * S] /= tot;
    for (int j = count; j < taps; ++j) wt[(int64_t)j * S] = 0.f;
  } else {
    // upsample_bilinear2d: source index max(scale (o + 0.5) - 0.5, 0); the second tap is clamped to the last pixel in the gather
    float real = scale * ((float)o + 0.5f) - 0.5f;
    real = real < 0.f ? 0.f : real;
    start = min((int)real, in - 1);
    count = 2;
    const float l1 = fminf(fmaxf(real - (float)start, 0.f), 1.f);
    // start == in - 1: the gather clamps the second tap onto the first one's pixel, so the two are one tap of weight 1.  Stored as
    // (1 - l1, l1) they sum to 1 only within 2^-24, and a one-pixel crop (every coordinate of which is this case) would not resize
    // to a constant plane: autocontrast would then stretch that rounding noise to [0, 1] instead of taking its max == min branch.
    const bool last = start >= in - 1;
    wt[0] = last ? 1.0f : 1.0f - l1;
    wt[S] = last ? 0.0f : l1;
  }
  int32_t* r = ranges + (((int64_t)clip * 2 + axis) * S + o) * 2;
  r[0] = start;
  r[1] = count;
}

// grid (cdiv(S, 64) * cdiv(S, 16) * F), block (64, 4).  TAPS = 2: plain bilinear, the tap loops unrolled so that the 12 byte loads of a
// pixel issue together; TAPS = 0: the antialiased tables, tap counts read per coordinate.
template <int TAPS>
__global__ __launch_bounds__(256) void video_transform_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ boxes,
                                                              const int32_t* __restrict__ ranges, const float* __restrict__ wy,
                                                              const float* __restrict__ wx, float* __restrict__ out, int* __restrict__ keys,
                                                              int clip_frames, int H0, int W0, int S, int ty, int tx, float a0, float a1,
                                                              float a2, float b0, float b1, float b2) {
  const int bx = (S + VT_BX - 1) / VT_BX, by = (S + VT_BY * VT_ROWS - 1) / (VT_BY * VT_ROWS);
  const int64_t f = blockIdx.x / (bx * by);
  const int tile = blockIdx.x % (bx * by);
  const int ox = (tile % bx) * VT_BX + threadIdx.x;
  const int oy0 = (tile / bx) * (VT_BY * VT_ROWS) + threadIdx.y;
  const int clip = (int)(f / clip_frames);
  int top, left, h, w;
  vt_box(boxes, clip, H0, W0, top, left, h, w);
  const uint8_t* frame = src + f * H0 * W0 * 3;
  const int32_t* ry = ranges + (int64_t)clip * 2 * S * 2;
  const int32_t* rx = ry + S * 2;
  const float* wyc = wy + (int64_t)clip * ty * S;
  const float* wxc = wx + (int64_t)clip * tx * S;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (ox < S) {
    const int xs = rx[ox * 2], xc = TAPS ? TAPS : rx[ox * 2 + 1];
    for (int k = 0; k < VT_ROWS; ++k) {
      const int oy = oy0 + k * VT_BY;
      if (oy >= S) break;
      const int ys = ry[oy * 2], yc = TAPS ? TAPS : ry[oy * 2 + 1];
      float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll 2
      for (int i = 0; i < yc; ++i) {
        const uint8_t* row = frame + ((int64_t)(top + min(ys + i, h - 1)) * W0 + left) * 3;
        float hs[3] = {0.f, 0.f, 0.f};
#pragma unroll 2
        for (int j = 0; j < xc; ++j) {
          const uint8_t* p = row + min(xs + j, w - 1) * 3;
          const float wj = wxc[(int64_t)j * S + ox];
          hs[0] += wj * (float)p[0];
          hs[1] += wj * (float)p[1];
          hs[2] += wj * (float)p[2];
        }
        const float wi = wyc[(int64_t)i * S + oy];
        acc[0] += wi * hs[0];
        acc[1] += wi * hs[1];
        acc[2] += wi * hs[2];
      }
      const float v0 = acc[0] * a0 + b0, v1 = acc[1] * a1 + b1, v2 = acc[2] * a2 + b2;
      float* o = out + (f * 3 * S + oy) * S + ox;
      o[0] = v0;
      o[(int64_t)S * S] = v1;
      o[(int64_t)2 * S * S] = v2;
      lo[0] = fminf(lo[0], v0); hi[0] = fmaxf(hi[0], v0);
      lo[1] = fminf(lo[1], v1); hi[1] = fmaxf(hi[1], v1);
      lo[2] = fminf(lo[2], v2); hi[2] = fmaxf(hi[2], v2);
    }
  }
  if (keys == nullptr) return;                         // uniform over the grid
  __shared__ float red[VT_BY][6];
  const int wave = threadIdx.y;
  const float v[6] = {wave_min(lo[0]), wave_max(hi[0]), wave_min(lo[1]), wave_max(hi[1]), wave_min(lo[2]), wave_max(hi[2])};
  wg_park(red, v, wave, threadIdx.x);
  __syncthreads();
  if (wave == 0 && threadIdx.x < 3) {                  // a lane per channel
    const int c = threadIdx.x;
    const float l = wg_col<WG_MIN>(red, 2 * c), u = wg_col<WG_MAX>(red, 2 * c + 1);
    if (l <= u) {                                      // the block holds at least one pixel of this frame
      atomicMin(keys + (f * 3 + c) * 2, vt_key(l));
      atomicMax(keys + (f * 3 + c) * 2 + 1, vt_key(u));
    }
  }
}

__global__ __launch_bounds__(256) void video_transform_keys_init_kernel(int* __restrict__ keys, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = (i & 1) ? INT_MIN : INT_MAX;
}

// torchvision autocontrast on a float image (bound 1.0): scale = 1 / (max - min); where it is not finite, min = 0 and scale = 1
__global__ __launch_bounds__(256) void video_transform_autocontrast_kernel(float* __restrict__ out, const int* __restrict__ keys,
                                                                           int64_t n4, int plane4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t p = i / plane4;
    float lo = vt_unkey(keys[p * 2]);
    const float hi = vt_unkey(keys[p * 2 + 1]);
    float scale = 1.0f / (hi - lo);
    if (!isfinite(scale)) {
      lo = 0.f;
      scale = 1.f;
    }
    float4 v = reinterpret_cast<float4*>(out)[i];
    v.x = fminf(fmaxf((v.x - lo) * scale, 0.f), 1.f);
    v.y = fminf(fmaxf((v.y - lo) * scale, 0.f), 1.f);
    v.z = fminf(fmaxf((v.z - lo) * scale, 0.f), 1.f);
    v.w = fminf(fmaxf((v.w - lo) * scale, 0.f), 1.f);
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

bool vt_shape_ok(int64_t F, int clip_frames, int H0, int W0, int S) {
  return F > 0 && clip_frames > 0 && F % clip_frames == 0 && H0 > 0 && W0 > 0 && S >= 8 && S % 4 == 0 && S <= 8192 &&
         (int64_t)H0 * W0 <= ((int64_t)1 << 28);
}

}  // namespace

extern "C" int64_t maavss_video_transform_ws_bytes(int64_t F, int clip_frames, int H0, int W0, int S, int antialias, int autocontrast) {
  if (!vt_shape_ok(F, clip_frames, H0, W0, S)) return -1;
  return vt_layout(F, clip_frames, H0, W0, S, antialias != 0, autocontrast != 0).total;
}

extern "C" int maavss_video_transform(const void* src, const int32_t* boxes, const int32_t* host_boxes, float* out, void* ws, int64_t ws_bytes,
                                      int64_t F, int clip_frames, int H0, int W0, int S, float mean0, float mean1, float mean2, float std0,
                                      float std1, float std2, int antialias, int autocontrast, void* stream) {
  MAAVSS_CHECK_ARG(src && boxes && host_boxes && out && ws, "video_transform: null pointer");
  MAAVSS_CHECK_ARG(F > 0 && clip_frames > 0 && F % clip_frames == 0,
                   "video_transform: F (%lld) must be a positive multiple of clip_frames (%d)", (long long)F, clip_frames);
  MAAVSS_CHECK_ARG(S >= 8 && S % 4 == 0 && S <= 8192, "video_transform: output side S = %d must be >= 8 and a multiple of 4", S);
  MAAVSS_CHECK_ARG(vt_shape_ok(F, clip_frames, H0, W0, S), "video_transform: bad frame size %d x %d", H0, W0);
  MAAVSS_CHECK_ARG(std0 != 0.f && std1 != 0.f && std2 != 0.f, "video_transform: std must be non-zero");
  MAAVSS_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)ws & 15) == 0, "video_transform: out and ws must be 16-byte aligned");
  const int aa = antialias != 0, ac = autocontrast != 0;
  const VtLayout L = vt_layout(F, clip_frames, H0, W0, S, aa, ac);
  MAAVSS_CHECK_ARG(ws_bytes >= L.total, "video_transform: workspace of %lld bytes, needs %lld", (long long)ws_bytes, (long long)L.total);
  const int64_t nclips = F / clip_frames;
  MAAVSS_CHECK_ARG(nclips <= 65535, "video_transform: at most 65535 clips per call (got %lld)", (long long)nclips);
  for (int64_t c = 0; c < nclips; ++c) {
    const int32_t t = host_boxes[c * 4], l = host_boxes[c * 4 + 1], h = host_boxes[c * 4 + 2], w = host_boxes[c * 4 + 3];
    MAAVSS_CHECK_ARG(h >= 1 && w >= 1 && t >= 0 && l >= 0 && (int64_t)t + h <= H0 && (int64_t)l + w <= W0,
                     "video_transform: box %lld = (top %d, left %d, h %d, w %d) is not inside the %d x %d frame", (long long)c, t, l, h, w,
                     H0, W0);
  }
  const int bx = cdiv(S, VT_BX), by = cdiv(S, VT_BY * VT_ROWS);
  MAAVSS_CHECK_ARG((int64_t)bx * by * F < ((int64_t)1 << 31), "video_transform: grid too large");
  hipStream_t st = (hipStream_t)stream;
  char* w8 = (char*)ws;
  int32_t* ranges = (int32_t*)(w8 + L.ranges);
  float* wy = (float*)(w8 + L.wy);
  float* wx = (float*)(w8 + L.wx);
  int* keys = ac ? (int*)(w8 + L.keys) : nullptr;
  hipLaunchKernelGGL(video_transform_tables_kernel, dim3(cdiv(S, 256), (unsigned)nclips, 2), dim3(256), 0, st, boxes, ranges, wy, wx, H0, W0,
                     S, L.ty, L.tx, aa);
  MAAVSS_LAUNCH_CHECK("video_transform_tables_kernel");
  if (ac) {
    hipLaunchKernelGGL(video_transform_keys_init_kernel, dim3(cdiv(F * 6, 256)), dim3(256), 0, st, keys, F * 6);
    MAAVSS_LAUNCH_CHECK("video_transform_keys_init_kernel");
  }
  // a = 1 / (255 std), b = -mean / std: (x / 255 - mean) / std as one affine step on the interpolated byte values
  const float a0 = (float)(1.0 / (255.0 * std0)), a1 = (float)(1.0 / (255.0 * std1)), a2 = (float)(1.0 / (255.0 * std2));
  const float b0 = (float)(-(double)mean0 / std0), b1 = (float)(-(double)mean1 / std1), b2 = (float)(-(double)mean2 / std2);
  if (aa)
    hipLaunchKernelGGL(video_transform_kernel<0>, dim3((unsigned)(bx * by * F)), dim3(VT_BX, VT_BY), 0, st, (const uint8_t*)src, boxes, ranges,
                       wy, wx, out, keys, clip_frames, H0, W0, S, L.ty, L.tx, a0, a1, a2, b0, b1, b2);
  else
    hipLaunchKernelGGL(video_transform_kernel<2>, dim3((unsigned)(bx * by * F)), dim3(VT_BX, VT_BY), 0, st, (const uint8_t*)src, boxes, ranges,
                       wy, wx, out, keys, clip_frames, H0, W0, S, L.ty, L.tx, a0, a1, a2, b0, b1, b2);
  MAAVSS_LAUNCH_CHECK("video_transform_kernel");
  if (ac) {
    const int64_t n4 = F * 3 * S * S / 4;
    const int64_t grid = std::min<int64_t>(cdiv(n4, 256), 8192);
    hipLaunchKernelGGL(video_transform_autocontrast_kernel, dim3((unsigned)grid), dim3(256), 0, st, out, keys, n4, S * S / 4);
    MAAVSS_LAUNCH_CHECK("video_transform_autocontrast_kernel");
  }
  return MAAVSS_OK;
}
