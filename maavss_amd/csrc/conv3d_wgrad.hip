// K8: weight gradient of the Conv3d(3,5,5) layers with C_in in {16,32,64}, narrow form, and the entry point of both forms.
//   dW = sum over positions of x^T . dy; the position is the MFMA K dimension, read from channels-last LDS tiles with ds_read_b64_tr_b16
//   (hardware transpose; scalar reads in f32 mode).  A workgroup owns one (kd,kh) and the 5 kw taps, walks a chunk of position tiles and writes a
//   partial; conv3d_wgrad_reduce_kernel sums the chunks (deterministic, no atomics) for this kernel and the wide one, conv3d_c1_wgrad_reduce_kernel for conv3d_c1.hip.
// maavss_conv3d_wgrad sends 16->32 and 32->64 (every mode) and 64->64 (bf16) to the wide kernel (conv3d_wgrad_wide.hip): on the shipped
// 16-bit path conv3d_wgrad_kernel runs 64->16 only; in the f32 (precise=True) and IEEE-half modes also 64->64.
#include "conv3d_tile.h"

// DY16: dy arrives already rounded to the MFMA operand format (bn_pool_act_bwd writes it as bf16): copied, not converted
template <int PRECISE, int CI, int CO, bool DY16 = false>
__global__ __launch_bounds__(256) void conv3d_wgrad_kernel(const float* __restrict__ x, const void* __restrict__ dy_,
                                                           float* __restrict__ partials, int BT, int T, int H, int W,
                                                           int Ho, int Wo, int pad, int tiles_x, int tiles_y,
                                                           int tiles_per_chunk, int nchunk) {
  using M = Mma<PRECISE>;
  using E = typename M::elem;
  constexpr int MT = CI / 16, NT = CO / 16, NPAIR = 5 * MT, PW = (NPAIR + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  E* xs = reinterpret_cast<E*>(smem);  // [16 rows][20 cols][CI]
  E* ds = xs + 16 * 20 * CI;           // [16][16][CO]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int G = lane >> 4, l16 = lane & 15;
  // XCD-aware mapping: the 15 (kd,kh) blocks of one chunk walk the SAME x / dy tiles; give them 15 consecutive
  // slots of one XCD so that 14 of the 15 reads hit that XCD's L2 (measured before: 14.3 GB fetched per launch).
  // Each XCD owns a contiguous eighth of the chunks, so chunks that re-read each other's frames (kd planes) share an L2.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int chunk = xcd * ((nchunk + 7) / 8) + slot / 15, tg = slot % 15;
  if (chunk >= nchunk) return;
  const int kd = tg / 5, kh = tg % 5;
  f32x4 acc[PW][NT];
#pragma unroll
  for (int p = 0; p < PW; ++p)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[p][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int tiles_total = BT * tiles_x * tiles_y;
  const int tile_beg = chunk * tiles_per_chunk;
  const int tile_end = min(tiles_total, tile_beg + tiles_per_chunk);
  for (int tile = tile_beg; tile < tile_end; ++tile) {
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, bt = tile / (tiles_x * tiles_y);
    const int t = bt % T, tt = t + kd - 1;
    if (tt < 0 || tt >= T) continue;  // block-uniform
    const int x0 = tx * 16, y0 = ty * 16;
    __syncthreads();
    const float* xp = x + (int64_t)(bt + kd - 1) * H * W * CI;
    for (int i = tid; i < 320 * (CI / 4); i += 256) {
      const int pos = i / (CI / 4), c4 = (i % (CI / 4)) * 4;
      const int r = pos / 20, c = pos % 20;
      const int iy = y0 + r + kh - pad, ix = x0 + c - pad;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const float4*>(xp + ((int64_t)iy * W + ix) * CI + c4);
      E* d = xs + pos * CI + c4;
      d[0] = M::cvt(v.x); d[1] = M::cvt(v.y); d[2] = M::cvt(v.z); d[3] = M::cvt(v.w);
    }
    if constexpr (DY16) {
      static_assert(PRECISE != MODE_F32, "16-bit dy needs a 16-bit MFMA mode");
      const unsigned short* dp = reinterpret_cast<const unsigned short*>(dy_) + (int64_t)bt * Ho * Wo * CO;
      for (int i = tid; i < 256 * (CO / 8); i += 256) {
        const int pos = i / (CO / 8), c8 = (i % (CO / 8)) * 8;
        const int oy = y0 + pos / 16, ox = x0 + pos % 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (oy < Ho && ox < Wo) v = *reinterpret_cast<const uint4*>(dp + ((int64_t)oy * Wo + ox) * CO + c8);
        *reinterpret_cast<uint4*>(ds + pos * CO + c8) = v;
      }
    } else {
      const float* dp = reinterpret_cast<const float*>(dy_) + (int64_t)bt * Ho * Wo * CO;
      for (int i = tid; i < 256 * (CO / 4); i += 256) {
        const int pos = i / (CO / 4), c4 = (i % (CO / 4)) * 4;
        const int oy = y0 + pos / 16, ox = x0 + pos % 16;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (oy < Ho && ox < Wo) v = *reinterpret_cast<const float4*>(dp + ((int64_t)oy * Wo + ox) * CO + c4);
        E* d = ds + pos * CO + c4;
        d[0] = M::cvt(v.x); d[1] = M::cvt(v.y); d[2] = M::cvt(v.z); d[3] = M::cvt(v.w);
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < 8; ++ks) {
      // K step = output rows 2ks, 2ks+1; k = 0..31 -> (row 2ks + k/16, col k%16)
      typename M::frag fb[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if constexpr (PRECISE == MODE_F32) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int k = 8 * G + e;
            const float v = ds[((2 * ks + (k >> 4)) * 16 + (k & 15)) * CO + j * 16 + l16];
            if (e < 4) fb[j].lo[e] = v; else fb[j].hi[e - 4] = v;
          }
        } else {
          bf16x4 h[2];
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            const int k = 8 * G + 4 * hh + (l16 >> 2);
            const E* a = ds + ((2 * ks + (k >> 4)) * 16 + (k & 15)) * CO + j * 16 + (l16 & 3) * 4;
            h[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)(a));
          }
          fb[j] = concat4(h[0], h[1]);
        }
      }
#pragma unroll
      for (int p = 0; p < PW; ++p) {
        const int q = wv + 4 * p;
        if (q < NPAIR) {  // wave-uniform
          const int kw = q / MT, mi = q % MT;
          typename M::frag fa;
          if constexpr (PRECISE == MODE_F32) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int k = 8 * G + e;
              const float v = xs[((2 * ks + (k >> 4)) * 20 + (k & 15) + kw) * CI + mi * 16 + l16];
              if (e < 4) fa.lo[e] = v; else fa.hi[e - 4] = v;
            }
          } else {
            bf16x4 h[2];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
              const int k = 8 * G + 4 * hh + (l16 >> 2);
              const E* a = xs + ((2 * ks + (k >> 4)) * 20 + (k & 15) + kw) * CI + mi * 16 + (l16 & 3) * 4;
              h[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)(a));
            }
            fa = concat4(h[0], h[1]);
          }
#pragma unroll
          for (int j = 0; j < NT; ++j) M::mma(acc[p][j], fa, fb[j]);
        }
      }
    }
  }
  // partials[chunk][tg][kw][ci][co]
  float* out = partials + ((int64_t)chunk * 15 + tg) * 5 * CI * CO;
#pragma unroll
  for (int p = 0; p < PW; ++p) {
    const int q = wv + 4 * p;
    if (q < NPAIR) {
      const int kw = q / MT, mi = q % MT;
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[((int64_t)kw * CI + mi * 16 + G * 4 + r) * CO + j * 16 + l16] = acc[p][j][r];
    }
  }
}

// dW[co][ci][kd][kh][kw] (+)= sum_chunk partials[chunk][kd*5+kh][kw][ci][co]
__global__ __launch_bounds__(256) void conv3d_wgrad_reduce_kernel(const float* __restrict__ partials, float* __restrict__ dw, int nchunk, int CI,
                                           int CO, int beta) {
  const int total = 75 * CI * CO;
  bool owner;
  int i;
  const float s = chunk_sum16(partials, total, nchunk, blockIdx.x * 16, owner, i);
  if (owner) {
    const int co = i % CO, ci = (i / CO) % CI, tap = i / (CO * CI);  // tap = (kd*5+kh)*5+kw
    float* d = dw + ((int64_t)co * CI + ci) * 75 + tap;
    *d = beta ? *d + s : s;
  }
}

__global__ __launch_bounds__(256) void conv3d_c1_wgrad_reduce_kernel(const float* __restrict__ partials, float* __restrict__ dw, int nchunk, int beta) {
  bool owner;
  int i;
  const float s = chunk_sum16(partials, 1200, nchunk, blockIdx.x * 16, owner, i);
  if (owner) dw[i] = beta ? dw[i] + s : s;
}
void conv3d_c1_wgrad_reduce(const float* ws, float* dw, int nchunk, int beta, hipStream_t st) {
  hipLaunchKernelGGL(conv3d_c1_wgrad_reduce_kernel, dim3(75), dim3(256), 0, st, ws, dw, nchunk, beta);
}

extern "C" int64_t maavss_conv3d_wgrad_ws_bytes(int c_in, int c_out, int nchunk) {
  return (int64_t)nchunk * 75 * c_in * c_out * 4;
}

template <int PRECISE, int CI, int CO, bool DY16 = false>
static void launch_wgrad(const float* x, const void* dy, float* ws, int BT, int T, int H, int W, int Ho, int Wo, int pad,
                         int nchunk, hipStream_t st) {
  using E = typename Mma<PRECISE>::elem;
  const size_t smem = (320 * CI + 256 * CO) * sizeof(E);
  auto kern = conv3d_wgrad_kernel<PRECISE, CI, CO, DY16>;
  if (smem > 64 * 1024) hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const int tiles_x = cdiv(Wo, 16), tiles_y = cdiv(Ho, 16);
  const int tiles_total = BT * tiles_x * tiles_y;
  const int tpc = cdiv(tiles_total, nchunk);
  hipLaunchKernelGGL(kern, dim3(15 * cdiv(nchunk, 8) * 8), dim3(256), smem, st, x, dy, ws, BT, T, H, W, Ho, Wo, pad, tiles_x,
                     tiles_y, tpc, nchunk);
}

extern "C" int maavss_conv3d_wgrad(const void* x_, const void* dy, float* dw, float* ws, int nchunk, int B, int T, int H,
                                   int W, int c_in, int c_out, int pad, int beta, int precise, int in16, void* stream) {
  const float* x = reinterpret_cast<const float*>(x_);
  const int dy16 = in16 & 1, x16 = (in16 >> 1) & 1;      // bit 0: dy is bf16, bit 1: x is bf16 too
  MAAVSS_CHECK_ARG(x && dy && dw && ws, "conv3d_wgrad: null pointer");
  MAAVSS_CHECK_ARG(in16 >= 0 && in16 <= 3, "conv3d_wgrad: in16 is a 2-bit mask (1: dy bf16, 2: x bf16)");
  MAAVSS_CHECK_ARG(!dy16 || precise == MODE_BF16, "conv3d_wgrad: a 16-bit dy is bf16 and needs precise = 0");
  MAAVSS_CHECK_ARG(!x16 || (dy16 && ((c_in == 16 && c_out == 32) || (c_in == 32 && c_out == 64) || (c_in == 64 && c_out == 64))),
                   "conv3d_wgrad: a bf16 x needs a bf16 dy and one of the shapes 16->32, 32->64, 64->64 (got %d->%d)", c_in, c_out);
  MAAVSS_CHECK_ARG(nchunk >= 1, "conv3d_wgrad: nchunk must be >= 1");
  MAAVSS_CHECK_ARG(precise >= 0 && precise <= 2, "conv3d_wgrad: mode must be 0 (bf16), 1 (f32) or 2 (f16)");
  const int Ho = H + 2 * pad - 4, Wo = W + 2 * pad - 4;
  MAAVSS_CHECK_ARG(Ho > 0 && Wo > 0 && B > 0 && T > 0, "conv3d_wgrad: empty output");
  hipStream_t st = (hipStream_t)stream;
  // the two large-M layers use the wide kernel (conv3d_wgrad_wide.hip): every tile staged once / three times
  if (maavss_conv3d_wgrad_wide_try(x, dy, ws, nchunk, B, T, H, W, Ho, Wo, c_in, c_out, pad, precise, dy16, x16, st)) {
    MAAVSS_LAUNCH_CHECK("conv3d_wgrad_wide_kernel");
    hipLaunchKernelGGL(conv3d_wgrad_reduce_kernel, dim3(cdiv(75 * c_in * c_out, 16)), dim3(256), 0, st, ws, dw, nchunk, c_in,
                       c_out, beta);
    MAAVSS_LAUNCH_CHECK("conv3d_wgrad_reduce_kernel");
    return MAAVSS_OK;
  }
#define CASE(CI, CO)                                                                         \
  if (c_in == CI && c_out == CO) {                                                           \
    if (precise == MODE_F32) launch_wgrad<MODE_F32, CI, CO>(x, dy, ws, B * T, T, H, W, Ho, Wo, pad, nchunk, st);      \
    else if (precise == MODE_F16) launch_wgrad<MODE_F16, CI, CO>(x, dy, ws, B * T, T, H, W, Ho, Wo, pad, nchunk, st); \
    else if (dy16) launch_wgrad<MODE_BF16, CI, CO, true>(x, dy, ws, B * T, T, H, W, Ho, Wo, pad, nchunk, st);        \
    else launch_wgrad<MODE_BF16, CI, CO>(x, dy, ws, B * T, T, H, W, Ho, Wo, pad, nchunk, st);                        \
    MAAVSS_LAUNCH_CHECK("conv3d_wgrad_kernel");                                              \
    hipLaunchKernelGGL(conv3d_wgrad_reduce_kernel, dim3(cdiv(75 * CI * CO, 16)), dim3(256), 0, st, ws, dw, nchunk, CI, CO, beta); \
    MAAVSS_LAUNCH_CHECK("conv3d_wgrad_reduce_kernel");                                       \
    return MAAVSS_OK;                                                                        \
  }
  CASE(16, 32) CASE(32, 64) CASE(64, 64) CASE(64, 16)
#undef CASE
  maavss_set_error("conv3d_wgrad: unsupported channels %d -> %d", c_in, c_out);
  return MAAVSS_ERR_ARG;
}
