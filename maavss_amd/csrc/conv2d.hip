// K10 (convolution part): the STFT encoder's Conv2d(k=(3,9), stride (sh,sw) in {1,2}^2, pad (1,pw), bias=False)
// layers (reference avse_model_final.py:98-102), forward / input gradient / weight gradient.
// 2 -> 4 -> 8 -> 16 (-> 16) channels on at most [128 x 257] maps: a few MFLOP per clip, direct kernels, latency-bound.
// One thread per POSITION with all output (input) channels in registers -- every loaded value feeds C FMAs against
// wave-uniform weights -- and a weight gradient whose blocks own a (ci, kh) row of 9 taps x all C_out; one thread per output
// ELEMENT, as the generic kernels of conv2d_gen.hip work, re-reads each input C times and cost 1.05 ms per step for 0.2 GFLOP.
// These are what maavss_conv2d_gen_{small,big,wgrad} launch when the call is such a layer (conv2d_geom.h); every other call
// runs the generic kernels.  In the terms of CGen the convolution's input x is the big map G (dense NCHW -- the network input
// x_stft [B,2,T_a,F] -- or dense NHWC), its output y the small map S (dense NHWC); weights stay in the reference layout
// [Co][Ci][3][9] = [Cs][Cb][3][9].
#include "conv2d_geom.h"

// the big map is dense (the launchers below check it): NHWC when its channel stride is 1, else NCHW
__device__ __forceinline__ int64_t big_index(const CGen& g, int b, int cb, int by, int bx) {
  return g.gsc == 1 ? (((int64_t)b * g.Hb + by) * g.Wb + bx) * g.Cb + cb : (((int64_t)b * g.Cb + cb) * g.Hb + by) * g.Wb + bx;
}

template <int CO>
__global__ __launch_bounds__(256) void conv2d_fwd_pos_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             float* __restrict__ y, CGen g) {
  // Weights in LDS as [ci][kh][kw][CO]: the CO weights of a tap are CO / 4 broadcast 16-byte reads.  Straight from global memory they were CO
  // scalar loads per tap -- 1.4 scalar-memory instructions per vector instruction, a quarter of the waves' cycles on the scalar unit
  // (profiles/r3_f_scalar_pmc.json).  Same FMA order: results unchanged.
  __shared__ __attribute__((aligned(16))) float wl[16 * 27 * CO];
  for (int i = threadIdx.x; i < g.Cb * 27 * CO; i += 256) {
    const int c = i % CO, t = i / CO;                  // t = ci * 27 + kh * 9 + kw
    wl[i] = w[(int64_t)c * g.Cb * 27 + t];
  }
  __syncthreads();
  const int64_t npos = (int64_t)g.B * g.Hs * g.Ws;
  for (int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x; pos < npos; pos += (int64_t)gridDim.x * 256) {
    const int ox = (int)(pos % g.Ws), oy = (int)((pos / g.Ws) % g.Hs), b = (int)(pos / ((int64_t)g.Ws * g.Hs));
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = 0.f;
    for (int ci = 0; ci < g.Cb; ++ci)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int iy = oy * g.sh + kh - 1;
        const bool oky = iy >= 0 && iy < g.Hb;
#pragma unroll
        for (int kw = 0; kw < 9; ++kw) {
          const int ix = ox * g.sw + kw - g.pw;
          float v = 0.f;
          if (oky && ix >= 0 && ix < g.Wb) v = x[big_index(g, b, ci, iy, ix)];
          const float4* wp = reinterpret_cast<const float4*>(wl + ((ci * 3 + kh) * 9 + kw) * CO);
#pragma unroll
          for (int c = 0; c < CO; c += 4) {
            const float4 w4 = wp[c / 4];
            acc[c] = fmaf(v, w4.x, acc[c]); acc[c + 1] = fmaf(v, w4.y, acc[c + 1]);
            acc[c + 2] = fmaf(v, w4.z, acc[c + 2]); acc[c + 3] = fmaf(v, w4.w, acc[c + 3]);
          }
        }
      }
    float4* yp = reinterpret_cast<float4*>(y + pos * CO);
#pragma unroll
    for (int c = 0; c < CO; c += 4) yp[c / 4] = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
  }
}

// one thread per INPUT position, all CI gradients in registers; dy rows read as float4
template <int CI>
__global__ __launch_bounds__(256) void conv2d_dgrad_pos_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                               float* __restrict__ dx, CGen g) {
  // weights in LDS as [kh][kw][co][CI] (see conv2d_fwd_pos_kernel): the CI weights of (tap, co) are CI / 4 broadcast reads (CI = 2: one 8-byte read)
  __shared__ __attribute__((aligned(16))) float wl[27 * 16 * CI];
  for (int i = threadIdx.x; i < 27 * g.Cs * CI; i += 256) {
    const int c = i % CI, co = (i / CI) % g.Cs, t = i / (CI * g.Cs);      // t = kh * 9 + kw
    wl[i] = w[((int64_t)co * CI + c) * 27 + t];
  }
  __syncthreads();
  const int64_t npos = (int64_t)g.B * g.Hb * g.Wb;
  for (int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x; pos < npos; pos += (int64_t)gridDim.x * 256) {
    const int ix = (int)(pos % g.Wb), iy = (int)((pos / g.Wb) % g.Hb), b = (int)(pos / ((int64_t)g.Wb * g.Hb));
    float acc[CI];
#pragma unroll
    for (int c = 0; c < CI; ++c) acc[c] = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ty = iy + 1 - kh;
      if (ty < 0 || ty % g.sh != 0) continue;
      const int oy = ty / g.sh;
      if (oy >= g.Hs) continue;
#pragma unroll
      for (int kw = 0; kw < 9; ++kw) {
        const int tx = ix + g.pw - kw;
        if (tx < 0 || tx % g.sw != 0) continue;
        const int ox = tx / g.sw;
        if (ox >= g.Ws) continue;
        const float4* dp = reinterpret_cast<const float4*>(dy + (((int64_t)b * g.Hs + oy) * g.Ws + ox) * g.Cs);
        for (int c4 = 0; c4 < g.Cs / 4; ++c4) {
          const float4 d = dp[c4];
          const float dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float* wp = wl + ((kh * 9 + kw) * g.Cs + c4 * 4 + e) * CI;
            if constexpr (CI % 4 == 0) {
#pragma unroll
              for (int c = 0; c < CI; c += 4) {
                const float4 w4 = *reinterpret_cast<const float4*>(wp + c);
                acc[c] = fmaf(dd[e], w4.x, acc[c]); acc[c + 1] = fmaf(dd[e], w4.y, acc[c + 1]);
                acc[c + 2] = fmaf(dd[e], w4.z, acc[c + 2]); acc[c + 3] = fmaf(dd[e], w4.w, acc[c + 3]);
              }
            } else {
#pragma unroll
              for (int c = 0; c < CI; ++c) acc[c] = fmaf(dd[e], wp[c], acc[c]);
            }
          }
        }
      }
    }
    float* xp = dx + pos * CI;
    if constexpr (CI % 4 == 0) {
#pragma unroll
      for (int c = 0; c < CI; c += 4) *reinterpret_cast<float4*>(xp + c) = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
    } else {
#pragma unroll
      for (int c = 0; c < CI; ++c) xp[c] = acc[c];
    }
  }
}

// partials[chunk][co][ci][27]; block = ((ci, kh), chunk): 9 taps x all CO accumulators per thread, x row values loaded once
template <int CO>
__global__ __launch_bounds__(256) void conv2d_wgrad_row_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ partials, CGen g, int64_t pos_per_chunk) {
  __shared__ float red[4][CO * 9];
  const int ci = blockIdx.x / 3, kh = blockIdx.x % 3;
  const int64_t npos = (int64_t)g.B * g.Hs * g.Ws;
  const int64_t p0 = (int64_t)blockIdx.y * pos_per_chunk, p1 = min(npos, p0 + pos_per_chunk);
  float acc[CO][9];
#pragma unroll
  for (int c = 0; c < CO; ++c)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[c][k] = 0.f;
  for (int64_t pos = p0 + threadIdx.x; pos < p1; pos += 256) {
    const int ox = (int)(pos % g.Ws), oy = (int)((pos / g.Ws) % g.Hs), b = (int)(pos / ((int64_t)g.Ws * g.Hs));
    const int iy = oy * g.sh + kh - 1;
    if (iy < 0 || iy >= g.Hb) continue;
    float xv[9];
#pragma unroll
    for (int kw = 0; kw < 9; ++kw) {
      const int ix = ox * g.sw + kw - g.pw;
      xv[kw] = (ix >= 0 && ix < g.Wb) ? x[big_index(g, b, ci, iy, ix)] : 0.f;
    }
    const float4* dp = reinterpret_cast<const float4*>(dy + pos * CO);
#pragma unroll
    for (int c4 = 0; c4 < CO / 4; ++c4) {
      const float4 d = dp[c4];
      const float dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int kw = 0; kw < 9; ++kw) acc[c4 * 4 + e][kw] = fmaf(dd[e], xv[kw], acc[c4 * 4 + e][kw]);
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CO; ++c)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float s = wave_sum(acc[c][k]);
      if (lane == 0) red[wv][c * 9 + k] = s;
    }
  __syncthreads();
  for (int i = threadIdx.x; i < CO * 9; i += 256) {
    const int co = i / 9, kw = i % 9;
    partials[((int64_t)blockIdx.y * CO * g.Cb + (int64_t)co * g.Cb + ci) * 27 + kh * 9 + kw] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
  }
}

// the row kernel's partials through chunk_sum16 (one thread per output walking up to 256 chunks serially was a chain of dependent
// loads: 60 us for the 216 weights of the first layer); fixed summation order: deterministic
__global__ __launch_bounds__(256) void conv2d_wgrad_reduce_kernel(const float* __restrict__ partials, float* __restrict__ dw, int n, int nchunk, int beta) {
  bool owner;
  int i;
  const float t = chunk_sum16(partials, n, nchunk, blockIdx.x * 16, owner, i);
  if (owner) dw[i] = beta ? dw[i] + t : t;
}

// ---- which calls the kernels above were written for.  Strides are compared with ==: a channel-padded map must not reach a
// kernel that stores float4 rows.
static bool dense_nhwc(int64_t sb, int64_t sy, int64_t sx, int64_t sc, int C, int H, int W) {
  return sc == 1 && sx == C && sy == (int64_t)W * C && sb == (int64_t)H * W * C;
}
static bool dense_nchw(int64_t sb, int64_t sy, int64_t sx, int64_t sc, int C, int H, int W) {
  return sx == 1 && sy == W && sc == (int64_t)H * W && sb == (int64_t)C * H * W;
}
// kernel (3,9), pad (1, pw <= 8), strides in {1,2}^2, the small map dense NHWC and of the size the convolution arithmetic gives
static bool k39_layer(const CGen& g) {
  return g.kh == 3 && g.kw == 9 && g.ph == 1 && g.pw <= 8 && (g.sh == 1 || g.sh == 2) && (g.sw == 1 || g.sw == 2) &&
         g.Hs == (g.Hb + 2 - 3) / g.sh + 1 && g.Ws == (g.Wb + 2 * g.pw - 9) / g.sw + 1 &&
         dense_nhwc(g.ssb, g.ssy, g.ssx, g.ssc, g.Cs, g.Hs, g.Ws);
}
static bool big_nhwc(const CGen& g) { return dense_nhwc(g.gsb, g.gsy, g.gsx, g.gsc, g.Cb, g.Hb, g.Wb); }
static bool big_nchw(const CGen& g) { return dense_nchw(g.gsb, g.gsy, g.gsx, g.gsc, g.Cb, g.Hb, g.Wb); }

bool conv2d_k39_small(const float* big, const float* w, float* small, const CGen& g, hipStream_t st) {
  if (!k39_layer(g) || !(big_nhwc(g) || big_nchw(g)) || g.Cb > 16) return false;      // LDS weight image: C_in <= 16
  const int64_t npos = (int64_t)g.B * g.Hs * g.Ws;
  const dim3 pgrid(min((int64_t)8192, (npos + 255) / 256));
  if (g.Cs == 4) hipLaunchKernelGGL(conv2d_fwd_pos_kernel<4>, pgrid, dim3(256), 0, st, big, w, small, g);
  else if (g.Cs == 8) hipLaunchKernelGGL(conv2d_fwd_pos_kernel<8>, pgrid, dim3(256), 0, st, big, w, small, g);
  else if (g.Cs == 16) hipLaunchKernelGGL(conv2d_fwd_pos_kernel<16>, pgrid, dim3(256), 0, st, big, w, small, g);
  else return false;
  return true;
}

bool conv2d_k39_big(const float* small, const float* w, float* big, const CGen& g, hipStream_t st) {
  if (!k39_layer(g) || !big_nhwc(g) || g.Cs > 16 || g.Cs % 4 != 0) return false;      // LDS weight image: C_out <= 16; dy rows as float4
  const int64_t npos = (int64_t)g.B * g.Hb * g.Wb;
  const dim3 pgrid(min((int64_t)8192, (npos + 255) / 256));
  if (g.Cb == 2) hipLaunchKernelGGL(conv2d_dgrad_pos_kernel<2>, pgrid, dim3(256), 0, st, small, w, big, g);
  else if (g.Cb == 4) hipLaunchKernelGGL(conv2d_dgrad_pos_kernel<4>, pgrid, dim3(256), 0, st, small, w, big, g);
  else if (g.Cb == 8) hipLaunchKernelGGL(conv2d_dgrad_pos_kernel<8>, pgrid, dim3(256), 0, st, small, w, big, g);
  else if (g.Cb == 16) hipLaunchKernelGGL(conv2d_dgrad_pos_kernel<16>, pgrid, dim3(256), 0, st, small, w, big, g);
  else return false;
  return true;
}

// blocks = (ci, kh) rows x chunks: as many chunks as fill the device, at least 1024 positions each
int conv2d_k39_wgrad_nchunk(const CGen& g) {
  if (!k39_layer(g) || !(big_nhwc(g) || big_nchw(g)) || !(g.Cs == 4 || g.Cs == 8 || g.Cs == 16)) return 0;
  const int64_t npos = (int64_t)g.B * g.Hs * g.Ws;
  int64_t n = 1536 / ((int64_t)g.Cb * 3);
  if (n < 1) n = 1;
  if (n > (npos + 1023) / 1024) n = (npos + 1023) / 1024;
  return (int)n;
}

void conv2d_k39_wgrad(const float* small, const float* big, float* dw, float* ws, const CGen& g, int nchunk, int beta, hipStream_t st) {
  const int64_t npos = (int64_t)g.B * g.Hs * g.Ws, ppc = (npos + nchunk - 1) / nchunk;
  const dim3 grid(g.Cb * 3, nchunk);
  if (g.Cs == 4) hipLaunchKernelGGL(conv2d_wgrad_row_kernel<4>, grid, dim3(256), 0, st, big, small, ws, g, ppc);
  else if (g.Cs == 8) hipLaunchKernelGGL(conv2d_wgrad_row_kernel<8>, grid, dim3(256), 0, st, big, small, ws, g, ppc);
  else hipLaunchKernelGGL(conv2d_wgrad_row_kernel<16>, grid, dim3(256), 0, st, big, small, ws, g, ppc);
  const int n = g.Cs * g.Cb * 27;
  hipLaunchKernelGGL(conv2d_wgrad_reduce_kernel, dim3(cdiv(n, 16)), dim3(256), 0, st, ws, dw, n, nchunk, beta);
}
