// K7: forward and input gradient of the Conv3d(k=(3,5,5), stride 1, pad (1,p,p), bias=False) layers with C_in in {16,32,64} of the visual encoder
// (reference avse_model_final.py:39,44,49,54), as an implicit GEMM on MFMA.  Activations are channels-last [B,T,H,W,C].  One workgroup = a
// 16-wide, 14- or 16-high tile of output positions of one (b,t) plane x all C_out; per kd the 20x20xC_in input halo is staged once into LDS
// (swizzled 16-byte chunks) and re-read for the 25 (kh,kw) taps.  The input gradient is the same kernel on flipped / transposed weights, pad 4-p.
//   conv3d_prep_w_kernel    weight re-layout for either direction, in the operand format
//   conv3d_igemm16_kernel   the shipped 16-bit path (bf16 / IEEE-half operands, f32 or 16-bit x): unrolled K steps, weight tiles by LDS-DMA
//                           into a ring of four
//   conv3d_igemm_kernel     the exact-f32 form (precise=True): f32 LDS images, weight tiles through registers into a double buffer
// The first layer (C_in = 1) is conv3d_c1.hip, the weight gradients are conv3d_wgrad.hip and conv3d_wgrad_wide.hip.
#include <type_traits>
#include <utility>
#include "conv3d_tile.h"

// --------------------------------------------------------------------------------------------
// weight re-layout: reference [CO][CI][3][5][5] f32  ->  wt[kd][n][KP] (k = (kh*5+kw)*CIN + ci), elem type.
//   mode 0 (forward): n = co, CIN = CI, value W[co][ci][kd][kh][kw]
//   mode 1 (dgrad)  : n = ci, CIN = CO, value W[co][ci][2-kd][4-kh][4-kw]
template <int PRECISE>
__global__ void conv3d_prep_w_kernel(const float* __restrict__ w, typename Mma<PRECISE>::elem* __restrict__ wt, int CO, int CI,
                                     int KP, int mode) {
  const int nN = mode ? CI : CO, cin = mode ? CO : CI;
  const int64_t total = 3LL * nN * KP;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int kk = (int)(i % KP);
    const int n = (int)((i / KP) % nN);
    const int kd = (int)(i / ((int64_t)KP * nN));
    float v = 0.f;
    if (kk < 25 * cin) {
      const int tap = kk / cin, c = kk % cin, kh = tap / 5, kw = tap % 5;
      if (!mode) v = w[(((int64_t)n * CI + c) * 3 + kd) * 25 + kh * 5 + kw];
      else v = w[(((int64_t)c * CI + n) * 3 + (2 - kd)) * 25 + (4 - kh) * 5 + (4 - kw)];
    }
    wt[i] = Mma<PRECISE>::cvt(v);
  }
}

// The exact-f32 implicit GEMM (precise = MODE_F32; the 16-bit modes are conv3d_igemm16_kernel below): x, the weights and the LDS images
// are f32, a 32-deep K step is eight v_mfma_f32_16x16x4_f32 (mma.h).  Per kd the 20x20xC_in halo is staged once; the weight tiles of
// 64 k go global -> registers -> LDS one chunk ahead of their use, into a double buffer.
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void conv3d_igemm_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                           float* __restrict__ y, float* __restrict__ stat_partials,
                                                           int n_bt, int T, int H, int W, int Ho, int Wo, int pad, int KP, int th) {
  using M = Mma<MODE_F32>;
  constexpr int EPC = 4;                              // f32 elements per 16-byte chunk
  constexpr int RBH = CIN * 4, NCH = RBH / 16;        // halo: bytes / chunks per position
  constexpr int RBW = 64 * 4, NCW = RBW / 16;         // weight tile: bytes / chunks per row (64 k)
  constexpr int NT = COUT / 16;
  constexpr int NCHUNK = (25 * CIN + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* halo = reinterpret_cast<float*>(smem);                 // [20*20][CIN] swizzled
  float* wl = halo + 400 * CIN;                                 // [2][COUT][64] swizzled
  float* red = wl + 2 * COUT * 64;                              // [4][2][COUT] stats scratch

  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l16 = lane & 15;
  const int ny = (Ho + th - 1) / th;
  const TileId tile = xcd_tile((Wo + 15) / 16, ny, (int64_t)((Wo + 15) / 16) * ny * n_bt);
  if (!tile.valid) return;
  const int x0 = tile.tx * 16, y0 = tile.ty * th;
  const int row0 = tile_row0(wv, th);
  const bool four = tile_nrows(wv, th) == 4;      // wave-uniform: the wave's fourth row exists
  const int hpos = (th + 4) * 20;                 // halo positions of a tile
  const int bt = tile.bt, t = bt % T;
  f32x4 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- halo staging.  C_in = 64: the 25 float4 of a thread's share of the NEXT frame's halo are requested before this
  // frame's MFMAs and written to LDS after them (register prefetch).  With a plain load -> store
  // loop one load is in flight per thread: 25 dependent round trips per frame, and these variants run only two
  // workgroups per CU (60 - 70 KB of LDS each), too few to cover that; the same LDS limit leaves 256 VGPRs per lane,
  // so the 100 staging registers are free.  (Scratch build without the halo loads: igemm 4.3 -> 2.9 ms per step.)
  // The smaller C_in variants run 3 - 5 workgroups per CU and keep the plain loop (batched loads cost them occupancy).
  constexpr int HV = 400 * (CIN / 4), NV = (HV + 255) / 256;
  constexpr bool PREFETCH = CIN >= 64;
  float4 hv[PREFETCH ? NV : 1];
  auto fetch = [&](int kd) __attribute__((always_inline)) {
    const int64_t plane = (int64_t)(bt + kd - 1) * H * W * CIN;
    int tv = tid;
    asm volatile("" : "+v"(tv));   // the index arithmetic is redone per call: hoisted out of the kd loop it costs 100+ registers
#pragma unroll
    for (int j = 0; j < (PREFETCH ? NV : 1); ++j) {
      const int i = tv + j * 256;
      const int pos = i / (CIN / 4), cv = (i % (CIN / 4)) * 4;
      const int r = pos / 20, c = pos % 20;
      const int iy = y0 + r - pad, ix = x0 + c - pad;
      hv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < HV && iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const int64_t e = plane + ((int64_t)iy * W + ix) * CIN + cv;
        hv[j] = *reinterpret_cast<const float4*>(x + e);
      }
    }
  };
  auto stash = [&]() __attribute__((always_inline)) {
    int tv = tid;
    asm volatile("" : "+v"(tv));
#pragma unroll
    for (int j = 0; j < (PREFETCH ? NV : 1); ++j) {
      const int i = tv + j * 256;
      if (i < HV) {
        const int pos = i / (CIN / 4), cv = (i % (CIN / 4)) * 4, c = pos % 20;
        float* d = halo + (pos * NCH + swz<RBH>(c, cv / EPC)) * EPC;
        d[0] = hv[j].x; d[1] = hv[j].y; d[2] = hv[j].z; d[3] = hv[j].w;
      }
    }
  };
  const int kd_lo = t == 0 ? 1 : 0, kd_hi = t == T - 1 ? 1 : 2;   // frames t + kd - 1 inside the clip (block-uniform)
  if constexpr (PREFETCH) fetch(kd_lo);
  for (int kd = kd_lo; kd <= kd_hi; ++kd) {
    __syncthreads();
    // ---- stage the 20x20xC_in halo of frame t + kd - 1 (zero-filled outside the image)
    if constexpr (PREFETCH) {
      stash();
    } else {
      const float* xp = x + (int64_t)(bt + kd - 1) * H * W * CIN;
      for (int i = tid; i < hpos * (CIN / 4); i += 256) {
        const int pos = i / (CIN / 4), c4 = (i % (CIN / 4)) * 4;
        const int r = pos / 20, c = pos % 20;
        const int iy = y0 + r - pad, ix = x0 + c - pad;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const float4*>(xp + ((int64_t)iy * W + ix) * CIN + c4);
        float* d = halo + (pos * NCH + swz<RBH>(c, c4 / EPC)) * EPC;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    }
    // ---- weight chunks of this kd: the 16-byte piece c of row n of chunk q starts at k = 64 q + 4 c
    const float* wk = wt + (int64_t)kd * COUT * KP;
    auto wsrc = [&](int i, int q) __attribute__((always_inline)) { return wk + (int64_t)(i / NCW) * KP + q * 64 + (i % NCW) * EPC; };
    constexpr int WV = (COUT * NCW + 255) / 256;
    for (int i = tid; i < COUT * NCW; i += 256) {
      const int n = i / NCW, c = i % NCW;
      *reinterpret_cast<uint4*>(wl + (n * NCW + swz<RBW>(n, c)) * EPC) = *reinterpret_cast<const uint4*>(wsrc(i, 0));
    }
    __syncthreads();
    if constexpr (PREFETCH) {
      if (kd < kd_hi) fetch(kd + 1);
    }
    for (int ch = 0; ch < NCHUNK; ++ch) {
      // the next chunk's tile, global -> registers; unconditional (clamped) loads keep wreg in registers: a conditionally written
      // array lands in scratch
      uint4 wreg[WV];
      const int chn = ch + 1 < NCHUNK ? ch + 1 : ch;
#pragma unroll
      for (int v = 0; v < WV; ++v) {
        int i = v * 256 + tid;
        i = i < COUT * NCW ? i : 0;
        wreg[v] = *reinterpret_cast<const uint4*>(wsrc(i, chn));
      }
      const float* wb = wl + (ch & 1) * COUT * 64;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int kk = ch * 64 + s * 32 + 8 * g;
        int tap = kk / CIN;
        const int ci = kk % CIN;
        tap = tap > 24 ? 24 : tap;  // padded tail: weights are zero there
        const int kh = tap / 5, kw = tap % 5;
        M::frag fa[4], fb[NT];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = row0 + i + kh, c = l16 + kw;
          const float* base = halo + (r * 20 + c) * NCH * EPC;
          fa[i].lo = *reinterpret_cast<const f32x4*>(base + swz<RBH>(c, ci / EPC) * EPC);
          fa[i].hi = *reinterpret_cast<const f32x4*>(base + swz<RBH>(c, ci / EPC + 1) * EPC);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int n = j * 16 + l16;
          const float* base = wb + n * 64;
          const int c0 = (s * 32 + 8 * g) / EPC;
          fb[j].lo = *reinterpret_cast<const f32x4*>(base + swz<RBW>(n, c0) * EPC);
          fb[j].hi = *reinterpret_cast<const f32x4*>(base + swz<RBW>(n, c0 + 1) * EPC);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < 3 || four) {
#pragma unroll
            for (int j = 0; j < NT; ++j) M::mma(acc[i][j], fa[i], fb[j]);
          }
      }
      if (ch + 1 < NCHUNK) {
        float* wn = wl + ((ch + 1) & 1) * COUT * 64;
#pragma unroll
        for (int v = 0; v < WV; ++v) {
          const int i = v * 256 + tid;
          if (i < COUT * NCW) {
            const int n = i / NCW, c = i % NCW;
            *reinterpret_cast<uint4*>(wn + (n * NCW + swz<RBW>(n, c)) * EPC) = wreg[v];
          }
        }
      }
      __syncthreads();
    }
  }
  // ---- epilogue: store + optional per-block BatchNorm partial sums (sum, sum of squares per channel)
  float* yp = y + (int64_t)bt * Ho * Wo * COUT;
  float s1[NT], s2[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) s1[j] = s2[j] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int oy = y0 + row0 + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ox = x0 + g * 4 + r;
      if ((i < 3 || four) && oy < Ho && ox < Wo) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const float v = acc[i][j][r];
          yp[((int64_t)oy * Wo + ox) * COUT + j * 16 + l16] = v;
          s1[j] += v;
          s2[j] += v * v;
        }
      }
    }
  }
  if (stat_partials != nullptr) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      s1[j] = rows4_sum(s1[j]);
      s2[j] = rows4_sum(s2[j]);
      if (g == 0) {
        red[(wv * 2 + 0) * COUT + j * 16 + l16] = s1[j];
        red[(wv * 2 + 1) * COUT + j * 16 + l16] = s2[j];
      }
    }
    __syncthreads();
    if (tid < 2 * COUT) {
      const float v = red[tid] + red[2 * COUT + tid] + red[4 * COUT + tid] + red[6 * COUT + tid];
      stat_partials[tile.lin * 2 * COUT + tid] = v;
    }
  }
}

template <int CIN, int COUT>
static int launch_igemm(const void* x, const void* wt, float* y, float* stats, int B, int T, int H, int W, int Ho,
                        int Wo, int pad, int KP, hipStream_t st) {
  const int th = maavss_conv_tile_h(Ho);
  const size_t smem = (400 * CIN + 2 * COUT * 64 + 8 * COUT) * sizeof(float);      // halo, two weight tiles, stats scratch
  auto kern = conv3d_igemm_kernel<CIN, COUT>;
  if (smem > 64 * 1024) hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const int64_t tiles = (int64_t)cdiv(Wo, 16) * cdiv(Ho, th) * B * T;
  hipLaunchKernelGGL(kern, dim3(xcd_grid(tiles)), dim3(256), smem, st, reinterpret_cast<const float*>(x), reinterpret_cast<const float*>(wt), y, stats,
                     B * T, T, H, W, Ho, Wo, pad, KP, th);
  return 0;
}

// f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{}): a loop whose index is a compile-time constant in the body
template <class F, int... S>
__device__ __forceinline__ void static_for_impl(F& f, std::integer_sequence<int, S...>) { (f(std::integral_constant<int, S>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// --------------------------------------------------------------------------------------------
// The 16-bit modes of the implicit GEMM (round 4): the tile, the K order (kd, 32-channel half of a 64-channel input, tap, channel), the halo
// image and the epilogue of conv3d_igemm_kernel, with the inner loop rebuilt around what its counters showed (35-45 % matrix-pipe busy, 3-4.5
// vector instructions per MFMA, waves waiting 45-64 % of their cycles; profiles/r3_e_kernel_pmc.json):
//   * the 13 / 25 K steps of a halo stage are unrolled with the tap as a compile-time constant: a lane keeps one swizzled byte offset per
//     kw (32-channel stages) or one offset + a per-step select (16-channel stages: a 32-deep step spans two taps), the row / tap part is the
//     ds_read's immediate -- no address arithmetic in the loop;
//   * the fragments of step t + 1 are read before the MFMAs of step t (two register sets);
//   * the weight chunks (64 k) go global -> LDS by DMA into a ring of four tiles, requested three chunks ahead, so the fragments of the next
//     chunk can be read before the barrier that ends this one and a request has two chunks of time to land; the barrier waits for the
//     request before the newest only.
template <int PRECISE, int CIN, int COUT, bool IN16>
__global__ __launch_bounds__(256) void conv3d_igemm16_kernel(const void* __restrict__ x_, const typename Mma<PRECISE>::elem* __restrict__ wt,
                                                             float* __restrict__ y, float* __restrict__ stat_partials, int n_bt, int T, int H,
                                                             int W, int Ho, int Wo, int pad, int KP, int th) {
  using M = Mma<PRECISE>;
  using E = typename M::elem;
  static_assert(PRECISE != MODE_F32 && sizeof(E) == 2, "16-bit MFMA modes only");
  constexpr int CH = CIN == 64 ? 32 : CIN;            // channels per halo stage
  constexpr int NH = CIN / CH;                        // halo stages per kd plane
  constexpr int PB = CH * 2;                          // bytes per halo position
  constexpr int NCH = PB / 16;                        // 16-byte chunks per halo position
  constexpr int NT = COUT / 16;
  constexpr int STEPS = (25 * CH + 31) / 32;          // 32-deep K steps per stage: 13 (two taps each, the last half phantom) or 25 (one tap each)
  constexpr int NCHUNK = (STEPS + 1) / 2;             // 64-k weight chunks per stage
  constexpr int WB = COUT * 128;                      // bytes of one weight tile [COUT][64]
  constexpr int WV = (COUT * 8 + 255) / 256;          // 16-byte pieces of a weight tile per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* halo = smem;                                  // [400][PB], chunk-swizzled (swz_halo)
  constexpr int RING = 4;
  char* ring = smem + 400 * PB;                       // [RING][COUT][128 B], chunk ^= (n >> 1) & 7
  float* red = reinterpret_cast<float*>(ring + RING * WB);
  const float* x = reinterpret_cast<const float*>(x_);
  const unsigned short* x16 = reinterpret_cast<const unsigned short*>(x_);

  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l16 = lane & 15;
  const int ny = (Ho + th - 1) / th;
  const TileId tile = xcd_tile((Wo + 15) / 16, ny, (int64_t)((Wo + 15) / 16) * ny * n_bt);
  if (!tile.valid) return;
  const int x0 = tile.tx * 16, y0 = tile.ty * th;
  const int row0 = tile_row0(wv, th);
  const bool four = tile_nrows(wv, th) == 4;      // wave-uniform: the wave's fourth row exists
  const int hpos = (th + 4) * 20;                 // halo positions of a tile
  const int bt = tile.bt, t = bt % T;
  f32x4 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- per-lane LDS byte offsets.  A (halo): position (row 4 wv + i + kh, column l16 + kw), chunk = the lane's 8 channels
  unsigned a_off[CH == 32 ? 5 : 1];
  if constexpr (CH == 32) {
#pragma unroll
    for (int kw = 0; kw < 5; ++kw) {
      const int c = l16 + kw;
      a_off[kw] = (unsigned)(((row0 * 20 + c) * NCH + swz_halo<PB, 2>(c, g)) * 16);
    }
  } else {
    a_off[0] = (unsigned)(((row0 * 20 + l16) * NCH + (g & 1)) * 16);      // + tap offset of the lane's half of the step
  }
  // B (weight tile): row n = 16 j + l16, chunk 4 s + g of the row, swizzled with (n >> 1) & 7 = (l16 >> 1) & 7
  unsigned b_off[2];
#pragma unroll
  for (int sp = 0; sp < 2; ++sp) b_off[sp] = (unsigned)((l16 * 8 + ((sp * 4 + g) ^ ((l16 >> 1) & 7))) * 16);

  typename M::frag fa[2][4], fb[2][NT];
  // fragments of step `st` (compile-time) of the current stage into register set `set`; `slot_b` = byte offset of the ring tile of its chunk
  auto load_frags = [&](auto st_c, int set, unsigned slot_b) __attribute__((always_inline)) {
    constexpr int st = decltype(st_c)::value;
    unsigned ab;
    int imm;                                           // compile-time part of the A address (rows / taps)
    if constexpr (CH == 32) {
      constexpr int kh = st / 5, kw = st % 5;
      ab = a_off[kw];
      imm = kh * 20 * PB;
    } else {
      constexpr int t0 = 2 * st, t1 = 2 * st + 1 > 24 ? 24 : 2 * st + 1;       // tap 25 is the zero tail of the weight rows
      constexpr int o0 = ((t0 / 5) * 20 + t0 % 5) * PB, o1 = ((t1 / 5) * 20 + t1 % 5) * PB;
      ab = a_off[0] + (g >= 2 ? (unsigned)o1 : (unsigned)o0);
      imm = 0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[set][i] = *reinterpret_cast<const typename M::frag*>(halo + ab + imm + i * 20 * PB);
    const unsigned bb = slot_b + b_off[st & 1];
#pragma unroll
    for (int j = 0; j < NT; ++j) fb[set][j] = *reinterpret_cast<const typename M::frag*>(ring + bb + j * 16 * 128);
  };
  auto mfmas = [&](int set) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < 3 || four) {       // (the fourth row's fragment is read either way: inside the 20-row halo allocation)
#pragma unroll
        for (int j = 0; j < NT; ++j) M::mma(acc[i][j], fa[set][i], fb[set][j]);
      }
  };

  // ---- weight tiles by LDS-DMA: piece i of a tile = 16 bytes, lane-linear destination (row n = i / 8, PHYSICAL chunk i % 8): the swizzle is
  // applied on the source side
  const int kd_lo = t == 0 ? 1 : 0, kd_hi = t == T - 1 ? 1 : 2;   // frames t + kd - 1 inside the clip (block-uniform)
  auto wdma = [&](const E* wk, int hh, int q, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < WV; ++v) {
      const int i = v * 256 + tid;
      if (WV * 256 == COUT * 8 || i < COUT * 8) {
        const int n = i >> 3, c = (i & 7) ^ ((n >> 1) & 7);
        const E* src = CIN == 64 ? wk + (int64_t)n * KP + (2 * q + (c >> 2)) * 64 + hh * 32 + (c & 3) * 8 : wk + (int64_t)n * KP + q * 64 + c * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(ring + slot * WB + (int64_t)i * 16), 16, 0, 0);
      }
    }
  };

  for (int kd = kd_lo; kd <= kd_hi; ++kd)
  for (int hh = 0; hh < NH; ++hh) {
    // (every wave is past its last read of the previous stage's halo and ring: the barrier that ended its last chunk)
    // ---- halo of frame t + kd - 1, channels [hh CH, hh CH + CH), zero outside the image
    if constexpr (IN16) {
      // LDS-DMA, 16 B per lane, lane-linear destination: the swizzle is applied on the SOURCE side (XOR: its own inverse); positions outside
      // the image read the zero tail of weight row 0 (k >= 25 C_in: maavss_conv3d_kp leaves at least 64 bytes)
      const unsigned short* xp = x16 + (int64_t)(bt + kd - 1) * H * W * CIN + hh * CH;
      const unsigned short* zeros = reinterpret_cast<const unsigned short*>(wt) + 25 * CIN;
      int tv = tid;
      asm volatile("" : "+v"(tv));   // the index arithmetic is redone per stage: hoisted out of the stage loop it costs 60 registers
      for (int i0 = 0; i0 < hpos * NCH; i0 += 256) {
        const int i = i0 + tv;
        if (i < hpos * NCH) {
          const int pos = i / NCH, pc = i % NCH;
          const int r = pos / 20, c = pos % 20;
          const int iy = y0 + r - pad, ix = x0 + c - pad;
          const unsigned short* src = zeros;
          if (iy >= 0 && iy < H && ix >= 0 && ix < W) src = xp + ((int64_t)iy * W + ix) * CIN + swz_halo<PB, 2>(c, pc) * 8;
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                           (__attribute__((address_space(3))) void*)(halo + (int64_t)i * 16), 16, 0, 0);
        }
      }
    } else {
      const float* xp = x + (int64_t)(bt + kd - 1) * H * W * CIN + hh * CH;
      int tv = tid;
      asm volatile("" : "+v"(tv));
      for (int i = tv; i < hpos * (CH / 4); i += 256) {
        const int pos = i / (CH / 4), c4 = (i % (CH / 4)) * 4;
        const int r = pos / 20, c = pos % 20;
        const int iy = y0 + r - pad, ix = x0 + c - pad;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const float4*>(xp + ((int64_t)iy * W + ix) * CIN + c4);
        E* d = reinterpret_cast<E*>(halo + (pos * NCH + swz_halo<PB, 2>(c, c4 / 8)) * 16) + (c4 % 8);
        d[0] = M::cvt(v.x); d[1] = M::cvt(v.y); d[2] = M::cvt(v.z); d[3] = M::cvt(v.w);
      }
    }
    // ---- weight chunks 0 .. 2 of the stage into ring tiles 0 .. 2
    const E* wk = wt + (int64_t)kd * COUT * KP;
    wdma(wk, hh, 0, 0);
    if (NCHUNK > 1) wdma(wk, hh, 1, 1);
    if (NCHUNK > 2) wdma(wk, hh, 2, 2);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // halo (DMA or stores) and the three tiles have landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    load_frags(std::integral_constant<int, 0>{}, 0, 0u);
    __builtin_amdgcn_sched_barrier(0);
    // ---- the K steps of the stage.  Chunk c + 3 is requested when chunk c starts (its tile was chunk c - 1's: every wave is past the barrier
    // that ended it) and has to be visible when chunk c + 1 ends (the fragments of chunk c + 2's first step are read there): two chunks of time.
    auto step = [&](auto st_c) __attribute__((always_inline)) {
      constexpr int st = decltype(st_c)::value;
      constexpr int c = st / 2;                        // chunk of this step
      if constexpr ((st & 1) == 0 && c + 3 < NCHUNK) wdma(wk, hh, c + 3, (c + 3) % RING);
      if constexpr (st + 1 < STEPS) load_frags(std::integral_constant<int, st + 1>{}, (st + 1) & 1, (unsigned)((((st + 1) / 2) % RING) * WB));
      __builtin_amdgcn_sched_barrier(0);
      mfmas(st & 1);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr ((st & 1) || st + 1 == STEPS) {     // the chunk ends: chunk c + 2 has landed (chunk c + 3 may stay in flight)
        if constexpr (c + 3 < NCHUNK) {
          if constexpr (WV == 2) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    };
    static_for<STEPS>(step);
  }
  // ---- epilogue: store + optional per-block BatchNorm partial sums (sum, sum of squares per channel)
  float* yp = y + (int64_t)bt * Ho * Wo * COUT;
  float s1[NT], s2[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) s1[j] = s2[j] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int oy = y0 + row0 + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ox = x0 + g * 4 + r;
      if ((i < 3 || four) && oy < Ho && ox < Wo) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const float v = acc[i][j][r];
          yp[((int64_t)oy * Wo + ox) * COUT + j * 16 + l16] = v;
          s1[j] += v;
          s2[j] += v * v;
        }
      }
    }
  }
  if (stat_partials != nullptr) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      s1[j] = rows4_sum(s1[j]);
      s2[j] = rows4_sum(s2[j]);
      if (g == 0) {
        red[(wv * 2 + 0) * COUT + j * 16 + l16] = s1[j];
        red[(wv * 2 + 1) * COUT + j * 16 + l16] = s2[j];
      }
    }
    __syncthreads();
    if (tid < 2 * COUT) {
      const float v = red[tid] + red[2 * COUT + tid] + red[4 * COUT + tid] + red[6 * COUT + tid];
      stat_partials[tile.lin * 2 * COUT + tid] = v;
    }
  }
}

template <int PRECISE, int CIN, int COUT, bool IN16>
static int launch_igemm16(const void* x, const void* wt, float* y, float* stats, int B, int T, int H, int W, int Ho, int Wo, int pad, int KP,
                          hipStream_t st) {
  {
    using E = typename Mma<PRECISE>::elem;
    const size_t smem = 400 * (CIN == 64 ? 32 : CIN) * 2 + 4 * COUT * 128 + 8 * COUT * sizeof(float);
    auto kern = conv3d_igemm16_kernel<PRECISE, CIN, COUT, IN16>;
    if (smem > 64 * 1024) hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    const int th = maavss_conv_tile_h(Ho);
    const int64_t tiles = (int64_t)cdiv(Wo, 16) * cdiv(Ho, th) * B * T;
    hipLaunchKernelGGL(kern, dim3(xcd_grid(tiles)), dim3(256), smem, st, x, reinterpret_cast<const E*>(wt), y, stats, B * T, T, H, W, Ho, Wo, pad, KP, th);
    return 0;
  }
}

// padded K of a weight row: a multiple of 64 that leaves at least 32 zero elements (64 bytes) behind the 25 C_in real ones -- the zero source of
// the halo LDS-DMA and the phantom tap of the split-halo variants
extern "C" int maavss_conv3d_kp(int c_in) { return ((25 * c_in + 32 + 63) / 64) * 64; }

extern "C" int maavss_conv3d_prep_weights(const float* w, void* wt, int c_out, int c_in, int mode, int precise, void* stream) {
  MAAVSS_CHECK_ARG(w && wt, "conv3d_prep_weights: null pointer");
  const int cin = mode ? c_out : c_in, nN = mode ? c_in : c_out;
  const int KP = maavss_conv3d_kp(cin);
  const int64_t total = 3LL * nN * KP;
  dim3 grid(min(1024, cdiv(total, 256)));
  MAAVSS_CHECK_ARG(precise >= 0 && precise <= 2, "conv3d_prep_weights: mode must be 0 (bf16), 1 (f32) or 2 (f16)");
  if (precise == MODE_F32) hipLaunchKernelGGL(conv3d_prep_w_kernel<MODE_F32>, grid, dim3(256), 0, (hipStream_t)stream, w, (float*)wt, c_out, c_in, KP, mode);
  else if (precise == MODE_F16) hipLaunchKernelGGL(conv3d_prep_w_kernel<MODE_F16>, grid, dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)wt, c_out, c_in, KP, mode);
  else hipLaunchKernelGGL(conv3d_prep_w_kernel<MODE_BF16>, grid, dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)wt, c_out, c_in, KP, mode);
  MAAVSS_LAUNCH_CHECK("conv3d_prep_w_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_conv3d_igemm(const void* x, const void* wt, float* y, float* stat_partials, int B, int T, int H,
                                   int W, int c_in, int c_out, int pad, int precise, int x16, void* stream) {
  MAAVSS_CHECK_ARG(x && wt && y, "conv3d_igemm: null pointer");
  MAAVSS_CHECK_ARG(!x16 || precise != MODE_F32, "conv3d_igemm: 16-bit input needs precise = 0 (bf16) or 2 (f16)");
  MAAVSS_CHECK_ARG(pad >= 0 && pad <= 4, "conv3d_igemm: pad must be in [0,4]");
  MAAVSS_CHECK_ARG(precise >= 0 && precise <= 2, "conv3d_igemm: mode must be 0 (bf16), 1 (f32) or 2 (f16)");
  const int Ho = H + 2 * pad - 4, Wo = W + 2 * pad - 4;
  MAAVSS_CHECK_ARG(Ho > 0 && Wo > 0 && B > 0 && T > 0, "conv3d_igemm: empty output");
  MAAVSS_CHECK_ARG((int64_t)cdiv(Wo, 16) * cdiv(Ho, 16) * B * T < (1LL << 31) - 8, "conv3d_igemm: too many output tiles");
  const int KP = maavss_conv3d_kp(c_in);
  hipStream_t st = (hipStream_t)stream;
  // MODE_F32: the exact-f32 kernel; the 16-bit modes: the pipelined kernel (conv3d_igemm16_kernel)
#define CASE(CI, CO)                                                                                          \
  if (c_in == CI && c_out == CO) {                                                                            \
    if (precise == MODE_F32) launch_igemm<CI, CO>(x, wt, y, stat_partials, B, T, H, W, Ho, Wo, pad, KP, st);  \
    else if (precise == MODE_F16 && x16) launch_igemm16<MODE_F16, CI, CO, true>(x, wt, y, stat_partials, B, T, H, W, Ho, Wo, pad, KP, st); \
    else if (precise == MODE_F16) launch_igemm16<MODE_F16, CI, CO, false>(x, wt, y, stat_partials, B, T, H, W, Ho, Wo, pad, KP, st); \
    else if (x16) launch_igemm16<MODE_BF16, CI, CO, true>(x, wt, y, stat_partials, B, T, H, W, Ho, Wo, pad, KP, st);         \
    else launch_igemm16<MODE_BF16, CI, CO, false>(x, wt, y, stat_partials, B, T, H, W, Ho, Wo, pad, KP, st);                        \
    MAAVSS_LAUNCH_CHECK("conv3d_igemm_kernel");                                                               \
    return MAAVSS_OK;                                                                                         \
  }
  CASE(16, 32) CASE(32, 64) CASE(64, 64) CASE(64, 16) CASE(32, 16) CASE(64, 32) CASE(16, 64)
#undef CASE
  maavss_set_error("conv3d_igemm: unsupported channels %d -> %d", c_in, c_out);
  return MAAVSS_ERR_ARG;
}
