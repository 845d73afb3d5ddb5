// The first Conv3d(3,5,5) layer of the visual encoder (C_in = 1, C_out = 16, K = 75; reference avse_model_final.py:34): forward and weight
// gradient (the network input needs no gradient).  x [BT][H][W] is the reference's NCDHW input as is, y [BT][H][W][16] channels-last.
// The shipped 16-bit path runs on the matrix pipe and never stores the conv output: conv3d_c1_fwd_mfma_kernel<1> (conv -> BatchNorm partial
// sums), <2> (conv again -> BatchNorm, 2x2 max pool, LeakyReLU) and conv3d_c1_wgrad_mfma_kernel<true> (conv a third time inside the fused
// BatchNorm / pool / activation backward and weight gradient).  With a stored conv output: conv3d_c1_fwd_mfma_kernel<0> (eval-mode forward) and
// conv3d_c1_wgrad_mfma_kernel<false> (the same kernel body, y read instead of recomputed).  precise=True: conv3d_c1_prep_kernel,
// conv3d_c1_fwd_kernel and conv3d_c1_wgrad_kernel<false|true>, an exact-f32 direct convolution on the VALU from an LDS halo tile, weights as
// wave-uniform scalar operands.  The per-chunk partials of both weight-gradient kernels are summed by conv3d_c1_wgrad_reduce_kernel
// (conv3d_wgrad.hip).
#include "conv3d_tile.h"
#include "bn_act.h"      // the BatchNorm / pool / LeakyReLU scalars this file shares with bn_pool.hip

// value of element i of the [3][20][20] f32 halo of the tile at (bt, t, y0, x0): zero outside the clip and the frame
__device__ __forceinline__ float c1_halo_f32(const float* __restrict__ x, int i, int bt, int t, int y0, int x0, int T, int H, int W) {
  const int d = i / 400, r = (i % 400) / 20, c = i % 20;
  const int tt = t + d - 1, iy = y0 + r - 2, ix = x0 + c - 2;
  float v = 0.f;
  if (tt >= 0 && tt < T && iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[((int64_t)(bt + d - 1) * H + iy) * W + ix];
  return v;
}

// The exact-f32 forward, a direct convolution.  x [BT][H][W], w16 [75][16] (tap-major), y [BT][H][W][16].
__global__ __launch_bounds__(256) void conv3d_c1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w16,
                                                            float* __restrict__ y, float* __restrict__ stat_partials,
                                                            int n_bt, int T, int H, int W) {
  __shared__ float halo[3][20][21];
  __shared__ float red[4][2][16];
  const int tid = threadIdx.x;
  const TileId tile = xcd_tile((W + 15) / 16, (H + 15) / 16, (int64_t)((W + 15) / 16) * ((H + 15) / 16) * n_bt);
  if (!tile.valid) return;
  const int x0 = tile.tx * 16, y0 = tile.ty * 16, bt = tile.bt, t = bt % T;
  for (int i = tid; i < 1200; i += 256) halo[i / 400][(i % 400) / 20][i % 20] = c1_halo_f32(x, i, bt, t, y0, x0, T, H, W);
  __syncthreads();
  const int ly = tid >> 4, lx = tid & 15;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
#pragma unroll
  for (int kd = 0; kd < 3; ++kd)
#pragma unroll
    for (int kh = 0; kh < 5; ++kh)
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) {
        const float v = halo[kd][ly + kh][lx + kw];
        const float* wp = w16 + ((kd * 5 + kh) * 5 + kw) * 16;  // wave-uniform -> scalar loads
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = fmaf(v, wp[c], acc[c]);
      }
  const int oy = y0 + ly, ox = x0 + lx;
  const bool ok = oy < H && ox < W;
  if (ok) {
    float4* o = reinterpret_cast<float4*>(y + (((int64_t)bt * H + oy) * W + ox) * 16);
    o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    o[2] = make_float4(acc[8], acc[9], acc[10], acc[11]);
    o[3] = make_float4(acc[12], acc[13], acc[14], acc[15]);
  }
  if (stat_partials != nullptr) {
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const float v = ok ? acc[c] : 0.f;
      const float s1 = wave_sum(v), s2 = wave_sum(v * v);
      if (lane == 0) { red[wv][0][c] = s1; red[wv][1][c] = s2; }
    }
    __syncthreads();
    if (tid < 32) {
      const int which = tid >> 4, c = tid & 15;
      const float v = red[0][which][c] + red[1][which][c] + red[2][which][c] + red[3][which][c];
      stat_partials[tile.lin * 32 + tid] = v;
    }
  }
}

// The same layer on the matrix pipe (16-bit path): implicit GEMM  y[pos][co] = sum_k A[pos][k] W[k][co].  One workgroup = a 16x16
// output tile of one (b, t) plane (as the f32 kernel); a wave owns 4 rows of 16 positions = 4 M-tiles.
// K layout (round 3, second form): the 15 (kd, kh) tap rows are the 16-lane K groups, each 8 wide: kw = 0..4 + three zero-weight
// slots, K = 128 = four 32-deep MFMA steps, group G = 4 m + g <-> (kd, kh) = (G / 5, G % 5), G = 15 all zero.  A lane's fragment is
// then 8 CONSECUTIVE halo columns l16 .. l16 + 7 of one row: 16 bytes.  To make that one aligned LDS read the halo is kept as FOUR
// copies shifted by 0..3 columns (copy s [kd][row][j] = halo[kd][row][j + s], 20 columns, 2400 B each -- a stride that puts the four
// copies 32 B apart modulo the 128-B bank cycle): lane l16 = 4 q + s reads copy s at column 4 q, 8-byte aligned, as one ds_read2_b64.
// 16 LDS reads + 16 MFMAs per wave and tile.  The first form (k = kh * 5 + kw over one 32-deep step per kd plane) built each fragment
// from eight ds_read_u16 and four packs: 96 LDS instructions + 52 VALU per wave and tile, and with the per-tile 64-bit index
// divisions on the CU's one scalar unit the statistics pass alone took 355 us; see DESIGN.md 9.
// A workgroup walks C1_TPW consecutive tiles (tx fastest): weight fragments and addresses are set up once, the next tile's halo is
// requested before this tile's MFMAs and written to the other LDS image after them, BatchNorm partial sums are reduced once per
// workgroup (one row of `stat_partials` per workgroup).
//
// The conv output of this layer (1.6 GB at 32 x 16 x 224^2, the largest tensor of the step) does not have to exist.  The layer is
// 59 GFLOP on a matrix pipe that is idle here and its input is 103 MB -- so the 16-bit path runs the convolution THREE times instead
// of writing it once and reading it twice:
//   EPI 1  (conv3d_c1_stats)        conv -> BatchNorm partial sums only (the store happens only when a channel's |gamma| is below
//                                   BN_INV_MIN_GAMMA: the backward reduction then has to gather xhat from y, bn_pool.hip);
//   EPI 2  (conv3d_c1_bn_pool_act)  conv again -> gamma (y - mean) invstd + beta -> 2x2 max pool -> LeakyReLU: the pooled
//                                   activation (f32 + IEEE half) and the argmax byte, bit-identical to bn_pool_act_fwd_kernel on
//                                   the stored y (the scalars of bn_act.h in the same scan order dy, dx);
//   conv3d_c1_wgrad_mfma_kernel<true>  conv a third time for xhat at every position of the BatchNorm backward.
// EPI 0 is the storing form (eval-mode forward, tests).
#define C1_TPW 8
#define C1H_COPY 1200             // halves per shifted copy [3][20][20]
#define C1H_IMG (4 * C1H_COPY)    // halves per halo image (four copies): 9600 B (+ 16 B: the dump slot of C1Halo::stash)
#define C1H_IMG_ALLOC (C1H_IMG + 8)

// the five halo elements of a thread (element i = tid + 256 j of the [3][20][20] halo): tile-independent constants
struct C1Halo {
  int off[5];                     // offset inside the [bt][H][W] frame stack relative to (bt, y0, x0)
  int lds[5];                     // half index inside copy 0 = (kd * 20 + row) * 20 + column
  __device__ __forceinline__ void setup(int tid, int H, int W) {
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int i = tid + j * 256;
      const int d = i / 400, rr = (i % 400) / 20, cc = i % 20;
      off[j] = ((d - 1) * H + (rr - 2)) * W + (cc - 2);
      lds[j] = i;
    }
  }
  // values of the tile at (bt, t, y0, x0): zero outside the clip / the frame
  __device__ __forceinline__ void fetch(const float* __restrict__ x, int tid, int bt, int t, int y0, int x0, int T, int H, int W, float v[5]) const {
    const float* base = x + ((int64_t)bt * H + y0) * W + x0;
    const bool inner = t >= 1 && t + 1 < T && y0 >= 2 && y0 + 18 <= H && x0 >= 2 && x0 + 18 <= W;      // uniform
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      v[j] = 0.f;
      if (j < 4 || tid < 1200 - 1024) {
        if (inner) {
          v[j] = base[off[j]];
        } else {
          const int i = lds[j], d = i / 400, rr = (i % 400) / 20, cc = i % 20;
          const int tt = t + d - 1, iy = y0 + rr - 2, ix = x0 + cc - 2;
          if (tt >= 0 && tt < T && iy >= 0 && iy < H && ix >= 0 && ix < W) v[j] = base[off[j]];
        }
      }
    }
  }
  // write the 16-bit values into the four shifted copies of one image
  __device__ __forceinline__ void stash(unsigned short* img, int tid, const unsigned short h[5]) const {
#pragma unroll
    for (int j = 0; j < 5; ++j)
      if (j < 4 || tid < 1200 - 1024) {
        const int cc = (tid + j * 256) % 20;
#pragma unroll
        for (int sft = 0; sft < 4; ++sft)      // column cc of the halo is column cc - sft of copy sft; the first sft columns go to a dump slot (no branch)
          img[cc >= sft ? sft * (C1H_COPY - 1) + lds[j] : C1H_IMG] = h[j];
      }
  }
};

// forward operands of a lane (co / position column l16 = 4 q + s, K group g, wave wv): weight fragments of the four K steps and the
// byte offsets of its halo fragments (tile row 4 wv + i: add 40 i)
struct C1Conv {
  bf16x8 fw[4];
  unsigned ra[4];
  __device__ __forceinline__ void setup(const float* __restrict__ w, int l16, int g, int wv) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int G = 4 * m + g, Gc = G < 15 ? G : 14, kd = Gc / 5, kh = Gc % 5;
      const float* wp = w + l16 * 75 + kd * 25 + kh * 5;
      const bool live = G < 15;
      const float w0 = live ? wp[0] : 0.f, w1 = live ? wp[1] : 0.f, w2 = live ? wp[2] : 0.f, w3 = live ? wp[3] : 0.f, w4 = live ? wp[4] : 0.f;
      fw[m] = __builtin_bit_cast(bf16x8, make_uint4(pack2<MODE_F16>(w0, w1), pack2<MODE_F16>(w2, w3), pack2<MODE_F16>(w4, 0.f), 0u));
      ra[m] = (unsigned)(((l16 & 3) * C1H_COPY + (kd * 20 + 4 * wv + kh) * 20 + (l16 & ~3)) * 2);
    }
  }
  // acc[i][r] += y(channel 4 g + r, position (row 4 wv + i, column l16)) of the tile whose IEEE-half image is `img`
  __device__ __forceinline__ void tile(const unsigned short* img, f32x4 acc[4]) const {
    const char* hb = reinterpret_cast<const char*>(img);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint2 lo = *reinterpret_cast<const uint2*>(hb + ra[m] + i * 40), hi = *reinterpret_cast<const uint2*>(hb + ra[m] + i * 40 + 8);
        Mma<MODE_F16>::mma(acc[i], fw[m], __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y)));   // D[channel][position]
      }
  }
};

struct C1EpiArgs {
  const float* mean;
  const float* invstd;
  const float* gamma;             // EPI 1: decides the conditional store; EPI 2: the affine part
  const float* beta;
  float* out;                     // [BT][Hp][Wp][16] pooled activation
  unsigned short* out16;          // the same as IEEE half (next conv's operand), may be null
  unsigned short* out_bf16;       // the same as bf16 (the next conv's weight-gradient operand), may be null
  unsigned char* argmax;          // [BT][Hp][Wp][16] window position dy * 2 + dx of the maximum
  int Hp, Wp;
};
template <int EPI>
__global__ __launch_bounds__(256) void conv3d_c1_fwd_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 float* __restrict__ y, float* __restrict__ stat_partials,
                                                                 int n_bt, int T, int H, int W, C1EpiArgs ep) {
  __shared__ __attribute__((aligned(16))) unsigned short halo[2][C1H_IMG_ALLOC];
  __shared__ float red[4][2][16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = lane & 15, g = lane >> 4;
  // tile list in 32-bit arithmetic (the entry points check nx * ny * n_bt < 2^31) and advanced one tile at a time: 64-bit
  // divisions per tile run on the one scalar unit of a CU, shared by its 16 waves
  const unsigned nx = (W + 15) / 16, ny = (H + 15) / 16;
  const unsigned total = nx * ny * (unsigned)n_bt, nsuper = (total + C1_TPW - 1) / C1_TPW;
  const unsigned per = (nsuper + 7) / 8;
  const unsigned sup = (blockIdx.x & 7) * per + (blockIdx.x >> 3);             // XCD k walks the k-th eighth of the tile list
  if ((blockIdx.x >> 3) >= per || sup >= nsuper) return;
  const unsigned lin0 = sup * C1_TPW;
  const int ntile = (int)((total - lin0) < C1_TPW ? (total - lin0) : C1_TPW);
  // columns 20 - s .. 19 of copy s are never written (no halo column behind them; zero-weight K slots read them): zero once
  for (int i = tid; i < 2 * C1H_IMG_ALLOC / 8; i += 256) reinterpret_cast<uint4*>(&halo[0][0])[i] = make_uint4(0, 0, 0, 0);
  C1Conv cv;
  cv.setup(w, l16, g, wv);
  C1Halo hl;
  hl.setup(tid, H, W);
  float hreg[5];
  unsigned ftx = lin0 % nx, fty = (lin0 / nx) % ny, fbt = lin0 / (nx * ny), ft = fbt % (unsigned)T;      // the tile being fetched
  auto fetch = [&]() __attribute__((always_inline)) {
    hl.fetch(x, tid, (int)fbt, (int)ft, (int)fty * 16, (int)ftx * 16, T, H, W, hreg);
    if (++ftx == nx) { ftx = 0; if (++fty == ny) { fty = 0; ++fbt; if (++ft == (unsigned)T) ft = 0; } }
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
    unsigned short h16[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) h16[j] = Mma<MODE_F16>::cvt(hreg[j]);
    hl.stash(&halo[buf][0], tid, h16);
  };
  fetch();
  __syncthreads();                 // the zero fill is complete
  stash(0);
  __syncthreads();
  unsigned ctx = lin0 % nx, cty = (lin0 / nx) % ny, cbt = lin0 / (nx * ny);    // the tile being computed
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  bool store = EPI == 0;
  float sc[4] = {0.f, 0.f, 0.f, 0.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (EPI == 1) {
    if (y != nullptr)
      for (int c = 0; c < 16; ++c) store |= fabsf(ep.gamma[c]) < BN_INV_MIN_GAMMA;      // uniform over the grid
  }
  if constexpr (EPI == 2) {
    // channels 4 g .. 4 g + 3
    const float4 ga = *reinterpret_cast<const float4*>(ep.gamma + 4 * g), is = *reinterpret_cast<const float4*>(ep.invstd + 4 * g);
    const float4 be = *reinterpret_cast<const float4*>(ep.beta + 4 * g), mu = *reinterpret_cast<const float4*>(ep.mean + 4 * g);
    bn_scale_shift(ga.x, is.x, be.x, mu.x, sc[0], sh[0]); bn_scale_shift(ga.y, is.y, be.y, mu.y, sc[1], sh[1]);
    bn_scale_shift(ga.z, is.z, be.z, mu.z, sc[2], sh[2]); bn_scale_shift(ga.w, is.w, be.w, mu.w, sc[3], sh[3]);
  }
  for (int kt = 0; kt < ntile; ++kt) {
    const int bt = (int)cbt, x0 = (int)ctx * 16, y0 = (int)cty * 16;
    if (++ctx == nx) { ctx = 0; if (++cty == ny) { cty = 0; ++cbt; } }
    if (kt + 1 < ntile) fetch();
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    cv.tile(&halo[kt & 1][0], acc);
    // ---- lane holds channels 4 g + (0..3) of position (row 4 wv + i, column l16)
    if constexpr (EPI != 2) {
      // 16-byte stores, the 16 lanes of a row group write 16 consecutive positions = 1 KiB contiguous per store instruction
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int oy = y0 + 4 * wv + i, ox = x0 + l16;
        if (oy < H && ox < W) {
          if (store) *reinterpret_cast<float4*>(y + (((int64_t)bt * H + oy) * W + ox) * 16 + 4 * g) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
#pragma unroll
          for (int r = 0; r < 4; ++r) { s1[r] += acc[i][r]; s2[r] += acc[i][r] * acc[i][r]; }
        }
      }
    } else {
      // 2x2 windows: rows (4 wv + 0, 1) and (4 wv + 2, 3) live in this lane, columns (l16 even, odd) in a lane pair.  The even
      // lane finishes the upper window, the odd lane the lower one: each sends the partner the two rows it does not finish.
      const bool odd = (l16 & 1) != 0;
      float own[2][4], rcv[2][4];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float va = bn_affine(acc[k][r], sc[r], sh[r]), vb = bn_affine(acc[2 + k][r], sc[r], sh[r]);
          own[k][r] = odd ? vb : va;
          rcv[k][r] = dpp_f32<0xB1, 0xf>(odd ? va : vb, 0.f);                       // quad_perm [1,0,3,2]: the pair partner's value
        }
      const int py = (y0 >> 1) + 2 * wv + (odd ? 1 : 0), px = (x0 >> 1) + (l16 >> 1);
      if (py < ep.Hp && px < ep.Wp) {
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bi[4] = {0, 0, 0, 0};
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int dx = 0; dx < 2; ++dx)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float v = (dx == 1) == odd ? own[dy][r] : rcv[dy][r];
              if (pool_take(v, best[r])) { best[r] = v; bi[r] = dy * 2 + dx; }
            }
        float a4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a4[r] = leaky_fwd(best[r]);
        const int64_t pp = (((int64_t)bt * ep.Hp + py) * ep.Wp + px) * 16 + 4 * g;
        *reinterpret_cast<float4*>(ep.out + pp) = make_float4(a4[0], a4[1], a4[2], a4[3]);
        if (ep.out16 != nullptr) *reinterpret_cast<uint2*>(ep.out16 + pp) = make_uint2(pack2<2>(a4[0], a4[1]), pack2<2>(a4[2], a4[3]));
        if (ep.out_bf16 != nullptr) *reinterpret_cast<uint2*>(ep.out_bf16 + pp) = make_uint2(pack2<0>(a4[0], a4[1]), pack2<0>(a4[2], a4[3]));
        *reinterpret_cast<uchar4*>(ep.argmax + pp) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
      }
    }
    if (kt + 1 < ntile) stash((kt + 1) & 1);
    __syncthreads();
  }
  if (EPI != 2 && stat_partials != nullptr) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s1[r] = row16_sum(s1[r]);
      s2[r] = row16_sum(s2[r]);
      if (l16 == 0) { red[wv][0][4 * g + r] = s1[r]; red[wv][1][4 * g + r] = s2[r]; }
    }
    __syncthreads();
    if (tid < 32) {
      const int which = tid >> 4, c = tid & 15;
      stat_partials[(int64_t)sup * 32 + tid] = red[0][which][c] + red[1][which][c] + red[2][which][c] + red[3][which][c];
    }
  }
}

// reference layout [16][1][3][5][5] -> [75][16]
__global__ void conv3d_c1_prep_kernel(const float* __restrict__ w, float* __restrict__ w16) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 1200) w16[i] = w[(i % 16) * 75 + i / 16];
}

// x / pool for pool = 2 or 3 (x >= 0, x < 98304) without the runtime integer division (~25 vector instructions each, sixteen of them
// per wave and tile in the first layer's weight-gradient kernels: 768 -> 697 us for the recompute kernel)
__device__ __forceinline__ int c1_pdiv(int x, int pool) { return pool == 2 ? (x >> 1) : (int)(((unsigned)x * 43691u) >> 17); }

struct C1BnArgs {
  const float* dout;            // [BT][Hp][Wp][16] gradient of the pooled, activated output
  const float* out;             // [BT][Hp][Wp][16] that output
  const unsigned char* argmax;  // [BT][Hp][Wp][16] window position of the maximum
  const float* mean;
  const float* invstd;
  const float* coef;            // [3][16]: gamma*invstd, mean(dz), mean(dz*xhat)   (bn_bwd_finalize_kernel)
  const float* beta;            // recompute kernel only: the sign of the pooled output is re-derived from the recomputed y
  int pool, Hp, Wp;
};
// dW[16][75] partial per block; dy tile and x halo in LDS.  Thread = ((kd,kh) pair, 4-channel group, row worker): it walks
// rows of the 16x16 tile keeping the five x values of the kw window in registers (one new LDS value per position) and
// reading its 4 dy channels once per position -- 20 FMAs per 2 LDS reads.  (The first version, one thread per tap
// reading all 16 channels, spent 5 LDS reads per 16 FMAs and was LDS-bound at 17 us per tile.)
// FUSE_BN: `dy` is the pre-BatchNorm conv output y and the gradient is formed on the way into LDS from the pooled
// gradient / output / argmax and the BatchNorm backward coefficients -- the bn_pool_act_bwd_dx pass of the first layer
// (whose only consumer is this kernel: the network input needs no gradient) and its 1.6 GB dy round trip disappear.
template <bool FUSE_BN>
__global__ __launch_bounds__(256) void conv3d_c1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              float* __restrict__ partials, int T, int H, int W,
                                                              int tiles_x, int tiles_y, int BT, int tiles_per_chunk, int nchunk,
                                                              C1BnArgs bn) {
  __shared__ float halo[3][20][21];
  __shared__ __attribute__((aligned(16))) float buf[4 * 1200];   // dy tile [256][16]; at the end the cross-worker reduction [4][1200]
  float (*dys)[16] = reinterpret_cast<float (*)[16]>(buf);
  const int tid = threadIdx.x;
  const bool active = tid < 240;
  const int worker = tid / 60, q = tid % 60, khd = q >> 2, c4 = (q & 3) * 4;
  const int kd = khd / 5, kh = khd % 5;
  float acc[5][4];
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[k][c] = 0.f;
  const int tiles_total = BT * tiles_x * tiles_y;
  const int chunk = xcd_chunk(nchunk);
  if (chunk >= nchunk) return;
  const int tile_beg = chunk * tiles_per_chunk, tile_end = min(tiles_total, tile_beg + tiles_per_chunk);
  for (int tile = tile_beg; tile < tile_end; ++tile) {
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, bt = tile / (tiles_x * tiles_y), t = bt % T;
    const int x0 = tx * 16, y0 = ty * 16;
    __syncthreads();
    for (int i = tid; i < 1200; i += 256) halo[i / 400][(i % 400) / 20][i % 20] = c1_halo_f32(x, i, bt, t, y0, x0, T, H, W);
    for (int i = tid; i < 1024; i += 256) {
      const int pos = i >> 2, cc = (i & 3) * 4;
      const int oy = y0 + (pos >> 4), ox = x0 + (pos & 15);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (oy < H && ox < W) {
        v = *reinterpret_cast<const float4*>(dy + (((int64_t)bt * H + oy) * W + ox) * 16 + cc);
        if constexpr (FUSE_BN) {
          const int py = c1_pdiv(oy, bn.pool), px = c1_pdiv(ox, bn.pool);
          float gg[4] = {0.f, 0.f, 0.f, 0.f};
          if (py < bn.Hp && px < bn.Wp) {
            const int64_t pp = (((int64_t)bt * bn.Hp + py) * bn.Wp + px) * 16 + cc;
            const int here = (oy - py * bn.pool) * bn.pool + (ox - px * bn.pool);
            const uchar4 am = *reinterpret_cast<const uchar4*>(bn.argmax + pp);
            if (am.x == here || am.y == here || am.z == here || am.w == here) {
              const float4 dv = *reinterpret_cast<const float4*>(bn.dout + pp), ov = *reinterpret_cast<const float4*>(bn.out + pp);
              if (am.x == here) gg[0] = dv.x * leaky_slope(ov.x);
              if (am.y == here) gg[1] = dv.y * leaky_slope(ov.y);
              if (am.z == here) gg[2] = dv.z * leaky_slope(ov.z);
              if (am.w == here) gg[3] = dv.w * leaky_slope(ov.w);
            }
          }
          const float4 mu = *reinterpret_cast<const float4*>(bn.mean + cc), is = *reinterpret_cast<const float4*>(bn.invstd + cc);
          const float4 k0 = *reinterpret_cast<const float4*>(bn.coef + cc), k1 = *reinterpret_cast<const float4*>(bn.coef + 16 + cc);
          const float4 k2 = *reinterpret_cast<const float4*>(bn.coef + 32 + cc);
          v.x = bn_dy(gg[0], v.x, mu.x, is.x, k0.x, k1.x, k2.x);
          v.y = bn_dy(gg[1], v.y, mu.y, is.y, k0.y, k1.y, k2.y);
          v.z = bn_dy(gg[2], v.z, mu.z, is.z, k0.z, k1.z, k2.z);
          v.w = bn_dy(gg[3], v.w, mu.w, is.w, k0.w, k1.w, k2.w);
        }
      }
      *reinterpret_cast<float4*>(&dys[pos][cc]) = v;
    }
    __syncthreads();
    if (active) {
      for (int ry = worker; ry < 16; ry += 4) {
        const float* xr = &halo[kd][ry + kh][0];
        float w[5] = {xr[0], xr[1], xr[2], xr[3], 0.f};
#pragma unroll
        for (int p = 0; p < 16; ++p) {
          w[4] = xr[p + 4];
          const float4 d = *reinterpret_cast<const float4*>(&dys[ry * 16 + p][c4]);
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            acc[k][0] = fmaf(w[k], d.x, acc[k][0]);
            acc[k][1] = fmaf(w[k], d.y, acc[k][1]);
            acc[k][2] = fmaf(w[k], d.z, acc[k][2]);
            acc[k][3] = fmaf(w[k], d.w, acc[k][3]);
          }
          w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = w[4];
        }
      }
    }
  }
  __syncthreads();
  float* red = buf;                        // [4 workers][16 c][75 taps]
  if (active)
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c) red[(worker * 16 + c4 + c) * 75 + khd * 5 + k] = acc[k][c];
  __syncthreads();
  for (int i = tid; i < 1200; i += 256)     // i = c * 75 + tap: [chunk][c][tap]
    partials[(int64_t)chunk * 1200 + i] = red[i] + red[1200 + i] + red[2400 + i] + red[3600 + i];
}

// The first layer's weight gradient on the matrix pipe (16-bit path), BatchNorm / max-pool / LeakyReLU backward fused as in
// conv3d_c1_wgrad_kernel<true>:  dW[tap][co] = sum over positions of x[pos + tap] * dy[pos][co]  as an MFMA product with the
// 75 taps as rows (5 tiles of 16, the last 5 rows unused), co as columns and the POSITION as the K dimension (32 positions =
// two tile rows per step).  A wave takes 2 of the tile's 8 K-steps for all 5 tap tiles and keeps its 5 accumulators across the
// chunk's tiles; the waves are summed once per chunk.  75 FMAs per (position, channel) on the VALU become 5 MFMAs per 32 positions.
// The gradient on the way into the product is formed in the two steps of bn_pool_act_bwd_dx_kernel and with its scalars (bn_act.h),
// per channel.  LeakyReLU(0.01) + max pool: the pooled gradient dv, for the window position that is the channel's argmax (else 0),
// times leaky_slope of the pooled output (or of the pre-activation it is recomputed from: the same sign).  Then bn_dy on the conv
// output y.  It is rounded to bf16 and stored TRANSPOSED [co][pos], so that a B fragment (8 consecutive positions of one channel)
// is one 16-byte LDS read.
// RECOMPUTE = false: `src` is the stored conv output y (bound by reading it: 1.6 GB at the benched shape), the sign comes from
// bn.out.  RECOMPUTE = true: `src` is the layer's weights and the tile's y is recomputed from the halo that is staged anyway (C1Conv on
// an IEEE-half image of it: the arithmetic of conv3d_c1_fwd_mfma_kernel, so xhat is bit-identical to what the forward normalised).
// The MFMA result layout of that conv -- lane (column l16, channel group g) holds channels 4 g .. 4 g + 3 of the positions
// (row 4 wv + i, l16) -- is the dy-formation mapping of both forms: each lane forms its 4 x 4 values from registers (of y: a float4
// load per position, 1 KiB contiguous per wave and row) and writes them transposed.
// The bf16 halo of the weight-gradient product is kept in the four-shifted-copies form of the forward: the A fragment of lane
// (tap, k group) is 8 consecutive columns starting at kw + 8 (g & 1), i.e. copy kw & 3 at an 8-byte aligned column -- one
// ds_read2_b64 instead of the eight 16-bit reads and four packs a single [3][20][24] image takes.  The images are double-buffered
// and the next tile's halo is fetched a tile ahead.
template <bool RECOMPUTE>
__global__ __launch_bounds__(256) void conv3d_c1_wgrad_mfma_kernel(const float* __restrict__ x, const float* __restrict__ src,
                                                                   float* __restrict__ partials, int T, int H, int W, int tiles_x,
                                                                   int tiles_y, int BT, int tiles_per_chunk, int nchunk, C1BnArgs bn) {
  constexpr int DYS = 256 + 8;                                        // dyT row stride (elements): 528 B, 16-byte aligned
  constexpr int NIMG = RECOMPUTE ? 2 : 1;                             // images per buffer: [IEEE half |] bf16
  constexpr int RED = 4 * 80 * 16 * 4;                                // bytes of the final reduction [4 waves][80 taps][16 co] f32, which reuses the buffers
  constexpr int IMG = RECOMPUTE ? C1H_IMG_ALLOC : RED / 4;            // halves per image: two bf16-only images (19232 B) are padded up to RED
  static_assert(IMG >= C1H_IMG_ALLOC && IMG % 8 == 0, "halo image");
  __shared__ __attribute__((aligned(16))) unsigned short img[2][NIMG][IMG];
  __shared__ __attribute__((aligned(16))) unsigned short dyT[16 * DYS];
  static_assert(sizeof(img) >= RED, "reduction scratch");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = lane & 15, g = lane >> 4;
  const int tiles_total = BT * tiles_x * tiles_y;
  const int chunk = xcd_chunk(nchunk);
  if (chunk >= nchunk) return;
  // columns 20 - s .. 19 of copy s are never written: zero once
  for (int i = tid; i < 2 * NIMG * IMG / 8; i += 256) reinterpret_cast<uint4*>(&img[0][0][0])[i] = make_uint4(0, 0, 0, 0);
  // byte offsets of the A fragments of the 5 tap tiles (K step ks: add 80 ks)
  unsigned abase[5];
#pragma unroll
  for (int mt = 0; mt < 5; ++mt) {
    int tap = 16 * mt + l16;
    tap = tap < 75 ? tap : 74;                                       // rows 75..79 of the last tile: computed, never stored
    const int kd = tap / 25, kh = (tap % 25) / 5, kw = tap % 5;
    abase[mt] = (unsigned)(((kw & 3) * C1H_COPY + (kd * 20 + kh + (g >> 1)) * 20 + (kw & ~3) + 8 * (g & 1)) * 2);
  }
  C1Conv cv;
  if constexpr (RECOMPUTE) cv.setup(src, l16, g, wv);
  C1Halo hl;
  hl.setup(tid, H, W);
  // the per-channel constants of the dy formula live in LDS (24 registers otherwise, which cost the third wave per SIMD)
  // mean, invstd, gamma invstd, mean(dz), mean(dz xhat) and, to recompute the sign, beta - mean gamma invstd
  __shared__ __attribute__((aligned(16))) float cst[RECOMPUTE ? 6 : 5][16];
  if (tid < 16) {
    const float m_ = bn.mean[tid], c0_ = bn.coef[tid];
    cst[0][tid] = m_; cst[1][tid] = bn.invstd[tid]; cst[2][tid] = c0_; cst[3][tid] = bn.coef[16 + tid]; cst[4][tid] = bn.coef[32 + tid];
    if constexpr (RECOMPUTE) cst[5][tid] = bn_shift(bn.beta[tid], m_, c0_);
  }
  f32x4 acc[5];
#pragma unroll
  for (int mt = 0; mt < 5; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tile_beg = chunk * tiles_per_chunk, tile_end = min(tiles_total, tile_beg + tiles_per_chunk);
  if (tile_beg >= tile_end) {                                        // an empty chunk still owns its row of partials
    for (int i = tid; i < 1200; i += 256) partials[(int64_t)chunk * 1200 + i] = 0.f;
    return;
  }
  int tx = tile_beg % tiles_x, ty = (tile_beg / tiles_x) % tiles_y, bt = tile_beg / (tiles_x * tiles_y), t = bt % T;
  float hreg[5];
  auto stash = [&](int buf) __attribute__((always_inline)) {
    unsigned short h16[5], b16[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) { h16[j] = Mma<MODE_F16>::cvt(hreg[j]); b16[j] = f2bf(hreg[j]); }
    if constexpr (RECOMPUTE) hl.stash(&img[buf][0][0], tid, h16);
    hl.stash(&img[buf][NIMG - 1][0], tid, b16);
  };
  hl.fetch(x, tid, bt, t, ty * 16, tx * 16, T, H, W, hreg);
  __syncthreads();                                                   // zero fill complete
  stash(0);
  __syncthreads();
  for (int tile = tile_beg, it = 0; tile < tile_end; ++tile, ++it) {
    const int x0 = tx * 16, y0 = ty * 16, cbt = bt;
    if (++tx == tiles_x) { tx = 0; if (++ty == tiles_y) { ty = 0; ++bt; if (++t == T) t = 0; } }
    // the operands of this lane's four positions and the next tile's halo: issued first, used after the conv.  Coordinates are
    // clamped instead of predicated (edge tiles: the values are discarded below).
    float4 dv[4], ov[4];
    uchar4 am[4];
    f32x4 z[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int oy = min(y0 + 4 * wv + i, H - 1), ox = min(x0 + l16, W - 1);
      const int py = min(c1_pdiv(oy, bn.pool), bn.Hp - 1), px = min(c1_pdiv(ox, bn.pool), bn.Wp - 1);
      const int64_t pp = (((int64_t)cbt * bn.Hp + py) * bn.Wp + px) * 16 + 4 * g;
      if constexpr (!RECOMPUTE) z[i] = *reinterpret_cast<const f32x4*>(src + (((int64_t)cbt * H + oy) * W + ox) * 16 + 4 * g);
      am[i] = *reinterpret_cast<const uchar4*>(bn.argmax + pp);
      dv[i] = *reinterpret_cast<const float4*>(bn.dout + pp);
      if constexpr (!RECOMPUTE) ov[i] = *reinterpret_cast<const float4*>(bn.out + pp);
    }
    if (tile + 1 < tile_end) hl.fetch(x, tid, bt, t, ty * 16, tx * 16, T, H, W, hreg);
    // ---- y of the tile (forward arithmetic)
    if constexpr (RECOMPUTE) {
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      cv.tile(&img[it & 1][0][0], z);
    }
    // ---- dy of this lane's positions, transposed bf16 into LDS
    const float4 mu = *reinterpret_cast<const float4*>(&cst[0][4 * g]), is = *reinterpret_cast<const float4*>(&cst[1][4 * g]);
    const float4 k0 = *reinterpret_cast<const float4*>(&cst[2][4 * g]), k1 = *reinterpret_cast<const float4*>(&cst[3][4 * g]);
    const float4 k2 = *reinterpret_cast<const float4*>(&cst[4][4 * g]);
    float4 sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (RECOMPUTE) sh = *reinterpret_cast<const float4*>(&cst[5][4 * g]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int oy = y0 + 4 * wv + i, ox = x0 + l16, pos = (4 * wv + i) * 16 + l16;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (oy < H && ox < W) {
        const int py = c1_pdiv(oy, bn.pool), px = c1_pdiv(ox, bn.pool);
        float gg[4] = {0.f, 0.f, 0.f, 0.f};
        if (py < bn.Hp && px < bn.Wp) {
          const int here = (oy - py * bn.pool) * bn.pool + (ox - px * bn.pool);
          // RECOMPUTE: the pooled output is positive exactly when the forward's pre-activation at the argmax was: bn_affine with
          // (gamma invstd, beta - mean gamma invstd), as conv3d_c1_fwd_mfma_kernel<2> formed it on the same recomputed y -- `out` is not read
          if (am[i].x == here) gg[0] = dv[i].x * leaky_slope(RECOMPUTE ? bn_affine(z[i][0], k0.x, sh.x) : ov[i].x);
          if (am[i].y == here) gg[1] = dv[i].y * leaky_slope(RECOMPUTE ? bn_affine(z[i][1], k0.y, sh.y) : ov[i].y);
          if (am[i].z == here) gg[2] = dv[i].z * leaky_slope(RECOMPUTE ? bn_affine(z[i][2], k0.z, sh.z) : ov[i].z);
          if (am[i].w == here) gg[3] = dv[i].w * leaky_slope(RECOMPUTE ? bn_affine(z[i][3], k0.w, sh.w) : ov[i].w);
        }
        v.x = bn_dy(gg[0], z[i][0], mu.x, is.x, k0.x, k1.x, k2.x);
        v.y = bn_dy(gg[1], z[i][1], mu.y, is.y, k0.y, k1.y, k2.y);
        v.z = bn_dy(gg[2], z[i][2], mu.z, is.z, k0.z, k1.z, k2.z);
        v.w = bn_dy(gg[3], z[i][3], mu.w, is.w, k0.w, k1.w, k2.w);
      }
      dyT[(4 * g + 0) * DYS + pos] = f2bf(v.x);
      dyT[(4 * g + 1) * DYS + pos] = f2bf(v.y);
      dyT[(4 * g + 2) * DYS + pos] = f2bf(v.z);
      dyT[(4 * g + 3) * DYS + pos] = f2bf(v.w);
    }
    __syncthreads();
    const char* hb0 = reinterpret_cast<const char*>(&img[it & 1][NIMG - 1][0]);
#pragma unroll
    for (int ksl = 0; ksl < 2; ++ksl) {
      const int ks = wv * 2 + ksl;                                   // positions 32 ks .. 32 ks + 31 = tile rows 2 ks, 2 ks + 1
      const bf16x8 fb = *reinterpret_cast<const bf16x8*>(dyT + l16 * DYS + 32 * ks + 8 * g);
      const char* hb = hb0 + ks * 80;
#pragma unroll
      for (int mt = 0; mt < 5; ++mt) {
        const uint2 lo = *reinterpret_cast<const uint2*>(hb + abase[mt]), hi = *reinterpret_cast<const uint2*>(hb + abase[mt] + 8);
        Mma<MODE_BF16>::mma(acc[mt], __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y)), fb);
      }
    }
    if (tile + 1 < tile_end) stash((it + 1) & 1);
    __syncthreads();
  }
  // ---- sum the four waves: lane (co = l16, g) holds taps 16 mt + 4 g + r
  float* red = reinterpret_cast<float*>(&img[0][0][0]);                      // [4 waves][80 taps][16 co]
#pragma unroll
  for (int mt = 0; mt < 5; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(wv * 80 + 16 * mt + 4 * g + r) * 16 + l16] = acc[mt][r];
  __syncthreads();
  for (int i = tid; i < 1200; i += 256) {     // i = c * 75 + tap: [chunk][c][tap]
    const int c = i / 75, tap = i % 75;
    partials[(int64_t)chunk * 1200 + i] = red[tap * 16 + c] + red[(80 + tap) * 16 + c] + red[(160 + tap) * 16 + c] + red[(240 + tap) * 16 + c];
  }
}

// 16x16 output tiles of a problem; the kernels count them in 32-bit arithmetic; the grid of the MFMA forward (C1_TPW tiles per workgroup)
static inline int64_t c1_tiles(int B, int T, int H, int W) { return (int64_t)cdiv(W, 16) * cdiv(H, 16) * B * T; }
static inline bool c1_tiles_fit(int B, int T, int H, int W) { return c1_tiles(B, T, H, W) < (1LL << 31); }
static inline dim3 c1_fwd_grid(int B, int T, int H, int W) { return dim3(xcd_grid(cdiv(c1_tiles(B, T, H, W), C1_TPW))); }

// rows of `stat_partials` ([rows][2][16] floats) maavss_conv3d_c1_fwd writes: one per workgroup
extern "C" int64_t maavss_conv3d_c1_fwd_nparts(int B, int T, int H, int W, int precise) {
  return precise == MODE_F16 ? cdiv(c1_tiles(B, T, H, W), C1_TPW) : c1_tiles(B, T, H, W);
}

extern "C" int maavss_conv3d_c1_fwd(const float* x, const float* w, float* w16_ws, float* y, float* stat_partials, int B,
                                    int T, int H, int W, int precise, void* stream) {
  MAAVSS_CHECK_ARG(x && w && w16_ws && y, "conv3d_c1_fwd: null pointer");
  MAAVSS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "conv3d_c1_fwd: empty problem");
  MAAVSS_CHECK_ARG(c1_tiles_fit(B, T, H, W) && (int64_t)B * T * H * W < (1LL << 40), "conv3d_c1: too many tiles");
  MAAVSS_CHECK_ARG(precise == MODE_F32 || precise == MODE_F16, "conv3d_c1_fwd: mode must be 1 (exact f32 VALU) or 2 (IEEE-half MFMA)");
  hipStream_t st = (hipStream_t)stream;
  if (precise == MODE_F16) {
    hipLaunchKernelGGL(conv3d_c1_fwd_mfma_kernel<0>, c1_fwd_grid(B, T, H, W), dim3(256), 0, st, x, w, y, stat_partials, B * T, T, H, W, C1EpiArgs{});
    MAAVSS_LAUNCH_CHECK("conv3d_c1_fwd_mfma_kernel");
    return MAAVSS_OK;
  }
  hipLaunchKernelGGL(conv3d_c1_prep_kernel, dim3(5), dim3(256), 0, st, w, w16_ws);
  hipLaunchKernelGGL(conv3d_c1_fwd_kernel, dim3(xcd_grid(c1_tiles(B, T, H, W))), dim3(256), 0, st, x, w16_ws, y, stat_partials, B * T, T, H, W);
  MAAVSS_LAUNCH_CHECK("conv3d_c1_fwd_kernel");
  return MAAVSS_OK;
}

// The 16-bit first layer without its conv output (see conv3d_c1_fwd_mfma_kernel): pass 1, BatchNorm partial sums.  `y` is written
// only when some |gamma[c]| < 1e-2 (the backward reduction then gathers xhat from it); stat_partials as maavss_conv3d_c1_fwd(.., 2).
extern "C" int maavss_conv3d_c1_stats(const float* x, const float* w, const float* gamma, float* y, float* stat_partials, int B, int T,
                                      int H, int W, void* stream) {
  MAAVSS_CHECK_ARG(x && w && gamma && y && stat_partials, "conv3d_c1_stats: null pointer");
  MAAVSS_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "conv3d_c1_stats: empty problem");
  MAAVSS_CHECK_ARG(c1_tiles_fit(B, T, H, W) && (int64_t)B * T * H * W < (1LL << 40), "conv3d_c1: too many tiles");
  C1EpiArgs ep = {};
  ep.gamma = gamma;
  hipLaunchKernelGGL(conv3d_c1_fwd_mfma_kernel<1>, c1_fwd_grid(B, T, H, W), dim3(256), 0, (hipStream_t)stream, x, w, y, stat_partials, B * T, T, H, W, ep);
  MAAVSS_LAUNCH_CHECK("conv3d_c1_fwd_mfma_kernel<1>");
  return MAAVSS_OK;
}

// pass 2: conv again -> BatchNorm -> MaxPool(1,2,2) -> LeakyReLU(0.01).  out [B*T][H/2][W/2][16] f32, out16 the same as IEEE half
// and out_bf16 as bf16 (both may be null), argmax one byte per element.
extern "C" int maavss_conv3d_c1_bn_pool_act(const float* x, const float* w, const float* mean, const float* invstd, const float* gamma,
                                            const float* beta, float* out, void* out16, void* out_bf16, void* argmax, int B, int T, int H,
                                            int W, void* stream) {
  MAAVSS_CHECK_ARG(x && w && mean && invstd && gamma && beta && out && argmax, "conv3d_c1_bn_pool_act: null pointer");
  MAAVSS_CHECK_ARG(B > 0 && T > 0 && H >= 2 && W >= 2, "conv3d_c1_bn_pool_act: empty problem");
  MAAVSS_CHECK_ARG(c1_tiles_fit(B, T, H, W) && (int64_t)B * T * H * W < (1LL << 40), "conv3d_c1: too many tiles");
  C1EpiArgs ep;
  ep.mean = mean; ep.invstd = invstd; ep.gamma = gamma; ep.beta = beta; ep.out = out; ep.out16 = (unsigned short*)out16;
  ep.out_bf16 = (unsigned short*)out_bf16;
  ep.argmax = (unsigned char*)argmax; ep.Hp = H / 2; ep.Wp = W / 2;
  hipLaunchKernelGGL(conv3d_c1_fwd_mfma_kernel<2>, c1_fwd_grid(B, T, H, W), dim3(256), 0, (hipStream_t)stream, x, w, nullptr, nullptr, B * T, T, H, W, ep);
  MAAVSS_LAUNCH_CHECK("conv3d_c1_fwd_mfma_kernel<2>");
  return MAAVSS_OK;
}

// one of the weight-gradient kernels (C1_VALU without `bn`: the plain gradient from dy) and the reduction of its partials;
// `src` is dy, the stored conv output y, or for C1_RECOMPUTE the layer's weights
enum C1Wgrad { C1_VALU, C1_MFMA, C1_RECOMPUTE };
static int c1_wgrad_launch(C1Wgrad which, const float* x, const float* src, float* dw, float* ws, int nchunk, int B, int T, int H, int W, int beta,
                           const C1BnArgs* bn, hipStream_t st) {
  const int tiles_x = cdiv(W, 16), tiles_y = cdiv(H, 16);
  C1BnArgs none = {};
  auto kern = which == C1_RECOMPUTE ? conv3d_c1_wgrad_mfma_kernel<true> : which == C1_MFMA ? conv3d_c1_wgrad_mfma_kernel<false>
              : bn              ? conv3d_c1_wgrad_kernel<true> : conv3d_c1_wgrad_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(cdiv(nchunk, 8) * 8), dim3(256), 0, st, x, src, ws, T, H, W, tiles_x, tiles_y, B * T,
                     cdiv(c1_tiles(B, T, H, W), nchunk), nchunk, bn ? *bn : none);
  MAAVSS_LAUNCH_CHECK(which == C1_VALU ? "conv3d_c1_wgrad_kernel" : "conv3d_c1_wgrad_mfma_kernel");
  conv3d_c1_wgrad_reduce(ws, dw, nchunk, beta, st);
  MAAVSS_LAUNCH_CHECK("conv3d_c1_wgrad_reduce_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_conv3d_c1_wgrad(const float* x, const float* dy, float* dw, float* ws, int nchunk, int B, int T,
                                      int H, int W, int beta, void* stream) {
  MAAVSS_CHECK_ARG(x && dy && dw && ws, "conv3d_c1_wgrad: null pointer");
  MAAVSS_CHECK_ARG(nchunk >= 1 && B > 0 && T > 0, "conv3d_c1_wgrad: bad sizes");
  MAAVSS_CHECK_ARG(H > 0 && W > 0 && c1_tiles_fit(B, T, H, W), "conv3d_c1_wgrad: empty image or too many tiles");
  return c1_wgrad_launch(C1_VALU, x, dy, dw, ws, nchunk, B, T, H, W, beta, nullptr, (hipStream_t)stream);
}

// maavss_conv3d_c1_wgrad_bn on the 16-bit path without the stored conv output: `w` = the layer's weights [16][1][3][5][5], y is
// recomputed per tile (conv3d_c1_wgrad_mfma_kernel<true>).  bf16 backward operands, IEEE-half forward operands for the recompute.
extern "C" int maavss_conv3d_c1_wgrad_bn_recompute(const float* x, const float* w, const float* dout, const void* argmax,
                                                   const float* mean, const float* invstd, const float* bn_beta, const float* coef, int pool,
                                                   float* dw, float* ws, int nchunk, int B, int T, int H, int W, int beta, void* stream) {
  MAAVSS_CHECK_ARG(x && w && dout && argmax && mean && invstd && bn_beta && coef && dw && ws, "conv3d_c1_wgrad_bn_recompute: null pointer");
  MAAVSS_CHECK_ARG(nchunk >= 1 && B > 0 && T > 0 && pool >= 2 && pool <= 3, "conv3d_c1_wgrad_bn_recompute: bad sizes (pool must be 2 or 3)");
  // H / pool >= 1 (the kernel clamps pooled indices to Hp - 1), c1_pdiv's multiply-shift division by 3 holds for x < 98304, the
  // tile count is an int
  MAAVSS_CHECK_ARG(H >= pool && W >= pool && H < 98304 && W < 98304, "conv3d_c1_wgrad_bn_recompute: H, W must be in [pool, 98304) (got %d x %d)", H, W);
  MAAVSS_CHECK_ARG(c1_tiles_fit(B, T, H, W), "conv3d_c1_wgrad_bn_recompute: too many tiles");
  const C1BnArgs bn = {dout, nullptr, (const unsigned char*)argmax, mean, invstd, coef, bn_beta, pool, H / pool, W / pool};
  return c1_wgrad_launch(C1_RECOMPUTE, x, w, dw, ws, nchunk, B, T, H, W, beta, &bn, (hipStream_t)stream);
}

extern "C" int maavss_conv3d_c1_wgrad_bn(const float* x, const float* y, const float* dout, const float* out, const void* argmax,
                                         const float* mean, const float* invstd, const float* coef, int pool, float* dw, float* ws,
                                         int nchunk, int B, int T, int H, int W, int beta, int precise, void* stream) {
  MAAVSS_CHECK_ARG(x && y && dout && out && argmax && mean && invstd && coef && dw && ws, "conv3d_c1_wgrad_bn: null pointer");
  MAAVSS_CHECK_ARG(precise == MODE_F32 || precise == MODE_BF16, "conv3d_c1_wgrad_bn: mode must be 1 (exact f32 VALU) or 0 (bf16 MFMA)");
  MAAVSS_CHECK_ARG(nchunk >= 1 && B > 0 && T > 0 && pool >= 2 && pool <= 3, "conv3d_c1_wgrad_bn: bad sizes (pool must be 2 or 3)");
  MAAVSS_CHECK_ARG(H >= pool && W >= pool && H < 98304 && W < 98304 && c1_tiles_fit(B, T, H, W),
                   "conv3d_c1_wgrad_bn: H, W must be in [pool, 98304) and the tile count below 2^31 (got %d x %d)", H, W);
  const C1BnArgs bn = {dout, out, (const unsigned char*)argmax, mean, invstd, coef, nullptr, pool, H / pool, W / pool};
  return c1_wgrad_launch(precise == MODE_BF16 ? C1_MFMA : C1_VALU, x, y, dw, ws, nchunk, B, T, H, W, beta, &bn, (hipStream_t)stream);
}
