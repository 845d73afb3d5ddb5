// Reverberation (maavss_amd.Reverb): synthetic room responses and their direct-form FIR convolution with audio that lies in one
// flat buffer (a batch of clips, or the clip bank's recordings, whose samples in front of a clip are the clip's history).
// include/maavss.h holds the definitions and the order of every sum; tests/reverb_twin.py restates them.  Compiled with
// -ffp-contract=off (Makefile): the fusions are the fma() calls written out below, and every fused product is one of two f32 values,
// exact in f64, so fma(h, x, a) has the bits of a + h * x.  No atomics, no workgroup waits on another; every index taken from a
// device table is clamped, and maavss_reverb checks the host copies of its tables before the launch.
//   rir_synth   one workgroup of 256 per response.  Pass 1: thread t forms the tail terms t_k = g[k] * exp(-lam k) of the quads
//               (four consecutive taps) t, t + 256, ... and adds their squares in tap order; wave_sum_d; (w0 + w1) + (w2 + w3).
//               Pass 2 forms the same t_k again (the same instructions on the same inputs) and stores f32(s t_k).  Reads the noise
//               twice (the second time from L2) or draws it twice; writes 4 B a tap.
//   reverb      one workgroup of 128 per RV_TILE = 1024 consecutive outputs of one row, thread t the outputs 8 t .. 8 t + 7.
//               The taps go through LDS in chunks of RV_KC = 1024, converted to f64 once, beside the RV_TILE + RV_KC - 1 input
//               samples the chunk's taps reach from the tile (f64 too; a position below the row's floor or outside the row holds
//               0.0 and is never multiplied).  Per block of 8 taps a thread reads a window of 15 samples and the 8 taps as twelve
//               16-byte LDS reads (ds_read_b128, the taps a broadcast) for 64 v_fma_f64 into 8 outputs x 4 partial sums (tap k ->
//               partial k mod 4): the arithmetic is 256 cycles a block and SIMD, the LDS 48 cycles a block and wave.  A thread's
//               window starts 8 samples (64 B) after its neighbour's, which alone would put four lanes of a read's sixteen on every
//               bank slot: the sample array leaves 16 B empty after every 8 samples (rv_slot), so lanes are 80 B apart and the
//               reads are conflict-free wherever the window has slid to.  (Adjacent 8-byte reads become ds_read2_b64, at a quarter
//               of the bytes per LDS cycle and with conflicts: the first version, 2.2 times slower.)  A block whose taps all count
//               for all of a thread's outputs runs unguarded; the block that straddles an output's last tap (K - 1, or the tap that
//               reaches the floor) tests every term, and chunks past the tile's last tap are not staged at all.
//               LDS 8 KiB of taps + 20 KiB of samples: five workgroups a CU.  Reads 4 B a sample and tap per chunk (from L2 after
//               the first tile), writes 4 B an output.
#include "common.h"
#include "bank_load.h"      // bank_clamp

namespace {

constexpr int RV_MAX_K = 32768;
constexpr int RV_THREADS = 128, RV_PER = 8, RV_TILE = RV_THREADS * RV_PER;      // outputs per thread / workgroup
constexpr int RV_KC = 1024;                                                     // taps per LDS chunk
constexpr int RV_SPAN = RV_TILE + RV_KC - 1;                                    // samples those taps reach from a tile
constexpr int64_t RV_MAX_ROWS = (int64_t)1 << 19;                               // rows of a table: the counter layout's row field
constexpr uint64_t RV_PHILOX_STREAM = (uint64_t)0x52455642u << 32;              // "REVB": keeps these counters off the STFT noise's

typedef double rv_d2 __attribute__((ext_vector_type(2)));
// where sample i of the staged span lies: 8 samples (64 B), then 16 B left empty.  A thread's window starts 8 samples after its
// neighbour's, so lanes are 80 B = 5 * 16 B apart and any 16 lanes with distinct numbers mod 16 -- every lane group of a 16-byte
// LDS read -- fall on distinct 16-byte bank slots, wherever the window has slid to.
__device__ __forceinline__ int rv_slot(int i) { return i + 2 * (i >> 3); }

// params f64 [n][3]: lam, 10^(drr_db / 10), predelay
struct rv_row {
  double lam, drr;
  int k0;
};
__device__ __forceinline__ rv_row rv_load_row(const double* __restrict__ params, int64_t r, int K) {
  rv_row q;
  q.lam = params[3 * r];
  q.drr = params[3 * r + 1];
  const double pd = params[3 * r + 2];
  q.k0 = pd >= (double)K ? K : (pd >= 1.0 ? (int)pd : 1);      // a NaN reads as 1
  return q;
}
// the four tail terms of quad q (taps 4 q .. 4 q + 3), 0 in front of the predelay and behind the last tap
__device__ __forceinline__ void rv_quad(const float* __restrict__ noise, uint64_t seed, int64_t r, int q, int K, const rv_row& row,
                                        double t[4]) {
  float g[4];
  if (noise) {
#pragma unroll
    for (int c = 0; c < 4; ++c) g[c] = 4 * q + c < K ? noise[4 * q + c] : 0.f;
  } else {
    philox_normal4(seed, RV_PHILOX_STREAM | ((uint64_t)r << 13) | (uint64_t)q, g);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = 4 * q + c;
    const double e = exp(-row.lam * (double)k);
    t[c] = (k >= row.k0 && k < K) ? (double)g[c] * e : 0.0;
  }
}

__global__ __launch_bounds__(256) void rir_synth_kernel(const double* __restrict__ params, const float* __restrict__ noise,
                                                        int64_t ld_noise, uint64_t seed, int64_t row0, int K, float* __restrict__ rirs,
                                                        int64_t ld) {
  __shared__ double red[4][1];
  const int64_t r = blockIdx.x;
  const rv_row row = rv_load_row(params, r, K);
  const float* __restrict__ g = noise ? noise + r * ld_noise : nullptr;
  const int quads = (K + 3) / 4;
  double t[4], sum = 0.0;
  for (int q = threadIdx.x; q < quads; q += 256) {
    if (4 * q + 3 < row.k0) continue;                 // the whole quad lies in front of the predelay: four zeros
    rv_quad(g, seed, row0 + r, q, K, row, t);
#pragma unroll
    for (int c = 0; c < 4; ++c) sum += t[c] * t[c];      // the square rounded, then added; k < k0 and k >= K add +0.0: no bit changes
  }
  const double energy = wg_reduce<WG_ALL, WG_SUM>(wave_sum_d(sum), red, threadIdx.x >> 6, threadIdx.x & 63);
  const double s = energy > 0.0 ? sqrt(1.0 / (row.drr * energy)) : 0.0;
  float* __restrict__ h = rirs + r * ld;
  for (int q = threadIdx.x; q < quads; q += 256) {
    const bool tail = 4 * q + 3 >= row.k0 && s != 0.0;
    if (tail) rv_quad(g, seed, row0 + r, q, K, row, t);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = 4 * q + c;
      if (k < K) h[k] = k == 0 ? 1.f : ((tail && k >= row.k0) ? (float)(s * t[c]) : 0.f);
    }
  }
}

// one block of 8 taps at chunk offset kr (a multiple of 8), tap k0 first, into the thread's 8 x 4 partial sums.  GUARD: the term of
// output i and tap k counts when k <= klim + i (the tap that reads the row's floor sample, one further per output) and k <= kcap = K - 1.
template <bool GUARD>
__device__ __forceinline__ void rv_block(const double* __restrict__ hs, const double* __restrict__ xs, int kr, int k0, int64_t klim,
                                         int kcap, double (&acc)[RV_PER][4]) {
  // the window: samples unit .. unit + 14, unit a multiple of 8: two runs of 8 samples, each four 16-byte reads (the sixteenth
  // sample is read and not used; behind the span's last sample it is whatever the LDS holds)
  const int unit = RV_PER * (int)threadIdx.x - kr + RV_KC - 8;
  const rv_d2* __restrict__ wp = reinterpret_cast<const rv_d2*>(xs + rv_slot(unit));
  const rv_d2* __restrict__ hp = reinterpret_cast<const rv_d2*>(hs + kr);
  double w[16], h[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const rv_d2 a = wp[j], b = wp[5 + j], c = hp[j];      // the second run starts 80 B = 5 reads after the first
    w[2 * j] = a.x, w[2 * j + 1] = a.y;
    w[8 + 2 * j] = b.x, w[8 + 2 * j + 1] = b.y;
    h[2 * j] = c.x, h[2 * j + 1] = c.y;
  }
  // output i, tap k0 + u reads sample (n0 + i) - (k0 + u): window element 7 + i - u
#pragma unroll
  for (int u = 0; u < 8; ++u) {
#pragma unroll
    for (int i = 0; i < RV_PER; ++i) {
      if (!GUARD || (k0 + u <= klim + i && k0 + u <= kcap)) acc[i][u & 3] = fma(h[u], w[7 + i - u], acc[i][u & 3]);
    }
  }
}

__global__ __launch_bounds__(RV_THREADS) void reverb_kernel(const float* __restrict__ src, int64_t n_src,
                                                            const int64_t* __restrict__ start, const int64_t* __restrict__ floor_,
                                                            int64_t L, int64_t tiles, const float* __restrict__ rirs, int64_t n_rirs,
                                                            int64_t ld_rir, int K, const int32_t* __restrict__ rir_index,
                                                            float* __restrict__ out, int64_t ld_out) {
  __shared__ __attribute__((aligned(16))) double hs[RV_KC];
  __shared__ __attribute__((aligned(16))) double xs[(RV_SPAN / 8 + 1) * 10];
  const int64_t b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * RV_TILE;
  const int64_t s0 = bank_clamp(start[b], n_src - L);
  const int64_t fl = bank_clamp(floor_[b], s0);
  const float* __restrict__ h = rirs + bank_clamp(rir_index[b], n_rirs - 1) * ld_rir;
  const int64_t n0 = t0 + RV_PER * (int64_t)threadIdx.x;      // the thread's first output
  const int64_t reach = s0 + n0 - fl;                          // the tap of output n0 that reads the floor sample
  const int64_t klim = reach < K - 1 ? reach : K - 1;          // output n0 + i ends at min(klim + i, K - 1)
  // the tile's last output reaches furthest back: chunks past its last tap hold no term of the tile
  const int64_t tile_last = s0 + (t0 + RV_TILE - 1 < L - 1 ? t0 + RV_TILE - 1 : L - 1) - fl;
  const int k_end = (int)(tile_last < K - 1 ? tile_last : K - 1) + 1;
  double acc[RV_PER][4];
#pragma unroll
  for (int i = 0; i < RV_PER; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  }
  for (int c0 = 0; c0 < k_end; c0 += RV_KC) {
    if (c0) __syncthreads();                                   // the previous chunk has been read
    for (int i = threadIdx.x; i < RV_KC; i += RV_THREADS) hs[i] = c0 + i < K ? (double)h[c0 + i] : 0.0;
    const int64_t pbase = s0 + t0 - c0 - (RV_KC - 1);          // the sample in slot 0
    for (int i = threadIdx.x; i < RV_SPAN; i += RV_THREADS) {
      const int64_t p = pbase + i;
      xs[rv_slot(i)] = (p >= fl && p < s0 + L) ? (double)src[p] : 0.0;
    }
    __syncthreads();
    if (n0 < L) {
      for (int kr = 0; kr < RV_KC; kr += 8) {
        const int k0 = c0 + kr;
        if (k0 > klim + (RV_PER - 1) || k0 >= K) break;        // no output of the thread has a tap from here on
        if (k0 + 7 <= klim) rv_block<false>(hs, xs, kr, k0, klim, K - 1, acc);
        else rv_block<true>(hs, xs, kr, k0, klim, K - 1, acc);
      }
    }
  }
  if (n0 < L) {
    float* __restrict__ o = out + b * ld_out + n0;
#pragma unroll
    for (int i = 0; i < RV_PER; ++i) {
      if (n0 + i < L) o[i] = (float)((acc[i][0] + acc[i][1]) + (acc[i][2] + acc[i][3]));
    }
  }
}

inline bool rv_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
// [a, a + na) and [b, b + nb) floats share no element
inline bool rv_disjoint(const float* a, int64_t na, const float* b, int64_t nb) { return a + na <= b || b + nb <= a; }

}  // namespace

extern "C" int maavss_rir_max_taps(void) { return RV_MAX_K; }

extern "C" int maavss_rir_synth(const double* params, const float* noise, int64_t ld_noise, uint64_t seed, int64_t row0, int64_t n_rirs,
                                int K, float* rirs, int64_t ld_rir, void* stream) {
  MAAVSS_CHECK_ARG(params && rirs, "rir_synth: null pointer");
  MAAVSS_CHECK_ARG(n_rirs >= 1 && row0 >= 0 && row0 + n_rirs <= RV_MAX_ROWS, "rir_synth: rows [%lld, %lld + %lld) must lie in [0, %lld)",
                   (long long)row0, (long long)row0, (long long)n_rirs, (long long)RV_MAX_ROWS);
  MAAVSS_CHECK_ARG(K >= 1 && K <= RV_MAX_K, "rir_synth: K = %d must be in [1, %d]", K, RV_MAX_K);
  MAAVSS_CHECK_ARG(ld_rir >= K && (!noise || ld_noise >= K), "rir_synth: ld_rir = %lld / ld_noise = %lld are shorter than K = %d", (long long)ld_rir,
                   (long long)ld_noise, K);
  MAAVSS_CHECK_ARG(rv_aligned(params, 8) && rv_aligned(rirs, 4) && rv_aligned(noise, 4), "rir_synth: params must be 8-byte aligned, rirs and noise 4-byte");
  MAAVSS_CHECK_ARG(!noise || rv_disjoint(rirs, (n_rirs - 1) * ld_rir + K, noise, (n_rirs - 1) * ld_noise + K), "rir_synth: rirs overlaps noise");
  hipLaunchKernelGGL(rir_synth_kernel, dim3((unsigned)n_rirs), dim3(256), 0, (hipStream_t)stream, params, noise, ld_noise, seed, row0, K, rirs,
                     ld_rir);
  MAAVSS_LAUNCH_CHECK("rir_synth_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_reverb(const float* src, int64_t n_src, const int64_t* start, const int64_t* floor, const int64_t* host_start,
                             const int64_t* host_floor, int64_t B, int64_t L, const float* rirs, int64_t n_rirs, int64_t ld_rir, int K,
                             const int32_t* rir_index, const int32_t* host_rir_index, float* out, int64_t ld_out, void* stream) {
  MAAVSS_CHECK_ARG(src && start && floor && host_start && host_floor && rirs && rir_index && host_rir_index && out, "reverb: null pointer");
  MAAVSS_CHECK_ARG(B >= 1 && L >= 1 && n_src >= L, "reverb: B = %lld, L = %lld must be positive and n_src = %lld at least L", (long long)B,
                   (long long)L, (long long)n_src);
  MAAVSS_CHECK_ARG(K >= 1 && K <= RV_MAX_K, "reverb: K = %d must be in [1, %d]", K, RV_MAX_K);
  MAAVSS_CHECK_ARG(n_rirs >= 1 && ld_rir >= K, "reverb: n_rirs = %lld must be positive and ld_rir = %lld at least K = %d", (long long)n_rirs,
                   (long long)ld_rir, K);
  MAAVSS_CHECK_ARG(B == 1 || ld_out >= L, "reverb: ld_out = %lld is shorter than a row of %lld samples", (long long)ld_out, (long long)L);
  MAAVSS_CHECK_ARG(rv_aligned(start, 8) && rv_aligned(floor, 8) && rv_aligned(rir_index, 4) && rv_aligned(src, 4) && rv_aligned(rirs, 4) &&
                       rv_aligned(out, 4),
                   "reverb: start and floor must be 8-byte aligned, src, rirs, rir_index and out 4-byte");
  const int64_t tiles = (L + RV_TILE - 1) / RV_TILE;
  MAAVSS_CHECK_ARG(L < (int64_t)1 << 40 && B <= 0x7fffffff / tiles, "reverb: %lld rows of %lld samples exceed the grid", (long long)B, (long long)L);
  const int64_t out_span = (B - 1) * ld_out + L;
  MAAVSS_CHECK_ARG(rv_disjoint(out, out_span, src, n_src), "reverb: out overlaps src");
  MAAVSS_CHECK_ARG(rv_disjoint(out, out_span, rirs, (n_rirs - 1) * ld_rir + K), "reverb: out overlaps rirs");
  for (int64_t b = 0; b < B; ++b) {
    MAAVSS_CHECK_ARG(host_start[b] >= 0 && host_start[b] <= n_src - L, "reverb: row %lld (samples [%lld, %lld + %lld)) lies outside src's %lld samples",
                     (long long)b, (long long)host_start[b], (long long)host_start[b], (long long)L, (long long)n_src);
    MAAVSS_CHECK_ARG(host_floor[b] >= 0 && host_floor[b] <= host_start[b], "reverb: row %lld: floor %lld must be in [0, start = %lld]", (long long)b,
                     (long long)host_floor[b], (long long)host_start[b]);
    MAAVSS_CHECK_ARG(host_rir_index[b] >= 0 && host_rir_index[b] < n_rirs, "reverb: row %lld: response %d is outside [0, %lld)", (long long)b,
                     host_rir_index[b], (long long)n_rirs);
  }
  hipLaunchKernelGGL(reverb_kernel, dim3((unsigned)(B * tiles)), dim3(RV_THREADS), 0, (hipStream_t)stream, src, n_src, start, floor, L, tiles,
                     rirs, n_rirs, ld_rir, K, rir_index, out, ld_out);
  MAAVSS_LAUNCH_CHECK("reverb_kernel");
  return MAAVSS_OK;
}
