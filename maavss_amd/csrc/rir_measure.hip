// Room-acoustic figures of a table of room responses (maavss_amd.Reverb.measure): energy, EDT, T20, T30, C50 and the
// direct-to-reverberant ratio of every row, from the Schroeder backward integral of its squared taps.  include/maavss.h holds the
// definition, operation by operation; tests/rir_measure_twin.py restates it in float64.  Compiled with -ffp-contract=off (Makefile):
// every f64 operation below is rounded on its own, in the order written.  The squares are exact in f64 (two f32 factors), so only the
// order of the additions matters, and it is ONE order: no atomic, and nothing that depends on the launch.
//   rir_measure   one workgroup of 256 per row; the row is never held whole.  It is cut into blocks of RM_BLOCK = 32 taps and visited in
//                 chunks of 256 blocks (8192 taps) that are staged through LDS with coalesced loads, 33 floats a block so that the 64
//                 lanes of a wave read 64 different banks; thread t owns block 256 c + t of chunk c.
//                 Pass A (chunks ascending): the block's total from its last tap towards its first, and its two forward partial sums
//                 (taps in front of k_direct / k_early, first tap towards last).  Thread 0 then turns the totals into carries from the
//                 last block towards the first (C[b] = C[b + 1] + T[b + 1]; E[0] falls out), threads 64 and 128 add the forward
//                 partials from the first block on: three serial chains of at most 1024 additions, side by side.
//                 Pass B (chunks descending; the last chunk is still staged): every thread forms its block's suffix sums again,
//                 E[k] = s[k] + C[b], compares each with the four thresholds E[0] c and keeps, per level, its lowest k >= 1 with
//                 E[k] <= E[0] c together with E[k] and E[k - 1] (the predecessor of a block's first tap is its own square plus the
//                 previous block's carry).  The lowest k of the row is a minimum of integers below 2^24 taken as floats through
//                 reduce.h (wave_min, WG_MIN): exact, and no order to state.  The owner of the crossing leaves its two energies in
//                 LDS, ten threads take one log10 each, thread 0 writes the row's six figures.
#include "metric_f64.h"

namespace {

constexpr int RM_THREADS = 256, RM_BLOCK = 32, RM_PAD = RM_BLOCK + 1;
constexpr int RM_CHUNK = RM_THREADS * RM_BLOCK;                  // taps staged at a time
constexpr int RM_MAX_K = 32768;                                  // reverb.hip's tap cap
constexpr int RM_MAX_BLOCKS = RM_MAX_K / RM_BLOCK;
constexpr int64_t RM_MAX_ROWS = (int64_t)1 << 19;                // the table's row cap (reverb.hip's)
constexpr int RM_AHEAD = 16;                                     // loads a thread keeps in flight while it stages a chunk
constexpr int RM_BATCH = 16;                                   // block totals the carry chain reads ahead
constexpr int RM_LEVELS = 4;                                   // -5, -10, -25, -35 dB
constexpr int RM_NONE = 0x7fffffff;                              // no crossing
constexpr float RM_NONE_F = 1e9f;

struct rm_thresholds {
  double c[RM_LEVELS];
};

__device__ __forceinline__ double rm_level_db(int l) { return l == 0 ? -5.0 : (l == 1 ? -10.0 : (l == 2 ? -25.0 : -35.0)); }
__device__ __forceinline__ double rm_sq(float x) {
  const double d = (double)x;
  return d * d;
}

__device__ __forceinline__ void rm_stage(float* tile, const float* __restrict__ h, int c0, int K) {
  const int n = K - c0 < RM_CHUNK ? K - c0 : RM_CHUNK;
  // RM_AHEAD loads a thread in flight before the first is stored: a loop of load, store, load pays the memory's latency every time
  for (int i0 = threadIdx.x; i0 < n; i0 += RM_AHEAD * RM_THREADS) {
    float v[RM_AHEAD];
#pragma unroll
    for (int u = 0; u < RM_AHEAD; ++u) {
      const int i = i0 + u * RM_THREADS;
      v[u] = i < n ? h[c0 + i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < RM_AHEAD; ++u) {
      const int i = i0 + u * RM_THREADS;
      if (i < n) tile[(i >> 5) * RM_PAD + (i & (RM_BLOCK - 1))] = v[u];
    }
  }
}

__global__ __launch_bounds__(RM_THREADS) void rir_measure_kernel(const float* __restrict__ rirs, int64_t ld, int K, double sr, int k_direct,
                                                                 int k_early, rm_thresholds thr, double* __restrict__ out) {
  __shared__ float tile[RM_THREADS * RM_PAD];
  __shared__ double carry[RM_MAX_BLOCKS];                        // pass A: the block totals T[b]; then the carries C[b]
  __shared__ double fwd[2][RM_MAX_BLOCKS];                       // forward partial sums in front of k_direct / k_early
  __shared__ double scal[5];                                     // E[0], early and late at k_direct, early and late at k_early
  __shared__ double cross[RM_LEVELS][2];                         // E[j - 1], E[j] of each level's crossing
  __shared__ double dbs[2 * RM_LEVELS + 2];
  __shared__ float red[RM_THREADS / 64][RM_LEVELS];
  const float* __restrict__ h = rirs + (int64_t)blockIdx.x * ld;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nblk = (K + RM_BLOCK - 1) / RM_BLOCK, nchunk = (K + RM_CHUNK - 1) / RM_CHUNK;
  const float* row = tile + tid * RM_PAD;

  // ---- pass A: block totals (last tap towards first) and forward partials (first tap towards last)
  for (int c = 0; c < nchunk; ++c) {
    if (c) __syncthreads();
    rm_stage(tile, h, c * RM_CHUNK, K);
    __syncthreads();
    const int b = c * RM_THREADS + tid;
    if (b < nblk) {
      const int first = b * RM_BLOCK, cnt = K - first < RM_BLOCK ? K - first : RM_BLOCK;
      double s = 0.0, fd = 0.0, fe = 0.0;
#pragma unroll
      for (int i = RM_BLOCK - 1; i >= 0; --i)
        if (i < cnt) s = s + rm_sq(row[i]);
#pragma unroll
      for (int i = 0; i < RM_BLOCK; ++i) {
        if (i < cnt) {
          const double q = rm_sq(row[i]);
          if (first + i < k_direct) fd = fd + q;
          if (first + i < k_early) fe = fe + q;
        }
      }
      carry[b] = s, fwd[0][b] = fd, fwd[1][b] = fe;
    }
  }
  __syncthreads();
  if (tid == 0) {                                                // C[nblk - 1] = 0, C[b] = C[b + 1] + T[b + 1]; E[0] = C[0] + T[0]
    double c = 0.0;
    for (int b0 = nblk - 1; b0 >= 0; b0 -= RM_BATCH) {          // RM_BATCH totals read at once: the chain waits for additions, not for LDS
      double t[RM_BATCH];
#pragma unroll
      for (int i = 0; i < RM_BATCH; ++i) t[i] = b0 - i >= 0 ? carry[b0 - i] : 0.0;
#pragma unroll
      for (int i = 0; i < RM_BATCH; ++i) {
        if (b0 - i >= 0) {
          carry[b0 - i] = c;
          c = c + t[i];
        }
      }
    }
    scal[0] = c;
    scal[2] = 0.0, scal[4] = 0.0;                                // late = 0 when the boundary lies at or behind K
  } else if (tid == 64 || tid == 128) {
    const int w = tid == 64 ? 0 : 1, kb = w ? k_early : k_direct;
    const int nb = kb >= K ? nblk : (kb + RM_BLOCK - 1) / RM_BLOCK;
    double e = 0.0;
#pragma unroll 16
    for (int b = 0; b < nb; ++b) e = e + fwd[w][b];
    scal[1 + 2 * w] = e;
  } else if (tid >= 192 && tid < 192 + 2 * RM_LEVELS) {
    (&cross[0][0])[tid - 192] = nan_d();
  }
  __syncthreads();
  const double e0 = scal[0];
  double lim[RM_LEVELS], ej[RM_LEVELS], em1[RM_LEVELS];
  int jl[RM_LEVELS];
#pragma unroll
  for (int l = 0; l < RM_LEVELS; ++l) lim[l] = e0 * thr.c[l], ej[l] = 0.0, em1[l] = 0.0, jl[l] = RM_NONE;

  // ---- pass B: E[k] = s[k] + C[b] against the thresholds; a thread's taps come in descending order, so its last hit is its lowest
  for (int c = nchunk - 1; c >= 0; --c) {
    if (c != nchunk - 1) {
      __syncthreads();
      rm_stage(tile, h, c * RM_CHUNK, K);
      __syncthreads();
    }
    const int b = c * RM_THREADS + tid;
    if (b < nblk) {
      const int first = b * RM_BLOCK, cnt = K - first < RM_BLOCK ? K - first : RM_BLOCK;
      const double cb = carry[b];
      double s = 0.0;
#pragma unroll
      for (int i = RM_BLOCK - 1; i >= 0; --i) {
        if (i < cnt) {
          const int k = first + i;
          s = s + rm_sq(row[i]);
          const double e = s + cb;
#pragma unroll
          for (int l = 0; l < RM_LEVELS; ++l) {
            if (jl[l] == k + 1) em1[l] = e;
            if (k >= 1 && e <= lim[l]) jl[l] = k, ej[l] = e;
          }
          if (k == k_direct) scal[2] = e;
          if (k == k_early) scal[4] = e;
        }
      }
      if (first >= 1) {                                          // E[first - 1] = s[first - 1] + C[b - 1], s of a block's last tap its square
        const double e = rm_sq(h[first - 1]) + carry[b - 1];
#pragma unroll
        for (int l = 0; l < RM_LEVELS; ++l)
          if (jl[l] == first) em1[l] = e;
      }
    }
  }
  float jf[RM_LEVELS];
#pragma unroll
  for (int l = 0; l < RM_LEVELS; ++l) jf[l] = wave_min(jl[l] == RM_NONE ? RM_NONE_F : (float)jl[l]);
  wg_reduce<WG_ALL, WG_MIN>(jf, red, wave, lane);
#pragma unroll
  for (int l = 0; l < RM_LEVELS; ++l)
    if (jl[l] != RM_NONE && (float)jl[l] == jf[l]) cross[l][0] = em1[l], cross[l][1] = ej[l];
  __syncthreads();
  if (tid < 2 * RM_LEVELS) {
    dbs[tid] = 10.0 * log10((&cross[0][0])[tid] / e0);
  } else if (tid == 64 || tid == 128) {
    const int w = tid == 64 ? 0 : 1;
    dbs[2 * RM_LEVELS + w] = 10.0 * log10(scal[1 + 2 * w] / scal[2 + 2 * w]);
  }
  __syncthreads();
  if (tid == 0) {
    double t[RM_LEVELS];
#pragma unroll
    for (int l = 0; l < RM_LEVELS; ++l) {
      const double da = dbs[2 * l], db = dbs[2 * l + 1];
      t[l] = jf[l] < RM_NONE_F ? (double)((int)jf[l] - 1) + (da - rm_level_db(l)) / (da - db) : nan_d();
    }
    double* o = out + (int64_t)blockIdx.x * 6;
    o[0] = e0;
    o[1] = (6.0 * t[1]) / sr;
    o[2] = (3.0 * (t[2] - t[0])) / sr;
    o[3] = (2.0 * (t[3] - t[0])) / sr;
    o[4] = dbs[2 * RM_LEVELS + 1];
    o[5] = dbs[2 * RM_LEVELS];
  }
}

}  // namespace

extern "C" int maavss_rir_measure(const float* rirs, int64_t n_rows, int K, int64_t ld_rir, double sr, int k_direct, int k_early,
                                  const double* thresholds, int n_thresholds, double* out, void* stream) {
  MAAVSS_CHECK_ARG(rirs && thresholds && out, "rir_measure: null pointer");
  MAAVSS_CHECK_ARG(n_rows >= 1 && n_rows <= RM_MAX_ROWS, "rir_measure: n_rows = %lld must be in [1, %lld]", (long long)n_rows, (long long)RM_MAX_ROWS);
  MAAVSS_CHECK_ARG(K >= 1 && K <= RM_MAX_K, "rir_measure: K = %d must be in [1, %d]", K, RM_MAX_K);
  MAAVSS_CHECK_ARG(ld_rir >= K && ld_rir < (int64_t)1 << 40, "rir_measure: ld_rir = %lld must be at least K = %d", (long long)ld_rir, K);
  MAAVSS_CHECK_ARG(sr > 0.0 && sr < 1e9, "rir_measure: sr = %g must be positive and finite", sr);
  MAAVSS_CHECK_ARG(k_direct >= 0 && k_early >= 0, "rir_measure: k_direct = %d and k_early = %d must not be negative", k_direct, k_early);
  MAAVSS_CHECK_ARG(n_thresholds == RM_LEVELS, "rir_measure: n_thresholds = %d, the figures need the %d levels -5, -10, -25, -35 dB", n_thresholds,
                   RM_LEVELS);
  rm_thresholds thr;
  for (int l = 0; l < RM_LEVELS; ++l) {
    thr.c[l] = thresholds[l];
    MAAVSS_CHECK_ARG(thr.c[l] > 0.0 && thr.c[l] < (l ? thr.c[l - 1] : 1.0), "rir_measure: thresholds[%d] = %g: the thresholds must descend inside (0, 1)", l,
                     thr.c[l]);
  }
  MAAVSS_CHECK_ARG(((uintptr_t)rirs & 3) == 0 && ((uintptr_t)out & 7) == 0, "rir_measure: rirs must be 4-byte aligned, out 8-byte");
  hipLaunchKernelGGL(rir_measure_kernel, dim3((unsigned)n_rows), dim3(RM_THREADS), 0, (hipStream_t)stream, rirs, ld_rir, K, sr, k_direct, k_early, thr,
                     out);
  MAAVSS_LAUNCH_CHECK("rir_measure_kernel");
  return MAAVSS_OK;
}
