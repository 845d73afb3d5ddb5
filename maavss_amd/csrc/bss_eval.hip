// EXTENSION (the reference reports its training loss only): BSS-eval SDR, SIR and SAR (Vincent et al. 2006) of est [rows][n] against a known
// target and K known other sources, with a time-invariant distortion filter of L taps, per row, all arithmetic f64 over the f32 data in a
// fixed order -- what maavss_amd.bss_eval_metrics and Validator(bss_filter=...) read.  include/maavss.h states the definition;
// tests/bss_twin.py is its float64 restatement and the contract.
//
//   screen    one workgroup per (row, signal, chunk of BS_CCH samples): the sum of the exact squares and a flag for a non-finite sample
//   plan      one wave per row adds the chunks in index order: status 1 (non-finite) or 2 (silent target), the live sources, J, n = J L
//   corr      one workgroup per (row, ordered pair (a, b), chunk): c[d] = sum_m a[m] b[m + d] for the lags d < L, thread d (and d + 256),
//             exact products added in sample order; b is a live source or the estimate.  corr_sum adds the chunks in index order
//   gram      the row's matrix in the workspace, 64 x 64 tiles, lower triangle: G[(a, t), (b, u)] = c_ab[t - u] (c_ba[u - t] below zero),
//             padded to whole tiles with the identity, and under it one more tile row whose first row is the right-hand side A^T e
//   cholesky  right-looking, one tile column k per step and two launches: `panel` (every workgroup factors the diagonal tile for itself,
//             in registers, then one wave solves its own tile's 64 rows against it, a row per lane in registers) and `update` (one workgroup
//             per trailing tile, C -= P_i P_j^T with both panel tiles in LDS, 4 x 4 per thread, k in index order).  The right-hand-side
//             tile row is solved and updated like any other, so when the last step is done its first row is y = Lf^-1 A^T e: the forward
//             substitution costs nothing of its own.  The factored diagonal tiles are kept beside the matrix, not in it: within a
//             panel launch every workgroup reads the unfactored tile, whenever it starts.  The leading L x L block of the factor is the factor of the target's own Gram
//             matrix and y[0..L) its forward substitution, so the target projection needs no second factorisation
//   backsolve one workgroup per (row, projection): Lf^T c = y from the last tile up, the diagonal tile inside one wave
//   fir       one workgroup per (row, BS_FCH outputs): p_t and p from the coefficients and the sources in LDS, the five sums directly
//   finalize  one wave per row adds the fir partials in index order and writes the row
// A workgroup whose row has a status, or fewer tiles than the launch was sized for, leaves at once.  No floating-point atomic; every sum
// has one order, so two runs give the same bytes, and a row's bytes do not depend on the other rows of the call.  The Makefile compiles
// this file with -ffp-contract=off; the fma() calls are the fusions there are.
// Plain f64 VALU arithmetic: the MFMA f64 instructions were not tried (HISTORY.md gives the measured times per stage).
#include "common.h"
#include "metric_f64.h"

#define BS_LMAX 512
#define BS_KMAX 3
#define BS_NB 64                     // tile edge
#define BS_LD 65                     // LDS stride of a tile row (doubles)
#define BS_CCH 2048                  // samples per correlation / screening chunk
#define BS_FCH 1024                  // outputs per fir workgroup
#define BS_COLS 10                   // out row: s_tt, s_ee, s_ii, s_aa, s_pp, sdr_db, sir_db, sar_db, n_sources, status
#define BS_META 8                    // ints per row: J, status, mask of live slots, n = J L, live[0..3]

struct bs_in {
  const float* est;
  int64_t est_stride;
  const float* ref;
  int64_t ref_stride;
  const float* oth;
  int64_t oth_row, oth_src;
  int64_t N;
  int K, L;
};
// signal s of a row: 0 the target, 1..K the other sources, K + 1 the estimate
__device__ __forceinline__ const float* bs_sig(const bs_in& in, int64_t row, int s) {
  if (s == 0) return in.ref + row * in.ref_stride;
  if (s == in.K + 1) return in.est + row * in.est_stride;
  return in.oth + row * in.oth_row + (int64_t)(s - 1) * in.oth_src;
}

struct bs_plan {
  int nsig, njobs, nbt;              // K + 2 signals; (K + 1) (K + 2) ordered pairs (a, b); tile rows of the largest matrix
  int64_t ld, msz, ncc, nfc;         // leading dimension 64 nbt; doubles per row's matrix (64 nbt + 64) ld; chunks; fir chunks
  int64_t o_en, o_cpart, o_corr, o_mat, o_dtile, o_coef, o_fpart, bytes;
};
static inline bs_plan bs_make_plan(int64_t rows, int64_t N, int K, int L) {
  bs_plan p;
  p.nsig = K + 2;
  p.njobs = (K + 1) * (K + 2);
  p.nbt = ((K + 1) * L + BS_NB - 1) / BS_NB;
  p.ld = (int64_t)p.nbt * BS_NB;
  p.msz = (p.ld + BS_NB) * p.ld;
  p.ncc = (N + BS_CCH - 1) / BS_CCH;
  p.nfc = (N + L - 1 + BS_FCH - 1) / BS_FCH;
  p.o_en = align256(rows * BS_META * 4);
  p.o_cpart = p.o_en + align256(rows * p.nsig * p.ncc * 2 * 8);
  p.o_corr = p.o_cpart + align256(rows * p.njobs * p.ncc * L * 8);
  p.o_mat = p.o_corr + align256(rows * p.njobs * L * 8);
  p.o_dtile = p.o_mat + align256(rows * p.msz * 8);
  p.o_coef = p.o_dtile + align256(rows * p.nbt * BS_NB * BS_NB * 8);
  p.o_fpart = p.o_coef + align256(rows * 2 * p.ld * 8);
  p.bytes = p.o_fpart + align256(rows * p.nfc * 5 * 8);
  return p;
}

// the value lane `lane` (uniform over the wave) holds
__device__ __forceinline__ double bs_readlane_d(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

__global__ __launch_bounds__(256) void bss_screen_kernel(bs_in in, int64_t ncc, double* __restrict__ en) {
  __shared__ double red[4][2];
  const int nsig = in.K + 2;
  const int64_t c = blockIdx.x % ncc, row = blockIdx.x / (ncc * nsig);
  const int s = (int)((blockIdx.x / ncc) % nsig);
  const float* __restrict__ x = bs_sig(in, row, s) + c * BS_CCH;
  const int len = (int)(in.N - c * BS_CCH < BS_CCH ? in.N - c * BS_CCH : BS_CCH);
  const int tid = threadIdx.x;
  double e = 0.0, bad = 0.0;
  for (int k = tid; k < len; k += 256) {
    const double v = (double)x[k];
    bad += __builtin_isfinite(v) ? 0.0 : 1.0;
    e = fma(v, v, e);                           // an exact product of f32 values
  }
  double v[2] = {wave_sum_d(e), wave_sum_d(bad)};
  wg_reduce<WG_THREAD0, WG_SUM>(v, red, tid >> 6, tid & 63);
  if (tid == 0) {
    en[2 * (int64_t)blockIdx.x] = v[0];
    en[2 * (int64_t)blockIdx.x + 1] = v[1];
  }
}

// one wave per row
__global__ __launch_bounds__(64) void bss_plan_kernel(const double* __restrict__ en, int64_t ncc, int K, int L, int* __restrict__ meta) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  double bad = 0.0;
  int mask = 0, J = 0, live[BS_KMAX + 1] = {0, 0, 0, 0};
  for (int s = 0; s < K + 2; ++s) {
    const double* __restrict__ p = en + (row * (K + 2) + s) * ncc * 2;
    const double e = wave_strided_sum_d(p, ncc, 2, lane);
    bad += wave_strided_sum_d(p + 1, ncc, 2, lane);
    if (s <= K && e != 0.0) {                   // a sum of squares is 0 only when every sample is: the order cannot matter here
      mask |= 1 << s;
      if (s > 0) live[++J] = s;                 // live[0] = 0, the target's place
    }
  }
  if (lane != 0) return;
  int status = 0;
  if (bad != 0.0) status = 1;
  else if (!(mask & 1)) status = 2;
  J = status == 0 ? J + 1 : 0;
  int* __restrict__ m = meta + row * BS_META;
  m[0] = J;
  m[1] = status;
  m[2] = status == 0 ? mask : 0;
  m[3] = J * L;
  for (int q = 0; q < BS_KMAX + 1; ++q) m[4 + q] = live[q];
}

// is the ordered pair `job` = a (K + 2) + b of this row computed: a a live source, b a live source or the estimate
__device__ __forceinline__ bool bs_job_live(const int* __restrict__ m, int job, int K) {
  const int a = job / (K + 2), b = job % (K + 2);
  return m[1] == 0 && ((m[2] >> a) & 1) && (b == K + 1 || ((m[2] >> b) & 1));
}

// grid (chunk, job, row); thread d takes the lags d and d + 256
__global__ __launch_bounds__(256) void bss_corr_kernel(bs_in in, int64_t ncc, const int* __restrict__ meta, double* __restrict__ cpart) {
  __shared__ double A[BS_CCH], B[BS_CCH + BS_LMAX];
  const int64_t c = blockIdx.x, row = blockIdx.z;
  const int job = blockIdx.y, K = in.K, L = in.L;
  if (!bs_job_live(meta + row * BS_META, job, K)) return;       // uniform: no barrier was reached
  const int64_t m0 = c * BS_CCH;
  const float* __restrict__ a = bs_sig(in, row, job / (K + 2)) + m0;
  const float* __restrict__ b = bs_sig(in, row, job % (K + 2)) + m0;
  const int64_t left = in.N - m0;
  const int len = (int)(left < BS_CCH ? left : BS_CCH);
  const int tid = threadIdx.x;
  for (int k = tid; k < BS_CCH; k += 256) A[k] = k < len ? (double)a[k] : 0.0;
  for (int k = tid; k < BS_CCH + BS_LMAX; k += 256) B[k] = k < left ? (double)b[k] : 0.0;
  __syncthreads();
  double* __restrict__ o = cpart + ((row * gridDim.y + job) * ncc + c) * L;
  if (tid + 256 < L) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int k = 0; k < len; ++k) {
      const double x = A[k];
      s0 = fma(x, B[k + tid], s0);              // exact products of f32 values: one rounding, that of the sum
      s1 = fma(x, B[k + tid + 256], s1);
    }
    o[tid] = s0;
    o[tid + 256] = s1;
  } else if (tid < L) {
    double s0 = 0.0;
#pragma unroll 4
    for (int k = 0; k < len; ++k) s0 = fma(A[k], B[k + tid], s0);
    o[tid] = s0;
  }
}

// grid (ceil(L / 256), job, row): the chunks of one lag in index order
__global__ __launch_bounds__(256) void bss_corr_sum_kernel(const double* __restrict__ cpart, int64_t ncc, int K, int L,
                                                           const int* __restrict__ meta, double* __restrict__ corr) {
  const int64_t row = blockIdx.z;
  const int job = blockIdx.y, d = blockIdx.x * 256 + threadIdx.x;
  if (d >= L || !bs_job_live(meta + row * BS_META, job, K)) return;
  const double* __restrict__ p = cpart + (row * gridDim.y + job) * ncc * L + d;
  double s = 0.0;
  for (int64_t c = 0; c < ncc; ++c) s += p[c * L];
  corr[(row * gridDim.y + job) * L + d] = s;
}

// grid (tile row ti <= nbt, tile column tj < nbt, row); tile row nbt holds the right-hand side
__global__ __launch_bounds__(256) void bss_gram_kernel(const double* __restrict__ corr, int K, int L, int nbt, int64_t msz,
                                                       const int* __restrict__ meta, double* __restrict__ mat) {
  const int64_t row = blockIdx.z;
  const int ti = blockIdx.x, tj = blockIdx.y;
  const int* __restrict__ m = meta + row * BS_META;
  const int n = m[3], nbr = (n + BS_NB - 1) / BS_NB;
  if (m[1] != 0 || tj >= nbr || (ti < nbt && (ti >= nbr || ti < tj))) return;
  const int njobs = (K + 1) * (K + 2);
  const int64_t ld = (int64_t)nbt * BS_NB;
  const double* __restrict__ cr = corr + row * njobs * L;
  double* __restrict__ M = mat + row * msz;
  for (int idx = threadIdx.x; idx < BS_NB * BS_NB; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    const int gi = ti * BS_NB + r, gj = tj * BS_NB + c;
    double v;
    if (ti == nbt) {
      v = r == 0 && gj < n ? cr[(m[4 + gj / L] * (K + 2) + K + 1) * L + gj % L] : 0.0;
    } else if (gi < n && gj < n) {
      const int sa = m[4 + gi / L], sb = m[4 + gj / L], d = gi % L - gj % L;
      v = d >= 0 ? cr[(sa * (K + 2) + sb) * L + d] : cr[(sb * (K + 2) + sa) * L - d];
    } else {
      v = gi == gj ? 1.0 : 0.0;
    }
    M[(int64_t)gi * ld + gj] = v;
  }
}

#define BS_DP(r, c) Dp[(r) * ((r) + 1) / 2 + (c)]      // the lower triangle of the diagonal tile, packed by rows

// step k, grid (tile row i = k + blockIdx.x, row); the last one is the right-hand-side tile row (i = nbt).  The diagonal tile is factored
// in registers: thread (tr4, tc4) holds the 4 x 4 block of rows 4 tr4.., columns 4 tc4.. (the blocks on and under the diagonal work) and
// its own copy of the running diagonal of its four columns, so that the threads that hold column p know its pivot without being told:
// one barrier per column, for the scaled column that goes through LDS.
// The factored diagonal tile goes to `dtile`, not back in place: the other workgroups of the launch read the unfactored one, and a
// workgroup that starts late must still find it.
__global__ __launch_bounds__(256) void bss_panel_kernel(int k, int nbt, int64_t msz, int* __restrict__ meta, double* __restrict__ mat,
                                                        double* __restrict__ dtile) {
  __shared__ double Dp[BS_NB * (BS_NB + 1) / 2], Xs[BS_NB * BS_LD], col[2][BS_NB];
  __shared__ int flag;
  const int64_t row = blockIdx.y;
  const int i = k + blockIdx.x;
  int* __restrict__ m = meta + row * BS_META;
  const int nbr = (m[3] + BS_NB - 1) / BS_NB;
  if (m[1] != 0 || k >= nbr || (i >= nbr && i != nbt)) return;
  const int64_t ld = (int64_t)nbt * BS_NB;
  double* __restrict__ M = mat + row * msz;
  const double* __restrict__ Mk = M + ((int64_t)k * BS_NB) * ld + k * BS_NB;
  double* __restrict__ Mi = M + ((int64_t)i * BS_NB) * ld + k * BS_NB;
  const int tid = threadIdx.x, tr4 = tid >> 4, tc4 = tid & 15;
  const bool active = tr4 >= tc4;
  if (i != k)
    for (int idx = tid; idx < BS_NB * BS_NB; idx += 256) {
      const int r = idx >> 6, c = idx & 63;
      Xs[r * BS_LD + c] = Mi[(int64_t)r * ld + c];
    }
  double d[4][4], diag[4];
#pragma unroll
  for (int y = 0; y < 4; ++y) {
    diag[y] = Mk[(int64_t)(4 * tc4 + y) * ld + 4 * tc4 + y];
#pragma unroll
    for (int x = 0; x < 4; ++x) d[x][y] = active ? Mk[(int64_t)(4 * tr4 + x) * ld + 4 * tc4 + y] : 0.0;
  }
  if (tid == 0) flag = 0;
  __syncthreads();
#pragma unroll
  for (int p = 0; p < BS_NB; ++p) {
    const int pb = p >> 2, py = p & 3;
    if (tc4 == pb && tr4 >= pb) {               // the threads that hold column p: scale it, hand it on (rows above p: never read)
      const double piv = diag[py], s = sqrt(piv);
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int r = 4 * tr4 + x;
        const double l = r == p ? s : d[x][py] / s;
        d[x][py] = l;
        col[p & 1][r] = l;
      }
      if (tr4 == pb && (!(piv > 0.0) || !__builtin_isfinite(piv))) flag = 1;
    }
    __syncthreads();                            // col[p & 1] is written again two columns on, behind the next barrier
    if (active && 4 * tc4 + 3 > p) {
      double lr[4], lc[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        lr[x] = col[p & 1][4 * tr4 + x];
        lc[x] = col[p & 1][4 * tc4 + x];
      }
#pragma unroll
      for (int y = 0; y < 4; ++y)
        if (4 * tc4 + y > p) {
          diag[y] = fma(-lc[y], lc[y], diag[y]);
#pragma unroll
          for (int x = 0; x < 4; ++x) d[x][y] = fma(-lr[x], lc[y], d[x][y]);
        }
    }
  }
  if (i == k) {
    if (active) {
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y)
          if (4 * tc4 + y <= 4 * tr4 + x) dtile[((row * nbt + k) * BS_NB + 4 * tr4 + x) * BS_NB + 4 * tc4 + y] = d[x][y];
    }
    __syncthreads();
    if (tid == 0 && flag) m[1] = 3;             // every later launch leaves this row alone
    return;
  }
  if (active) {
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y)
        if (4 * tc4 + y <= 4 * tr4 + x) BS_DP(4 * tr4 + x, 4 * tc4 + y) = d[x][y];
  }
  __syncthreads();
  if (tid < BS_NB) {                            // X Lkk^T = A: lane r owns row r; column c gets its terms in the order q = 0 .. c - 1
    double x[BS_NB];
#pragma unroll
    for (int c = 0; c < BS_NB; ++c) x[c] = Xs[tid * BS_LD + c];
#pragma unroll
    for (int q = 0; q < BS_NB; ++q) {
      x[q] = x[q] / BS_DP(q, q);
#pragma unroll
      for (int c = q + 1; c < BS_NB; ++c) x[c] = fma(-x[q], BS_DP(c, q), x[c]);
    }
#pragma unroll
    for (int c = 0; c < BS_NB; ++c) Xs[tid * BS_LD + c] = x[c];
  }
  __syncthreads();
  for (int idx = tid; idx < BS_NB * BS_NB; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    Mi[(int64_t)r * ld + c] = Xs[r * BS_LD + c];
  }
}

// step k, grid (i', j', row): tile (i, j) = (k + 1 + i', k + 1 + j') with j <= i; i' = nbt - k - 1 is the right-hand-side tile row
__global__ __launch_bounds__(256) void bss_update_kernel(int k, int nbt, int64_t msz, const int* __restrict__ meta, double* __restrict__ mat) {
  __shared__ double At[32 * BS_LD], Bt[32 * BS_LD];             // half of the panel's 64 columns at a time, [kk][r]
  const int64_t row = blockIdx.z;
  if (blockIdx.x < blockIdx.y) return;
  const int i = k + 1 + blockIdx.x, j = k + 1 + blockIdx.y;
  const int* __restrict__ m = meta + row * BS_META;
  const int nbr = (m[3] + BS_NB - 1) / BS_NB;
  if (m[1] != 0 || j >= nbr || (i >= nbr && i != nbt)) return;
  const int64_t ld = (int64_t)nbt * BS_NB;
  double* __restrict__ M = mat + row * msz;
  const double* __restrict__ Pi = M + ((int64_t)i * BS_NB) * ld + k * BS_NB;
  const double* __restrict__ Pj = M + ((int64_t)j * BS_NB) * ld + k * BS_NB;
  double* __restrict__ C = M + ((int64_t)i * BS_NB) * ld + j * BS_NB;
  const int tid = threadIdx.x, tr = (tid >> 4) * 4, tc = (tid & 15) * 4;
  double acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;
  for (int h = 0; h < 2; ++h) {
    if (h) __syncthreads();
    for (int idx = tid; idx < BS_NB * 32; idx += 256) {
      const int r = idx >> 5, kk = idx & 31;
      At[kk * BS_LD + r] = Pi[(int64_t)r * ld + h * 32 + kk];
      Bt[kk * BS_LD + r] = Pj[(int64_t)r * ld + h * 32 + kk];
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < 32; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        a[x] = At[kk * BS_LD + tr + x];
        b[x] = Bt[kk * BS_LD + tc + x];
      }
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], b[y], acc[x][y]);
    }
  }
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      double* __restrict__ p = C + (int64_t)(tr + x) * ld + tc + y;
      *p = *p - acc[x][y];
    }
}

// grid (projection, row): 0 the target's own (the leading L x L block), 1 the full one (only with J > 1)
__global__ __launch_bounds__(256) void bss_backsolve_kernel(int L, int nbt, int64_t msz, const int* __restrict__ meta,
                                                            const double* __restrict__ mat, const double* __restrict__ dtile,
                                                            double* __restrict__ coef) {
  __shared__ double yv[(BS_KMAX + 1) * BS_LMAX], D[BS_NB * BS_LD];
  const int64_t row = blockIdx.y;
  const int which = blockIdx.x;
  const int* __restrict__ m = meta + row * BS_META;
  if (m[1] != 0 || (which == 1 && m[0] < 2)) return;
  const int nloc = which == 0 ? L : m[3];
  const int nb = (nloc + BS_NB - 1) / BS_NB;
  const int64_t ld = (int64_t)nbt * BS_NB;
  const double* __restrict__ M = mat + row * msz;
  const int tid = threadIdx.x;
  for (int i = tid; i < nloc; i += 256) yv[i] = M[ld * ld + i];             // row 0 of the right-hand-side tile row
  for (int k = nb - 1; k >= 0; --k) {
    const int cnt = nloc - k * BS_NB < BS_NB ? nloc - k * BS_NB : BS_NB;
    __syncthreads();
    for (int idx = tid; idx < BS_NB * BS_NB; idx += 256) {
      const int r = idx >> 6, c = idx & 63;
      if (c <= r && r < cnt) D[r * BS_LD + c] = dtile[((row * nbt + k) * BS_NB + r) * BS_NB + c];
    }
    __syncthreads();
    if (tid < BS_NB) {
      double y = tid < cnt ? yv[k * BS_NB + tid] : 0.0;
      for (int c = cnt - 1; c >= 0; --c) {
        const double cv = bs_readlane_d(y, c) / D[c * BS_LD + c];
        if (tid < c) y = fma(-D[c * BS_LD + tid], cv, y);
        if (tid == c) y = cv;
      }
      if (tid < cnt) yv[k * BS_NB + tid] = y;
    }
    __syncthreads();
    for (int i = tid; i < k * BS_NB; i += 256) {
      double a = yv[i];
      const double* __restrict__ Lc = M + ((int64_t)k * BS_NB) * ld + i;     // column i of the tile row k: the loads do not wait for the sum
      if (cnt == BS_NB) {
#pragma unroll
        for (int c = 0; c < BS_NB; ++c) a = fma(-Lc[(int64_t)c * ld], yv[k * BS_NB + c], a);
      } else {
        for (int c = 0; c < cnt; ++c) a = fma(-Lc[(int64_t)c * ld], yv[k * BS_NB + c], a);
      }
      yv[i] = a;
    }
  }
  __syncthreads();
  for (int i = tid; i < nloc; i += 256) coef[(row * 2 + which) * ld + i] = yv[i];
}

// grid (chunk of BS_FCH outputs, row)
__global__ __launch_bounds__(256) void bss_fir_kernel(bs_in in, int nbt, int64_t nfc, const int* __restrict__ meta,
                                                      const double* __restrict__ coef, double* __restrict__ fpart) {
  __shared__ double ct[BS_LMAX], cf[(BS_KMAX + 1) * BS_LMAX];
  __shared__ float seg[BS_KMAX + 1][BS_FCH + BS_LMAX];
  __shared__ double red[4][5];
  const int64_t row = blockIdx.y, base = (int64_t)blockIdx.x * BS_FCH;
  const int* __restrict__ m = meta + row * BS_META;
  if (m[1] != 0) return;
  const int J = m[0], L = in.L, tid = threadIdx.x;
  const int64_t N = in.N, T = N + L - 1, ld = (int64_t)nbt * BS_NB;
  for (int t = tid; t < L; t += 256) ct[t] = coef[(row * 2) * ld + t];
  if (J > 1)
    for (int t = tid; t < J * L; t += 256) cf[t] = coef[(row * 2 + 1) * ld + t];
  for (int j = 0; j < J; ++j) {
    const float* __restrict__ s = bs_sig(in, row, m[4 + j]);
    for (int q = tid; q < BS_FCH + L - 1; q += 256) {
      const int64_t si = base - (L - 1) + q;
      seg[j][q] = si >= 0 && si < N ? s[si] : 0.f;
    }
  }
  __syncthreads();
  double pt[4] = {0.0, 0.0, 0.0, 0.0}, pf[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = 0; t < L; ++t) {
    const double c = ct[t];
    const float* __restrict__ sp = &seg[0][tid + L - 1 - t];
#pragma unroll
    for (int o = 0; o < 4; ++o) pt[o] = fma(c, (double)sp[256 * o], pt[o]);
  }
  if (J > 1) {
    for (int j = 0; j < J; ++j)
      for (int t = 0; t < L; ++t) {
        const double c = cf[j * L + t];
        const float* __restrict__ sp = &seg[j][tid + L - 1 - t];
#pragma unroll
        for (int o = 0; o < 4; ++o) pf[o] = fma(c, (double)sp[256 * o], pf[o]);
      }
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o) pf[o] = pt[o];  // one live source: p is p_t itself
  }
  const float* __restrict__ e = in.est + row * in.est_stride;
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int64_t n = base + tid + 256 * o;
    if (n < T) {
      const double en = n < N ? (double)e[n] : 0.0;
      const double de = en - pt[o], di = pf[o] - pt[o], da = en - pf[o];
      v[0] += pt[o] * pt[o];
      v[1] += de * de;
      v[2] += di * di;
      v[3] += da * da;
      v[4] += pf[o] * pf[o];
    }
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) v[q] = wave_sum_d(v[q]);
  wg_reduce<WG_THREAD0, WG_SUM>(v, red, tid >> 6, tid & 63);
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) fpart[(row * nfc + blockIdx.x) * 5 + q] = v[q];
  }
}

// one wave per row
__global__ __launch_bounds__(64) void bss_finalize_kernel(const double* __restrict__ fpart, int64_t nfc, const int* __restrict__ meta,
                                                          double* __restrict__ out) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int* __restrict__ m = meta + row * BS_META;
  double* __restrict__ o = out + row * BS_COLS;
  const int status = m[1];
  if (status != 0) {
    if (lane == 0) {
      for (int q = 0; q < 8; ++q) o[q] = nan_d();
      o[8] = (double)m[0];
      o[9] = (double)status;
    }
    return;
  }
  double s[5];
  for (int q = 0; q < 5; ++q) s[q] = wave_strided_sum_d(fpart + row * nfc * 5 + q, nfc, 5, lane);
  if (lane != 0) return;
  for (int q = 0; q < 5; ++q) o[q] = s[q];
  o[5] = 10.0 * log10(s[0] / s[1]);
  o[6] = 10.0 * log10(s[0] / s[2]);
  o[7] = 10.0 * log10(s[4] / s[3]);
  o[8] = (double)m[0];
  o[9] = 0.0;
}

static inline bool bs_sizes_ok(int64_t rows, int64_t n, int K, int L) {
  return rows >= 1 && rows <= 65535 && K >= 0 && K <= BS_KMAX && L >= 1 && L <= BS_LMAX && n >= (int64_t)(K + 1) * L && n < (int64_t)1 << 31 &&
         ((n + BS_CCH - 1) / BS_CCH) * (K + 2) <= (((int64_t)1 << 31) - 1) / rows;
}

extern "C" int64_t maavss_bss_eval_ws_bytes(int64_t rows, int64_t n, int K, int L) {
  if (!bs_sizes_ok(rows, n, K, L)) return 0;
  return bs_make_plan(rows, n, K, L).bytes;
}

extern "C" int maavss_bss_eval(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, const float* others,
                               int64_t others_row_stride, int64_t others_src_stride, int K, int64_t rows, int64_t n, int L, double* out,
                               void* ws, int64_t ws_bytes, void* stream) {
  MAAVSS_CHECK_ARG(est && ref && out && ws, "bss_eval: null pointer");
  MAAVSS_CHECK_ARG(K >= 0 && K <= BS_KMAX, "bss_eval: K = %d other sources, 0..%d are served", K, BS_KMAX);
  MAAVSS_CHECK_ARG(K == 0 || others, "bss_eval: K = %d but no other sources", K);
  MAAVSS_CHECK_ARG(L >= 1 && L <= BS_LMAX, "bss_eval: filter length %d, 1..%d are served", L, BS_LMAX);
  MAAVSS_CHECK_ARG(rows >= 1 && rows <= 65535, "bss_eval: %lld rows, 1..65535 per call are served", (long long)rows);
  MAAVSS_CHECK_ARG(n >= (int64_t)(K + 1) * L, "bss_eval: n = %lld samples are fewer than the (K + 1) L = %lld unknowns", (long long)n,
                   (long long)(K + 1) * L);
  MAAVSS_CHECK_ARG(bs_sizes_ok(rows, n, K, L), "bss_eval: %lld rows of %lld samples are beyond the kernels' index range", (long long)rows,
                   (long long)n);
  const int64_t lim = (int64_t)1 << 40;
  MAAVSS_CHECK_ARG(rows == 1 || (est_stride >= 0 && ref_stride >= 0 && est_stride < lim && ref_stride < lim &&
                                 (K == 0 || (others_row_stride >= 0 && others_row_stride < lim))),
                   "bss_eval: row strides %lld, %lld, %lld: rows would not be addressable (strides are >= 0; rows may overlap)",
                   (long long)est_stride, (long long)ref_stride, (long long)others_row_stride);
  MAAVSS_CHECK_ARG(K < 2 || (others_src_stride >= 0 && others_src_stride < lim), "bss_eval: source stride %lld", (long long)others_src_stride);
  MAAVSS_CHECK_ARG((((uintptr_t)est | (uintptr_t)ref | (uintptr_t)others) & 3) == 0, "bss_eval: est, ref and others must be 4-byte aligned");
  MAAVSS_CHECK_ARG((((uintptr_t)out | (uintptr_t)ws) & 7) == 0, "bss_eval: out and workspace must be 8-byte aligned");
  const bs_plan p = bs_make_plan(rows, n, K, L);
  MAAVSS_CHECK_ARG(ws_bytes >= p.bytes, "bss_eval: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)p.bytes);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  int* meta = (int*)w;
  double* en = (double*)(w + p.o_en);
  double* cpart = (double*)(w + p.o_cpart);
  double* corr = (double*)(w + p.o_corr);
  double* mat = (double*)(w + p.o_mat);
  double* dtile = (double*)(w + p.o_dtile);
  double* coef = (double*)(w + p.o_coef);
  double* fpart = (double*)(w + p.o_fpart);
  bs_in in;
  in.est = est;
  in.est_stride = rows == 1 ? 0 : est_stride;
  in.ref = ref;
  in.ref_stride = rows == 1 ? 0 : ref_stride;
  in.oth = others;
  in.oth_row = rows == 1 || K == 0 ? 0 : others_row_stride;
  in.oth_src = K < 2 ? 0 : others_src_stride;
  in.N = n;
  in.K = K;
  in.L = L;
  const unsigned R = (unsigned)rows;
  hipLaunchKernelGGL(bss_screen_kernel, dim3((unsigned)(rows * p.nsig * p.ncc)), dim3(256), 0, st, in, p.ncc, en);
  MAAVSS_LAUNCH_CHECK("bss_screen_kernel");
  hipLaunchKernelGGL(bss_plan_kernel, dim3(R), dim3(64), 0, st, en, p.ncc, K, L, meta);
  MAAVSS_LAUNCH_CHECK("bss_plan_kernel");
  hipLaunchKernelGGL(bss_corr_kernel, dim3((unsigned)p.ncc, p.njobs, R), dim3(256), 0, st, in, p.ncc, meta, cpart);
  MAAVSS_LAUNCH_CHECK("bss_corr_kernel");
  hipLaunchKernelGGL(bss_corr_sum_kernel, dim3((L + 255) / 256, p.njobs, R), dim3(256), 0, st, cpart, p.ncc, K, L, meta, corr);
  MAAVSS_LAUNCH_CHECK("bss_corr_sum_kernel");
  hipLaunchKernelGGL(bss_gram_kernel, dim3(p.nbt + 1, p.nbt, R), dim3(256), 0, st, corr, K, L, p.nbt, p.msz, meta, mat);
  MAAVSS_LAUNCH_CHECK("bss_gram_kernel");
  for (int k = 0; k < p.nbt; ++k) {
    hipLaunchKernelGGL(bss_panel_kernel, dim3(p.nbt - k + 1, R), dim3(256), 0, st, k, p.nbt, p.msz, meta, mat, dtile);
    MAAVSS_LAUNCH_CHECK("bss_panel_kernel");
    const int mt = p.nbt - k - 1;
    if (mt > 0) {
      hipLaunchKernelGGL(bss_update_kernel, dim3(mt + 1, mt, R), dim3(256), 0, st, k, p.nbt, p.msz, meta, mat);
      MAAVSS_LAUNCH_CHECK("bss_update_kernel");
    }
  }
  hipLaunchKernelGGL(bss_backsolve_kernel, dim3(2, R), dim3(256), 0, st, L, p.nbt, p.msz, meta, mat, dtile, coef);
  MAAVSS_LAUNCH_CHECK("bss_backsolve_kernel");
  hipLaunchKernelGGL(bss_fir_kernel, dim3((unsigned)p.nfc, R), dim3(256), 0, st, in, p.nbt, p.nfc, meta, coef, fpart);
  MAAVSS_LAUNCH_CHECK("bss_fir_kernel");
  hipLaunchKernelGGL(bss_finalize_kernel, dim3(R), dim3(64), 0, st, fpart, p.nfc, meta, out);
  MAAVSS_LAUNCH_CHECK("bss_finalize_kernel");
  return MAAVSS_OK;
}
