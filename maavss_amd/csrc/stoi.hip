// EXTENSION (the reference reports its training loss only): short-time objective intelligibility (STOI, Taal et al. 2011) and its extended
// form (ESTOI, Jensen & Taal 2016) of est [rows][n] against ref [rows][n], f32 at 10 kHz, per row, all arithmetic f64 in a fixed order --
// what maavss_amd.stoi_metrics and Validator(intelligibility_sr=...) read.  include/maavss.h states the definition; tests/stoi_twin.py is
// its float64 restatement and the contract.
//
//   tables    w[256] = 0.5 - 0.5 cos(2 pi (n + 1) / 257) and the 256 twiddles exp(-2 pi i k / 512), into the workspace
//   energies  one wave per (row, frame k): E[k] = sum (w ref_k)^2, and an explicit flag for a non-finite sample of est or ref in the
//             frame's hop (the last wave of a row also takes the samples past the last frame)
//   select    one workgroup per row walks its frames: max E, then the mask E 1e4 > max E, an exclusive scan of it, src[] and n_kept
//   bands     one workgroup per (row, frame k < n_kept - 1) of the silence-free signal.  Sample n of that frame is the overlap-add of the
//             kept windowed frames src[k-1], src[k], src[k+1]; it is built directly from them (two products and one addition, as the
//             twin's overlap-add does), windowed again and transformed; the silence-free waveform never reaches memory.  ref and est
//             go through two separate real-input 512-point radix-2 transforms in LDS that share their twiddle loads: packed as one
//             complex transform, a silent est would come out as the rounding residue of ref (1e-16 of it) instead of exactly zero, and
//             the clipped, normalised correlation of that residue is not small.  15 third-octave band magnitudes each -> X, Y
//   segments  one wave per (row, 30-frame segment): lane j < 15 is band j (STOI's clipped correlation, ESTOI's row normalisation),
//             lane t < 30 is frame t (ESTOI's column normalisation)
//   finalize  one wave per row adds the row's segments in index order
// Rows of one call share n but not n_kept: every kernel reads its row's count from the workspace and a workgroup past it leaves.
// No floating-point atomic; every sum has one order, so two runs give the same bytes.  The Makefile compiles this file with
// -ffp-contract=off: the silence-free frames are then the twin's bit for bit (up to the last bit of cos), and what differs from the
// twin is the order of sums and the transform's rounding.
#include "common.h"
#include "metric_f64.h"

#define ST_FRAME 256
#define ST_HOP 128
#define ST_NFFT 512
#define ST_J 15
#define ST_N 30
#define ST_COLS 4                    // out row: stoi, estoi, n_kept, n_segments
#define ST_EPS 0x1p-52
#define ST_CLIP 0x1.a7e600b234626p+2 // 1 + 10^(15 / 20) = 6.623413251903491, the double the twin computes
#define ST_TAB_DOUBLES (ST_FRAME + ST_NFFT)

// band j sums the bins [st_edge[j], st_edge[j + 1]): the bins of linspace(0, 10000, 513)[:257] nearest to 150 * 2^(j / 3) * 2^(-+1/6)
__device__ const int st_edge[ST_J + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

static inline int64_t st_frames(int64_t n) { return n > ST_FRAME ? (n - ST_FRAME + ST_HOP - 1) / ST_HOP : 0; }      // len(range(0, n - 256, 128))

struct st_plan {
  int64_t nf, nfc, mcap, scap;                      // frames; max(nf, 1); the most frames of a silence-free signal; the most segments
  int64_t o_e, o_bad, o_src, o_cnt, o_xy, o_part, bytes;
};
static inline st_plan st_make_plan(int64_t rows, int64_t n) {
  st_plan p;
  p.nf = st_frames(n);
  p.nfc = p.nf > 1 ? p.nf : 1;
  p.mcap = p.nf > 1 ? p.nf - 1 : 0;
  p.scap = p.mcap >= ST_N ? p.mcap - ST_N + 1 : 0;
  p.o_e = align256(ST_TAB_DOUBLES * 8);
  p.o_bad = p.o_e + align256(rows * p.nfc * 8);
  p.o_src = p.o_bad + align256(rows * p.nfc * 4);
  p.o_cnt = p.o_src + align256(rows * p.nfc * 4);
  p.o_xy = p.o_cnt + align256(rows * 2 * 4);
  p.o_part = p.o_xy + align256(rows * 2 * ST_J * p.mcap * 8);
  p.bytes = p.o_part + align256(rows * p.scap * 2 * 8);
  return p;
}

__global__ __launch_bounds__(256) void stoi_tables_kernel(double* __restrict__ tab) {
  const int t = threadIdx.x;
  tab[t] = 0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * (double)(t + 1) / 257.0);
  double s, c;
  sincospi((double)t / 256.0, &s, &c);          // exp(-2 pi i t / 512) = c - i s; the argument is exact
  tab[ST_FRAME + 2 * t] = c;
  tab[ST_FRAME + 2 * t + 1] = s;
}

// one wave per (row, slot k < nfc); nblk workgroups per row
__global__ __launch_bounds__(256) void stoi_energies_kernel(const float* __restrict__ est, int64_t est_stride, const float* __restrict__ ref,
                                                            int64_t ref_stride, int64_t n, int64_t nf, int64_t nfc, int64_t nblk,
                                                            const double* __restrict__ tab, double* __restrict__ E, int* __restrict__ badv) {
  const int64_t row = blockIdx.x / nblk;
  const int64_t k = (blockIdx.x % nblk) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= nfc) return;
  const float* __restrict__ e = est + row * est_stride;
  const float* __restrict__ r = ref + row * ref_stride;
  const int64_t base = k * ST_HOP;
  double s = 0.0;
  if (k < nf) {                                 // frame k < nf ends before n: 128 k + 256 < n
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = lane + 64 * q;
      const double v = tab[i] * (double)r[base + i];
      s += v * v;
    }
  }
  // the samples this slot answers for: its hop, and in a row's last slot everything up to n (at most 384 samples)
  const int64_t hi = k == nfc - 1 ? n : base + ST_HOP;
  bool bad = false;
  for (int64_t i = base + lane; i < hi; i += 64) bad |= !__builtin_isfinite(e[i]) || !__builtin_isfinite(r[i]);
  s = wave_sum_d(s);
  const bool any_bad = __ballot(bad) != 0;
  if (lane == 0) {
    E[row * nfc + k] = s;
    badv[row * nfc + k] = any_bad ? 1 : 0;
  }
}

// one workgroup per row: cnt[row] = {n_kept, non-finite flag}, src[row][j] = the j-th kept frame
__global__ __launch_bounds__(256) void stoi_select_kernel(const double* __restrict__ E, const int* __restrict__ badv, int64_t nf, int64_t nfc,
                                                          int* __restrict__ src, int* __restrict__ cnt) {
  __shared__ double red_m[4][1];
  __shared__ int red_b[4][1];
  __shared__ int wtot[4];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double* __restrict__ Er = E + row * nfc;
  const int* __restrict__ br = badv + row * nfc;
  int* __restrict__ sr = src + row * nfc;
  double m = 0.0;
  int bad = 0;
  for (int64_t k = tid; k < nfc; k += 256) {
    bad |= br[k];
    const double v = Er[k];
    m = v > m ? v : m;                          // never reached with a NaN that matters: a flagged row stops below
  }
  const double wm[1] = {wave_max_d(m)};
  const int wb[1] = {__ballot(bad != 0) != 0};
  wg_park(red_m, wm, wave, lane);             // two types behind one barrier
  wg_park(red_b, wb, wave, lane);
  __syncthreads();
  if (red_b[0][0] | red_b[1][0] | red_b[2][0] | red_b[3][0]) {
    if (tid == 0) {
      cnt[2 * row] = 0;
      cnt[2 * row + 1] = 1;
    }
    return;
  }
  m = wg_col<WG_MAX>(red_m, 0);
  int base = 0;
  for (int64_t k0 = 0; k0 < nf; k0 += 256) {
    const int64_t k = k0 + tid;
    const bool keep = k < nf && Er[k] * 1e4 > m;              // the 40 dB rule on squared norms; max E = 0 keeps nothing
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wtot[wave] = __popcll(mask);
    __syncthreads();
    int off = 0;
    for (int q = 0; q < wave; ++q) off += wtot[q];
    const int total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    if (keep) sr[base + off + __popcll(mask & ((1ull << lane) - 1ull))] = (int)k;
    base += total;
    __syncthreads();                            // wtot is written again in the next round
  }
  if (tid == 0) {
    cnt[2 * row] = base;
    cnt[2 * row + 1] = 0;
  }
}

// one workgroup per (row, frame k of the silence-free signal); thread t is sample t, then one butterfly of each signal per stage
__global__ __launch_bounds__(256) void stoi_bands_kernel(const float* __restrict__ est, int64_t est_stride, const float* __restrict__ ref,
                                                         int64_t ref_stride, int64_t nfc, int64_t mcap, const double* __restrict__ tab,
                                                         const int* __restrict__ src, const int* __restrict__ cnt, double* __restrict__ xy) {
  __shared__ double zr[2][ST_NFFT], zi[2][ST_NFFT];
  __shared__ double tw[ST_NFFT];
  const int64_t row = blockIdx.x / mcap;
  const int k = (int)(blockIdx.x % mcap);
  const int M = cnt[2 * row] - 1;
  if (M < ST_N || k >= M) return;               // uniform over the workgroup: no barrier was reached
  const int t = threadIdx.x;
  const int* __restrict__ sr = src + row * nfc;
  const int64_t s0 = sr[k];
  // the lower half of the frame overlaps the upper half of kept frame k - 1, the upper half the lower half of kept frame k + 1 (k + 1 <= M)
  const int64_t so = t < ST_HOP ? (k > 0 ? sr[k - 1] : -1) : sr[k + 1];
  const int to = t < ST_HOP ? t + ST_HOP : t - ST_HOP;
  const double wn = tab[t], wo = tab[to];
  tw[t] = tab[ST_FRAME + t];
  tw[t + 256] = tab[ST_FRAME + t + 256];
  const int p0 = (int)(__brev((unsigned)t) >> 23);            // 9-bit reversal: t < 256 lands on an even place, t + 256 on the next odd one
#pragma unroll
  for (int sig = 0; sig < 2; ++sig) {
    const float* __restrict__ x = sig == 0 ? ref + row * ref_stride : est + row * est_stride;
    const double a = wn * (double)x[s0 * ST_HOP + t];
    const double b = so >= 0 ? wo * (double)x[so * ST_HOP + to] : 0.0;
    zr[sig][p0] = wn * (a + b);
    zi[sig][p0] = 0.0;
    zr[sig][p0 + 1] = 0.0;                      // samples 256 .. 511 of the zero-padded frame
    zi[sig][p0 + 1] = 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    int i0, i1, j;
    fft2_index(t, s, i0, i1, j);
    const double c = tw[2 * (j << (8 - s))], sn = tw[2 * (j << (8 - s)) + 1];
#pragma unroll
    for (int sig = 0; sig < 2; ++sig) fft2_rotate_add(zr[sig], zi[sig], i0, i1, c, sn);
    __syncthreads();
  }
  if (t < 2 * ST_J) {
    const int sig = t / ST_J, j = t % ST_J;
    double p = 0.0;
    for (int b = st_edge[j]; b < st_edge[j + 1]; ++b) p += zr[sig][b] * zr[sig][b] + zi[sig][b] * zi[sig][b];
    xy[((row * 2 + sig) * ST_J + j) * mcap + k] = sqrt(p);
  }
}

// one wave per (row, segment)
__global__ __launch_bounds__(64) void stoi_segments_kernel(const double* __restrict__ xy, int64_t mcap, int64_t scap, const int* __restrict__ cnt,
                                                           double* __restrict__ part) {
  __shared__ double xs[ST_J][ST_N], ys[ST_J][ST_N];           // the segment, then its row-normalised form
  __shared__ double dj[ST_J], et[ST_N];
  const int64_t row = blockIdx.x / scap;
  const int seg = (int)(blockIdx.x % scap);
  const int M = cnt[2 * row] - 1;
  if (seg > M - ST_N) return;
  const int lane = threadIdx.x;
  if (lane < ST_J) {
    const int j = lane;
    const double* __restrict__ xp = xy + ((row * 2 + 0) * ST_J + j) * mcap + seg;
    const double* __restrict__ yp = xy + ((row * 2 + 1) * ST_J + j) * mcap + seg;
    double sxx = 0.0, syy = 0.0, sx = 0.0, sy = 0.0;
    for (int t = 0; t < ST_N; ++t) {
      const double x = xp[t], y = yp[t];
      xs[j][t] = x;
      ys[j][t] = y;
      sxx += x * x;
      syy += y * y;
      sx += x;
      sy += y;
    }
    const double alpha = sqrt(sxx) / (sqrt(syy) + ST_EPS);
    double sc = 0.0;
    for (int t = 0; t < ST_N; ++t) {
      const double a = alpha * ys[j][t], b = xs[j][t] * ST_CLIP;
      sc += a < b ? a : b;
    }
    const double mx = sx / ST_N, my = sy / ST_N, mc = sc / ST_N;
    double nx = 0.0, ny = 0.0, nc = 0.0;
    for (int t = 0; t < ST_N; ++t) {
      const double a = alpha * ys[j][t], b = xs[j][t] * ST_CLIP;
      const double dx = xs[j][t] - mx, dy = ys[j][t] - my, dc = (a < b ? a : b) - mc;
      nx += dx * dx;
      ny += dy * dy;
      nc += dc * dc;
    }
    nx = sqrt(nx) + ST_EPS;
    ny = sqrt(ny) + ST_EPS;
    nc = sqrt(nc) + ST_EPS;
    double d = 0.0;
    for (int t = 0; t < ST_N; ++t) {
      const double a = alpha * ys[j][t], b = xs[j][t] * ST_CLIP;
      const double xn = (xs[j][t] - mx) / nx;
      d += xn * (((a < b ? a : b) - mc) / nc);
      xs[j][t] = xn;                            // STOI's normalised reference band is ESTOI's row-normalised one
      ys[j][t] = (ys[j][t] - my) / ny;
    }
    dj[j] = d;
  }
  __syncthreads();
  if (lane < ST_N) {
    const int t = lane;
    double sx = 0.0, sy = 0.0;
    for (int j = 0; j < ST_J; ++j) {
      sx += xs[j][t];
      sy += ys[j][t];
    }
    const double mx = sx / ST_J, my = sy / ST_J;
    double nx = 0.0, ny = 0.0;
    for (int j = 0; j < ST_J; ++j) {
      const double dx = xs[j][t] - mx, dy = ys[j][t] - my;
      nx += dx * dx;
      ny += dy * dy;
    }
    nx = sqrt(nx) + ST_EPS;
    ny = sqrt(ny) + ST_EPS;
    double e = 0.0;
    for (int j = 0; j < ST_J; ++j) e += ((xs[j][t] - mx) / nx) * ((ys[j][t] - my) / ny);
    et[t] = e;
  }
  __syncthreads();
  if (lane == 0) {
    double d = 0.0, e = 0.0;
    for (int j = 0; j < ST_J; ++j) d += dj[j];
    for (int t = 0; t < ST_N; ++t) e += et[t];
    part[(row * scap + seg) * 2] = d;
    part[(row * scap + seg) * 2 + 1] = e / ST_N;
  }
}

// one wave per row
__global__ __launch_bounds__(64) void stoi_finalize_kernel(const double* __restrict__ part, int64_t scap, const int* __restrict__ cnt,
                                                           double* __restrict__ out) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int n_kept = cnt[2 * row];
  const int nseg = n_kept - 1 >= ST_N ? n_kept - ST_N : 0;     // M - 29 segments of M = n_kept - 1 frames; a flagged row has n_kept = 0
  double d = nan_d(), e = nan_d();
  if (nseg > 0) {
    d = wave_strided_sum_d(part + row * scap * 2, nseg, 2, lane) / (double)(ST_J * (int64_t)nseg);
    e = wave_strided_sum_d(part + row * scap * 2 + 1, nseg, 2, lane) / (double)nseg;
  }
  if (lane != 0) return;
  double* __restrict__ o = out + row * ST_COLS;
  o[0] = d;
  o[1] = e;
  o[2] = (double)n_kept;
  o[3] = (double)nseg;
}

static inline bool st_sizes_ok(int64_t rows, int64_t n) {
  if (rows < 1 || n < 1 || n >= (int64_t)1 << 31) return false;
  const int64_t nf = st_frames(n);
  return (nf > 1 ? nf : 1) <= (((int64_t)1 << 31) - 1) / rows;      // one workgroup per (row, frame) at the most
}

extern "C" int64_t maavss_stoi_ws_bytes(int64_t rows, int64_t n) {
  if (!st_sizes_ok(rows, n)) return 0;
  return st_make_plan(rows, n).bytes;
}

extern "C" int maavss_stoi(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, int64_t rows, int64_t n, double* out,
                           void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = metric_rows_check("stoi", est, est_stride, ref, ref_stride, rows, out, ws)) return rc;
  MAAVSS_CHECK_ARG(rows >= 1 && n >= 1, "stoi: bad sizes (rows %lld, n %lld)", (long long)rows, (long long)n);
  MAAVSS_CHECK_ARG(n < (int64_t)1 << 31, "stoi: n = %lld is beyond the kernels' index range (n < 2^31)", (long long)n);
  MAAVSS_CHECK_ARG(st_sizes_ok(rows, n), "stoi: %lld rows of %lld frames are more workgroups than one launch takes", (long long)rows,
                   (long long)st_frames(n));
  const st_plan p = st_make_plan(rows, n);
  MAAVSS_CHECK_ARG(ws_bytes >= p.bytes, "stoi: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)p.bytes);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  double* tab = (double*)w;
  double* E = (double*)(w + p.o_e);
  int* badv = (int*)(w + p.o_bad);
  int* src = (int*)(w + p.o_src);
  int* cnt = (int*)(w + p.o_cnt);
  double* xy = (double*)(w + p.o_xy);
  double* part = (double*)(w + p.o_part);
  const int64_t es = rows == 1 ? 0 : est_stride, rs = rows == 1 ? 0 : ref_stride;
  hipLaunchKernelGGL(stoi_tables_kernel, dim3(1), dim3(256), 0, st, tab);
  MAAVSS_LAUNCH_CHECK("stoi_tables_kernel");
  const int64_t nblk = (p.nfc + 3) / 4;
  hipLaunchKernelGGL(stoi_energies_kernel, dim3((unsigned)(rows * nblk)), dim3(256), 0, st, est, es, ref, rs, n, p.nf, p.nfc, nblk, tab, E, badv);
  MAAVSS_LAUNCH_CHECK("stoi_energies_kernel");
  hipLaunchKernelGGL(stoi_select_kernel, dim3((unsigned)rows), dim3(256), 0, st, E, badv, p.nf, p.nfc, src, cnt);
  MAAVSS_LAUNCH_CHECK("stoi_select_kernel");
  if (p.scap > 0) {                             // shorter rows have no segment: nothing to transform
    hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)(rows * p.mcap)), dim3(256), 0, st, est, es, ref, rs, p.nfc, p.mcap, tab, src, cnt, xy);
    MAAVSS_LAUNCH_CHECK("stoi_bands_kernel");
    hipLaunchKernelGGL(stoi_segments_kernel, dim3((unsigned)(rows * p.scap)), dim3(64), 0, st, xy, p.mcap, p.scap, cnt, part);
    MAAVSS_LAUNCH_CHECK("stoi_segments_kernel");
  }
  hipLaunchKernelGGL(stoi_finalize_kernel, dim3((unsigned)rows), dim3(64), 0, st, part, p.scap, cnt, out);
  MAAVSS_LAUNCH_CHECK("stoi_finalize_kernel");
  return MAAVSS_OK;
}
