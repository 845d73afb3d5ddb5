// Image-source room responses (maavss_amd.Reverb.make_room_rirs): the second way to fill the table maavss_reverb convolves with.
// include/maavss.h holds the definition, operation by operation; tests/room_twin.py restates it in float64.  Compiled with
// -ffp-contract=off (Makefile): every f64 operation below is rounded on its own, in the order written.  A tap is an INTEGER sum of
// contributions rounded to multiples of 2^-40, so the order in which the images arrive cannot change a bit: no float atomic, and no
// atomic on global memory at all.
//   room_rir   one workgroup of 512 per (row, tile of RR_TILE = 1024 taps); the tile is an int64 array in LDS (8 KiB), the
//              fractional-delay table beside it when it has at most RR_TAB_LDS entries (16 KiB reserved; H = 8, R = 32 uses 4), read
//              from global memory otherwise.  The workgroup visits only the spherical shell of images whose taps can fall into its
//              tile: thread t takes the columns (ny, nz, py, pz, px) t, t + 512, ...; per column it forms uy^2, uz^2 and the four
//              y / z wall powers once, and a conservative interval of nx on either side of the microphone from the shell's radii (one
//              sample of slack in the radii, one cell in the interval; the two intervals merged where they touch, so no image is
//              visited twice).  A wave walks its 64 columns one candidate per lane and step; a candidate takes the definition's own
//              test (d, tau, k0 against the tile), and an accepted one gets its amplitude and goes to the wave's queue in LDS
//              (2 KiB a wave; slots by ballot and prefix count, no atomic).  Whenever the queue holds 64 images every lane takes one
//              and adds its 2 H taps: the long part of the work runs with all lanes busy however the columns' runs differ in length
//              (with the taps inside the candidate loop, lanes waited for the longest run: 2.5 times slower).  The order in which
//              images leave the queue is free, the sums being integers.  Contributions go to the tile with 64-bit integer LDS adds
//              (ds_add_u64; a zero is not added); the tile is written once with plain stores after int64 -> f64 -> f32.  Outer
//              tiles hold more images than inner ones (a shell's volume grows with the square of its radius): the grid hands out
//              the last tile of every row first.  Every value read from the device copy of the lattice bounds is clamped;
//              maavss_room_rir checks the host copy of the geometry before the launch.
#include "common.h"

namespace {

constexpr int RR_MAX_K = 32768;
constexpr int RR_THREADS = 512, RR_TILE = 1024;
constexpr int RR_QUEUE = 128;                                 // a wave's queue: drained at 64, a step adds at most 64
constexpr int RR_MAX_H = 32, RR_MAX_R = 256;
constexpr int RR_TAB_LDS = 2 * 32 * 32 + 1;                  // table entries kept in LDS (H = 32 at R = 32)
constexpr int64_t RR_MAX_ROWS = (int64_t)1 << 19;            // the table's row cap (reverb.hip's)
constexpr double RR_MAX_CELLS = 2147483648.0;                // images of a row's lattice box
constexpr int RR_MAX_N = 1 << 28;                            // what a lattice bound read from the device is clamped to
constexpr int RR_GEOM = 15;                                  // doubles per row: L[3], m[3], s[3], beta[6]
constexpr double RR_SCALE = 1099511627776.0;                 // 2^40
constexpr double RR_ROUND = 6755399441055744.0;              // 1.5 * 2^52

__device__ __forceinline__ double rr_ipow(double b, int e) {
  double r = 1.0;
  while (e) {
    if (e & 1) r = r * b;
    b = b * b;
    e >>= 1;
  }
  return r;
}
__device__ __forceinline__ double rr_offset(int n, int p, double L, double s, double m) {
  return ((double)(2 * n) * L + (double)(1 - 2 * p) * s) - m;
}
__device__ __forceinline__ int rr_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// floor(x) as an int inside [-lim - 2, lim + 2] (x may be huge or a NaN: a NaN reads as the lower end)
__device__ __forceinline__ int rr_cell(double x, int lim) {
  const double l = (double)(lim + 2);
  return (int)(x >= -l ? (x <= l ? x : l) : -l);
}
// the lanes of a wave hand queue entries to each other through LDS: what was written before is visible behind
__device__ __forceinline__ void rr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the taps of one image that fall into the tile [t0, t1)
__device__ __forceinline__ void rr_taps(double amp, double tau, int H, int R, int i_max, const double* __restrict__ tab, long long* tile, int t0,
                                        int t1) {
  const double kf = floor(tau), Hd = (double)H, Rd = (double)R;
  const int k0 = (int)kf;
  const double f = tau - kf;
  for (int m = -H + 1; m <= H; ++m) {
    const int k = k0 + m;
    if (k < t0 || k >= t1) continue;
    const double pos = (((double)m - f) + Hd) * Rd;
    const int i = rr_clampi((int)pos, 0, i_max);                  // pos >= 0 (f <= 1): the conversion's truncation is floor
    const double t = pos - (double)i;
    const double ta = tab[i];
    const double w = ta + t * (tab[i + 1] - ta);
    // llrint of |x| <= 2^40 without the 64-bit conversion: x + 1.5 * 2^52 is x rounded to an integer, ties to even, by the addition's
    // own rounding, and it lies in the binade whose doubles are 2^52 + integers, so the difference of the bit patterns is the integer
    const double x = (amp * w) * RR_SCALE;
    const long long q = __double_as_longlong(x + RR_ROUND) - __double_as_longlong(RR_ROUND);
    if (q) atomicAdd(reinterpret_cast<unsigned long long*>(&tile[k - t0]), (unsigned long long)q);
  }
}

template <bool TAB_LDS>
__global__ __launch_bounds__(RR_THREADS) void room_rir_kernel(const double* __restrict__ geom, const int32_t* __restrict__ bounds,
                                                              const double* __restrict__ table, int H, int R, double rate,
                                                              double metres_per_tap, int K, int tiles, int64_t rows,
                                                              float* __restrict__ rirs, int64_t ld) {
  __shared__ long long tile[RR_TILE];
  __shared__ double tab_s[TAB_LDS ? RR_TAB_LDS : 1];
  __shared__ double queue[RR_THREADS / 64][RR_QUEUE][2];                     // per wave: (amplitude, tau) of accepted images
  const int64_t row = blockIdx.x % rows;
  const int t0 = (tiles - 1 - (int)(blockIdx.x / rows)) * RR_TILE;          // the outermost (heaviest) tiles start first
  const int t1 = t0 + RR_TILE < K ? t0 + RR_TILE : K;
  const int n_tab = 2 * H * R + 1;
  for (int i = threadIdx.x; i < RR_TILE; i += RR_THREADS) tile[i] = 0;
  if (TAB_LDS) {
    for (int i = threadIdx.x; i < n_tab; i += RR_THREADS) tab_s[i] = table[i];
  }
  const double* __restrict__ tab = TAB_LDS ? tab_s : table;
  __syncthreads();

  const double* __restrict__ g = geom + row * RR_GEOM;
  const double Lx = g[0], Ly = g[1], Lz = g[2], mx = g[3], my = g[4], mz = g[5], sx = g[6], sy = g[7], sz = g[8];
  const double bx0 = g[9], bx1 = g[10], by0 = g[11], by1 = g[12], bz0 = g[13], bz1 = g[14];
  const int Nx = rr_clampi(bounds[3 * row], 0, RR_MAX_N), Ny = rr_clampi(bounds[3 * row + 1], 0, RR_MAX_N),
            Nz = rr_clampi(bounds[3 * row + 2], 0, RR_MAX_N);
  const double vx = rr_offset(0, 0, Lx, sx, mx), vy = rr_offset(0, 0, Ly, sy, my), vz = rr_offset(0, 0, Lz, sz, mz);
  const double d0 = sqrt((vx * vx + vy * vy) + vz * vz);
  // the shell of this tile: an image reaches a tap of [t0, t1) only when t0 - H <= tau < t1 + H - 1; one sample of slack either side
  const double rlo = d0 + (double)(t0 - H - 1) * metres_per_tap, rhi = d0 + (double)(t1 + H) * metres_per_tap;
  const double lo2 = rlo > 0.0 ? rlo * rlo : 0.0, hi2 = rhi * rhi;
  const double inv2l = 1.0 / (2.0 * Lx);
  const int64_t wz = 2 * (int64_t)Nz + 1, ncol = 8 * wz * (2 * (int64_t)Ny + 1);
  const double lo_k = (double)t0 - (double)H, hi_k = (double)t1 + (double)H - 1.0;      // k0 of an image with a tap in the tile: [lo_k, hi_k)
  const int i_max = n_tab - 2;
  const int lane = threadIdx.x & 63;
  double(*q)[2] = queue[threadIdx.x >> 6];
  int count = 0;                                                             // entries in this wave's queue (the same in all its lanes)

  for (int64_t base = 0; base < ncol; base += RR_THREADS) {
    // this lane's column (ny, nz, py, pz, px): at most two runs of nx, [nx, b1] and [a2, last]; an empty column has nx > last
    const int64_t col = base + threadIdx.x;
    int nx = 1, b1 = 0, a2 = 1, last = 0, px = 0;
    double uy2 = 0.0, uz2 = 0.0, y0p = 0.0, y1p = 0.0, z0p = 0.0, z1p = 0.0;
    if (col < ncol) {
      px = (int)(col & 1);
      const int pz = (int)((col >> 1) & 1), py = (int)((col >> 2) & 1);
      const int64_t cell = col >> 3;
      const int nz = (int)(cell % wz) - Nz, ny = (int)(cell / wz) - Ny;
      const double uy = rr_offset(ny, py, Ly, sy, my), uz = rr_offset(nz, pz, Lz, sz, mz);
      uy2 = uy * uy, uz2 = uz * uz;
      const double ryz = uy2 + uz2;
      if (ryz <= hi2) {
        const double a = lo2 > ryz ? sqrt(lo2 - ryz) : 0.0, b = sqrt(hi2 - ryz);        // |ux| of the shell lies in [a, b]
        const double o = (double)(1 - 2 * px) * sx - mx;                              // ux = 2 n Lx + o
        // nx with ux in [-b, -a] and with ux in [a, b], each widened by a cell, inside the lattice box
        const int nlo = rr_clampi(rr_cell(floor((-b - o) * inv2l), Nx) - 1, -Nx, Nx + 1), nhi = rr_clampi(rr_cell(ceil((-a - o) * inv2l), Nx) + 1, -Nx - 1, Nx);
        const int plo = rr_clampi(rr_cell(floor((a - o) * inv2l), Nx) - 1, -Nx, Nx + 1), phi = rr_clampi(rr_cell(ceil((b - o) * inv2l), Nx) + 1, -Nx - 1, Nx);
        const bool merged = nhi >= plo - 1;                                           // the two runs touch: one run, every nx once
        nx = nlo, last = phi;
        b1 = merged ? phi : nhi;
        a2 = merged ? phi + 1 : plo;
        y0p = rr_ipow(by0, abs(ny - py)), y1p = rr_ipow(by1, abs(ny)), z0p = rr_ipow(bz0, abs(nz - pz)), z1p = rr_ipow(bz1, abs(nz));
      }
    }
    // the wave walks its 64 columns one candidate per lane and step; accepted images go to the queue, and whenever it holds 64 every
    // lane takes one and adds its taps: the long part of the work runs with all lanes busy, however the runs differ in length
    for (;;) {
      if (nx > b1 && nx < a2) nx = a2;                                                // over the gap between the two runs
      const bool active = nx <= last;
      if (!__any(active)) break;
      bool accept = false;
      double amp = 0.0, tau = 0.0;
      if (active) {
        const double ux = rr_offset(nx, px, Lx, sx, mx);
        const double d = sqrt((ux * ux + uy2) + uz2);
        tau = (d - d0) * rate;
        const double kf = floor(tau);
        if (kf >= lo_k && kf < hi_k) {                                                // the definition's own test (false for a NaN)
          amp = ((((((rr_ipow(bx0, abs(nx - px)) * rr_ipow(bx1, abs(nx))) * y0p) * y1p) * z0p) * z1p) * d0) / d;
          accept = amp != 0.0;                                                        // amplitude 0: every contribution is the integer 0
        }
        ++nx;
      }
      const unsigned long long mask = __ballot(accept);
      if (accept) {
        const int slot = count + __popcll(mask & ((1ull << lane) - 1ull));
        q[slot][0] = amp, q[slot][1] = tau;
      }
      count += __popcll(mask);
      if (count >= 64) {
        rr_wave_sync();
        count -= 64;
        const double qa = q[count + lane][0], qt = q[count + lane][1];
        rr_wave_sync();                                                               // read before the next step writes these slots
        rr_taps(qa, qt, H, R, i_max, tab, tile, t0, t1);
      }
    }
  }
  rr_wave_sync();
  if (lane < count) rr_taps(q[lane][0], q[lane][1], H, R, i_max, tab, tile, t0, t1);
  __syncthreads();
  float* __restrict__ h = rirs + row * ld + t0;
  for (int i = threadIdx.x; t0 + i < t1; i += RR_THREADS) h[i] = (float)((double)tile[i] * (1.0 / RR_SCALE));
}

inline bool rr_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool rr_inside(double v, double L) { return v > 0.0 && v < L; }      // false for a NaN

}  // namespace

extern "C" int maavss_room_rir(const double* geom, const int32_t* bounds, const double* host_geom, const int32_t* host_bounds,
                               int64_t n_rows, const double* table, int H, int R, double sr, double c, int K, float* rirs,
                               int64_t ld_rir, void* stream) {
  MAAVSS_CHECK_ARG(geom && bounds && host_geom && host_bounds && table && rirs, "room_rir: null pointer");
  MAAVSS_CHECK_ARG(n_rows >= 1 && n_rows <= RR_MAX_ROWS, "room_rir: n_rows = %lld must be in [1, %lld]", (long long)n_rows, (long long)RR_MAX_ROWS);
  MAAVSS_CHECK_ARG(K >= 1 && K <= RR_MAX_K, "room_rir: K = %d must be in [1, %d]", K, RR_MAX_K);
  MAAVSS_CHECK_ARG(H >= 1 && H <= RR_MAX_H && R >= 1 && R <= RR_MAX_R, "room_rir: H = %d must be in [1, %d] and R = %d in [1, %d]", H, RR_MAX_H, R,
                   RR_MAX_R);
  MAAVSS_CHECK_ARG(sr > 0.0 && sr < 1e9 && c > 0.0 && c < 1e9, "room_rir: sr = %g and c = %g must be positive and finite", sr, c);
  MAAVSS_CHECK_ARG(ld_rir >= K, "room_rir: ld_rir = %lld is shorter than K = %d", (long long)ld_rir, K);
  MAAVSS_CHECK_ARG(rr_aligned(geom, 8) && rr_aligned(table, 8) && rr_aligned(bounds, 4) && rr_aligned(rirs, 4),
                   "room_rir: geom and table must be 8-byte aligned, bounds and rirs 4-byte");
  for (int64_t r = 0; r < n_rows; ++r) {
    const double* g = host_geom + r * RR_GEOM;
    const int32_t* n = host_bounds + 3 * r;
    for (int a = 0; a < 3; ++a) {
      MAAVSS_CHECK_ARG(g[a] > 0.0 && g[a] < 1e9, "room_rir: row %lld: dimension %d = %g must be positive and finite", (long long)r, a, g[a]);
      MAAVSS_CHECK_ARG(rr_inside(g[3 + a], g[a]) && rr_inside(g[6 + a], g[a]),
                       "room_rir: row %lld: microphone %g and source %g must lie strictly inside (0, %g) on axis %d", (long long)r, g[3 + a], g[6 + a],
                       g[a], a);
      MAAVSS_CHECK_ARG(n[a] >= 0 && n[a] <= RR_MAX_N, "room_rir: row %lld: lattice bound %d on axis %d must be in [0, %d]", (long long)r, n[a], a, RR_MAX_N);
    }
    for (int w = 0; w < 6; ++w) {
      MAAVSS_CHECK_ARG(g[9 + w] >= 0.0 && g[9 + w] <= 1.0, "room_rir: row %lld: beta[%d] = %g must be in [0, 1]", (long long)r, w, g[9 + w]);
    }
    MAAVSS_CHECK_ARG(g[3] != g[6] || g[4] != g[7] || g[5] != g[8], "room_rir: row %lld: the source lies on the microphone", (long long)r);
    MAAVSS_CHECK_ARG(8.0 * (2.0 * n[0] + 1.0) * (2.0 * n[1] + 1.0) * (2.0 * n[2] + 1.0) <= RR_MAX_CELLS,
                     "room_rir: row %lld: the lattice box (%d, %d, %d) holds more than 2^31 images", (long long)r, n[0], n[1], n[2]);
  }
  const int tiles = (K + RR_TILE - 1) / RR_TILE;
  const dim3 grid((unsigned)(n_rows * tiles));
  if (2 * H * R + 1 <= RR_TAB_LDS) {
    hipLaunchKernelGGL(room_rir_kernel<true>, grid, dim3(RR_THREADS), 0, (hipStream_t)stream, geom, bounds, table, H, R, sr / c, c / sr, K, tiles,
                       n_rows, rirs, ld_rir);
  } else {
    hipLaunchKernelGGL(room_rir_kernel<false>, grid, dim3(RR_THREADS), 0, (hipStream_t)stream, geom, bounds, table, H, R, sr / c, c / sr, K, tiles,
                       n_rows, rirs, ld_rir);
  }
  MAAVSS_LAUNCH_CHECK("room_rir_kernel");
  return MAAVSS_OK;
}
