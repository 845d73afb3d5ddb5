// The reference's callback images (train_avse_frames.py:191-215, utilities.py:230-245, 286-356, 386-416) as RGBA bytes made on the device:
// what maavss_amd.figures (viridis_image, specgram_planes, stft_panels, filmstrip_image, CallbackFigures) reads.  include/maavss.h states
// the definitions; tests/figures_twin.py is their float64 restatement and the contract.
//
//   viridis_range     one workgroup per image: minimum and maximum over the finite elements, f64, no atomics (min and max do not depend
//                     on the order)
//   viridis_colour    u = (double(x) - vmin) / (vmax - vmin), pixel = LUT[clamp(trunc(256 u), 0, 255)], a non-finite element (0, 0, 0, 0).
//                     The range comes from device memory (or from the arguments), the LUT is staged in LDS as 256 packed RGBA words,
//                     every thread makes four consecutive output pixels and stores them as one 16-byte word.  Element strides, transpose,
//                     row flip and integer nearest replication are index arithmetic: no copy of the image is made
//   specgram          one workgroup per (row, segment) of matplotlib's Axes.specgram(mode='magnitude' | 'phase') with its defaults: the
//                     Hann-windowed segment in LDS as f64, a radix-2 transform (the butterfly of metric_f64.h), 20 log10(|F| / sum w)
//                     and atan2 per bin, then np.unwrap along the column inside the workgroup: the corrections in parallel, their running
//                     sum by one thread in bin order (numpy's cumsum order; two runs give the same bytes)
//   filmstrip_max     64 workgroups per tensor: partial maxima of the target attention, the predicted attention and the video (torch.max);
//                     the strip kernel folds them, no atomics
//   filmstrip         v * (1 / (max + 1e-7)) clipped to [0, 1], all in f32 as the reference forms it; attention through the colour map with
//                     the fixed range [-1, 1], video as trunc(255 v) bytes; frames side by side, rows video, y, y-hat
// The Makefile compiles this file with -ffp-contract=off: the three f64 operations of the colour mapping are then the twin's, and
// viridis_colour is bit-exact against it on every element.
#include "common.h"
#include "metric_f64.h"
#include "viridis_lut.h"

#define SG_MAX 1024                  // the largest transform: 8 KB of f64 per LDS array
#define SG_PI 3.141592653589793      // np.pi
#define SG_2PI 6.283185307179586     // 2 * np.pi

// one workgroup per image: range[2 n] = min, range[2 n + 1] = max over the finite elements (+inf, -inf when there is none)
template <typename T>
__global__ __launch_bounds__(256) void viridis_range_kernel(const T* __restrict__ x, int64_t H, int64_t W, int64_t sn, int64_t sh, int64_t sw,
                                                            double* __restrict__ range) {
  __shared__ double red[4][2];
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x;
  const T* __restrict__ img = x + n * sn;
  double lo = inf_d(), hi = -inf_d();
  const int64_t count = H * W;
  for (int64_t e = tid; e < count; e += 256) {
    const double v = (double)img[(e / W) * sh + (e % W) * sw];
    if (__builtin_isfinite(v)) {
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
  }
  const double v[2] = {wave_min_d(lo), wave_max_d(hi)};
  wg_park(red, v, tid >> 6, tid & 63);
  __syncthreads();
  if (tid == 0) {
    range[2 * n] = wg_col<WG_MIN>(red, 0);
    range[2 * n + 1] = wg_col<WG_MAX>(red, 1);
  }
}

// the index into the LUT of one value; -1 for a non-finite one.  Three f64 operations: a difference, a quotient, a product
__device__ __forceinline__ int viridis_index(double v, double lo, double hi) {
  if (!__builtin_isfinite(v)) return -1;
  const double d = hi - lo;
  const double u = d == 0.0 ? 0.0 : (v - lo) / d;
  const double s = u * 256.0;
  return !(s >= 0.0) ? 0 : s >= 256.0 ? 255 : (int)s;
}

__device__ __forceinline__ void stage_lut(unsigned* lut) {      // 256 threads: R, G, B, A = 255 in memory order
  const int t = threadIdx.x;
  lut[t] = (unsigned)viridis_lut[t][0] | (unsigned)viridis_lut[t][1] << 8 | (unsigned)viridis_lut[t][2] << 16 | 0xff000000u;
}

// four consecutive pixels of the flat output per thread: one 16-byte store when `out` is 16-byte aligned; the last group of an output
// whose pixel count is no multiple of 4, and every group of an output that starts off a 16-byte boundary, pixel by pixel
__device__ __forceinline__ void store_pixels(unsigned* __restrict__ out, int64_t p0, int64_t total, const unsigned px[4]) {
  if (p0 + 4 <= total && ((uintptr_t)out & 15) == 0) {
    *reinterpret_cast<uint4*>(out + p0) = make_uint4(px[0], px[1], px[2], px[3]);
  } else {
    for (int q = 0; q < 4; ++q)
      if (p0 + q < total) out[p0 + q] = px[q];
  }
}

// Hi x Wi: the image after the transpose; Ho = Hi sy, Wo = Wi sx
template <typename T>
__global__ __launch_bounds__(256) void viridis_colour_kernel(const T* __restrict__ x, int64_t sn, int64_t sh, int64_t sw, const double* __restrict__ range,
                                                             int fixed, double vmin, double vmax, int transpose, int flip_rows, int64_t Hi, int64_t Wi,
                                                             int sy, int sx, unsigned* __restrict__ out, int64_t total) {
  __shared__ unsigned lut[VIRIDIS_N];
  stage_lut(lut);
  __syncthreads();
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= total) return;
  const int64_t Wo = Wi * sx, per_image = Hi * sy * Wo;
  unsigned px[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t p = p0 + q;
    px[q] = 0u;
    if (p >= total) continue;
    const int64_t n = p / per_image, rem = p % per_image;
    int64_t iy = (rem / Wo) / sy;
    const int64_t ix = (rem % Wo) / sx;
    if (flip_rows) iy = Hi - 1 - iy;
    const int64_t r = transpose ? ix : iy, c = transpose ? iy : ix;
    const double lo = (fixed & 1) ? vmin : range[2 * n], hi = (fixed & 2) ? vmax : range[2 * n + 1];
    const int idx = viridis_index((double)x[n * sn + r * sh + c * sw], lo, hi);
    if (idx >= 0) px[q] = lut[idx];
  }
  store_pixels(out, p0, total, px);
}

// np.mod for a positive divisor: the remainder takes the divisor's sign
__device__ __forceinline__ double py_mod(double a, double b) {
  double r = fmod(a, b);
  if (r != 0.0) {
    if (r < 0.0) r += b;
  } else {
    r = 0.0;
  }
  return r;
}

// one workgroup per (row, segment); mag, ph: [rows][nfft / 2 + 1][nseg], row 0 of a plane is the Nyquist bin
__global__ __launch_bounds__(256) void specgram_kernel(const float* __restrict__ wave, int64_t stride, int64_t L, int nfft, int lg, int step,
                                                       int64_t nseg, double* __restrict__ mag, double* __restrict__ ph) {
  __shared__ double zr[SG_MAX], zi[SG_MAX];
  __shared__ double twc[SG_MAX / 2], tws[SG_MAX / 2];
  __shared__ double ang[SG_MAX / 2 + 1], cor[SG_MAX / 2 + 1];
  __shared__ double red[4][1];
  const int64_t row = blockIdx.x / nseg, seg = blockIdx.x % nseg;
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const int half_n = nfft >> 1, nb = half_n + 1;
  const float* __restrict__ x = wave + row * stride + seg * (int64_t)step;
  const int64_t avail = L - seg * (int64_t)step;               // a signal shorter than nfft is zero-padded; otherwise avail >= nfft
  double ws = 0.0;
  for (int k = t; k < nfft; k += 256) {
    // np.hanning(nfft): 0.5 + 0.5 cos(pi n / (nfft - 1)), n = 2 k + 1 - nfft
    const double w = 0.5 + 0.5 * cospi((double)(2 * k + 1 - nfft) / (double)(nfft - 1));
    const double v = k < avail ? (double)x[k] : 0.0;
    const int p = (int)(__brev((unsigned)k) >> (32 - lg));
    zr[p] = v * w;
    zi[p] = 0.0;
    ws += w;
  }
  for (int k = t; k < half_n; k += 256) {
    double s, c;
    sincospi((double)k / (double)half_n, &s, &c);              // exp(-2 pi i k / nfft) = c - i s; the argument is exact
    twc[k] = c;
    tws[k] = s;
  }
  ws = wave_sum_d(ws);
  ws = wg_reduce<WG_ALL, WG_SUM>(ws, red, wv, lane);            // its barrier also covers zr, zi and the twiddles
  for (int s = 0; s < lg; ++s) {
    for (int b = t; b < half_n; b += 256) {
      int i0, i1, j;
      fft2_index(b, s, i0, i1, j);
      fft2_rotate_add(zr, zi, i0, i1, twc[j << (lg - 1 - s)], tws[j << (lg - 1 - s)]);
    }
    __syncthreads();
  }
  double* __restrict__ mo = mag + row * nb * nseg + seg;
  double* __restrict__ po = ph + row * nb * nseg + seg;
  for (int k = t; k < nb; k += 256) {
    const double re = zr[k], im = zi[k];
    mo[(int64_t)(nb - 1 - k) * nseg] = 20.0 * log10(hypot(re, im) / ws);
    ang[k] = atan2(im, re);
  }
  __syncthreads();
  // np.unwrap along the column: dd = diff(p), m = mod(dd + pi, 2 pi) - pi with m = pi where m == -pi and dd > 0, correction m - dd,
  // zero where |dd| < pi, and its cumulative sum added to p[1:]
  for (int k = t; k < nb; k += 256) {
    double c = 0.0;
    if (k > 0) {
      const double dd = ang[k] - ang[k - 1];
      double m = py_mod(dd + SG_PI, SG_2PI) - SG_PI;
      if (m == -SG_PI && dd > 0.0) m = SG_PI;
      c = m - dd;
      if (fabs(dd) < SG_PI) c = 0.0;
    }
    cor[k] = c;
  }
  __syncthreads();
  if (t == 0) {
    double run = 0.0;
    for (int k = 1; k < nb; ++k) {                             // numpy's cumsum order
      run += cor[k];
      cor[k] = run;
    }
  }
  __syncthreads();
  for (int k = t; k < nb; k += 256) po[(int64_t)(nb - 1 - k) * nseg] = k == 0 ? ang[0] : ang[k] + cor[k];
}

// torch.max of y, yh and video (a NaN is ignored here, see include/maavss.h) in two steps without atomics: workgroup (b, which) takes
// every FILM_PARTS-th run of 256 elements of tensor `which` and writes parts[which][b]; film_maxes folds the parts in the strip kernel
#define FILM_PARTS 64
__global__ __launch_bounds__(256) void filmstrip_max_kernel(const float* __restrict__ y, const float* __restrict__ yh, const float* __restrict__ video,
                                                            int64_t n_attn, int64_t n_video, float* __restrict__ parts) {
  __shared__ float red[4][1];
  const int which = blockIdx.y;
  const float* __restrict__ x = which == 0 ? y : which == 1 ? yh : video;
  const int64_t n = which == 2 ? n_video : n_attn;
  const int tid = threadIdx.x;
  float m = -__builtin_inff();
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)FILM_PARTS * 256) m = fmaxf(m, x[i]);
  m = wave_max(m);
  m = wg_reduce<WG_THREAD0, WG_MAX>(m, red, tid >> 6, tid & 63);
  if (tid == 0) parts[which * FILM_PARTS + blockIdx.x] = m;
}
// the three maxima into LDS: wave w < n_tensors folds the FILM_PARTS parts of tensor w (max does not depend on the order)
__device__ __forceinline__ void film_maxes(const float* __restrict__ parts, int n_tensors, float* smax) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < n_tensors) {
    const float m = wave_max(parts[wave * FILM_PARTS + lane]);
    if (lane == 0) smax[wave] = m;
  }
}

// the reference's scale and clip, every operation one f32 operation: s = 1 / (max + 1e-7), v s, clip to [0, 1]
__device__ __forceinline__ float film_scale(float m) { return 1.0f / (m + 1e-7f); }
__device__ __forceinline__ float film_clip(float v, float s) {
  const float p = v * s;
  return p < 0.0f ? 0.0f : p > 1.0f ? 1.0f : p;              // a NaN stays a NaN
}

// out [R H][T W] RGBA, R = 3 with a video (rows video, y, yh) and 2 without (y, yh)
__global__ __launch_bounds__(256) void filmstrip_kernel(const float* __restrict__ y, const float* __restrict__ yh, const float* __restrict__ video,
                                                        const float* __restrict__ parts, int T, int H, int W, unsigned* __restrict__ out, int64_t total) {
  __shared__ unsigned lut[VIRIDIS_N];
  __shared__ float maxes[3];
  stage_lut(lut);
  film_maxes(parts, video ? 3 : 2, maxes);
  __syncthreads();
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= total) return;
  const int64_t Wo = (int64_t)T * W, plane = (int64_t)T * H * W;
  const int first_attn = video ? 1 : 0;
  unsigned px[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t p = p0 + q;
    px[q] = 0u;
    if (p >= total) continue;
    const int64_t oy = p / Wo, ox = p % Wo;
    const int strip = (int)(oy / H);
    const int64_t src = ((ox / W) * H + oy % H) * W + ox % W;      // frame ox / W, row oy % H, column ox % W of [T][H][W]
    if (strip < first_attn) {
      const float s = film_scale(maxes[2]);
      unsigned word = 0xff000000u;
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = film_clip(video[c * plane + src], s);
        bad |= v != v;
        word |= (unsigned)(int)(v * 255.0f) << (8 * c);
      }
      px[q] = bad ? 0u : word;
    } else {
      const int a = strip - first_attn;
      const float v = film_clip((a == 0 ? y : yh)[src], film_scale(maxes[a]));
      const int idx = viridis_index((double)v, -1.0, 1.0);
      if (idx >= 0) px[q] = lut[idx];
    }
  }
  store_pixels(out, p0, total, px);
}

static inline bool fig_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline int64_t sg_segments(int64_t L, int nfft, int noverlap) { return ((L > nfft ? L : nfft) - noverlap) / (nfft - noverlap); }

#define FIG_MAX_PIXELS ((int64_t)1 << 40)

static int fig_image_args(const char* who, const void* x, int dtype, int64_t n_img, int64_t H, int64_t W, int64_t sn, int64_t sh, int64_t sw) {
  MAAVSS_CHECK_ARG(x, "%s: null pointer", who);
  MAAVSS_CHECK_ARG(dtype == 0 || dtype == 1, "%s: dtype %d (0 = float32, 1 = float64)", who, dtype);
  MAAVSS_CHECK_ARG(n_img >= 1 && H >= 1 && W >= 1, "%s: zero-sized image (%lld images of %lld x %lld)", who, (long long)n_img, (long long)H, (long long)W);
  MAAVSS_CHECK_ARG(n_img < (int64_t)1 << 31 && H < (int64_t)1 << 31 && W < (int64_t)1 << 31 && H * W <= FIG_MAX_PIXELS / n_img,
                   "%s: %lld images of %lld x %lld are beyond the kernels' index range", who, (long long)n_img, (long long)H, (long long)W);
  MAAVSS_CHECK_ARG(sn >= 0 && sh >= 0 && sw >= 0 && sn < (int64_t)1 << 40 && sh < (int64_t)1 << 40 && sw < (int64_t)1 << 40,
                   "%s: element strides %lld, %lld, %lld must be >= 0 (and below 2^40)", who, (long long)sn, (long long)sh, (long long)sw);
  MAAVSS_CHECK_ARG(((uintptr_t)x & (dtype == 0 ? 3 : 7)) == 0, "%s: the image must be aligned to its element size", who);
  return MAAVSS_OK;
}

extern "C" int maavss_viridis_range(const void* x, int dtype, int64_t n_img, int64_t H, int64_t W, int64_t sn, int64_t sh, int64_t sw,
                                    double* range, void* stream) {
  MAAVSS_CHECK_ARG(range, "viridis_range: null pointer");
  if (int rc = fig_image_args("viridis_range", x, dtype, n_img, H, W, sn, sh, sw)) return rc;
  MAAVSS_CHECK_ARG(((uintptr_t)range & 7) == 0, "viridis_range: range must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL(viridis_range_kernel<float>, dim3((unsigned)n_img), dim3(256), 0, st, (const float*)x, H, W, sn, sh, sw, range);
  else
    hipLaunchKernelGGL(viridis_range_kernel<double>, dim3((unsigned)n_img), dim3(256), 0, st, (const double*)x, H, W, sn, sh, sw, range);
  MAAVSS_LAUNCH_CHECK("viridis_range_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_viridis_image(const void* x, int dtype, int64_t n_img, int64_t H, int64_t W, int64_t sn, int64_t sh, int64_t sw,
                                    const double* range, int fixed, double vmin, double vmax, int transpose, int flip_rows, int sy, int sx,
                                    void* out, void* stream) {
  MAAVSS_CHECK_ARG(out, "viridis_image: null pointer");
  if (int rc = fig_image_args("viridis_image", x, dtype, n_img, H, W, sn, sh, sw)) return rc;
  MAAVSS_CHECK_ARG(fixed >= 0 && fixed <= 3, "viridis_image: fixed = %d (bit 0: vmin, bit 1: vmax come from the arguments)", fixed);
  MAAVSS_CHECK_ARG(fixed == 3 || range, "viridis_image: null pointer (the range of an autoscaled image)");
  MAAVSS_CHECK_ARG(!range || ((uintptr_t)range & 7) == 0, "viridis_image: range must be 8-byte aligned");
  MAAVSS_CHECK_ARG((!(fixed & 1) || vmin == vmin) && (!(fixed & 2) || vmax == vmax) && (fixed != 3 || vmin <= vmax),
                   "viridis_image: a fixed range needs vmin <= vmax, got %g, %g", vmin, vmax);
  MAAVSS_CHECK_ARG(sy >= 1 && sx >= 1 && sy <= 64 && sx <= 64, "viridis_image: scale (%d, %d) must be integers in 1 .. 64", sy, sx);
  MAAVSS_CHECK_ARG(H * W <= FIG_MAX_PIXELS / n_img / (sy * sx), "viridis_image: the scaled output is beyond the kernels' index range");
  MAAVSS_CHECK_ARG(((uintptr_t)out & 3) == 0, "viridis_image: out must be 4-byte aligned");
  const int64_t Hi = transpose ? W : H, Wi = transpose ? H : W;
  const int64_t total = n_img * Hi * sy * Wi * sx;
  const int64_t blocks = (total + 1023) / 1024;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL(viridis_colour_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)x, sn, sh, sw, range, fixed, vmin, vmax,
                       transpose ? 1 : 0, flip_rows ? 1 : 0, Hi, Wi, sy, sx, (unsigned*)out, total);
  else
    hipLaunchKernelGGL(viridis_colour_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)x, sn, sh, sw, range, fixed, vmin, vmax,
                       transpose ? 1 : 0, flip_rows ? 1 : 0, Hi, Wi, sy, sx, (unsigned*)out, total);
  MAAVSS_LAUNCH_CHECK("viridis_colour_kernel");
  return MAAVSS_OK;
}

static int sg_args(const char* who, int64_t rows, int64_t L, int nfft, int noverlap) {
  MAAVSS_CHECK_ARG(fig_pow2(nfft) && nfft >= 32 && nfft <= SG_MAX, "%s: nfft = %d must be a power of two in 32 .. %d", who, nfft, SG_MAX);
  MAAVSS_CHECK_ARG(noverlap >= 0 && noverlap < nfft, "%s: noverlap = %d must be in [0, nfft = %d)", who, noverlap, nfft);
  MAAVSS_CHECK_ARG(rows >= 1 && L >= 1, "%s: bad sizes (rows %lld, L %lld)", who, (long long)rows, (long long)L);
  MAAVSS_CHECK_ARG(L < (int64_t)1 << 31, "%s: L = %lld is beyond the kernel's index range (L < 2^31)", who, (long long)L);
  MAAVSS_CHECK_ARG(sg_segments(L, nfft, noverlap) <= (((int64_t)1 << 31) - 1) / rows, "%s: %lld rows of %lld segments are more workgroups than one launch takes",
                   who, (long long)rows, (long long)sg_segments(L, nfft, noverlap));
  return MAAVSS_OK;
}

extern "C" int64_t maavss_specgram_segments(int64_t rows, int64_t L, int nfft, int noverlap) {
  if (sg_args("specgram_segments", rows, L, nfft, noverlap)) return 0;
  return sg_segments(L, nfft, noverlap);
}

extern "C" int maavss_specgram(const float* wave, int64_t stride, int64_t rows, int64_t L, int nfft, int noverlap, double* mag_db, double* phase,
                               void* stream) {
  MAAVSS_CHECK_ARG(wave && mag_db && phase, "specgram: null pointer");
  if (int rc = sg_args("specgram", rows, L, nfft, noverlap)) return rc;
  MAAVSS_CHECK_ARG(rows == 1 || (stride >= 0 && stride < (int64_t)1 << 40),
                   "specgram: row stride %lld: rows would not be addressable (strides are >= 0; rows may overlap)", (long long)stride);
  MAAVSS_CHECK_ARG(((uintptr_t)wave & 3) == 0, "specgram: wave must be 4-byte aligned");
  MAAVSS_CHECK_ARG((((uintptr_t)mag_db | (uintptr_t)phase) & 7) == 0, "specgram: the planes must be 8-byte aligned");
  const int64_t nseg = sg_segments(L, nfft, noverlap);
  int lg = 0;
  while ((1 << lg) < nfft) ++lg;
  hipLaunchKernelGGL(specgram_kernel, dim3((unsigned)(rows * nseg)), dim3(256), 0, (hipStream_t)stream, wave, rows == 1 ? 0 : stride, L, nfft, lg,
                     nfft - noverlap, nseg, mag_db, phase);
  MAAVSS_LAUNCH_CHECK("specgram_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_filmstrip(const float* y_attn, const float* yh_attn, const float* video, int T, int H, int W, float* maxes, void* out,
                                void* stream) {
  MAAVSS_CHECK_ARG(y_attn && yh_attn && maxes && out, "filmstrip: null pointer");
  MAAVSS_CHECK_ARG(T >= 1 && H >= 1 && W >= 1, "filmstrip: zero-sized image (%d frames of %d x %d)", T, H, W);
  MAAVSS_CHECK_ARG((int64_t)T * H * W <= (int64_t)1 << 32, "filmstrip: %d frames of %d x %d are beyond the kernels' index range", T, H, W);
  MAAVSS_CHECK_ARG((((uintptr_t)y_attn | (uintptr_t)yh_attn | (uintptr_t)video | (uintptr_t)maxes) & 3) == 0, "filmstrip: the inputs must be 4-byte aligned");
  MAAVSS_CHECK_ARG(((uintptr_t)out & 3) == 0, "filmstrip: out must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t plane = (int64_t)T * H * W;
  hipLaunchKernelGGL(filmstrip_max_kernel, dim3(FILM_PARTS, video ? 3 : 2), dim3(256), 0, st, y_attn, yh_attn, video, plane, 3 * plane, maxes);
  MAAVSS_LAUNCH_CHECK("filmstrip_max_kernel");
  const int64_t total = (video ? 3 : 2) * plane;
  hipLaunchKernelGGL(filmstrip_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, st, y_attn, yh_attn, video, maxes, T, H, W, (unsigned*)out, total);
  MAAVSS_LAUNCH_CHECK("filmstrip_kernel");
  return MAAVSS_OK;
}
