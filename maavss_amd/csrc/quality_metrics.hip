// EXTENSION (the reference validates with its training loss only, train_av_net.py:147-181): quality metrics of held-out data, reduced on
// the device in f64 and in a fixed order -- what maavss_amd.quality (wave_metrics, spectrum_metrics, Validator) reads.
//
// Wave metrics of est [B][L] against ref [B][L] (f32, row strides in elements, rows may overlap, 4-byte alignment is enough: every load
// is one dword per lane, consecutive lanes on consecutive samples):
//   pass 1      one workgroup per chunk of a row (<= WM_CH samples, a whole number of seg_len frames except for the row's trailing
//               partial frame): Sxx, Syy, Sxy, See and, per complete frame, clamp(10 log10(Sxx_f / See_f), -10, 35) -> one partial
//   finalize 1  one wave per row adds the row's partials in index order (lane l takes chunks l, l + 64, ..., then a fixed butterfly), writes
//               the four sums, snr_db, seg_snr_db, the frame count, and alpha = Sxy / Sxx for pass 2
//   pass 2      the same chunks again: Srr = sum (est - alpha ref)^2, summed directly (Syy - Sxy^2 / Sxx cancels at high quality)
//   finalize 2  Srr and si_sdr_db
// Spectrum metrics of pred [B][2][T][F] against tgt: one wave per (b, t) frame -> {squared error, sqrt(mean_F d^2)}, one wave per row
// adds the T frames in order.  The plain squared-error rows (the attention term) are pass 2's kernel with alpha = 1 over chunks of SQ_CH
// elements, then that row sum.  The wave and workgroup orders are those of reduce.h.
// No floating-point atomic anywhere: every output has the same bits in every run.  A product that is not exact is rounded before it is
// added, so the terms are the ones tests/quality_twin.py sums and only the order of the additions differs: the Makefile compiles this
// file with -ffp-contract=off (under the library's -ffp-contract=fast the backend fuses across `#pragma clang fp contract(off)`); the
// explicit fma() calls are on exact products of f32 values, where fused and unfused give the same bits.
#include "common.h"
#include "metric_f64.h"

#define WM_CH 4096           // chunk length in samples: one 60 s recording (960 000 samples) is 235 workgroups; a wave reduces several
                             // frames before the per-workgroup log10 and wave sums (at 1024 those were 9/10 of pass 1's time)
#define WM_COLS 9            // out row: Sxx, Syy, Sxy, See, Srr, snr_db, si_sdr_db, seg_snr_db, frames
#define SQ_CH 4096           // chunk length of the plain squared-error rows

struct wm_partial {
  double sxx, syy, sxy, see, seg, frames;
};
static_assert(sizeof(wm_partial) == 48, "workspace layout of include/maavss.h");

static inline int wm_chunk_len(int seg_len) { return WM_CH / seg_len * seg_len; }
static inline int64_t wm_chunks_per_row(int64_t L, int seg_len) { return (L + wm_chunk_len(seg_len) - 1) / wm_chunk_len(seg_len); }

// sum over the G (a power of two <= 64) consecutive lanes a lane's group is made of; every lane of the group gets it
__device__ __forceinline__ double qm_group_sum(double v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// G lanes per frame (the smallest power of two >= seg_len, at most 64): 256 / G frames per step of the workgroup.  A lane keeps the
// frame sums of G successive steps (step t stays in the lane whose index in its group is t % G), so that the f64 log10 runs once per
// G steps with every lane on a frame of its own.
__global__ __launch_bounds__(256) void wave_metrics_pass1_kernel(const float* __restrict__ est, int64_t est_stride,
                                                                 const float* __restrict__ ref, int64_t ref_stride, int64_t L, int seg_len,
                                                                 int cl, int64_t nch, int G, wm_partial* __restrict__ partials) {
  __shared__ double red[4][6];
  const int64_t row = blockIdx.x / nch, c = blockIdx.x % nch;
  const int64_t start = c * cl;
  const int len = (int)(L - start < cl ? L - start : cl);
  const float* __restrict__ e = est + row * est_stride + start;
  const float* __restrict__ r = ref + row * ref_stride + start;
  const int tid = threadIdx.x, gi = tid / G, i = tid % G, ng = 256 / G;
  const int nf = (len + seg_len - 1) / seg_len, nf_whole = len / seg_len;      // the row's trailing partial frame counts in the sums only
  double tx = 0.0, ty = 0.0, txy = 0.0, te = 0.0, seg = 0.0, frames = 0.0;
  double pend_x = 0.0, pend_e = 0.0;
  bool pend = false;
  const int steps = (nf + ng - 1) / ng;
  for (int t = 0; t < steps; ++t) {
    const int f = t * ng + gi;
    const int o = f * seg_len;
    const int flen = f < nf ? (len - o < seg_len ? len - o : seg_len) : 0;
    double fx = 0.0, fe = 0.0;
#pragma unroll 4
    for (int k = i; k < flen; k += G) {
      const double x = (double)r[o + k], y = (double)e[o + k];
      const double d = y - x;
      fx = fma(x, x, fx);     // exact products of f32 values: one rounding, that of the sum
      ty = fma(y, y, ty);
      txy = fma(x, y, txy);
      fe += d * d;
    }
    tx += fx;
    te += fe;
    fx = qm_group_sum(fx, G);
    fe = qm_group_sum(fe, G);
    const int slot = t % G;
    if (i == slot) {
      pend_x = fx;
      pend_e = fe;
      pend = f < nf_whole;
    }
    if (slot == G - 1 || t == steps - 1) {
      if (pend && pend_x > 0.0) {             // a frame without reference energy is left out
        double v = 10.0 * log10(pend_x / pend_e);
        v = v < -10.0 ? -10.0 : v;
        v = v > 35.0 ? 35.0 : v;
        seg += v;
        frames += 1.0;
      }
      pend = false;
    }
  }
  double v[6] = {wave_sum_d(tx), wave_sum_d(ty), wave_sum_d(txy), wave_sum_d(te), wave_sum_d(seg), wave_sum_d(frames)};
  wg_reduce<WG_THREAD0, WG_SUM>(v, red, tid >> 6, tid & 63);
  if (tid == 0) {
    double* __restrict__ p = reinterpret_cast<double*>(partials + blockIdx.x);      // sxx, syy, sxy, see, seg, frames
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = v[k];
  }
}

// one wave per row
__global__ __launch_bounds__(64) void wave_metrics_finalize1_kernel(const wm_partial* __restrict__ partials, int64_t nch,
                                                                    double* __restrict__ alpha, double* __restrict__ out) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const double* __restrict__ p = reinterpret_cast<const double*>(partials + row * nch);
  const double sxx = wave_strided_sum_d(p + 0, nch, 6, lane), syy = wave_strided_sum_d(p + 1, nch, 6, lane);
  const double sxy = wave_strided_sum_d(p + 2, nch, 6, lane), see = wave_strided_sum_d(p + 3, nch, 6, lane);
  const double seg = wave_strided_sum_d(p + 4, nch, 6, lane), frames = wave_strided_sum_d(p + 5, nch, 6, lane);
  if (lane != 0) return;
  double* __restrict__ o = out + row * WM_COLS;
  // the squares of finite f32 values cannot overflow an f64 sum: Sxx + Syy is finite exactly when every sample of the row is
  if (!__builtin_isfinite(sxx + syy)) {
    for (int k = 0; k < WM_COLS; ++k) o[k] = k == 8 ? 0.0 : nan_d();
    alpha[row] = nan_d();
    return;
  }
  o[0] = sxx;
  o[1] = syy;
  o[2] = sxy;
  o[3] = see;
  o[5] = sxx == 0.0 ? nan_d() : 10.0 * log10(sxx / see);      // no reference, no ratio (0 / See = 0 would read -inf)
  o[7] = seg / frames;                                          // 0 / 0 = NaN without a usable frame
  o[8] = frames;
  alpha[row] = sxy / sxx;
}

// Sum of (e - a r)^2 over one chunk (<= cl elements) of one row of length L: a = alpha[row] (SCALED, pass 2 of the wave metrics), or
// a = 1 (the plain squared-error rows: e - r itself, without an f64 multiply by one per element).
template <bool SCALED>
__global__ __launch_bounds__(256) void sqerr_scaled_chunks_kernel(const float* __restrict__ est, int64_t est_stride,
                                                                  const float* __restrict__ ref, int64_t ref_stride, int64_t L, int cl,
                                                                  int64_t nch, const double* __restrict__ alpha, double* __restrict__ partials) {
  __shared__ double red[4][1];
  const int64_t row = blockIdx.x / nch, c = blockIdx.x % nch;
  const int64_t start = c * cl;
  const int len = (int)(L - start < cl ? L - start : cl);
  const float* __restrict__ e = est + row * est_stride + start;
  const float* __restrict__ r = ref + row * ref_stride + start;
  const double a = SCALED ? alpha[row] : 1.0;
  const int tid = threadIdx.x;
  double s = 0.0;
#pragma unroll 4
  for (int k = tid; k < len; k += 256) {
    const double d = SCALED ? (double)e[k] - a * (double)r[k] : (double)e[k] - (double)r[k];
    s += d * d;
  }
  s = wg_reduce<WG_THREAD0, WG_SUM>(wave_sum_d(s), red, tid >> 6, tid & 63);
  if (tid == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void wave_metrics_finalize2_kernel(const double* __restrict__ srr_part, int64_t nch,
                                                                    const double* __restrict__ alpha, double* __restrict__ out) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const double srr = wave_strided_sum_d(srr_part + row * nch, nch, 1, lane);
  if (lane != 0) return;
  double* __restrict__ o = out + row * WM_COLS;
  const double a = alpha[row], sxx = o[0];          // o[0] was written by finalize 1, a launch earlier on the stream
  if (!__builtin_isfinite(sxx + o[1])) return;      // a non-finite sample: the row is NaN already
  o[4] = srr;
  o[6] = 10.0 * log10(a * a * sxx / srr);
}

// one wave per (b, t) frame of [B][2][T][F]
__global__ __launch_bounds__(256) void spectrum_metrics_frames_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int64_t BT,
                                                                      int64_t T, int64_t F, double floor_p, double* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int64_t bt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bt >= BT) return;
  const int64_t b = bt / T, t = bt % T;
  const int64_t re = (b * 2 * T + t) * F, im = ((b * 2 + 1) * T + t) * F;
  double sq = 0.0, ls = 0.0;
#pragma unroll 2
  for (int64_t f = lane; f < F; f += 64) {
    const double pr = (double)pred[re + f], pi = (double)pred[im + f], tr = (double)tgt[re + f], ti = (double)tgt[im + f];
    const double dr = pr - tr, di = pi - ti;
    sq += dr * dr;
    sq += di * di;
    double pp = fma(pr, pr, pi * pi), pt = fma(tr, tr, ti * ti);      // exact products: one rounding
    pp = pp < floor_p ? floor_p : pp;         // a NaN power stays a NaN
    pt = pt < floor_p ? floor_p : pt;
    const double d = 10.0 * log10(pp / pt);   // = 10 log10(pp) - 10 log10(pt) to within a few 2^-53 of the levels (tests/quality_twin.py)
    ls += d * d;
  }
  sq = wave_sum_d(sq);
  ls = wave_sum_d(ls);
  if (lane == 0) {
    partials[2 * bt] = sq;
    partials[2 * bt + 1] = sqrt(ls / (double)F);
  }
}

// one wave per row: out[row][k] = sum over the row's `per_row` partials of column k (K columns), column 1 divided by div1
__global__ __launch_bounds__(64) void rows_sum_kernel(const double* __restrict__ partials, int64_t per_row, int K, double div1,
                                                      double* __restrict__ out) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  for (int k = 0; k < K; ++k) {
    const double s = wave_strided_sum_d(partials + row * per_row * K + k, per_row, K, lane);
    if (lane == 0) out[row * K + k] = k == 1 ? s / div1 : s;
  }
}

// The Validator's additive accumulator, one wave.  acc[0] += sum of vals[i * stride], acc[1] += n * weight.
__global__ __launch_bounds__(64) void metric_add_sum_kernel(const double* __restrict__ vals, int64_t n, int64_t stride, double weight,
                                                            double* __restrict__ acc) {
  const int lane = threadIdx.x;
  const double s = wave_strided_sum_d(vals, n, stride, lane);
  if (lane == 0) {
    acc[0] += s;
    acc[1] += (double)n * weight;
  }
}

// per column c < cols: v_i = vals[i * stride + c] (- minus[i * stride + c]); acc[5 c ..] += {sum of the finite v, count finite, +inf, -inf, NaN}
__global__ __launch_bounds__(64) void metric_add_classes_kernel(const double* __restrict__ vals, const double* __restrict__ minus, int64_t n,
                                                                int64_t stride, int cols, double* __restrict__ acc) {
  const int lane = threadIdx.x;
  for (int c = 0; c < cols; ++c) {
    double s = 0.0, nf = 0.0, np = 0.0, nn = 0.0, nq = 0.0;
    for (int64_t i = lane; i < n; i += 64) {
      double v = vals[i * stride + c];
      if (minus != nullptr) v -= minus[i * stride + c];
      const bool fin = __builtin_isfinite(v);
      s += fin ? v : 0.0;
      nf += fin ? 1.0 : 0.0;
      np += v == (double)INFINITY ? 1.0 : 0.0;
      nn += v == -(double)INFINITY ? 1.0 : 0.0;
      nq += v != v ? 1.0 : 0.0;
    }
    s = wave_sum_d(s);
    nf = wave_sum_d(nf);
    np = wave_sum_d(np);
    nn = wave_sum_d(nn);
    nq = wave_sum_d(nq);
    if (lane == 0) {
      acc[5 * c] += s;
      acc[5 * c + 1] += nf;
      acc[5 * c + 2] += np;
      acc[5 * c + 3] += nn;
      acc[5 * c + 4] += nq;
    }
  }
}

int rows_sum_launch(const double* partials, int64_t rows, int64_t per_row, int K, double div1, double* out, hipStream_t st) {
  hipLaunchKernelGGL(rows_sum_kernel, dim3((unsigned)rows), dim3(64), 0, st, partials, per_row, K, div1, out);
  MAAVSS_LAUNCH_CHECK("rows_sum_kernel");
  return MAAVSS_OK;
}

// The two chunk passes of the wave metrics, also launched by wave_loss.hip (metric_f64.h): one copy of the sums.
int64_t wave_chunks_per_row(int64_t L, int seg_len) { return wm_chunks_per_row(L, seg_len); }

int wave_sums_launch(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, int64_t B, int64_t L, int seg_len,
                     void* partials, hipStream_t st) {
  int G = 1;
  while (G < seg_len && G < 64) G <<= 1;
  const int64_t nch = wm_chunks_per_row(L, seg_len);
  hipLaunchKernelGGL(wave_metrics_pass1_kernel, dim3((unsigned)(B * nch)), dim3(256), 0, st, est, est_stride, ref, ref_stride, L, seg_len,
                     wm_chunk_len(seg_len), nch, G, (wm_partial*)partials);
  MAAVSS_LAUNCH_CHECK("wave_metrics_pass1_kernel");
  return MAAVSS_OK;
}

int wave_scaled_sqerr_launch(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, int64_t B, int64_t L, int seg_len,
                             const double* alpha, double* partials, hipStream_t st) {
  const int64_t nch = wm_chunks_per_row(L, seg_len);
  hipLaunchKernelGGL(sqerr_scaled_chunks_kernel<true>, dim3((unsigned)(B * nch)), dim3(256), 0, st, est, est_stride, ref, ref_stride, L,
                     wm_chunk_len(seg_len), nch, alpha, partials);
  MAAVSS_LAUNCH_CHECK("sqerr_scaled_chunks_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_wave_metrics_chunk(void) { return WM_CH; }

extern "C" int64_t maavss_wave_metrics_ws_bytes(int64_t B, int64_t L, int seg_len) {
  if (B <= 0 || L <= 0 || seg_len < 1 || seg_len > WM_CH) return 0;
  const int64_t nch = wm_chunks_per_row(L, seg_len);
  if (nch > ((int64_t)1 << 31) / B) return 0;
  return align256(B * nch * (int64_t)sizeof(wm_partial)) + align256(B * nch * 8) + align256(B * 8);
}

extern "C" int maavss_wave_metrics(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, int64_t B, int64_t L,
                                   int seg_len, double* out, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = metric_rows_check("wave_metrics", est, est_stride, ref, ref_stride, B, out, ws)) return rc;
  MAAVSS_CHECK_ARG(B > 0 && L > 0 && L < (int64_t)1 << 40, "wave_metrics: bad sizes (B %lld, L %lld)", (long long)B, (long long)L);
  MAAVSS_CHECK_ARG(seg_len >= 1 && seg_len <= WM_CH, "wave_metrics: seg_len must be in 1..%d (got %d)", WM_CH, seg_len);
  const int64_t nch = wm_chunks_per_row(L, seg_len);
  MAAVSS_CHECK_ARG(nch <= (((int64_t)1 << 31) - 1) / B, "wave_metrics: %lld rows of %lld chunks are more workgroups than one launch takes",
                   (long long)B, (long long)nch);
  const int64_t need = maavss_wave_metrics_ws_bytes(B, L, seg_len);
  MAAVSS_CHECK_ARG(ws_bytes >= need, "wave_metrics: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  wm_partial* partials = (wm_partial*)ws;
  double* srr = (double*)((char*)ws + align256(B * nch * (int64_t)sizeof(wm_partial)));
  double* alpha = (double*)((char*)srr + align256(B * nch * 8));
  const int64_t es = B == 1 ? 0 : est_stride, rs = B == 1 ? 0 : ref_stride;
  if (int rc = wave_sums_launch(est, es, ref, rs, B, L, seg_len, partials, st)) return rc;
  hipLaunchKernelGGL(wave_metrics_finalize1_kernel, dim3((unsigned)B), dim3(64), 0, st, partials, nch, alpha, out);
  MAAVSS_LAUNCH_CHECK("wave_metrics_finalize1_kernel");
  if (int rc = wave_scaled_sqerr_launch(est, es, ref, rs, B, L, seg_len, alpha, srr, st)) return rc;
  hipLaunchKernelGGL(wave_metrics_finalize2_kernel, dim3((unsigned)B), dim3(64), 0, st, srr, nch, alpha, out);
  MAAVSS_LAUNCH_CHECK("wave_metrics_finalize2_kernel");
  return MAAVSS_OK;
}

extern "C" int64_t maavss_spectrum_metrics_ws_bytes(int64_t B, int64_t T) {
  if (B <= 0 || T <= 0 || T > ((int64_t)1 << 32) / B) return 0;
  return align256(B * T * 16);
}

extern "C" int maavss_spectrum_metrics(const float* pred, const float* tgt, int64_t B, int64_t T, int64_t F, double lsd_floor, double* out,
                                       void* ws, int64_t ws_bytes, void* stream) {
  MAAVSS_CHECK_ARG(pred && tgt && out && ws, "spectrum_metrics: null pointer");
  MAAVSS_CHECK_ARG(B > 0 && T > 0 && F > 0 && T <= ((int64_t)1 << 32) / B && F < (int64_t)1 << 24,
                   "spectrum_metrics: bad sizes (B %lld, T %lld, F %lld)", (long long)B, (long long)T, (long long)F);
  MAAVSS_CHECK_ARG(lsd_floor > 0.0 && __builtin_isfinite(lsd_floor), "spectrum_metrics: the power floor must be positive and finite (got %g)",
                   lsd_floor);
  MAAVSS_CHECK_ARG((((uintptr_t)pred | (uintptr_t)tgt) & 3) == 0, "spectrum_metrics: pred and tgt must be 4-byte aligned");
  MAAVSS_CHECK_ARG((((uintptr_t)out | (uintptr_t)ws) & 7) == 0, "spectrum_metrics: out and workspace must be 8-byte aligned");
  const int64_t need = maavss_spectrum_metrics_ws_bytes(B, T);
  MAAVSS_CHECK_ARG(ws_bytes >= need, "spectrum_metrics: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)ws;
  hipLaunchKernelGGL(spectrum_metrics_frames_kernel, dim3((unsigned)((B * T + 3) / 4)), dim3(256), 0, st, pred, tgt, B * T, T, F, lsd_floor,
                     partials);
  MAAVSS_LAUNCH_CHECK("spectrum_metrics_frames_kernel");
  return rows_sum_launch(partials, B, T, 2, (double)T, out, st);
}

extern "C" int maavss_sqerr_rows_chunk(void) { return SQ_CH; }

extern "C" int64_t maavss_sqerr_rows_ws_bytes(int64_t B, int64_t n) {
  if (B <= 0 || n <= 0) return 0;
  const int64_t nch = (n + SQ_CH - 1) / SQ_CH;
  if (nch > ((int64_t)1 << 31) / B) return 0;
  return align256(B * nch * 8);
}

extern "C" int maavss_sqerr_rows(const float* pred, const float* tgt, int64_t B, int64_t n, double* out, void* ws, int64_t ws_bytes,
                                 void* stream) {
  MAAVSS_CHECK_ARG(pred && tgt && out && ws, "sqerr_rows: null pointer");
  MAAVSS_CHECK_ARG(B > 0 && n > 0 && n < (int64_t)1 << 40, "sqerr_rows: bad sizes (B %lld, n %lld)", (long long)B, (long long)n);
  MAAVSS_CHECK_ARG((((uintptr_t)pred | (uintptr_t)tgt) & 3) == 0, "sqerr_rows: pred and tgt must be 4-byte aligned");
  MAAVSS_CHECK_ARG((((uintptr_t)out | (uintptr_t)ws) & 7) == 0, "sqerr_rows: out and workspace must be 8-byte aligned");
  const int64_t nch = (n + SQ_CH - 1) / SQ_CH;
  MAAVSS_CHECK_ARG(nch <= (((int64_t)1 << 31) - 1) / B, "sqerr_rows: %lld rows of %lld chunks are more workgroups than one launch takes",
                   (long long)B, (long long)nch);
  const int64_t need = maavss_sqerr_rows_ws_bytes(B, n);
  MAAVSS_CHECK_ARG(ws_bytes >= need, "sqerr_rows: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)ws;
  hipLaunchKernelGGL(sqerr_scaled_chunks_kernel<false>, dim3((unsigned)(B * nch)), dim3(256), 0, st, pred, n, tgt, n, n, SQ_CH, nch,
                     (const double*)nullptr, partials);
  MAAVSS_LAUNCH_CHECK("sqerr_scaled_chunks_kernel");
  return rows_sum_launch(partials, B, nch, 1, 1.0, out, st);
}

extern "C" int maavss_metric_add_sum(const double* vals, int64_t n, int64_t stride, double weight, double* acc, void* stream) {
  MAAVSS_CHECK_ARG(vals && acc, "metric_add_sum: null pointer");
  MAAVSS_CHECK_ARG(n > 0 && stride >= 1, "metric_add_sum: bad sizes (n %lld, stride %lld)", (long long)n, (long long)stride);
  MAAVSS_CHECK_ARG((((uintptr_t)vals | (uintptr_t)acc) & 7) == 0, "metric_add_sum: values and accumulator must be 8-byte aligned");
  hipLaunchKernelGGL(metric_add_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, vals, n, stride, weight, acc);
  MAAVSS_LAUNCH_CHECK("metric_add_sum_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_metric_add_classes(const double* vals, const double* minus, int64_t n, int64_t stride, int cols, double* acc,
                                         void* stream) {
  MAAVSS_CHECK_ARG(vals && acc, "metric_add_classes: null pointer");
  MAAVSS_CHECK_ARG(n > 0 && cols >= 1 && stride >= cols, "metric_add_classes: bad sizes (n %lld, stride %lld, %d columns)", (long long)n,
                   (long long)stride, cols);
  MAAVSS_CHECK_ARG((((uintptr_t)vals | (uintptr_t)minus | (uintptr_t)acc) & 7) == 0,
                   "metric_add_classes: values and accumulator must be 8-byte aligned");
  hipLaunchKernelGGL(metric_add_classes_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, vals, minus, n, stride, cols, acc);
  MAAVSS_LAUNCH_CHECK("metric_add_classes_kernel");
  return MAAVSS_OK;
}
