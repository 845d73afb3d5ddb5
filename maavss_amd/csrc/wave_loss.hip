// EXTENSION: a clip-level waveform loss (SI-SDR or SNR, in dB, lower is better) of pred [B][2][T][F] against tgt through the inverse
// STFT, and its gradient with respect to pred -- what maavss_amd.WaveformLoss and TrainStep(wave_loss=...) call.  include/maavss.h states
// the definition next to maavss_wave_loss; tests/wave_loss_twin.py is its float64 restatement.
//
//   waves      x = istft(pred), s = istft(tgt) by maavss_istft itself (stft.hip), twice: there is no second inverse STFT
//   sums       Sss, Sxx, Sxs, D = sum (x - s)^2 per chunk by the wave metrics' pass 1 (quality_metrics.hip through metric_f64.h), f64, fixed order
//   finalize   one wave per row adds the row's chunks in index order; SNR is finished here; SI-SDR writes alpha = Sxs / (Sss + eps)
//   pass 2     SI-SDR only: E = sum (x - alpha s)^2 per chunk, summed directly (the wave metrics' pass 2), then the second finalize
//              -> rows (l, Sxx, Sss, Sxs, E) and the row's two f64 gradient coefficients: g[n] = a x[n] + b s[n]
//   envelope   1 / den[n], den = the sum over the covering frames of w^2, in f64, once per call (it depends on the frame grid only): the
//              adjoint multiplies by it instead of dividing once per sample of every frame (measured: the launch's time is the same
//              either way, profiles/wave_loss_bench.json; the reciprocal is kept as the cheaper instruction stream)
//   adjoint    one wavefront per PAIR of consecutive frames (a pair may straddle two rows), as stft_kernel: the zero-padded frames
//              q_t[j] = c w[j] g[t hop + j - N/2] (1 / den[..]) are formed in f64 from x, s, the coefficients and den on the way into LDS and
//              rounded once to f32, two real frames as one complex frame; stft_fft.h's transform and split; the epilogue applies m_k and
//              grad_scale, zeroes the imaginary parts of DC and Nyquist and writes or adds both planes.  No gradient waveform and no frame
//              buffer goes through HBM.
// A row with a non-finite sample has NaN coefficients: its frames enter the transform as zeros (the frame of another row that shares the
// pair stays clean) and its gradient is written as NaN.  No floating-point atomics: two runs give identical bytes.
// This file is compiled with the library's -ffp-contract=fast (the transform wants it).  Two places where a fusion would change
// a contract hold their operands behind an empty asm: the accumulating epilogue, dst + v (v is rounded to f32 before the addition, so
// "added into dst" has the bits of "written, then added"), and g = a x + b s on the way in (wave_loss_g).
#include "common.h"
#include "metric_f64.h"
#include "stft_fft.h"

extern "C" int maavss_istft(const float* spec, int64_t batch, int n_frames, int n_bins_in, const float* window, int n_fft, int hop,
                            int normalized, float* frames_ws, float* audio, int64_t audio_stride, void* stream);

#define WL_SEG 256                 // frame length handed to the wave metrics' pass 1: whole chunks of maavss_wave_metrics_chunk() samples
#define WL_KIND_SI_SDR 0
#define WL_KIND_SNR 1
#define WL_COLS 5                  // rows: l, Sxx, Sss, Sxs, E

// rden[n] = 1 / den[n], n < L: den = the window-square envelope at position n + N/2 of the centre-padded signal, frames in index order, f64
__global__ __launch_bounds__(256) void wave_loss_envelope_kernel(const float* __restrict__ window, int n_fft, int hop, int n_frames, int L,
                                                                 double* __restrict__ rden) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= L) return;
  const int pos = n + n_fft / 2;
  int t_hi = pos / hop;
  if (t_hi > n_frames - 1) t_hi = n_frames - 1;
  int t_lo = (pos - n_fft + hop) / hop;                // smallest t with t*hop + n_fft > pos
  if (pos - n_fft + 1 <= 0) t_lo = 0;
  double d = 0.0;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int j = pos - t * hop;
    if (j < 0 || j >= n_fft) continue;
    const double w = (double)window[j];
    d += w * w;
  }
  rden[n] = 1.0 / d;
}

__device__ __forceinline__ double wl_db(double v) { return 10.0 * log10(v); }

// One wave per row.  stage 0: the sums of pass 1; an SNR row is finished, an SI-SDR row gets its alpha.  stage 1 (SI-SDR): E and the rest.
__global__ __launch_bounds__(64) void wave_loss_finalize_kernel(const double* __restrict__ partials, const double* __restrict__ e_part, int64_t nch,
                                                                int kind, int stage, double eps, double* __restrict__ alpha,
                                                                double* __restrict__ coef, double* __restrict__ rows) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  constexpr double K2 = 2.0 * 4.3429448190325182765;      // d(10 log10 v) = (10 / ln 10) dv / v, and d(sum e^2) = 2 e de
  double* __restrict__ o = rows + row * WL_COLS;
  if (stage == 0) {
    const double* __restrict__ p = partials + row * nch * WAVE_PARTIAL_DOUBLES;
    const double sss = wave_strided_sum_d(p + 0, nch, WAVE_PARTIAL_DOUBLES, lane), sxx = wave_strided_sum_d(p + 1, nch, WAVE_PARTIAL_DOUBLES, lane);
    const double sxs = wave_strided_sum_d(p + 2, nch, WAVE_PARTIAL_DOUBLES, lane), d = wave_strided_sum_d(p + 3, nch, WAVE_PARTIAL_DOUBLES, lane);
    if (lane != 0) return;
    // the squares of finite f32 values cannot overflow an f64 sum: Sxx + Sss is finite exactly when every sample of the row is
    if (!__builtin_isfinite(sxx + sss)) {
      for (int k = 0; k < WL_COLS; ++k) o[k] = nan_d();
      alpha[row] = nan_d();
      coef[2 * row] = coef[2 * row + 1] = nan_d();
      return;
    }
    o[1] = sxx;
    o[2] = sss;
    o[3] = sxs;
    if (kind == WL_KIND_SNR) {
      o[0] = wl_db(d + eps) - wl_db(sss + eps);
      o[4] = d;
      const double a = K2 / (d + eps);
      coef[2 * row] = a;
      coef[2 * row + 1] = -a;
      alpha[row] = 1.0;
    } else {
      alpha[row] = sxs / (sss + eps);
    }
    return;
  }
  const double e = wave_strided_sum_d(e_part + row * nch, nch, 1, lane);
  if (lane != 0) return;
  const double al = alpha[row];
  if (al != al) return;                                    // a non-finite sample: the row is NaN already
  const double sss = o[2];                                 // written by stage 0, a launch earlier on the stream
  const double d1 = e + eps, ps = sss + eps, d2 = al * al * sss + eps;
  o[0] = wl_db(d1) - wl_db(d2);
  o[4] = e;
  coef[2 * row] = K2 / d1;
  coef[2 * row + 1] = -K2 * al * ((1.0 + eps / ps) / d1 + sss / (ps * d2));
}

// g = a x + b s with BOTH products rounded before the addition (the empty asm keeps the backend from fusing one of them into the sum):
// with b = -a and x == s the two products are the same number and g is an exact zero, as in the twin
__device__ __forceinline__ double wave_loss_g(double a, float x, double b, float s) {
  double p = a * (double)x, q = b * (double)s;
  asm volatile("" : "+v"(p), "+v"(q));
  return p + q;
}

// dst[n] = (q_t0[n], q_t1[n]), n < NFFT: the zero-padded (NOT reflected) frame t of u = g (1 / den), windowed by c w; every operation in
// f64, one rounding to f32.  A frame that is not `live` (no second frame, or a row without finite coefficients) is zeros.
template <int NFFT>
__device__ __forceinline__ void wave_loss_load_pair(float2* dst, const float* __restrict__ window, const double* __restrict__ rden, double c, int lane,
                                                    int hop, int L, const float* __restrict__ x0, const float* __restrict__ s0, double a0, double b0,
                                                    int t0, bool live0, const float* __restrict__ x1, const float* __restrict__ s1, double a1,
                                                    double b1, int t1, bool live1) {
  for (int n = lane; n < NFFT; n += 64) {
    const double cw = c * (double)window[n];
    const int i0 = t0 * hop + n - NFFT / 2, i1 = t1 * hop + n - NFFT / 2;
    float q0 = 0.f, q1 = 0.f;
    if (live0 && i0 >= 0 && i0 < L) q0 = (float)(wave_loss_g(a0, x0[i0], b0, s0[i0]) * rden[i0] * cw);
    if (live1 && i1 >= 0 && i1 < L) q1 = (float)(wave_loss_g(a1, x1[i1], b1, s1[i1]) * rden[i1] * cw);
    dst[n] = make_float2(q0, q1);
  }
}

// frame t of the clip lands in block t / d_frames of the destination, a contiguous [B][2][d_frames][F] each, d_block_stride elements apart
template <int NFFT, int FPB>
__global__ __launch_bounds__(64 * FPB) void wave_loss_adjoint_kernel(const float* __restrict__ xw, const float* __restrict__ sw, int L,
                                                                     const double* __restrict__ coef, const double* __restrict__ rden,
                                                                     const float* __restrict__ window, double c, int hop, int n_frames,
                                                                     int n_bins, int total_frames, float gscale, float* __restrict__ dst,
                                                                     int d_frames, int64_t d_block_stride, int accumulate) {
  __shared__ float2 buf[STFT_NBUF<NFFT>][FPB][NFFT];
  __shared__ float2 tw[NFFT];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  stft_twiddles<NFFT>(tw);
  const int npairs = (total_frames + 1) / 2;
  const int n_low = n_bins < NFFT / 2 ? n_bins : NFFT / 2;
  const int64_t dplane = (int64_t)d_frames * n_bins;
  const float nanf32 = __uint_as_float(0x7fc00000u);
  for (int pid = blockIdx.x * FPB + wv; pid < npairs; pid += gridDim.x * FPB) {
    const int fid0 = 2 * pid, fid1 = fid0 + 1;
    const bool two_frames = fid1 < total_frames;
    const int b0 = fid0 / n_frames, t0 = fid0 % n_frames;
    const int b1 = two_frames ? fid1 / n_frames : b0, t1 = two_frames ? fid1 % n_frames : t0;
    const double a0 = coef[2 * b0], c0 = coef[2 * b0 + 1], a1 = coef[2 * b1], c1 = coef[2 * b1 + 1];
    const bool ok0 = __builtin_isfinite(a0) && __builtin_isfinite(c0), ok1 = __builtin_isfinite(a1) && __builtin_isfinite(c1);
    wave_loss_load_pair<NFFT>(&buf[0][wv][0], window, rden, c, lane, hop, L, xw + (int64_t)b0 * L, sw + (int64_t)b0 * L, a0, c0, t0, ok0,
                              xw + (int64_t)b1 * L, sw + (int64_t)b1 * L, a1, c1, t1, ok1 && two_frames);
    STFT_WAVE_SYNC();
    const int cur = fft_forward<NFFT>(&buf[0][wv][0], &buf[STFT_NBUF<NFFT> - 1][wv][0], tw, lane);
#pragma unroll
    for (int fr = 0; fr < 2; ++fr) {
      if (fr == 1 && !two_frames) break;
      const int b = fr ? b1 : b0, t = fr ? t1 : t0;
      const bool ok = fr ? ok1 : ok0;
      float* re = dst + (int64_t)(t / d_frames) * d_block_stride + ((int64_t)b * 2) * dplane + (int64_t)(t % d_frames) * n_bins;
      float* im = re + dplane;
      auto put = [&](float* p, float v) __attribute__((always_inline)) {
        if (accumulate) {
          asm volatile("" : "+v"(v));      // v is rounded here: no fused multiply-add into *p
          *p = *p + v;
        } else {
          *p = v;
        }
      };
      for (int f = lane; f < n_low; f += 64) {
        const float2 v = stft_split<NFFT>(&buf[cur][wv][0], f, fr);
        const float m = f == 0 ? gscale : 2.f * gscale;      // m_k grad_scale: the split's 1/2 is exact
        put(re + f, ok ? v.x * m : nanf32);
        put(im + f, ok ? (f == 0 ? 0.f : v.y * m) : nanf32);
      }
      if (n_bins > NFFT / 2 && lane == 0) {
        const float2 v = stft_split<NFFT>(&buf[cur][wv][0], NFFT / 2, fr);
        put(re + NFFT / 2, ok ? v.x * gscale : nanf32);
        put(im + NFFT / 2, ok ? 0.f : nanf32);
      }
    }
    STFT_WAVE_SYNC();      // the next pair overwrites buf[0][wv]
  }
}

struct wl_layout {
  int64_t L, nch, waves, frames, den, partials, epart, alpha, coef, total;
};
// -> false for sizes the entry refuses
static bool wl_plan(int64_t B, int64_t T, int n_fft, int hop, wl_layout& w) {
  if (B <= 0 || T < 2 || !(n_fft == 256 || n_fft == 512 || n_fft == 1024) || hop <= 0 || hop > n_fft) return false;
  if (T > ((int64_t)1 << 24) / B) return false;                              // B T frames: an int everywhere
  w.L = (int64_t)hop * (T - 1);
  if (w.L + n_fft >= (int64_t)1 << 31 || B * w.L >= (int64_t)1 << 34) return false;
  w.nch = wave_chunks_per_row(w.L, WL_SEG);
  w.waves = 0;
  w.frames = w.waves + align256(2 * B * w.L * 4);
  w.den = w.frames + align256(B * T * n_fft * 4);
  w.partials = w.den + align256(w.L * 8);
  w.epart = w.partials + align256(B * w.nch * WAVE_PARTIAL_DOUBLES * 8);
  w.alpha = w.epart + align256(B * w.nch * 8);
  w.coef = w.alpha + align256(B * 8);
  w.total = w.coef + align256(B * 16);
  return true;
}

extern "C" int64_t maavss_wave_loss_ws_bytes(int64_t B, int64_t T, int n_fft, int hop) {
  wl_layout w;
  return wl_plan(B, T, n_fft, hop, w) ? w.total : 0;
}

extern "C" int maavss_wave_loss(const float* pred, const float* tgt, int64_t B, int64_t T, int n_bins, const float* window, int n_fft, int hop,
                                int normalized, int kind, double eps, double grad_scale, float* d_pred, int64_t d_frames,
                                int64_t d_block_stride, int accumulate, double* rows, void* ws, int64_t ws_bytes, void* stream) {
  MAAVSS_CHECK_ARG(pred && tgt && window && rows && ws, "wave_loss: null pointer");
  STFT_CHECK_N_FFT("wave_loss", n_fft);
  MAAVSS_CHECK_ARG(B > 0 && T >= 2, "wave_loss: needs at least one row of two frames (B %lld, T %lld)", (long long)B, (long long)T);
  MAAVSS_CHECK_ARG(n_bins == n_fft / 2 || n_bins == n_fft / 2 + 1, "wave_loss: n_bins must be n_fft/2 (trimmed) or n_fft/2+1 (got %d)", n_bins);
  MAAVSS_CHECK_ARG(hop > 0 && hop <= n_fft, "wave_loss: hop must be in 1..n_fft (got %d)", hop);
  MAAVSS_CHECK_ARG(kind == WL_KIND_SI_SDR || kind == WL_KIND_SNR, "wave_loss: kind must be 0 (si_sdr) or 1 (snr), got %d", kind);
  MAAVSS_CHECK_ARG(eps > 0.0 && __builtin_isfinite(eps), "wave_loss: eps must be positive and finite (got %g)", eps);
  MAAVSS_CHECK_ARG(__builtin_isfinite(grad_scale), "wave_loss: grad_scale must be finite (got %g)", grad_scale);
  wl_layout w;
  MAAVSS_CHECK_ARG(wl_plan(B, T, n_fft, hop, w), "wave_loss: bad sizes (B %lld, T %lld): too many frames or samples for one call", (long long)B,
                   (long long)T);
  MAAVSS_CHECK_ARG((((uintptr_t)pred | (uintptr_t)tgt | (uintptr_t)window | (uintptr_t)d_pred) & 3) == 0,
                   "wave_loss: pred, tgt, window and d_pred must be 4-byte aligned");
  MAAVSS_CHECK_ARG((((uintptr_t)rows | (uintptr_t)ws) & 7) == 0, "wave_loss: rows and workspace must be 8-byte aligned");
  if (d_pred != nullptr) {
    MAAVSS_CHECK_ARG(d_frames >= 1 && d_frames <= T && T % d_frames == 0, "wave_loss: d_frames %lld does not divide the %lld frames",
                     (long long)d_frames, (long long)T);
    MAAVSS_CHECK_ARG(d_frames == T || d_block_stride >= B * 2 * d_frames * n_bins,
                     "wave_loss: d_block_stride %lld is smaller than a block of %lld elements", (long long)d_block_stride,
                     (long long)(B * 2 * d_frames * n_bins));
  }
  MAAVSS_CHECK_ARG(ws_bytes >= w.total, "wave_loss: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)w.total);
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  float* xw = (float*)(base + w.waves);
  float* sw = xw + B * w.L;
  float* frames = (float*)(base + w.frames);
  double* den = (double*)(base + w.den);
  double* partials = (double*)(base + w.partials);
  double* epart = (double*)(base + w.epart);
  double* alpha = (double*)(base + w.alpha);
  double* coef = (double*)(base + w.coef);
  const int L = (int)w.L;
  if (int rc = maavss_istft(pred, B, (int)T, n_bins, window, n_fft, hop, normalized, frames, xw, w.L, stream)) return rc;
  if (int rc = maavss_istft(tgt, B, (int)T, n_bins, window, n_fft, hop, normalized, frames, sw, w.L, stream)) return rc;
  // est = x, ref = s: the partial's "ref^2" is Sss, its "est^2" Sxx
  if (int rc = wave_sums_launch(xw, w.L, sw, w.L, B, w.L, WL_SEG, partials, st)) return rc;
  hipLaunchKernelGGL(wave_loss_finalize_kernel, dim3((unsigned)B), dim3(64), 0, st, partials, epart, w.nch, kind, 0, eps, alpha, coef, rows);
  MAAVSS_LAUNCH_CHECK("wave_loss_finalize_kernel");
  if (kind == WL_KIND_SI_SDR) {
    if (int rc = wave_scaled_sqerr_launch(xw, w.L, sw, w.L, B, w.L, WL_SEG, alpha, epart, st)) return rc;
    hipLaunchKernelGGL(wave_loss_finalize_kernel, dim3((unsigned)B), dim3(64), 0, st, partials, epart, w.nch, kind, 1, eps, alpha, coef, rows);
    MAAVSS_LAUNCH_CHECK("wave_loss_finalize_kernel");
  }
  if (d_pred == nullptr) return MAAVSS_OK;
  hipLaunchKernelGGL(wave_loss_envelope_kernel, dim3(cdiv(L, 256)), dim3(256), 0, st, window, n_fft, hop, (int)T, L, den);
  MAAVSS_LAUNCH_CHECK("wave_loss_envelope_kernel");
  const int total = (int)(B * T);
  const double c = (normalized ? sqrt((double)n_fft) : 1.0) / (double)n_fft;
#define LAUNCH(N, FPB)                                                                                                                     \
  hipLaunchKernelGGL((wave_loss_adjoint_kernel<N, FPB>), dim3(stft_pair_grid(cdiv(total, 2), FPB)), dim3(64 * FPB), 0, st, xw, sw, L, coef, \
                     den, window, c, hop, (int)T, n_bins, total, (float)grad_scale, d_pred, (int)d_frames, d_block_stride, accumulate ? 1 : 0)
  STFT_DISPATCH(n_fft, LAUNCH);
#undef LAUNCH
  MAAVSS_LAUNCH_CHECK("wave_loss_adjoint_kernel");
  return MAAVSS_OK;
}
