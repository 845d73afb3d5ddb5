// EXTENSION: the power-law compressed spectral loss of pred [B][2][T][F] against tgt and its gradient (maavss_amd.SpectralLoss,
// TrainStep(audio_loss=...), Validator(audio_loss=...)).  include/maavss.h states the definition; tests/spectral_loss_twin.py is its
// float64 restatement, operation for operation.  Every operation here is f64 on the exactly converted f32 inputs and is rounded on its own
// (the file is compiled with -ffp-contract=off): the differences M_p - M_t and p g_p - t g_t cancel, and in f32 they lose the result.
//   spectral_loss_frames_kernel   one wave per (b, t) frame, four frames per workgroup: the frame's two sums to the workspace, and with
//                                 GRAD the gradient, each element rounded once to f32
//   rows_sum_kernel               (quality_metrics.hip, through rows_sum_launch) one wave per row: the row's frames in index order
//                                 -> rows [B][2]
//   spectral_pair_finalize_kernel the rows in index order -> losses [3] and parts [2], next to mse_pair's attention term (mse_term.h)
// No floating-point atomics: the same input gives the same bytes, and a row's bytes do not depend on the rows beside it.
#include "common.h"
#include "metric_f64.h"
#include "mse_term.h"

struct sl_params {
  double hc, hg;          // c / 2 and (c - 1) / 2: the exponents of M and g
  double c, cm1;          // c and c - 1
  double lam, oml;        // mix and 1 - mix
  double eps, gs2;        // the power added inside, and 2 grad_scale
};

template <bool GRAD>
__global__ __launch_bounds__(256) void spectral_loss_frames_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int64_t BT,
                                                                   int64_t T, int64_t F, sl_params P, float* __restrict__ d_pred,
                                                                   double* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int64_t bt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bt >= BT) return;
  const int64_t b = bt / T, t = bt % T;
  const int64_t re = (b * 2 * T + t) * F, im = ((b * 2 + 1) * T + t) * F;
  double mag = 0.0, cplx = 0.0;
  for (int64_t f = lane; f < F; f += 64) {
    const double pr = (double)pred[re + f], pi = (double)pred[im + f], tr = (double)tgt[re + f], ti = (double)tgt[im + f];
    const double rp = pr * pr + pi * pi + P.eps, rt = tr * tr + ti * ti + P.eps;
    const double Mp = pow(rp, P.hc), Mt = pow(rt, P.hc);
    const double gp = pow(rp, P.hg), gt = pow(rt, P.hg);       // a pow of its own: c = 1 gives exactly 1
    const double er = pr * gp - tr * gt, ei = pi * gp - ti * gt;
    const double dm = Mp - Mt;
    mag += dm * dm;
    cplx += er * er + ei * ei;
    if (GRAD) {
      const double s = er * pr + ei * pi;
      const double q = P.cm1 * gp / rp;
      const double k = P.oml * dm * P.c * Mp / rp;
      d_pred[re + f] = (float)(P.gs2 * (k * pr + P.lam * (er * gp + q * s * pr)));
      d_pred[im + f] = (float)(P.gs2 * (k * pi + P.lam * (ei * gp + q * s * pi)));
    }
  }
  mag = wave_sum_d(mag);
  cplx = wave_sum_d(cplx);
  if (lane == 0) {
    partials[2 * bt] = mag;
    partials[2 * bt + 1] = cplx;
  }
}

// losses[0] = a_loss, [1] = v_loss as mse_pair forms it, [2] = (a_loss + coeff v_loss) inv_num_seq; parts = the two means a_loss mixes
__global__ __launch_bounds__(64) void spectral_pair_finalize_kernel(const double* __restrict__ rows, int64_t B, double n_a, double lam,
                                                                    double oml, const float* __restrict__ pv, int nv_blk, double nv,
                                                                    float coeff, float inv_num_seq, float* __restrict__ losses,
                                                                    double* __restrict__ parts) {
  const int lane = threadIdx.x;
  const double mag = wave_strided_sum_d(rows, B, 2, lane), cplx = wave_strided_sum_d(rows + 1, B, 2, lane);
  if (lane != 0) return;
  const double la = (oml * mag + lam * cplx) / n_a, lv = mse_term_mean(pv, nv_blk, nv);
  parts[0] = mag / n_a;
  parts[1] = cplx / n_a;
  losses[0] = (float)la;
  losses[1] = (float)lv;
  losses[2] = (float)((la + (double)coeff * lv) * (double)inv_num_seq);
}

static inline bool sl_sizes_ok(int64_t B, int64_t T) { return B > 0 && T > 0 && T <= ((int64_t)1 << 32) / B; }

extern "C" int64_t maavss_spectral_loss_ws_bytes(int64_t B, int64_t T) {
  if (!sl_sizes_ok(B, T)) return 0;
  return align256(B * T * 16);
}

extern "C" int64_t maavss_spectral_loss_pair_ws_bytes(int64_t B, int64_t T) {
  if (!sl_sizes_ok(B, T)) return 0;
  return align256(B * T * 16) + align256(B * 16) + align256(MSE_BLK * 4);
}

// the checks every entry makes of the audio operands and the parameters; `who` names the entry in the message
static int sl_check(const char* who, const float* pred, const float* tgt, int64_t B, int64_t T, int64_t F, double compress, double mix,
                    double eps, const float* d_pred) {
  MAAVSS_CHECK_ARG(pred && tgt, "%s: null pointer", who);
  MAAVSS_CHECK_ARG(sl_sizes_ok(B, T) && F > 0 && F < (int64_t)1 << 24, "%s: bad sizes (B %lld, T %lld, F %lld)", who, (long long)B,
                   (long long)T, (long long)F);
  MAAVSS_CHECK_ARG(compress > 0.0 && compress <= 1.0, "%s: compress must be in (0, 1] (got %g)", who, compress);
  MAAVSS_CHECK_ARG(mix >= 0.0 && mix <= 1.0, "%s: mix must be in [0, 1] (got %g)", who, mix);
  MAAVSS_CHECK_ARG(eps > 0.0 && __builtin_isfinite(eps), "%s: eps must be positive and finite, a power (got %g)", who, eps);
  MAAVSS_CHECK_ARG((((uintptr_t)pred | (uintptr_t)tgt | (uintptr_t)d_pred) & 3) == 0, "%s: pred, tgt and d_pred must be 4-byte aligned", who);
  return MAAVSS_OK;
}

static int sl_launch(const float* pred, const float* tgt, int64_t B, int64_t T, int64_t F, double compress, double mix, double eps,
                     double grad_scale, float* d_pred, double* rows, double* partials, hipStream_t st) {
  sl_params P;
  P.hc = 0.5 * compress;
  P.hg = 0.5 * (compress - 1.0);
  P.c = compress;
  P.cm1 = compress - 1.0;
  P.lam = mix;
  P.oml = 1.0 - mix;
  P.eps = eps;
  P.gs2 = 2.0 * grad_scale;
  const dim3 grid((unsigned)((B * T + 3) / 4));
  if (d_pred != nullptr)
    hipLaunchKernelGGL(spectral_loss_frames_kernel<true>, grid, dim3(256), 0, st, pred, tgt, B * T, T, F, P, d_pred, partials);
  else
    hipLaunchKernelGGL(spectral_loss_frames_kernel<false>, grid, dim3(256), 0, st, pred, tgt, B * T, T, F, P, d_pred, partials);
  MAAVSS_LAUNCH_CHECK("spectral_loss_frames_kernel");
  return rows_sum_launch(partials, B, T, 2, 1.0, rows, st);      // s / 1.0 is s
}

extern "C" int maavss_spectral_loss(const float* pred, const float* tgt, int64_t B, int64_t T, int64_t F, double compress, double mix,
                                    double eps, double grad_scale, float* d_pred, double* rows, void* ws, int64_t ws_bytes, void* stream) {
  const int rc = sl_check("spectral_loss", pred, tgt, B, T, F, compress, mix, eps, d_pred);
  if (rc != MAAVSS_OK) return rc;
  MAAVSS_CHECK_ARG(rows && ws, "spectral_loss: null pointer");
  MAAVSS_CHECK_ARG(__builtin_isfinite(grad_scale), "spectral_loss: grad_scale must be finite (got %g)", grad_scale);
  MAAVSS_CHECK_ARG((((uintptr_t)rows | (uintptr_t)ws) & 7) == 0, "spectral_loss: rows and workspace must be 8-byte aligned");
  const int64_t need = maavss_spectral_loss_ws_bytes(B, T);
  MAAVSS_CHECK_ARG(ws_bytes >= need, "spectral_loss: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  return sl_launch(pred, tgt, B, T, F, compress, mix, eps, grad_scale, d_pred, rows, (double*)ws, (hipStream_t)stream);
}

extern "C" int maavss_spectral_loss_pair(const float* a_pred, const float* a_tgt, int64_t B, int64_t T, int64_t F, double compress,
                                         double mix, double eps, const float* v_pred, const float* v_tgt, int64_t nv, float coeff,
                                         float inv_num_seq, float* d_a, float* d_v, float* losses, double* parts, void* ws,
                                         int64_t ws_bytes, void* stream) {
  const int rc = sl_check("spectral_loss_pair", a_pred, a_tgt, B, T, F, compress, mix, eps, d_a);
  if (rc != MAAVSS_OK) return rc;
  MAAVSS_CHECK_ARG(v_pred && v_tgt && losses && parts && ws, "spectral_loss_pair: null pointer");
  MAAVSS_CHECK_ARG(nv > 0, "spectral_loss_pair: bad sizes (nv %lld)", (long long)nv);
  MAAVSS_CHECK_ARG(__builtin_isfinite(coeff) && __builtin_isfinite(inv_num_seq) && inv_num_seq > 0.f,
                   "spectral_loss_pair: coeff must be finite and inv_num_seq positive and finite (got %g, %g)", (double)coeff,
                   (double)inv_num_seq);
  MAAVSS_CHECK_ARG((((uintptr_t)v_pred | (uintptr_t)v_tgt | (uintptr_t)d_v | (uintptr_t)losses) & 3) == 0,
                   "spectral_loss_pair: v_pred, v_tgt, d_v and losses must be 4-byte aligned");
  MAAVSS_CHECK_ARG((((uintptr_t)parts | (uintptr_t)ws) & 7) == 0, "spectral_loss_pair: parts and workspace must be 8-byte aligned");
  const int64_t need = maavss_spectral_loss_pair_ws_bytes(B, T);
  MAAVSS_CHECK_ARG(ws_bytes >= need, "spectral_loss_pair: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)ws;
  double* rows = (double*)((char*)ws + align256(B * T * 16));
  float* pv = (float*)((char*)rows + align256(B * 16));
  const double n_a = (double)(2 * B * T * F);
  const int rl = sl_launch(a_pred, a_tgt, B, T, F, compress, mix, eps, (double)inv_num_seq / n_a, d_a, rows, partials, st);
  if (rl != MAAVSS_OK) return rl;
  const int gv = mse_term_launch(v_pred, v_tgt, nv, mse_grad_scale(coeff, inv_num_seq, nv), d_v, pv, st);
  hipLaunchKernelGGL(spectral_pair_finalize_kernel, dim3(1), dim3(64), 0, st, rows, B, n_a, mix, 1.0 - mix, pv, gv, (double)nv, coeff,
                     inv_num_seq, losses, parts);
  MAAVSS_LAUNCH_CHECK("spectral_loss_pair");
  return MAAVSS_OK;
}
