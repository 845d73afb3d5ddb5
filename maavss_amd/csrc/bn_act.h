// The BatchNorm, max-pool and activation arithmetic that several kernels must compute bit for bit alike, in ONE copy: conv3d_c1.hip repeats
// bn_pool.hip's forward and backward on a recomputed conv output, the split (cross-rank) finalize kernels repeat the unsplit ones, and the dense
// passes of gemm.hip / linear_skinny.hip and the LSTM gates share one activation.  Device only, and scalars only: a kernel calls these once per
// channel (a form that takes the four channels of a float4 or an array compiles to other code).
#pragma once
#include <hip/hip_runtime.h>

#define ACT_LEAKY 0
#define ACT_TANH 1
#define BN_INV_MIN_GAMMA 1e-2f      // below this |gamma| xhat is not recoverable from the pooled output: those channels gather it from y

// gamma * (y - mean) * invstd + beta as y * sc + sh
__device__ __forceinline__ float bn_shift(float beta, float mean, float sc) { return beta - mean * sc; }
__device__ __forceinline__ void bn_scale_shift(float gamma, float invstd, float beta, float mean, float& sc, float& sh) { sc = gamma * invstd; sh = bn_shift(beta, mean, sc); }
__device__ __forceinline__ float bn_affine(float y, float sc, float sh) { return y * sc + sh; }
// a pool window is scanned in the order dy, dx: the first maximum wins, a NaN sticks
__device__ __forceinline__ bool pool_take(float v, float best) { return v > best || (v != v && best == best); }
__device__ __forceinline__ float leaky_fwd(float v) { return v > 0.f ? v : 0.01f * v; }
__device__ __forceinline__ float leaky_slope(float s) { return s > 0.f ? 1.f : 0.01f; }      // s: the output, or anything of its sign
__device__ __forceinline__ float leaky_inv(float out) { return out > 0.f ? out : out * 100.f; }
__device__ __forceinline__ float tanh_slope(float out) { return 1.f - out * out; }
__device__ __forceinline__ float sigmoid_slope(float out) { return out * (1.f - out); }
__device__ __forceinline__ float act_fwd(float v, int act) { return act == ACT_TANH ? tanhf(v) : leaky_fwd(v); }
__device__ __forceinline__ float act_bwd_from_out(float out, int act) { return act == ACT_TANH ? tanh_slope(out) : leaky_slope(out); }
// BatchNorm backward of one element: gg = the gradient routed to it, k0 = gamma invstd, k1 = mean(dz), k2 = mean(dz xhat)
__device__ __forceinline__ float bn_dy(float gg, float y, float mu, float is, float k0, float k1, float k2) { return k0 * (gg - k1 - (y - mu) * is * k2); }
// the dense activation (include/maavss.h `act`): 0 none, 1 tanh, 2 sigmoid
__device__ __forceinline__ float sigmoid_fast(float v) { return 1.0f / (1.0f + __expf(-v)); }
__device__ __forceinline__ float dense_act(float v, int act) { return act == 1 ? tanhf(v) : act == 2 ? sigmoid_fast(v) : v; }

// The two finalize bodies of channel c, from plain sums (unsplit: the workgroup's own; split: the all-reduced ones).
// mean / invstd (biased variance) and the running statistics (unbiased) from s1 = sum y, s2 = sum y^2 over `count` elements
__device__ __forceinline__ void bn_finalize_channel(int c, double s1, double s2, double count, float eps, float momentum, float* __restrict__ mean,
                                                    float* __restrict__ invstd, float* __restrict__ running_mean, float* __restrict__ running_var) {
  const double m = s1 / count;
  double var = s2 / count - m * m;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)m;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean != nullptr) {
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
  }
}
// dgamma / dbeta from this rank's sums (l1 = sum g, l2 = sum g xhat -- with beta_inv, sum g z of the inverse-LeakyReLU form, and
// sum g xhat = (l2 - beta l1) / gamma), coef[0..2][c] = gamma invstd, mean(g), mean(g xhat) from the global sums g1, g2
__device__ __forceinline__ void bn_bwd_finalize_channel(int c, int C, double l1, double l2, double g1, double g2, double count, const float* __restrict__ gamma,
                                                        const float* __restrict__ invstd, float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate,
                                                        float* __restrict__ coef, const float* __restrict__ beta_inv) {
  if (beta_inv != nullptr && fabsf(gamma[c]) >= BN_INV_MIN_GAMMA) {
    l2 = (l2 - (double)beta_inv[c] * l1) / (double)gamma[c];
    g2 = (g2 - (double)beta_inv[c] * g1) / (double)gamma[c];
  }
  if (dgamma != nullptr) {
    dgamma[c] = (accumulate ? dgamma[c] : 0.f) + (float)l2;
    dbeta[c] = (accumulate ? dbeta[c] : 0.f) + (float)l1;
  }
  coef[c] = gamma[c] * invstd[c];
  coef[C + c] = (float)(g1 / count);
  coef[2 * C + c] = (float)(g2 / count);
}
