// One MSE term of maavss_mse_pair, for the entries that form the same term next to another audio loss (spectral_loss.hip): the
// kernel, its grid, its gradient scale and the sum of its partials exist once, in elementwise.hip and here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MSE_BLK 512      // the most workgroups of one term, 4096 elements each below that; a term's partials are MSE_BLK floats

// d(losses[2]) / d(pred) = mse_grad_scale * (pred - target) for a term of weight `weight` in losses[2]
static inline float mse_grad_scale(float weight, float inv_num_seq, int64_t n) { return 2.f * weight * inv_num_seq / (float)n; }

// elementwise.hip: launches mse_partial_kernel over the n elements (dpred nullable) -> the number of partials written
int mse_term_launch(const float* pred, const float* target, int64_t n, float gscale, float* dpred, float* partials, hipStream_t st);

// the term's mean from its partials, added left to right in f64
__device__ __forceinline__ double mse_term_mean(const float* __restrict__ partials, int n_blk, double n) {
  double s = 0.0;
  for (int i = 0; i < n_blk; ++i) s += (double)partials[i];
  return s / n;
}
