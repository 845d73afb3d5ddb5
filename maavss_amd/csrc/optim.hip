// EXTENSION (not in the reference, whose optimizer is torch.optim.Adam at one fixed rate, train_avse_frames.py:92):
//   adamw_ema_step   AdamW's decoupled weight decay (per tensor), an exponential moving average of the weights and the skip of a step
//                    whose gradient norm is not finite, in the ONE pass that already streams p, g, m and v (28 B per parameter; 36 B
//                    with the EMA buffer).  tests/optim_twin.py is the contract: every f32 operation below is rounded on its own, so
//                    this file is compiled with -ffp-contract=off (Makefile) and the results equal the twin's bit for bit.
//   swap_f32         in-place exchange of two buffers (the weights and their average around a validation pass).
//
// How a thread finds the decay of its elements: the decay table (segment ends and one factor per segment, at most OPTIM_MAX_SEG = 64
// segments) travels BY VALUE in the kernel arguments; the first 64 threads of a workgroup stage it in LDS (768 bytes), and every thread
// keeps a cursor into it (segment, its end, its factor: registers) that only moves forward -- the float4 indices of a grid-stride loop
// ascend, so over the whole loop a thread takes at most n_seg cursor steps, and LDS is read only in an iteration that crosses a segment
// end, after that iteration's loads have been issued.  Chosen over
//   * indexing the by-value table directly: a per-lane index into kernel arguments makes the compiler spill the struct to scratch;
//   * a device-side table: one more allocation and a staging copy per change of the frozen set, for 768 bytes;
//   * contiguous slabs per workgroup: the loop would no longer be the grid-stride loop of the plain Adam kernel it is measured against.
// Tensors are 64-element aligned in FlatParams and the segment ends are multiples of 4, so a float4 never straddles two segments and
// the scalar tail (n % 4 elements) lies in the last segment that the last float4 lies in.
//
// Grid: min(n4 / 256 + 1, 4096) workgroups of 256 threads, as ew_grid() of elementwise.hip: the loop takes a second trip from
// n4 > 4096 * 256, that is n > 4 194 304 elements.
#include "common.h"

#define OPTIM_MAX_SEG 64
#define OPTIM_GRID_CAP 4096

struct OptimTable {
  int64_t end4[OPTIM_MAX_SEG];   // segment ends relative to the run, in float4 units (ascending; the last one covers n)
  float decay[OPTIM_MAX_SEG];    // (float)(1 - lr * weight_decay) of the segment, 1.0f for an undecayed tensor
  int n_seg;
};

struct OptimScalars {
  float lr_bc1, b1, b2, omb1, omb2, eps, inv_sqrt_bc2, gscale, d, one_m_d;
};

__device__ __forceinline__ bool optim_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// one element: the definition of include/maavss.h, one rounding per operation
template <bool EMA>
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float& e, const OptimScalars& c, float gscale, float decay) {
  const float gr = g * gscale;
  const float t1 = c.omb1 * gr;
  m = c.b1 * m + t1;
  const float t2 = (c.omb2 * gr) * gr;
  v = c.b2 * v + t2;
  const float pd = p * decay;
  const float num = c.lr_bc1 * m;
  const float den = sqrtf(v) * c.inv_sqrt_bc2 + c.eps;
  p = pd - num / den;
  if constexpr (EMA) {
    const float t3 = c.one_m_d * p;
    e = c.d * e + t3;
  }
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ ema, int64_t n4, int64_t n,
                                                        OptimScalars c, const float* __restrict__ scale_dev,
                                                        const float* __restrict__ norm_dev, int* __restrict__ skipped, OptimTable tab) {
  // the skip: the norm is one value for the whole grid, so every thread takes the same way and none has stored anything yet
  if (norm_dev != nullptr && optim_nonfinite(*norm_dev)) {
    if (skipped != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *skipped = *skipped + 1;     // launches on a stream are ordered: no atomic
    return;
  }
  __shared__ int64_t s_end[OPTIM_MAX_SEG];
  __shared__ float s_decay[OPTIM_MAX_SEG];
  if (threadIdx.x < OPTIM_MAX_SEG) {
    const int k = (int)threadIdx.x < tab.n_seg ? (int)threadIdx.x : tab.n_seg - 1;
    s_end[threadIdx.x] = tab.end4[k];
    s_decay[threadIdx.x] = tab.decay[k];
  }
  __syncthreads();
  const float gscale = scale_dev != nullptr ? *scale_dev : c.gscale;
  const int last = tab.n_seg - 1;
  // the cursor: segment s, its end and its factor live in registers; LDS is read only when the loop crosses a segment end
  int s = 0;
  int64_t cur_end = s_end[0];
  float decay = s_decay[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ee = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EMA) ee = reinterpret_cast<float4*>(ema)[i];
    if (i >= cur_end) {            // after the loads are issued: the walk hides behind them
      while (s < last && i >= cur_end) {
        ++s;
        cur_end = s_end[s];
      }
      decay = s_decay[s];
    }
    adamw_one<EMA>(pp.x, gg.x, mm.x, vv.x, ee.x, c, gscale, decay);
    adamw_one<EMA>(pp.y, gg.y, mm.y, vv.y, ee.y, c, gscale, decay);
    adamw_one<EMA>(pp.z, gg.z, mm.z, vv.z, ee.z, c, gscale, decay);
    adamw_one<EMA>(pp.w, gg.w, mm.w, vv.w, ee.w, c, gscale, decay);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if constexpr (EMA) reinterpret_cast<float4*>(ema)[i] = ee;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && n4 * 4 < n) {
    int st = 0;
    while (st < last && n4 >= s_end[st]) ++st;
    const float decay = s_decay[st];
    for (int64_t i = n4 * 4; i < n; ++i) {
      float pp = p[i], mm = m[i], vv = v[i], ee = 0.f;
      if constexpr (EMA) ee = ema[i];
      adamw_one<EMA>(pp, g[i], mm, vv, ee, c, gscale, decay);
      p[i] = pp;
      m[i] = mm;
      v[i] = vv;
      if constexpr (EMA) ema[i] = ee;
    }
  }
}

__global__ __launch_bounds__(256) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n4, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 x = reinterpret_cast<float4*>(a)[i], y = reinterpret_cast<float4*>(b)[i];
    reinterpret_cast<float4*>(a)[i] = y;
    reinterpret_cast<float4*>(b)[i] = x;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t i = n4 * 4; i < n; ++i) {
      const float x = a[i];
      a[i] = b[i];
      b[i] = x;
    }
  }
}

static inline int optim_grid(int64_t n4) { return (int)(n4 / 256 + 1 > OPTIM_GRID_CAP ? OPTIM_GRID_CAP : n4 / 256 + 1); }

extern "C" int maavss_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                                     float beta2, float eps, int64_t step, float grad_scale, const float* scale_dev,
                                     const float* norm_dev, int skip_nonfinite, int* skipped, int count_skip,
                                     const int64_t* host_seg_end, const float* host_seg_wd, int n_seg, float ema_decay, void* stream) {
  MAAVSS_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adamw_ema_step: bad arguments");
  MAAVSS_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0,
                   "adamw_ema_step: buffers must be 16-byte aligned");
  MAAVSS_CHECK_ARG(((uintptr_t)scale_dev & 3) == 0, "adamw_ema_step: scale_dev must be 4-byte aligned");
  MAAVSS_CHECK_ARG(!skip_nonfinite || norm_dev, "adamw_ema_step: skip_nonfinite needs norm_dev");
  MAAVSS_CHECK_ARG(((uintptr_t)norm_dev & 3) == 0, "adamw_ema_step: norm_dev must be 4-byte aligned");
  MAAVSS_CHECK_ARG(!count_skip || (skip_nonfinite && skipped), "adamw_ema_step: count_skip needs skip_nonfinite and skipped");
  MAAVSS_CHECK_ARG(((uintptr_t)skipped & 3) == 0, "adamw_ema_step: skipped must be 4-byte aligned");
  MAAVSS_CHECK_ARG(!ema || (ema_decay >= 0.f && ema_decay < 1.f), "adamw_ema_step: ema_decay must be in [0, 1)");
  MAAVSS_CHECK_ARG(host_seg_end && host_seg_wd, "adamw_ema_step: the decay table is missing");
  MAAVSS_CHECK_ARG(n_seg >= 1 && n_seg <= OPTIM_MAX_SEG, "adamw_ema_step: n_seg must be in 1..%d (split the run)", OPTIM_MAX_SEG);
  OptimTable tab;
  int64_t prev = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int64_t e = host_seg_end[s];
    MAAVSS_CHECK_ARG(e > prev && e % 4 == 0, "adamw_ema_step: segment ends must ascend and be multiples of 4 (segment %d ends at %lld)", s,
                     (long long)e);
    MAAVSS_CHECK_ARG(host_seg_wd[s] >= 0.f && host_seg_wd[s] < INFINITY, "adamw_ema_step: weight decay of segment %d must be finite and >= 0", s);
    prev = e;
    tab.end4[s] = e / 4;
    tab.decay[s] = (float)(1.0 - (double)lr * (double)host_seg_wd[s]);
  }
  MAAVSS_CHECK_ARG(prev >= n, "adamw_ema_step: the last segment ends at %lld, before n = %lld", (long long)prev, (long long)n);
  for (int s = n_seg; s < OPTIM_MAX_SEG; ++s) {
    tab.end4[s] = tab.end4[n_seg - 1];
    tab.decay[s] = tab.decay[n_seg - 1];
  }
  tab.n_seg = n_seg;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  OptimScalars c;
  c.lr_bc1 = (float)(lr / bc1);
  c.b1 = beta1;
  c.b2 = beta2;
  c.omb1 = 1.f - beta1;
  c.omb2 = 1.f - beta2;
  c.eps = eps;
  c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  c.gscale = grad_scale;
  c.d = ema_decay;
  c.one_m_d = (float)(1.0 - (double)ema_decay);
  const int64_t n4 = n / 4;
  const float* nd = skip_nonfinite ? norm_dev : nullptr;
  int* sk = count_skip ? skipped : nullptr;
  if (ema != nullptr)
    hipLaunchKernelGGL(adamw_ema_kernel<true>, dim3(optim_grid(n4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n4, n, c, scale_dev,
                       nd, sk, tab);
  else
    hipLaunchKernelGGL(adamw_ema_kernel<false>, dim3(optim_grid(n4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n4, n, c, scale_dev,
                       nd, sk, tab);
  MAAVSS_LAUNCH_CHECK("adamw_ema_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_swap_f32(float* a, float* b, int64_t n, void* stream) {
  MAAVSS_CHECK_ARG(a && b && n > 0, "swap_f32: bad arguments");
  MAAVSS_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "swap_f32: buffers must be 16-byte aligned");
  const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b, hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
  MAAVSS_CHECK_ARG(hi - lo >= (uintptr_t)n * 4, "swap_f32: the buffers overlap");
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(swap_f32_kernel, dim3(optim_grid(n4)), dim3(256), 0, (hipStream_t)stream, a, b, n4, n);
  MAAVSS_LAUNCH_CHECK("swap_f32_kernel");
  return MAAVSS_OK;
}
