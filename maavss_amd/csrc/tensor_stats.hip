// EXTENSION (not in the reference): per-tensor statistics of a flat f32 buffer (FlatParams' gradients or parameters) in one
// segmented, deterministic reduction -- what gradient-norm clipping and the wandb.watch stand-in (maavss_amd.ModelWatch) read.
//   pass 1     one workgroup per chunk (<= TS_CH elements of one segment): f64 sum of the exact squares, min, max of the finite
//              elements, counts of NaN / +inf / -inf -> one 32-byte partial per chunk in the workspace
//   finalize   one workgroup of 16 waves: a wave per segment adds the segment's partials (lane l takes chunks l, l + 64, ... in table order, then a
//              fixed butterfly), writes the per-segment outputs, zeroes the segment's histogram row; then wave 0 adds the selected
//              segments the same way and writes total_sumsq, norm, scale
//   pass 2     (histogram) one workgroup per chunk: torch.histc's f32 bin formula between the segment's min and max, counts in LDS,
//              one global integer atomic per non-empty bin
// No floating-point atomic anywhere: every output has the same bits in every run.  HBM-bound: 4 bytes read per element per pass,
// one f64 FMA per element in pass 1.
#include "common.h"
#include "metric_f64.h"

#define TS_CH 16384          // chunk length in elements (64 KB: 64 elements per thread of a 256-thread workgroup)
#define TS_MAX_BINS 1024

struct ts_partial {
  double sumsq;
  float mn, mx;
  int n_nan, n_pinf, n_ninf, pad;
};
static_assert(sizeof(ts_partial) == 32, "workspace layout of include/maavss.h");

// Per-lane running statistics: four independent f64 chains for the sum (the FMA's latency), one chain for the rest.
struct ts_acc {
  double s[4];
  float mn, mx;
  int n_nan, n_pinf, n_ninf;
  template <int K>
  __device__ __forceinline__ void add(float x) {      // branch-free: a non-finite element is a select, not a divergent path
    const unsigned u = __float_as_uint(x);
    const bool fin = (u & 0x7f800000u) != 0x7f800000u;
    const double d = (double)(fin ? x : 0.f);
    s[K] = fma(d, d, s[K]);                   // d * d is exact in f64 (24 x 24 bits): one rounding, that of the sum
    mn = fminf(mn, fin ? x : INFINITY);
    mx = fmaxf(mx, fin ? x : -INFINITY);
    n_nan += (u & 0x7fffffffu) > 0x7f800000u;
    n_pinf += u == 0x7f800000u;
    n_ninf += u == 0xff800000u;
  }
  __device__ __forceinline__ void add4(const float4 v) {
    add<0>(v.x);
    add<1>(v.y);
    add<2>(v.z);
    add<3>(v.w);
  }
};

// chunk table row c: chunks[3 * c + 0] = segment, + 1 = first element in buf, + 2 = length.  A row that does not lie inside [0, n)
// or is longer than TS_CH is read as empty (the table lives on the device: the host cannot check it before the launch).
__device__ __forceinline__ bool ts_chunk(const int64_t* __restrict__ chunks, int64_t c, int64_t n, int64_t n_segments, int64_t& seg,
                                         int64_t& start, int& len) {
  seg = chunks[3 * c];
  start = chunks[3 * c + 1];
  const int64_t l = chunks[3 * c + 2];
  const bool ok = seg >= 0 && seg < n_segments && start >= 0 && l >= 0 && l <= TS_CH && start <= n - l;
  len = ok ? (int)l : 0;
  return ok;
}

__global__ __launch_bounds__(256, 8) void tensor_stats_pass1_kernel(const float* __restrict__ buf, int64_t n, const int64_t* __restrict__ chunks,
                                                                 int64_t n_segments, ts_partial* __restrict__ partials) {
  __shared__ double red_s[4][1];
  __shared__ float red_f[4][2];
  __shared__ int red_c[4][3];
  int64_t seg, start;
  int len;
  ts_chunk(chunks, blockIdx.x, n, n_segments, seg, start, len);
  const float* __restrict__ x = buf + start;
  const int tid = threadIdx.x;
  ts_acc a = {{0.0, 0.0, 0.0, 0.0}, INFINITY, -INFINITY, 0, 0, 0};
  if ((start & 3) == 0) {      // 16-byte aligned chunk (buf is, the entry point checks): float4 loads
    const int len4 = len >> 2;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
    int i = tid;
    for (; i + 768 < len4; i += 1024) {      // four 16-byte loads in flight per lane before the first use (a full chunk: four rounds)
      const float4 v0 = x4[i], v1 = x4[i + 256], v2 = x4[i + 512], v3 = x4[i + 768];
      a.add4(v0);
      a.add4(v1);
      a.add4(v2);
      a.add4(v3);
    }
    for (; i < len4; i += 256) a.add4(x4[i]);
    const int t = (len4 << 2) + tid;
    if (t < len) a.add<0>(x[t]);
  } else {
    for (int i = tid; i < len; i += 256) a.add<0>(x[i]);
  }
  const double s[1] = {wave_sum_d((a.s[0] + a.s[1]) + (a.s[2] + a.s[3]))};
  const float f[2] = {wave_min(a.mn), wave_max(a.mx)};
  const int k[3] = {wave_sum_i(a.n_nan), wave_sum_i(a.n_pinf), wave_sum_i(a.n_ninf)};
  const int w = tid >> 6, lane = tid & 63;
  wg_park(red_s, s, w, lane);      // three types behind one barrier
  wg_park(red_f, f, w, lane);
  wg_park(red_c, k, w, lane);
  __syncthreads();
  if (tid == 0)
    partials[blockIdx.x] = {wg_col<WG_SUM>(red_s, 0), wg_col<WG_MIN>(red_f, 0), wg_col<WG_MAX>(red_f, 1), wg_col<WG_SUM>(red_c, 0),
                            wg_col<WG_SUM>(red_c, 1), wg_col<WG_SUM>(red_c, 2), 0};
}

// One workgroup of 1024 threads (16 waves).  seg_first[s] .. seg_first[s + 1] = the chunk rows of segment s (table order = buffer order).
// sel [n_segments] (workspace) = the sumsq of the selected segments, 0 for the others.
__global__ __launch_bounds__(1024) void tensor_stats_finalize_kernel(const ts_partial* __restrict__ partials, int64_t n_chunks,
                                                                    const int* __restrict__ seg_first, int64_t n_segments,
                                                                    const int* __restrict__ seg_mask, double* __restrict__ sel,
                                                                    double* __restrict__ sumsq, float* __restrict__ seg_min,
                                                                    float* __restrict__ seg_max, int* __restrict__ nonfinite,
                                                                    int* __restrict__ hist, int bins, int clip, double max_norm,
                                                                    double grad_scale, double* __restrict__ total_sumsq,
                                                                    float* __restrict__ norm, float* __restrict__ scale) {
  __shared__ int any_nan, any_inf;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) {
    any_nan = 0;
    any_inf = 0;
  }
  __syncthreads();
  for (int64_t sg = w; sg < n_segments; sg += 16) {
    int64_t c0 = seg_first[sg], c1 = seg_first[sg + 1];
    c0 = c0 < 0 ? 0 : c0;
    c1 = c1 > n_chunks ? n_chunks : c1;
    double s = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    int k0 = 0, k1 = 0, k2 = 0;
#pragma unroll 4
    for (int64_t c = c0 + lane; c < c1; c += 64) {      // independent loads, added in table order
      const ts_partial p = partials[c];
      s += p.sumsq;
      mn = fminf(mn, p.mn);
      mx = fmaxf(mx, p.mx);
      k0 += p.n_nan;
      k1 += p.n_pinf;
      k2 += p.n_ninf;
    }
    s = wave_sum_d(s);
    mn = wave_min(mn);
    mx = wave_max(mx);
    k0 = wave_sum_i(k0);
    k1 = wave_sum_i(k1);
    k2 = wave_sum_i(k2);
    if (lane == 0) {
      const bool none = mn > mx;        // no finite element: min = max = NaN
      sumsq[sg] = s;
      seg_min[sg] = none ? __uint_as_float(0x7fc00000u) : mn;
      seg_max[sg] = none ? __uint_as_float(0x7fc00000u) : mx;
      nonfinite[3 * sg] = k0;
      nonfinite[3 * sg + 1] = k1;
      nonfinite[3 * sg + 2] = k2;
      const bool on = seg_mask == nullptr || seg_mask[sg] != 0;
      sel[sg] = on ? s : 0.0;
      if (on && k0 > 0) atomicOr(&any_nan, 1);
      if (on && (k1 > 0 || k2 > 0)) atomicOr(&any_inf, 1);
    }
    if (hist != nullptr)
      for (int b = lane; b < bins; b += 64) hist[sg * bins + b] = 0;
  }
  if (!clip) return;
  __syncthreads();            // sel[] was written by this workgroup: visible to wave 0 after the barrier
  if (w != 0) return;
  const double t = wave_strided_sum_d(sel, n_segments, 1, lane);
  if (lane == 0) {
    *total_sumsq = t;
    // what IEEE arithmetic gives when the non-finite elements take part in the sum of squares: NaN with a NaN, otherwise +inf
    const double tt = any_nan ? (double)__uint_as_float(0x7fc00000u) : (any_inf ? (double)INFINITY : t);
    const double norm64 = sqrt(tt) * grad_scale;
    double c = max_norm / (norm64 + 1e-6);
    c = c > 1.0 ? 1.0 : c;             // torch.clamp(max = 1): a NaN stays a NaN (fmin would drop it)
    *norm = (float)norm64;
    *scale = (float)(grad_scale * c);
  }
}

// torch.histc's bin of x, in f32 with one rounding per operation (no contraction, IEEE division)
#pragma clang fp contract(off)
__device__ __forceinline__ int ts_bin(float x, float lo, float width, float fbins, int bins) {
  const float d = x - lo;
  const float e = d * fbins;
  const float q = __fdiv_rn(e, width);
  int b = (int)q;
  b = b >= bins ? bins - 1 : b;
  return b < 0 ? 0 : b;
}

__global__ __launch_bounds__(256) void tensor_stats_hist_kernel(const float* __restrict__ buf, int64_t n, const int64_t* __restrict__ chunks,
                                                                int64_t n_segments, const float* __restrict__ seg_min,
                                                                const float* __restrict__ seg_max, int* __restrict__ hist, int bins) {
  __shared__ int h[TS_MAX_BINS];
  int64_t seg, start;
  int len;
  if (!ts_chunk(chunks, blockIdx.x, n, n_segments, seg, start, len)) return;
  float lo = seg_min[seg], hi = seg_max[seg];
  if (!(lo <= hi)) return;          // no finite element in the segment: counts stay zero
  if (lo == hi) {
    lo -= 1.f;
    hi += 1.f;
  }
  const float width = hi - lo, fbins = (float)bins;
  const int tid = threadIdx.x;
  for (int b = tid; b < bins; b += 256) h[b] = 0;
  __syncthreads();
  const float* __restrict__ x = buf + start;
  if ((start & 3) == 0) {
    const int len4 = len >> 2;
    for (int i = tid; i < len4; i += 256) {
      const float4 v = reinterpret_cast<const float4*>(x)[i];
      if (!f32_nonfinite(v.x)) atomicAdd(&h[ts_bin(v.x, lo, width, fbins, bins)], 1);
      if (!f32_nonfinite(v.y)) atomicAdd(&h[ts_bin(v.y, lo, width, fbins, bins)], 1);
      if (!f32_nonfinite(v.z)) atomicAdd(&h[ts_bin(v.z, lo, width, fbins, bins)], 1);
      if (!f32_nonfinite(v.w)) atomicAdd(&h[ts_bin(v.w, lo, width, fbins, bins)], 1);
    }
    const int i = (len4 << 2) + tid;
    if (i < len && !f32_nonfinite(x[i])) atomicAdd(&h[ts_bin(x[i], lo, width, fbins, bins)], 1);
  } else {
    for (int i = tid; i < len; i += 256)
      if (!f32_nonfinite(x[i])) atomicAdd(&h[ts_bin(x[i], lo, width, fbins, bins)], 1);
  }
  __syncthreads();
  for (int b = tid; b < bins; b += 256)
    if (h[b] != 0) atomicAdd(&hist[seg * bins + b], h[b]);
}

extern "C" int maavss_tensor_stats_chunk(void) { return TS_CH; }

extern "C" int64_t maavss_tensor_stats_ws_bytes(int64_t n_chunks, int64_t n_segments, int bins) {
  if (n_chunks < 0 || n_segments <= 0 || bins < 1 || bins > TS_MAX_BINS) return 0;
  return align256(n_chunks * (int64_t)sizeof(ts_partial)) + align256(n_segments * 8);
}

extern "C" int maavss_tensor_stats(const float* buf, int64_t n, const int64_t* chunks, int64_t n_chunks, const int* seg_first,
                                   const int64_t* host_seg_offset, const int64_t* host_seg_numel, int64_t n_segments,
                                   const int* seg_mask, double* sumsq, float* seg_min, float* seg_max, int* nonfinite, int* hist,
                                   int bins, double max_norm, float grad_scale, double* total_sumsq, float* norm, float* scale,
                                   void* ws, int64_t ws_bytes, void* stream) {
  MAAVSS_CHECK_ARG(buf && chunks && seg_first && host_seg_offset && host_seg_numel && sumsq && seg_min && seg_max && nonfinite && ws,
                   "tensor_stats: null pointer");
  MAAVSS_CHECK_ARG(n > 0 && n_segments > 0 && n_segments < (1 << 24) && n_chunks >= 0 && n_chunks < (int64_t)1 << 31,
                   "tensor_stats: bad sizes (n %lld, %lld segments, %lld chunks)", (long long)n, (long long)n_segments, (long long)n_chunks);
  MAAVSS_CHECK_ARG(bins >= 1 && bins <= TS_MAX_BINS, "tensor_stats: bins must be in 1..%d (got %d)", TS_MAX_BINS, bins);
  MAAVSS_CHECK_ARG(((uintptr_t)buf & 15) == 0, "tensor_stats: the buffer must be 16-byte aligned");
  MAAVSS_CHECK_ARG((((uintptr_t)chunks | (uintptr_t)sumsq | (uintptr_t)ws | (uintptr_t)total_sumsq) & 7) == 0,
                   "tensor_stats: chunk table, f64 outputs and workspace must be 8-byte aligned");
  const int clip = max_norm >= 0.0;
  MAAVSS_CHECK_ARG(!clip || (total_sumsq && norm && scale), "tensor_stats: a clip needs the total_sumsq, norm and scale outputs (null pointer)");
  int64_t want_chunks = 0;
  for (int64_t s = 0; s < n_segments; ++s) {
    const int64_t o = host_seg_offset[s], k = host_seg_numel[s];
    MAAVSS_CHECK_ARG(k >= 0 && k < (int64_t)1 << 31, "tensor_stats: segment %lld has %lld elements; counts are int32, 2^31 or more are refused",
                     (long long)s, (long long)k);
    MAAVSS_CHECK_ARG(o >= 0 && o <= n - k, "tensor_stats: segment %lld [%lld, +%lld) leaves the buffer of %lld elements", (long long)s,
                     (long long)o, (long long)k, (long long)n);
    want_chunks += (k + TS_CH - 1) / TS_CH;
  }
  MAAVSS_CHECK_ARG(want_chunks == n_chunks, "tensor_stats: %lld chunks given, the segments cut at %d elements make %lld", (long long)n_chunks,
                   TS_CH, (long long)want_chunks);
  MAAVSS_CHECK_ARG(ws_bytes >= maavss_tensor_stats_ws_bytes(n_chunks, n_segments, bins), "tensor_stats: workspace of %lld bytes, %lld needed",
                   (long long)ws_bytes, (long long)maavss_tensor_stats_ws_bytes(n_chunks, n_segments, bins));
  hipStream_t st = (hipStream_t)stream;
  ts_partial* partials = (ts_partial*)ws;
  double* sel = (double*)((char*)ws + align256(n_chunks * (int64_t)sizeof(ts_partial)));
  if (n_chunks > 0) {
    hipLaunchKernelGGL(tensor_stats_pass1_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, buf, n, chunks, n_segments, partials);
    MAAVSS_LAUNCH_CHECK("tensor_stats_pass1_kernel");
  }
  hipLaunchKernelGGL(tensor_stats_finalize_kernel, dim3(1), dim3(1024), 0, st, partials, n_chunks, seg_first, n_segments, seg_mask, sel, sumsq,
                     seg_min, seg_max, nonfinite, hist, bins, clip, max_norm, (double)grad_scale, total_sumsq, norm, scale);
  MAAVSS_LAUNCH_CHECK("tensor_stats_finalize_kernel");
  if (hist != nullptr && n_chunks > 0) {
    hipLaunchKernelGGL(tensor_stats_hist_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, buf, n, chunks, n_segments, seg_min, seg_max, hist,
                       bins);
    MAAVSS_LAUNCH_CHECK("tensor_stats_hist_kernel");
  }
  return MAAVSS_OK;
}
