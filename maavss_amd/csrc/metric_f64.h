// What the f64 "measure and report" kernels share (quality_metrics, spectral_loss, stoi, bss_eval, figures, clip_select, tensor_stats):
// the non-finite constants and bit test, the index and the rotate-add of one radix-2 butterfly in LDS, the row sum of per-frame
// partials and the argument checks of an est / ref / out / workspace entry.
// fft2_rotate_add forms products and adds them, so unlike reduce.h this header is NOT indifferent to a file's -ffp-contract setting:
// the device helpers are header-inline and compile under the including file's own flag (the Makefile gives every f64 metric file
// -ffp-contract=off); none of them may move into a translation unit of its own.  rows_sum_kernel may live in one (it adds, and
// divides once: nothing to contract), and the library has no relocatable device code, so it is launched from there.
#pragma once
#include "common.h"

__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }      // the quiet NaN
__device__ __forceinline__ double inf_d() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ bool f32_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }      // NaN or +-inf

// Butterfly b of stage s (half = 2^s) of a decimation-in-time radix-2 transform over bit-reversed input: it joins elements i0 and
// i1 = i0 + half with twiddle exp(-2 pi i j / 2^(s + 1)).  The loops, the twiddle table and its stride stay with each kernel.
__device__ __forceinline__ void fft2_index(int b, int s, int& i0, int& i1, int& j) {
  const int half = 1 << s;
  j = b & (half - 1);
  i0 = ((b >> s) << (s + 1)) + j;
  i1 = i0 + half;
}
// z[i0], z[i1] = z[i0] +- (c - i sn) z[i1]
__device__ __forceinline__ void fft2_rotate_add(double* zr, double* zi, int i0, int i1, double c, double sn) {
  const double ur = zr[i0], ui = zi[i0], vr = zr[i1], vi = zi[i1];
  const double pr = c * vr + sn * vi, pi = c * vi - sn * vr;      // (c - i sn) (vr + i vi)
  zr[i0] = ur + pr;
  zi[i0] = ui + pi;
  zr[i1] = ur - pr;
  zi[i1] = ui - pi;
}

// quality_metrics.hip: launches rows_sum_kernel, one wave per row: out[row][k] = the sum over the row's `per_row` partials of column
// k < K in index order (wave_strided_sum_d), column 1 divided by div1 (1.0 leaves the sum's bits).  -> a status
int rows_sum_launch(const double* partials, int64_t rows, int64_t per_row, int K, double div1, double* out, hipStream_t st);

// quality_metrics.hip: the two chunk passes of the wave metrics, for wave_loss.hip.  A row of L samples is cut into
// wave_chunks_per_row(L, seg_len) chunks, one workgroup each.  wave_sums_launch: per chunk WAVE_PARTIAL_DOUBLES doubles
// {sum ref^2, sum est^2, sum ref est, sum (est - ref)^2, segmental sum, frames}; wave_scaled_sqerr_launch: per chunk
// sum (est - alpha[row] ref)^2.  A row's partials are added in index order (wave_strided_sum_d).  -> a status
#define WAVE_PARTIAL_DOUBLES 6
int64_t wave_chunks_per_row(int64_t L, int seg_len);
int wave_sums_launch(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, int64_t B, int64_t L, int seg_len,
                     void* partials, hipStream_t st);
int wave_scaled_sqerr_launch(const float* est, int64_t est_stride, const float* ref, int64_t ref_stride, int64_t B, int64_t L, int seg_len,
                             const double* alpha, double* partials, hipStream_t st);

// the checks an entry makes of est [rows][n], ref [rows][n] (f32, row strides in elements), out and its workspace (f64); `who`
// names the entry in the message.  The stride of a single row is not looked at: the entry passes 0 to its kernels then.
static inline int metric_rows_check(const char* who, const void* est, int64_t est_stride, const void* ref, int64_t ref_stride, int64_t rows,
                                    const void* out, const void* ws) {
  MAAVSS_CHECK_ARG(est && ref && out && ws, "%s: null pointer", who);
  MAAVSS_CHECK_ARG(rows == 1 || (est_stride >= 0 && ref_stride >= 0 && est_stride < (int64_t)1 << 40 && ref_stride < (int64_t)1 << 40),
                   "%s: row strides %lld, %lld: rows would not be addressable (strides are >= 0; rows may overlap)", who, (long long)est_stride,
                   (long long)ref_stride);
  MAAVSS_CHECK_ARG((((uintptr_t)est | (uintptr_t)ref) & 3) == 0, "%s: est and ref must be 4-byte aligned", who);
  MAAVSS_CHECK_ARG((((uintptr_t)out | (uintptr_t)ws) & 7) == 0, "%s: out and workspace must be 8-byte aligned", who);
  return MAAVSS_OK;
}
