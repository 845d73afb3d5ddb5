// Reductions over a wave and over the waves of a workgroup, each in ONE fixed order: the library's contract is that the same
// input gives the same bits in every run, and the order is part of those bits.  Included by common.h.  The helpers only add and
// compare (no product), so a file's -ffp-contract setting cannot change what they compute.
//   wave_sum (f32), wave_sum_i, wave_max, wave_min    DPP on the VALU, result uniform across the wave
//   wave_sum_d                                         f64 butterfly over __shfl_xor, offsets 32, 16, ..., 1; every lane gets the sum
//   wave_strided_sum_d                                 lane l adds elements l, l + 64, ... in index order, then wave_sum_d
//   wave_max_d, wave_min_d                             the same butterfly with a comparison (t > v ? t : v): a NaN is never picked up
//   WG_SUM                                             the four per-wave results pairwise: (0 + 1) + (2 + 3)
//   WG_MAX, WG_MIN                                     the NW per-wave results in wave index order: ((0, 1), 2), 3 ...; f32 through
//                                                      fmaxf / fminf, f64 through the comparison of wave_max_d / wave_min_d
//   chunk_sum16                                        a weight gradient's per-chunk partials: 16 phases of chunks, then the phases
// The f32 sums that add their per-wave slots left to right (mse_partial_kernel, vit_cls_attn_kernel, the conv and batch-norm
// partials) are a third order; they stay written out where they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Wave-wide reductions on the VALU (DPP), result uniform across the wave.  The __shfl_xor form goes through the LDS
// crossbar: six dependent ds_bpermute round trips (~500 cycles per reduction, stamped in the LayerNorm prologue).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i32(int x, int old) {
  return __builtin_amdgcn_update_dpp(old, x, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float x, float old) {
  return __builtin_bit_cast(float, dpp_i32<CTRL, ROW_MASK>(__builtin_bit_cast(int, x), __builtin_bit_cast(int, old)));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f32<0xB1, 0xf>(v, 0.f);    // quad_perm [1,0,3,2]
  v += dpp_f32<0x4E, 0xf>(v, 0.f);    // quad_perm [2,3,0,1]
  v += dpp_f32<0x141, 0xf>(v, 0.f);   // row_half_mirror
  v += dpp_f32<0x140, 0xf>(v, 0.f);   // row_mirror: every lane of a 16-lane row holds the row sum
  v += dpp_f32<0x142, 0xa>(v, 0.f);   // row_bcast:15 into rows 1, 3
  v += dpp_f32<0x143, 0xc>(v, 0.f);   // row_bcast:31 into rows 2, 3: lane 63 holds the total
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ int wave_sum_i(int v) {      // integer addition is exact: any order gives these bits
  v += dpp_i32<0xB1, 0xf>(v, 0);
  v += dpp_i32<0x4E, 0xf>(v, 0);
  v += dpp_i32<0x141, 0xf>(v, 0);
  v += dpp_i32<0x140, 0xf>(v, 0);
  v += dpp_i32<0x142, 0xa>(v, 0);
  v += dpp_i32<0x143, 0xc>(v, 0);
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_f32<0xB1, 0xf>(v, v));
  v = fmaxf(v, dpp_f32<0x4E, 0xf>(v, v));
  v = fmaxf(v, dpp_f32<0x141, 0xf>(v, v));
  v = fmaxf(v, dpp_f32<0x140, 0xf>(v, v));
  v = fmaxf(v, dpp_f32<0x142, 0xa>(v, v));   // masked-off rows keep their own value (old = v)
  v = fmaxf(v, dpp_f32<0x143, 0xc>(v, v));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// negation is exact, so this is wave_max's exchange order and its choice between zeros of either sign
__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
// sum of p[0], p[stride], ..., p[(count - 1) * stride] by one wave: lane l adds elements l, l + 64, ..., then the butterfly
__device__ __forceinline__ double wave_strided_sum_d(const double* __restrict__ p, int64_t count, int64_t stride, int lane) {
  double s = 0.0;
  for (int64_t i = lane; i < count; i += 64) s += p[i * stride];
  return wave_sum_d(s);
}

// Workgroup reductions: NW waves, N values at a time through `__shared__ T red[NW][N]`, one barrier.  `v` holds the wave's own
// results on entry (uniform over the wave, i.e. after a wave_* call above); `wave` and `lane` are the thread's wave in the
// workgroup and its lane in the wave.  A kernel that reduces twice through one `red` needs a barrier of its own between the
// first read-back and the second write.
enum wg_op { WG_SUM, WG_MAX, WG_MIN };
enum wg_who { WG_THREAD0, WG_ALL };      // who gets the result: thread 0 (wave 0, lane 0; `v` is unchanged in the others), or every thread

// The pieces, for a kernel that reduces values of several types behind one barrier: wg_park each array, __syncthreads(), wg_col.
template <int NW, int N, typename T>
__device__ __forceinline__ void wg_park(T (&red)[NW][N], const T (&v)[N], int wave, int lane) {
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[wave][k] = v[k];
  }
}
// one step of WG_MAX / WG_MIN in the value's own type (fmaxf on a double would narrow it to f32)
template <wg_op OP>
__device__ __forceinline__ float wg_pick(float m, float t) { return OP == WG_MAX ? fmaxf(m, t) : fminf(m, t); }
template <wg_op OP>
__device__ __forceinline__ double wg_pick(double m, double t) { return OP == WG_MAX ? (t > m ? t : m) : (t < m ? t : m); }
template <wg_op OP, int NW, int N, typename T>
__device__ __forceinline__ T wg_col(const T (&red)[NW][N], int k) {
  if constexpr (OP == WG_SUM) {
    static_assert(NW == 4, "the pairwise order is written out for four waves");
    return (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  } else {
    T m = red[0][k];
#pragma unroll
    for (int q = 1; q < NW; ++q) m = wg_pick<OP>(m, red[q][k]);
    return m;
  }
}

template <wg_who WHO, wg_op OP, int NW, int N, typename T>
__device__ __forceinline__ void wg_reduce(T (&v)[N], T (&red)[NW][N], int wave, int lane) {
  wg_park(red, v, wave, lane);
  __syncthreads();
  if (WHO == WG_ALL || (wave == 0 && lane == 0)) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wg_col<OP>(red, k);
  }
}
template <wg_who WHO, wg_op OP, int NW, typename T>      // one value: `red` is [NW][1]
__device__ __forceinline__ T wg_reduce(T x, T (&red)[NW][1], int wave, int lane) {
  T v[1] = {x};
  wg_reduce<WHO, OP>(v, red, wave, lane);
  return v[0];
}

// Sum of a weight gradient's per-chunk partials, partials[chunk][total], by a 256-thread block: 16 outputs (i0 ... i0 + 15) x 16 chunk
// phases (one thread per output walking all chunks serially took 70-260 us per Conv3d layer).  Phase p adds chunks p, p + 16, ...
// in that order, then the thread of phase 0 (`owner`; it gets the sum of output `i`) adds the 16 phases in index order.
__device__ __forceinline__ float chunk_sum16(const float* __restrict__ partials, int64_t total, int nchunk, int i0, bool& owner, int& i) {
  __shared__ float red[16][17];
  const int o = threadIdx.x & 15, ph = threadIdx.x >> 4;
  i = i0 + o;
  float s = 0.f;
  if (i < total)
    for (int c = ph; c < nchunk; c += 16) s += partials[(int64_t)c * total + i];
  red[ph][o] = s;
  __syncthreads();
  owner = ph == 0 && i < total;
  float t = 0.f;
  if (owner)
#pragma unroll
    for (int p = 0; p < 16; ++p) t += red[p][o];
  return t;
}

static inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }      // workspace sections start on 256 bytes
