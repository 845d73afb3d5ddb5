// Per-head thresholded attention masks of the ViT attention extractor: DINO's segmentation read-out, reference
// video_attention.py:59-78 (sort the CLS attention of a head over the patches, normalise, cumulative sum, keep the patches whose
// cumulative share exceeds 1 - threshold, undo the permutation, nearest upsample by the patch size).
//
//   vit_attn_masks    att [rows][n] f32 (rows = frames x heads, what vit_cls_attn wrote) -> 0 / 1 masks, uint8 or f32, at patch
//                     resolution [rows][hp][wp] or upsampled [rows][H][W] (zero outside the patch grid).
//
// One workgroup per row, the row in LDS as 64-bit keys  value_bits << 32 | patch index : the values are non-negative, so their bit
// patterns order like unsigned integers and the index in the low half is torch.sort(stable=True)'s tie rule.  Bitonic network
// over the keys (padded to a power of two with all-ones keys, which sort behind every real one), block scan of value / sum over
// the sorted row, first position whose cumulative share exceeds the cut -- everything from there on is kept, so the kept set is
// an exact suffix of the sorted order whatever the rounding of the scan --, flags scattered to a patch-resolution byte image in
// LDS, then the output rows as 16-byte stores in memory order (the only large traffic: H x W bytes or floats per row).
// No atomics: the result does not depend on scheduling.  Data never steers control flow or an address except through the index
// half of a key, which is a permutation of 0 .. n-1 for ANY input bits -- non-finite rows terminate and stay in bounds.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_N = 4096;

// compare-exchange steps j = JMAX .. 1 of one bitonic merge on E = 2 * JMAX keys held in registers
template <int E>
__device__ __forceinline__ void bitonic_steps_reg(uint64_t (&r)[E], bool up) {
#pragma unroll
  for (int j = E / 2; j > 0; j >>= 1) {
#pragma unroll
    for (int i = 0; i < E; ++i) {
      if ((i & j) == 0) {
        const uint64_t a = r[i], b = r[i | j];
        const bool sw = (a > b) == up;
        r[i] = sw ? b : a;
        r[i | j] = sw ? a : b;
      }
    }
  }
}

// 16 bytes of output pixels x0 .. x0 + VEC - 1 of pixel row y from the patch-resolution byte image
template <bool OUT_F32>
__device__ __forceinline__ uint4 mask_pixels16(const unsigned char* flags, int y, int x0, int hp, int wp, int patch) {
  if (patch == 8) {
    const int py = y >> 3, px = x0 >> 3;
    const unsigned char* fr = flags + py * wp;
    if (OUT_F32) {
      // 4 consecutive pixels from a multiple of 4 never straddle an 8-pixel patch
      const unsigned v = (py < hp && px < wp && fr[px]) ? 0x3f800000u : 0u;
      return make_uint4(v, v, v, v);
    }
    // 16 pixels = two patches
    const unsigned lo = (py < hp && px < wp && fr[px]) ? 0x01010101u : 0u;
    const unsigned hi = (py < hp && px + 1 < wp && fr[px + 1]) ? 0x01010101u : 0u;
    return make_uint4(lo, lo, hi, hi);
  }
  const int py = y / patch;
  unsigned w[4] = {0u, 0u, 0u, 0u};
  if (py < hp) {
    const unsigned char* fr = flags + py * wp;
    if (OUT_F32) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int px = (x0 + k) / patch;
        w[k] = (px < wp && fr[px]) ? 0x3f800000u : 0u;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int px = (x0 + k) / patch;
        w[k >> 2] |= (px < wp && fr[px]) ? (1u << ((k & 3) * 8)) : 0u;
      }
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <bool OUT_F32>
__device__ __forceinline__ void store_elem(void* out, int64_t i, bool on) {
  if (OUT_F32) reinterpret_cast<float*>(out)[i] = on ? 1.f : 0.f;
  else reinterpret_cast<unsigned char*>(out)[i] = on ? 1 : 0;
}

// LDS position of key i: one 8-byte pad after every 8 keys, so that the lanes of the register passes (8 consecutive keys each,
// 72 bytes apart) fall on distinct banks
__device__ __forceinline__ int ki(int i) { return i + (i >> 3); }

// LDS (dynamic, 16-byte aligned carve): keys [P + P / 8] u64 | flags [round16(n)] u8 | scratch 16 x 4 B
template <bool OUT_F32>
__global__ __launch_bounds__(THREADS) void vit_attn_masks_kernel(const float* __restrict__ att, void* __restrict__ out, int n, int P,
                                                                 int hp, int wp, int H, int W, int patch, int upsample, int vec,
                                                                 float cut, int* __restrict__ nonfinite) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem);
  unsigned char* flags = smem + (size_t)P * 9;
  float* scr = reinterpret_cast<float*>(flags + ((n + 15) & ~15));
  int* scri = reinterpret_cast<int*>(scr);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const float* ap = att + row * n;

  // ---- load: keys, row sum, finite check
  float part = 0.f;
  bool bad = false;
  for (int i = tid; i < P; i += THREADS) {
    uint64_t key = ~0ull;
    if (i < n) {
      const float x = ap[i];
      bad |= !(fabsf(x) <= 3.0e38f);                        // false for inf and for NaN
      part += x;
      const unsigned bits = (x == 0.f) ? 0u : __float_as_uint(x);   // -0 orders as +0
      key = ((uint64_t)bits << 32) | (unsigned)i;
    }
    keys[ki(i)] = key;
  }
  part = wave_sum(part);
  const bool wave_bad = __ballot(bad) != 0;
  if (lane == 0) { scr[wave] = part; scri[12 + wave] = wave_bad; }
  __syncthreads();
  // sticky flag: every writer stores the same value, so a plain store does (no atomic)
  if (tid == 0 && nonfinite != nullptr && (scri[12] | scri[13] | scri[14] | scri[15])) *nonfinite = 1;
  const float total = (scr[0] + scr[1]) + (scr[2] + scr[3]);

  // ---- bitonic sort, ascending.  Merge steps with partner distance j >= 8 go through LDS one step per barrier; the last
  // steps (j = 4, 2, 1) of every merge run on 8 consecutive keys in registers, and so do the whole merges k = 2, 4, 8.
  for (int c = tid; c < P / 8; c += THREADS) {
    uint64_t r[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = keys[c * 9 + e];
#pragma unroll
    for (int i = 0; i < 8; i += 2) {                        // k = 2: pairs, direction alternates with bit 1 of the index
      const uint64_t a = r[i], b = r[i + 1];
      const bool sw = (a > b) == ((i & 2) == 0);
      r[i] = sw ? b : a;
      r[i + 1] = sw ? a : b;
    }
#pragma unroll
    for (int h = 0; h < 8; h += 4) {                        // k = 4: quads, direction alternates with bit 2
      uint64_t q[4] = {r[h], r[h + 1], r[h + 2], r[h + 3]};
      bitonic_steps_reg<4>(q, (h & 4) == 0);
      r[h] = q[0]; r[h + 1] = q[1]; r[h + 2] = q[2]; r[h + 3] = q[3];
    }
    bitonic_steps_reg<8>(r, ((c * 8) & 8) == 0);            // k = 8
#pragma unroll
    for (int e = 0; e < 8; ++e) keys[c * 9 + e] = r[e];
  }
  __syncthreads();
  for (int k = 16; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= 8; j >>= 1) {
      for (int t = tid; t < P / 2; t += THREADS) {
        const int i = 2 * t - (t & (j - 1));                // t with a zero inserted at bit log2(j)
        const int ia = ki(i), ib = ki(i + j);
        const uint64_t a = keys[ia], b = keys[ib];
        if ((a > b) == ((i & k) == 0)) { keys[ia] = b; keys[ib] = a; }
      }
      __syncthreads();
    }
    for (int c = tid; c < P / 8; c += THREADS) {
      uint64_t r[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = keys[c * 9 + e];
      bitonic_steps_reg<8>(r, ((c * 8) & k) == 0);
#pragma unroll
      for (int e = 0; e < 8; ++e) keys[c * 9 + e] = r[e];
    }
    __syncthreads();
  }

  // ---- block scan of value / total over the sorted row: thread t owns positions [t * chunk, (t + 1) * chunk)
  const int chunk = P >= THREADS ? P / THREADS : 1;
  const int base = tid * chunk;
  float run = 0.f;
  for (int e = 0; e < chunk; ++e) {
    const int pos = base + e;
    if (pos < n) run += __uint_as_float((unsigned)(keys[ki(pos)] >> 32)) / total;
  }
  float inc = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) scr[4 + wave] = inc;
  float c = __shfl_up(inc, 1, 64);
  if (lane == 0) c = 0.f;
  __syncthreads();
  float woff = 0.f;
  for (int w = 0; w < wave; ++w) woff += scr[4 + w];
  c += woff;
  // first sorted position whose inclusive cumulative share exceeds the cut (NaN > cut is false: a zero row keeps nothing)
  int first = n;
  for (int e = 0; e < chunk; ++e) {
    const int pos = base + e;
    if (pos < n) {
      c += __uint_as_float((unsigned)(keys[ki(pos)] >> 32)) / total;
      if (c > cut && first == n) first = pos;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  if (lane == 0) scri[8 + wave] = first;
  __syncthreads();
  first = min(min(scri[8], scri[9]), min(scri[10], scri[11]));

  // ---- keep rule written back at each patch's own position
  for (int e = 0; e < chunk; ++e) {
    const int pos = base + e;
    if (pos < n) flags[(unsigned)keys[ki(pos)]] = pos >= first ? 1 : 0;
  }
  __syncthreads();

  // ---- output
  constexpr int VEC = OUT_F32 ? 4 : 16;                     // elements per 16-byte store
  if (!upsample) {
    const int64_t o0 = row * n;
    if (vec) {
      uint4* op = reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(out) + o0 * (OUT_F32 ? 4 : 1));
      for (int g = tid; g < n / VEC; g += THREADS) {
        uint4 v;
        if (OUT_F32) {
          const uchar4 f = reinterpret_cast<const uchar4*>(flags)[g];
          v = make_uint4(f.x ? 0x3f800000u : 0u, f.y ? 0x3f800000u : 0u, f.z ? 0x3f800000u : 0u, f.w ? 0x3f800000u : 0u);
        } else {
          v = reinterpret_cast<const uint4*>(flags)[g];
        }
        op[g] = v;
      }
    } else {
      for (int i = tid; i < n; i += THREADS) store_elem<OUT_F32>(out, o0 + i, flags[i] != 0);
    }
    return;
  }
  const int64_t o0 = row * (int64_t)H * W;
  if (vec) {
    // 16-byte groups in memory order: consecutive lanes store consecutive 16 bytes; (y, g) advance without a division
    uint4* op = reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(out) + o0 * (OUT_F32 ? 4 : 1));
    const int G = W / VEC;
    int y = tid / G, g = tid - y * G;
    const int dy = THREADS / G, dg = THREADS - dy * G;
    while (y < H) {
      op[(int64_t)y * G + g] = mask_pixels16<OUT_F32>(flags, y, g * VEC, hp, wp, patch);
      y += dy;
      g += dg;
      if (g >= G) { g -= G; ++y; }
    }
  } else {
    for (int i = tid; i < H * W; i += THREADS) {
      const int y = i / W, x = i - y * W, py = y / patch, px = x / patch;
      store_elem<OUT_F32>(out, o0 + i, py < hp && px < wp && flags[py * wp + px] != 0);
    }
  }
}

}  // namespace

extern "C" int maavss_vit_attn_masks(const float* att, void* out, int out_dtype, int64_t n_frames, int heads, int H, int W, int patch,
                                     int upsample, float threshold, int32_t* nonfinite_flag, void* stream) {
  MAAVSS_CHECK_ARG(att != nullptr && out != nullptr, "vit_attn_masks: null pointer (att %p, out %p)", (const void*)att, out);
  MAAVSS_CHECK_ARG(out_dtype == 0 || out_dtype == 1, "vit_attn_masks: out_dtype must be 0 (uint8) or 1 (float32), got %d", out_dtype);
  MAAVSS_CHECK_ARG(n_frames >= 1, "vit_attn_masks: n_frames must be at least 1, got %lld", (long long)n_frames);
  MAAVSS_CHECK_ARG(heads >= 1, "vit_attn_masks: heads must be at least 1, got %d", heads);
  MAAVSS_CHECK_ARG(patch >= 1, "vit_attn_masks: patch must be at least 1, got %d", patch);
  MAAVSS_CHECK_ARG(H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20), "vit_attn_masks: bad frame size %d x %d", H, W);
  const int hp = H / patch, wp = W / patch;
  const int64_t n64 = (int64_t)hp * wp;
  MAAVSS_CHECK_ARG(n64 >= 1, "vit_attn_masks: the frame %d x %d holds no %d x %d patch (n < 1)", H, W, patch, patch);
  MAAVSS_CHECK_ARG(n64 <= MAX_N, "vit_attn_masks: n = %lld patches per frame, at most %d are built (512^2 at patch 8)", (long long)n64, MAX_N);
  MAAVSS_CHECK_ARG(threshold >= 0.f && threshold <= 1.f, "vit_attn_masks: threshold must lie in [0, 1], got %g", (double)threshold);
  MAAVSS_CHECK_ARG(n_frames * heads <= 0x7fffffff, "vit_attn_masks: too many rows (n_frames x heads)");
  MAAVSS_CHECK_ARG((int64_t)H * W <= 0x7fffffff, "vit_attn_masks: frame too large");
  const int n = (int)n64;
  int P = 16;                                               // a multiple of 16 keeps the LDS carve 16-byte aligned
  while (P < n) P <<= 1;
  const int velems = out_dtype == 1 ? 4 : 16;
  const int vec = ((uintptr_t)out % 16 == 0) && ((upsample ? W : n) % velems == 0);
  const float cut = (float)(1.0 - (double)threshold);
  const size_t lds = (size_t)P * 9 + ((n + 15) & ~15) + 64;
  const dim3 grid((unsigned)(n_frames * heads)), block(THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == 1)
    hipLaunchKernelGGL(vit_attn_masks_kernel<true>, grid, block, lds, st, att, out, n, P, hp, wp, H, W, patch, upsample ? 1 : 0, vec, cut,
                       (int*)nonfinite_flag);
  else
    hipLaunchKernelGGL(vit_attn_masks_kernel<false>, grid, block, lds, st, att, out, n, P, hp, wp, H, W, patch, upsample ? 1 : 0, vec, cut,
                       (int*)nonfinite_flag);
  MAAVSS_LAUNCH_CHECK("vit_attn_masks_kernel");
  return MAAVSS_OK;
}
