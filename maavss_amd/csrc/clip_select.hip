// Per-clip activity statistics of the clip bank (maavss_amd.ClipBank.activity, maavss_amd.ClipSampler): which of a bank's clips are
// silent, still or cut, decided from one read of the bank on the device.  include/maavss.h holds the definitions and the order of
// every sum; tests/select_twin.py restates them.  All sums are f64 over exactly converted f32 data, in ONE fixed order, without
// atomics; no workgroup waits on another; every index taken from a device table is clamped, and the entry points check the host
// copies of the tables before any launch.  Compiled with -ffp-contract=off (Makefile): the squares are exact in f64 either way, the
// differences and quotients are rounded one by one.
//   cs_level_partial   per (recording, chunk of 16384 samples): thread t adds the squares of the chunk's finite samples t, t + 256,
//                      ... in index order, wave_sum_d, then (w0 + w1) + (w2 + w3).  Reads 4 B a banked sample, writes 8 B a chunk.
//   cs_level_final     one thread per recording adds its chunk partials in index order.  Reads 8 B a chunk.
//   cs_pair            one wave per pair of consecutive bank frames: lane l adds |m[f+1][e] - m[f][e]| (f64) for e = l, l + 64, ...,
//                      wave_sum_d, / P.  Reads every map value twice (once from L2), {4, 2} B each; writes 8 B a pair.
//   cs_clip            one workgroup per clip, wave w takes segments w, w + 4, ...: lane l adds the squares of the segment's samples
//                      l, l + 64, ..., wave_sum_d -> E_j in LDS; thread 0 adds the E_j and the clip's D_f in index order.  Dword loads
//                      (clip starts are arbitrary), 64-bit offsets.  Reads 4 B a clip sample (overlapping clips re-read, from L2
//                      where neighbouring workgroups run together) and 8 B a pair; writes 52 B a clip.
//   cs_select          one thread per clip: the table against the thresholds -> one reason byte.  Reads 44 B, writes 1 B a clip.
#include "common.h"
#include "metric_f64.h"
#include "bank_load.h"      // bank_load (both storages), bank_clamp

namespace {

constexpr int CS_MAX_J = 2048;          // segments of a clip the clip kernel keeps in LDS (16 KiB of f64)
constexpr int CS_CHUNK = 16384;         // samples per partial of the recording level
constexpr int64_t CS_MAX_CHUNKS = 65535;      // chunks of one recording: the grid's y extent

// rec_tab int64 [3][n_rec]: first sample, samples, first partial slot
__global__ __launch_bounds__(256) void cs_level_partial_kernel(const float* __restrict__ audio, int64_t n_samples,
                                                               const int64_t* __restrict__ rec_tab, int64_t n_rec, int64_t n_partials,
                                                               double* __restrict__ partials) {
  __shared__ double red[4][1];
  const int64_t r = blockIdx.x;
  const int64_t len = bank_clamp(rec_tab[n_rec + r], n_samples);
  const int64_t begin = (int64_t)blockIdx.y * CS_CHUNK;
  if (begin >= len) return;                                   // uniform over the workgroup
  const int64_t start = bank_clamp(rec_tab[r], n_samples - len);
  const int64_t slot = bank_clamp(rec_tab[2 * n_rec + r] + blockIdx.y, n_partials - 1);
  const int64_t count = len - begin < CS_CHUNK ? len - begin : CS_CHUNK;
  const float* __restrict__ p = audio + start + begin;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) {
    const float x = p[i];
    const double xd = f32_nonfinite(x) ? 0.0 : (double)x;
    s += xd * xd;
  }
  s = wg_reduce<WG_THREAD0, WG_SUM>(wave_sum_d(s), red, threadIdx.x >> 6, threadIdx.x & 63);
  if (threadIdx.x == 0) partials[slot] = s;
}

__global__ __launch_bounds__(64) void cs_level_final_kernel(const double* __restrict__ partials, const int64_t* __restrict__ rec_tab,
                                                            int64_t n_rec, int64_t n_samples, int64_t n_partials,
                                                            double* __restrict__ level) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= n_rec) return;
  const int64_t len = bank_clamp(rec_tab[n_rec + r], n_samples);
  const int64_t chunks = (len + CS_CHUNK - 1) / CS_CHUNK;
  const int64_t first = rec_tab[2 * n_rec + r];
  double s = 0.0;
  for (int64_t c = 0; c < chunks; ++c) s += partials[bank_clamp(first + c, n_partials - 1)];
  level[r] = s;
}

template <typename T>
__global__ __launch_bounds__(256) void cs_pair_kernel(const T* __restrict__ maps, int64_t n_pairs, int P, double* __restrict__ D) {
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= n_pairs) return;                                   // uniform over the wave
  const T* __restrict__ a = maps + f * P;
  double s = 0.0;
  for (int e = lane; e < P; e += 64) {
    const double d = (double)bank_load(a, (int64_t)P + e) - (double)bank_load(a, e);
    s += fabs(d);
  }
  s = wave_sum_d(s);
  if (lane == 0) D[f] = s / (double)P;
}

struct cs_clip_out {
  double *energy, *rms_db, *rel_db, *motion_mean, *motion_peak;
  float* peak;
  int32_t *n_bad, *n_active;
};

__global__ __launch_bounds__(256) void cs_clip_kernel(const float* __restrict__ audio, int64_t n_samples, const double* __restrict__ D,
                                                      int64_t n_frames, const double* __restrict__ level,
                                                      const int64_t* __restrict__ rec_tab, int64_t n_rec,
                                                      const int64_t* __restrict__ clip_sample, const int32_t* __restrict__ clip_frame,
                                                      const int32_t* __restrict__ clip_rec, int T, int J, int hop, double floor_factor,
                                                      cs_clip_out out) {
  __shared__ double E[CS_MAX_J];
  __shared__ float red_f[4][1];
  __shared__ int red_i[4][2];
  const int64_t b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t n = (int64_t)J * hop;
  const int64_t s0 = bank_clamp(clip_sample[b], n_samples - n);
  const int64_t r = bank_clamp(clip_rec[b], n_rec - 1);
  int64_t rec_n = bank_clamp(rec_tab[n_rec + r], n_samples);
  rec_n = rec_n < 1 ? 1 : rec_n;
  const double rec_power = level[r] / (double)rec_n;          // the recording's mean power
  const double floor_p = rec_power * floor_factor;
  float pk = 0.f;
  int cnt[2] = {0, 0};                                        // non-finite samples (per lane), active segments (per wave)
  for (int j = wave; j < J; j += 4) {
    const float* __restrict__ p = audio + s0 + (int64_t)j * hop;
    double e = 0.0;
    for (int i = lane; i < hop; i += 64) {
      const float x = p[i];
      const double xd = (double)x;
      e += xd * xd;
      pk = fmaxf(pk, fabsf(x));                               // fmaxf drops a NaN: the peak is over the samples that are numbers
      cnt[0] += f32_nonfinite(x) ? 1 : 0;
    }
    e = wave_sum_d(e);
    if (lane == 0) E[j] = e;
    cnt[1] += (e / (double)hop >= floor_p) ? 1 : 0;
  }
  cnt[0] = wave_sum_i(cnt[0]);
  pk = wg_reduce<WG_THREAD0, WG_MAX>(wave_max(pk), red_f, wave, lane);       // its barrier also publishes E
  wg_park(red_i, cnt, wave, lane);
  __syncthreads();
  if (threadIdx.x != 0) return;
  double energy = 0.0;
  for (int j = 0; j < J; ++j) energy += E[j];
  const double mean = energy / (double)n;
  out.energy[b] = energy;
  out.rms_db[b] = 10.0 * log10(mean);
  out.rel_db[b] = 10.0 * log10(mean / rec_power);
  out.peak[b] = pk;
  out.n_bad[b] = wg_col<WG_SUM>(red_i, 0);
  out.n_active[b] = wg_col<WG_SUM>(red_i, 1);
  double msum = 0.0, mmax = 0.0;
  if (T > 1) {
    const int64_t v = bank_clamp(clip_frame[b], n_frames - T);
    for (int t = 0; t < T - 1; ++t) {
      const double d = D[v + t];
      msum += d;
      mmax = d > mmax ? d : mmax;
    }
    msum = msum / (double)(T - 1);
  }
  out.motion_mean[b] = msum;
  out.motion_peak[b] = mmax;
}

struct cs_thresholds {
  double min_rms_db, min_rel_db, min_active, min_motion, max_motion_peak;      // min_active = min_active_fraction * J, formed on the host
  float max_peak;
  int enabled;                                                                 // bit k: reason k is tested
};

__global__ __launch_bounds__(256) void cs_select_kernel(const double* __restrict__ rms_db, const double* __restrict__ rel_db,
                                                        const int32_t* __restrict__ n_active, const double* __restrict__ motion_mean,
                                                        const double* __restrict__ motion_peak, const float* __restrict__ peak,
                                                        const int32_t* __restrict__ n_bad, int64_t n_clips, cs_thresholds th,
                                                        uint8_t* __restrict__ reasons) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= n_clips) return;
  int m = 0;
  m |= rms_db[b] < th.min_rms_db ? 1 : 0;
  m |= rel_db[b] < th.min_rel_db ? 2 : 0;
  m |= (double)n_active[b] < th.min_active ? 4 : 0;
  m |= motion_mean[b] < th.min_motion ? 8 : 0;
  m |= motion_peak[b] > th.max_motion_peak ? 16 : 0;
  m |= peak[b] >= th.max_peak ? 32 : 0;
  m |= n_bad[b] > 0 ? 64 : 0;
  reasons[b] = (uint8_t)(m & th.enabled);
}

inline bool cs_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int64_t maavss_bank_level_chunks(int64_t samples) { return samples < 0 ? -1 : (samples + CS_CHUNK - 1) / CS_CHUNK; }

extern "C" int maavss_bank_max_segments(void) { return CS_MAX_J; }

extern "C" int maavss_bank_recording_level(const float* audio, int64_t n_samples, const int64_t* rec_tab, const int64_t* host_rec_tab,
                                           int64_t n_rec, double* partials, int64_t n_partials, double* level, void* stream) {
  MAAVSS_CHECK_ARG(audio && rec_tab && host_rec_tab && partials && level, "bank_recording_level: null pointer");
  MAAVSS_CHECK_ARG(n_samples > 0 && n_rec > 0 && n_partials > 0, "bank_recording_level: n_samples = %lld, n_rec = %lld, n_partials = %lld must be positive",
                   (long long)n_samples, (long long)n_rec, (long long)n_partials);
  MAAVSS_CHECK_ARG(n_rec <= 0x7fffffff, "bank_recording_level: %lld recordings exceed the grid", (long long)n_rec);
  MAAVSS_CHECK_ARG(cs_aligned(rec_tab, 8) && cs_aligned(partials, 8) && cs_aligned(level, 8) && cs_aligned(audio, 4),
                   "bank_recording_level: rec_tab, partials and level must be 8-byte aligned, audio 4-byte");
  int64_t slot = 0, max_chunks = 0;
  for (int64_t r = 0; r < n_rec; ++r) {
    const int64_t start = host_rec_tab[r], len = host_rec_tab[n_rec + r], first = host_rec_tab[2 * n_rec + r];
    MAAVSS_CHECK_ARG(len > 0 && start >= 0 && start <= n_samples - len,
                     "bank_recording_level: recording %lld (samples [%lld, %lld + %lld)) lies outside the bank's %lld samples", (long long)r,
                     (long long)start, (long long)start, (long long)len, (long long)n_samples);
    const int64_t chunks = (len + CS_CHUNK - 1) / CS_CHUNK;
    MAAVSS_CHECK_ARG(chunks <= CS_MAX_CHUNKS, "bank_recording_level: recording %lld has %lld samples, more than %lld chunks of %d", (long long)r,
                     (long long)len, (long long)CS_MAX_CHUNKS, CS_CHUNK);
    MAAVSS_CHECK_ARG(first == slot, "bank_recording_level: recording %lld's first partial is %lld, expected %lld (the running chunk count)",
                     (long long)r, (long long)first, (long long)slot);
    slot += chunks;
    max_chunks = chunks > max_chunks ? chunks : max_chunks;
  }
  MAAVSS_CHECK_ARG(slot <= n_partials, "bank_recording_level: %lld chunk partials needed, room for %lld", (long long)slot, (long long)n_partials);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cs_level_partial_kernel, dim3((unsigned)n_rec, (unsigned)max_chunks), dim3(256), 0, st, audio, n_samples, rec_tab, n_rec,
                     n_partials, partials);
  MAAVSS_LAUNCH_CHECK("cs_level_partial_kernel");
  hipLaunchKernelGGL(cs_level_final_kernel, dim3((unsigned)((n_rec + 63) / 64)), dim3(64), 0, st, partials, rec_tab, n_rec, n_samples, n_partials,
                     level);
  MAAVSS_LAUNCH_CHECK("cs_level_final_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_bank_frame_motion(const void* maps, int storage, int64_t n_frames, int64_t frame_elems, double* D, void* stream) {
  MAAVSS_CHECK_ARG(maps && D, "bank_frame_motion: null pointer");
  MAAVSS_CHECK_ARG(storage == 0 || storage == 1, "bank_frame_motion: storage must be 0 (f32) or 1 (u16), got %d", storage);
  MAAVSS_CHECK_ARG(n_frames >= 2 && frame_elems >= 1, "bank_frame_motion: %lld frames of %lld values hold no pair", (long long)n_frames,
                   (long long)frame_elems);
  MAAVSS_CHECK_ARG(frame_elems <= (1 << 24) && n_frames <= (int64_t)1 << 32, "bank_frame_motion: %lld frames of %lld values exceed the kernel's index range",
                   (long long)n_frames, (long long)frame_elems);
  MAAVSS_CHECK_ARG(cs_aligned(maps, storage ? 2 : 4) && cs_aligned(D, 8), "bank_frame_motion: maps must be aligned to their element, D to 8 bytes");
  const int64_t n_pairs = n_frames - 1;
  const dim3 grid((unsigned)((n_pairs + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  if (storage) hipLaunchKernelGGL(cs_pair_kernel<uint16_t>, grid, dim3(256), 0, st, (const uint16_t*)maps, n_pairs, (int)frame_elems, D);
  else hipLaunchKernelGGL(cs_pair_kernel<float>, grid, dim3(256), 0, st, (const float*)maps, n_pairs, (int)frame_elems, D);
  MAAVSS_LAUNCH_CHECK("cs_pair_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_bank_clip_activity(const float* audio, int64_t n_samples, const double* D, int64_t n_frames, const double* level,
                                         const int64_t* rec_tab, int64_t n_rec, const int64_t* clip_sample, const int32_t* clip_frame,
                                         const int32_t* clip_rec, const int64_t* host_clip_sample, const int32_t* host_clip_frame,
                                         const int32_t* host_clip_rec, int64_t n_clips, int clip_frames, int hops_per_frame, int hop,
                                         double floor_factor, double* energy, double* rms_db, double* rel_db, double* motion_mean,
                                         double* motion_peak, float* peak, int32_t* n_bad, int32_t* n_active, void* stream) {
  MAAVSS_CHECK_ARG(audio && level && rec_tab && clip_sample && clip_frame && clip_rec && host_clip_sample && host_clip_frame && host_clip_rec,
                   "bank_clip_activity: null pointer");
  MAAVSS_CHECK_ARG(energy && rms_db && rel_db && motion_mean && motion_peak && peak && n_bad && n_active, "bank_clip_activity: null output pointer");
  MAAVSS_CHECK_ARG(n_clips > 0 && n_rec > 0 && n_samples > 0 && n_frames > 0,
                   "bank_clip_activity: n_clips = %lld, n_rec = %lld, n_samples = %lld, n_frames = %lld must be positive", (long long)n_clips,
                   (long long)n_rec, (long long)n_samples, (long long)n_frames);
  MAAVSS_CHECK_ARG(clip_frames > 0 && hops_per_frame > 0 && hop > 0, "bank_clip_activity: clip_frames, hops_per_frame and hop must be positive");
  const int64_t J = (int64_t)hops_per_frame * clip_frames;
  MAAVSS_CHECK_ARG(J <= CS_MAX_J, "bank_clip_activity: J = hops_per_frame * clip_frames = %lld segments, the kernel holds %d", (long long)J, CS_MAX_J);
  const int64_t n = J * hop;
  MAAVSS_CHECK_ARG(n_samples >= n && n_frames >= clip_frames, "bank_clip_activity: %lld samples / %lld frames hold no clip of %lld / %d",
                   (long long)n_samples, (long long)n_frames, (long long)n, clip_frames);
  MAAVSS_CHECK_ARG(clip_frames == 1 || D, "bank_clip_activity: D is required when clip_frames > 1");
  MAAVSS_CHECK_ARG(n_clips <= 0x7fffffff && n_rec <= 0x7fffffff, "bank_clip_activity: %lld clips exceed the grid", (long long)n_clips);
  MAAVSS_CHECK_ARG(floor_factor >= 0.0 && floor_factor <= 1.0, "bank_clip_activity: floor_factor = %g is outside [0, 1]", floor_factor);
  MAAVSS_CHECK_ARG(cs_aligned(clip_sample, 8) && cs_aligned(rec_tab, 8) && cs_aligned(level, 8) && cs_aligned(energy, 8) && cs_aligned(rms_db, 8) &&
                       cs_aligned(rel_db, 8) && cs_aligned(motion_mean, 8) && cs_aligned(motion_peak, 8) && (!D || cs_aligned(D, 8)),
                   "bank_clip_activity: the 8-byte tables and outputs must be 8-byte aligned");
  for (int64_t b = 0; b < n_clips; ++b) {
    MAAVSS_CHECK_ARG(host_clip_sample[b] >= 0 && host_clip_sample[b] <= n_samples - n && host_clip_frame[b] >= 0 &&
                         host_clip_frame[b] <= n_frames - clip_frames && host_clip_rec[b] >= 0 && host_clip_rec[b] < n_rec,
                     "bank_clip_activity: clip %lld (sample %lld, frame %d, recording %d) lies outside the bank (%lld samples, %lld frames, %lld recordings)",
                     (long long)b, (long long)host_clip_sample[b], host_clip_frame[b], host_clip_rec[b], (long long)n_samples, (long long)n_frames,
                     (long long)n_rec);
  }
  const cs_clip_out out = {energy, rms_db, rel_db, motion_mean, motion_peak, peak, n_bad, n_active};
  hipLaunchKernelGGL(cs_clip_kernel, dim3((unsigned)n_clips), dim3(256), 0, (hipStream_t)stream, audio, n_samples, D, n_frames, level, rec_tab, n_rec,
                     clip_sample, clip_frame, clip_rec, clip_frames, (int)J, hop, floor_factor, out);
  MAAVSS_LAUNCH_CHECK("cs_clip_kernel");
  return MAAVSS_OK;
}

extern "C" int maavss_bank_clip_select(const double* rms_db, const double* rel_db, const int32_t* n_active, const double* motion_mean,
                                       const double* motion_peak, const float* peak, const int32_t* n_bad, int64_t n_clips, int enabled,
                                       double min_rms_db, double min_rel_db, double min_active, double min_motion, double max_motion_peak,
                                       float max_peak, void* reasons, void* stream) {
  MAAVSS_CHECK_ARG(rms_db && rel_db && n_active && motion_mean && motion_peak && peak && n_bad && reasons, "bank_clip_select: null pointer");
  MAAVSS_CHECK_ARG(n_clips > 0 && n_clips <= ((int64_t)1 << 39), "bank_clip_select: n_clips = %lld must be in [1, 2^39]", (long long)n_clips);
  MAAVSS_CHECK_ARG(enabled >= 0 && enabled < 128, "bank_clip_select: enabled = %d names reasons beyond the seven defined", enabled);
  MAAVSS_CHECK_ARG(cs_aligned(rms_db, 8) && cs_aligned(rel_db, 8) && cs_aligned(motion_mean, 8) && cs_aligned(motion_peak, 8),
                   "bank_clip_select: the f64 columns must be 8-byte aligned");
  const cs_thresholds th = {min_rms_db, min_rel_db, min_active, min_motion, max_motion_peak, max_peak, enabled};
  hipLaunchKernelGGL(cs_select_kernel, dim3((unsigned)((n_clips + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rms_db, rel_db, n_active,
                     motion_mean, motion_peak, peak, n_bad, n_clips, th, (uint8_t*)reasons);
  MAAVSS_LAUNCH_CHECK("cs_select_kernel");
  return MAAVSS_OK;
}
