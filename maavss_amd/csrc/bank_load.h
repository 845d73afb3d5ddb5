// How a kernel reads the clip bank (maavss_amd.ClipBank): one stored map value as f32 for either storage, and the clamp every index
// taken from a device table goes through.  Shared by clip_bank.hip (the batch cut) and clip_select.hip (the activity statistics), so
// that both see the maps "exactly as bank_load returns them".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ float bank_load(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float bank_load(const uint16_t* p, int64_t i) { return __fdiv_rn((float)p[i], 65535.f); }

__device__ __forceinline__ int64_t bank_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
