// What more than one of the Conv3d sources uses (conv3d_igemm.hip, conv3d_wgrad.hip, conv3d_wgrad_wide.hip, conv3d_c1.hip): the LDS chunk
// swizzles, the XCD-aware tile / chunk order, the tile height and the prototypes of what one file launches for another.
#pragma once
#include "mma.h"

// 16-byte-chunk XOR swizzle for an LDS image with rows of RB bytes (RB = 32..256, power of two),
// so that 16 consecutive rows read at the same chunk hit 16 different 16-byte bank slots.
template <int RB>
__device__ __forceinline__ int swz(int row, int chunk) {
  constexpr int PPR = RB >= 256 ? 1 : 256 / RB;
  constexpr int NCH = RB / 16;
  return chunk ^ ((row / PPR) & (NCH - 1));
}

// Halo image of the implicit GEMM, 16-bit modes: chunk swizzle chosen for how ds_read_b128 is serviced -- four groups of 16 lanes,
// {0-3, 12-15, 20-27} etc. (MI355X_MICROARCH.md, LDS): a group holds the 16 positions of a fragment row, EIGHT of them with k
// sub-block g and eight with g + 1 (chunks c and c + 1 of a position).  The row-XOR above (chunk ^= column / PPR) makes every
// such read 2-way conflicted (PMC: 19-37 % of the LDS cycles of the igemm kernels were conflict cycles at 43-65 % LDS busy);
// a search over the linear maps of the column bits gives conflict-free ones: none for 2 chunks per position, bit 2 of the
// column into chunk bit 1 for 4 chunks, column bits 1-2 into chunk bits 1-2 for 8 chunks.  (XOR: the source-side swizzle of the
// LDS-DMA path is the same function.)
template <int RB, int ES>
__device__ __forceinline__ int swz_halo(int col, int chunk) {
  if constexpr (ES != 2) return swz<RB>(col, chunk);
  else if constexpr (RB == 32) return chunk;
  else if constexpr (RB == 64) return chunk ^ (((col >> 2) & 1) << 1);
  else if constexpr (RB == 128) return chunk ^ (col & 6);
  else return swz<RB>(col, chunk);
}

// XCD-aware tile order for the 16x16-output-tile kernels.  Workgroups are dealt round-robin to the 8 XCDs, each with
// its own L2: with a plain (tx, ty, bt) grid the tiles that share input -- x / y neighbours (20x20 halo for a 16x16
// tile) and the same tile of frames t-1, t, t+1 (three kd planes) -- land on eight different L2s and every re-read goes
// to HBM (PMC before: 3.1 GB fetched for a 0.79 GB input by the 32->16 dgrad, 3.3-3.9x on the other layers).  Here
// XCD k walks the k-th contiguous eighth of the tile list, tx fastest, then ty, then bt, so those re-reads meet in L2.
struct TileId { int tx, ty, bt; int64_t lin; bool valid; };
__device__ __forceinline__ TileId xcd_tile(int nx, int ny, int64_t total64) {
  // 32-bit unsigned arithmetic (the host checks total < 2^31): every wave of a workgroup runs this on the CU's one scalar
  // unit, and the 64-bit divisions of the first version were ~300 scalar instructions per wave
  const unsigned total = (unsigned)total64, per = (total + 7) / 8;
  const unsigned lin = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  TileId t;
  t.valid = (blockIdx.x >> 3) < per && lin < total;
  t.lin = lin;
  const unsigned row = lin / (unsigned)nx;
  t.tx = (int)(lin - row * (unsigned)nx);
  t.bt = (int)(row / (unsigned)ny);
  t.ty = (int)(row - (unsigned)t.bt * (unsigned)ny);
  return t;
}
static inline int xcd_grid(int64_t total) { return (int)(((total + 7) / 8) * 8); }

// Tile HEIGHT of the 16-wide output tiles (round 4): 14 rows when that covers the plane with as many tiles as 16 would (56 -> 4 x 14, 28 -> 2 x 14:
// the layers at 56^2 and 28^2 spent 12.5 % of their MFMAs on rows below the image), else 16.  A tile's rows are dealt to the four waves as
// 4 + 4 + 3 + 3 (first row 0, 4, 8, 11); the number of tiles -- and of BatchNorm partial rows -- is the same for both heights by construction.
inline int maavss_conv_tile_h(int Ho) { return cdiv(Ho, 14) == cdiv(Ho, 16) ? 14 : 16; }
__device__ __forceinline__ int tile_row0(int wv, int th) { return th == 14 ? 4 * wv - (wv > 2 ? wv - 2 : 0) : 4 * wv; }
__device__ __forceinline__ int tile_nrows(int wv, int th) { return th == 14 && wv >= 2 ? 3 : 4; }

// Chunk of a weight-gradient workgroup that walks one chunk of the tile list: each XCD owns a contiguous eighth of the chunks, so chunks that
// re-read each other's frames (kd planes) share an L2.  Workgroups with chunk >= nchunk have nothing to do.
__device__ __forceinline__ int xcd_chunk(int nchunk) { return (blockIdx.x & 7) * ((nchunk + 7) / 8) + (blockIdx.x >> 3); }

// conv3d_wgrad_wide.hip, called by maavss_conv3d_wgrad (conv3d_wgrad.hip)
int maavss_conv3d_wgrad_wide_try(const float* x, const void* dy, float* ws, int nchunk, int B, int T, int H, int W, int Ho,
                                 int Wo, int c_in, int c_out, int pad, int mode, int dy16, int x16, hipStream_t st);
// conv3d_wgrad.hip, called by c1_wgrad_launch (conv3d_c1.hip): both Conv3d reduce kernels sit in that file, around chunk_sum16 of reduce.h (alone in a file the first layer's compiles to another body)
void conv3d_c1_wgrad_reduce(const float* ws, float* dw, int nchunk, int beta, hipStream_t st);
