// Helpers shared by the tiled convolution kernels (the conv_mfma.h family of files, conv_split.hip).
#pragma once
#include "common.h"

// Host side: the launch of a persistent tile-run kernel.  A D x H x W grid in tz x ty x tx tiles gives ids_total tile ids
// (tile_coords below; padded to 8 z-tiles); the x dimension of the launch gets what is left of a budget of blocks after
// the blocks_yz blocks of the other two dimensions, each block walking ids_per_block consecutive ids.
struct TileRun { int ntx, nty, ntz, ids_total, ids_per_block, gx; };
static inline TileRun tile_run(int D, int H, int W, int tx, int ty, int tz, int budget_blocks, int blocks_yz) {
  TileRun r;
  r.ntx = (W + tx - 1) / tx; r.nty = (H + ty - 1) / ty; r.ntz = (D + tz - 1) / tz;
  r.ids_total = r.ntx * r.nty * ((r.ntz + 7) / 8) * 8;
  r.gx = budget_blocks / blocks_yz;
  if (r.gx < 1) r.gx = 1;
  if (r.gx > r.ids_total) r.gx = r.ids_total;
  r.ids_per_block = (r.ids_total + r.gx - 1) / r.gx;
  r.gx = (r.ids_total + r.ids_per_block - 1) / r.ids_per_block;      // (no block without an id)
  return r;
}

// a kernel that asks for more dynamic LDS than the 64 KB default: raise its limit to KB kilobytes (160: the whole CU's; 80:
// half, for two blocks per CU), once per kernel instance
template <auto KERNEL, int KB = 160> static void set_max_lds() {
  static const hipError_t once = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, KB * 1024);
  (void)once;
}

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;   // 8 bf16 = one MFMA A/B fragment
typedef __attribute__((ext_vector_type(16))) float f32x16_t;  // 32x32 accumulator fragment

// ---- element type of the activations / kernel-layout weights: bf16 (v_mfma_f32_32x32x16_bf16) or fp32
// (v_mfma_f32_32x32x2_f32: exact fp32 products and accumulation, 1/16 of the bf16 rate -- the "fp32 mode" of the model,
// north_star's 1e-3 tolerance path).  Both use the SAME LDS images: a row is 64 bytes = 4 pieces of 16 bytes
// (32 bf16 or 16 fp32 channels), and the 16-byte fragment a lane reads feeds one bf16 MFMA (K = 16: lane half h holds
// k = 8h..8h+7) or four fp32 MFMAs (K = 2 each: MFMA m takes channel 4h + m of the piece from lane half h, so the
// K pair of MFMA m is {m, 4 + m} of the 8 channels the two halves read -- the same for both operands).
template <typename T> struct elem;
template <> struct elem<bf16_t> { static constexpr int EPB = 8; };    // elements per 16-byte piece
template <> struct elem<float> { static constexpr int EPB = 4; };

__device__ __forceinline__ f32x16_t mma_piece(const uint4& a, const uint4& b, f32x16_t acc, bf16_t) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&a), *reinterpret_cast<const bf16x8_t*>(&b), acc, 0, 0, 0);
}
__device__ __forceinline__ f32x16_t mma_piece(const uint4& a, const uint4& b, f32x16_t acc, float) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  return acc;
}

// fused norm statistics: a block ADDS its {sum, sumsq} of one (group, channel) to the caller's zeroed fp64 record
// rec[COMA_STAT_REPLICAS][G][N][2] (replica stride rounded up to a 64-byte line) with global_atomic_add_f64; every consumer
// sums the replicas and derives mean / rstd itself (norm.hip, NormStat).  Replicas: float atomics execute at the memory
// side at ~25 ns per request to one 64-byte line, so a few hundred blocks adding to ONE record would queue for
// microseconds at the end of the kernel; spread over 8 replicas by block index the queue per line is 8x shorter.
__device__ __forceinline__ void stat_add(double2* rec, int G, int N, int g, int n, double a, double c) {
  const long rs = ((long)G * N * 2 + 7) & ~7L;
  double* q = reinterpret_cast<double*>(rec) + (long)(blockIdx.x & (COMA_STAT_REPLICAS - 1)) * rs + ((long)g * N + n) * 2;
  unsafeAtomicAdd(q, a);
  unsafeAtomicAdd(q + 1, c);
}

// blockIdx -> work-item remap: the dispatcher deals consecutive blocks round-robin over the 8 XCDs
// (each with a private 4 MiB L2); give every XCD one CONTIGUOUS range of the work so that
// neighbouring tiles (which share halo voxels) hit in the same L2.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
// tile id -> (tix, tiy, tiz): x slowest, then blocks of 8 z-tiles, then y, z-in-block fastest, so
// the ~64 tiles an XCD works on at once form an 8(y) x 8(z) patch (halo overlap 3.2x -> ~1.3x).
// ids run over ntx * ceil(ntz/8) * nty * 8; returns false for the padding ids (tiz >= ntz).
__device__ __forceinline__ bool tile_coords(int id, int ntx, int nty, int ntz, int& tix, int& tiy, int& tiz) {
  const int ntzb = (ntz + 7) >> 3;
  const int zin = id & 7;
  int t = id >> 3;
  tiy = t % nty; t /= nty;
  const int tzb = t % ntzb;
  tix = t / ntzb;
  tiz = tzb * 8 + zin;
  return tiz < ntz && tix < ntx;
}

// ---- stride-2 transposed convolution (conv_mfma_tconv_k, conv_split_tconv_k) ----
// The 27 (class, tap) pairs in two balanced groups of parity classes -- A = {0, 3, 5, 6} (13 pairs), B = {1, 2, 4, 7} (14
// pairs) -- each walked by halo offset delta.  A wave holds the accumulators of ONE group at a time (4 classes x 2 M-tiles =
// 128 registers; all 8 classes at once spilled 135 registers next to the 22 staging pieces in flight), so a tile is two
// passes over its channel chunks, each staging the halo and only the 13 / 14 taps it needs (75 KB of LDS).  Every tap
// belongs to exactly one pair: LDS weight slot k of a pass holds the tap of pair k.
__device__ constexpr int TC_NP[2] = {13, 14};
__device__ constexpr int TC_DELTA[2][14] = {{0, 0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 6, 6}, {0, 0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 6, 7}};
__device__ constexpr int TC_LCLS[2][14] = {{0, 1, 2, 3, 1, 2, 1, 3, 1, 2, 3, 2, 3, 3}, {0, 1, 2, 3, 0, 3, 1, 3, 3, 2, 3, 3, 3, 3}};
__device__ constexpr int TC_TAP[2][14] = {{13, 17, 23, 25, 15, 21, 11, 19, 9, 5, 7, 3, 1, 27}, {14, 16, 22, 26, 12, 24, 10, 20, 18, 4, 8, 6, 2, 0}};
__device__ constexpr int TC_CLS[2][4] = {{0, 3, 5, 6}, {1, 2, 4, 7}};
