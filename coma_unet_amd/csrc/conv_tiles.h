// Device helpers shared by the halo-tiled convolution kernels (conv_mfma.hip, conv_split.hip).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;   // 8 bf16 = one MFMA A/B fragment
typedef __attribute__((ext_vector_type(16))) float f32x16_t;  // 32x32 accumulator fragment

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
