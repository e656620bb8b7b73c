// Pointwise (coma_conv_desc.algo = 7): the 1x1x1 convolutions with several channels on both sides on fp32 tensors -- the
// attention gates' W_g / W_x (C -> C/2), their data gradients and their weight gradients -- on the exact fp32 MFMA
// (v_mfma_f32_32x32x2_f32: one fp32 product per fmaf, no split term).  Under every other algo value these problems run on
// conv_direct_fwd_k / conv_mfma_gather_k<*, 0, float> and conv_f32_wgrad_k<0, 1>.
#include "conv_mfma.h"

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// =====================================================================================
// conv_pw_f32_k<G, NT> -- forward and data gradient, the fp32 twin of conv_mfma_pw_k (conv_mfma.hip): HBM-bound, no LDS for
// the operands, (weights x voxels) orientation, a wave owns 32 voxels, the weight fragments stay in registers for the whole
// kernel.  G = C / 8 channel groups, NT = ceil(N / 32) row tiles.
//   K order: a lane (voxel fr, half fh) loads the 16 bytes x[v][8 g + 4 fh .. + 4] of every 8-channel group g; element q of
//   that load is the B operand of the group's MFMA q, whose two K slots are therefore the channels 8 g + q (fh = 0) and
//   8 g + 4 + q (fh = 1).  The A operand of lane (row fr, half fh) is w[n = fr][8 g + 4 fh + q]: the same 16-byte pattern on
//   the weight row.  One load feeds four MFMAs.
//   Output: accumulator register 4 g4 + q of lane (fr, fh) is channel 8 g4 + 4 fh + q of voxel fr -- four consecutive fp32
//   channels per register group: one 16-byte store (and, accumulating, one 16-byte load) with no lane exchange.
// The next tile's loads are issued before the current tile's MFMAs (C / 2 MFMAs of 64 cycles per row tile), and the old
// values of an accumulating launch before them too.
// Grid: a grid-stride tile loop under a block cap, as conv_mfma_pw_k -- but the cap is what the chip holds at once (CUs x
// resident blocks of the instance, shared by the samples), not 2048 per sample: at 64^3 a wave of a 2048-block grid owns
// ONE tile, nothing is prefetched and every wave pays the statistics reduction (32 channels x 10 shuffles, LDS, fp64
// atomics) for 32 voxels.
// =====================================================================================
struct PwF32P {
  const float* x; int ldx; long sbx; long V; int C;
  float* y; int ldy; long sby; int N;
  const float* w; long wsb;
  const float* bias; int bsb;
  int st16;            // output rows allow aligned 16-byte (4-channel) accesses
  double2* stats;      // optional fused {sum, sumsq} partials of the stored outputs (as conv_mfma_pw_k)
  int stats_inst;
  int accum;           // y += conv(x)
};


template <int G, int NT>
__global__ __launch_bounds__(256) void conv_pw_f32_k(PwF32P p) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int b = blockIdx.y;
  const float* xb = p.x + (long)b * p.sbx;
  const float* wb = p.w + (long)b * p.wsb;
  float* yb = p.y + (long)b * p.sby;
  // weight fragments: lane (row n = fr, half fh) holds w[n][8 g + 4 fh .. + 4]
  f32x4_t wf[NT][G];
  float bv[NT][4][4];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = j * 32 + fr;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      f32x4_t v = {0.f, 0.f, 0.f, 0.f};
      if (n < p.N) v = *reinterpret_cast<const f32x4_t*>(wb + (long)n * p.C + 8 * g + 4 * fh);
      wf[j][g] = v;
    }
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nn = j * 32 + 8 * g4 + 4 * fh + q;
        bv[j][g4][q] = (p.bias && nn < p.N) ? p.bias[b * p.bsb + nn] : 0.f;
      }
  }
  const bool do_stats = p.stats != nullptr;
  float st_s[NT][4][4], st_q[NT][4][4];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
      for (int q = 0; q < 4; ++q) { st_s[j][g4][q] = 0.f; st_q[j][g4][q] = 0.f; }
  const long mtiles = (p.V + 31) / 32, mstep = (long)gridDim.x * 4;
  auto load_x = [&](f32x4_t* xf, long mt) __attribute__((always_inline)) {
    const long v = mt * 32 + fr;
    const bool live = mt < mtiles && v < p.V;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      f32x4_t t = {0.f, 0.f, 0.f, 0.f};
      if (live) t = *reinterpret_cast<const f32x4_t*>(xb + v * p.ldx + 8 * g + 4 * fh);
      xf[g] = t;
    }
  };
  long mt = (long)blockIdx.x * 4 + wid;
  f32x4_t xf[G];
  load_x(xf, mt);
  for (; mt < mtiles; mt += mstep) {
    f32x4_t xn[G];
    load_x(xn, mt + mstep);                              // the next tile's loads fly while this one is multiplied
    const long v = mt * 32 + fr;
    const bool live = v < p.V;
    float* vox = yb + v * p.ldy + 4 * fh;
    // the lane's channel offset, made opaque once per tile: the ~6 lane masks per register group (cnt > 0, cnt >= 4, q < cnt)
    // are loop-invariant, and hoisted out of the tile loop they are 50-100 SGPR pairs live across it -- 87-279 spilled SGPRs.
    // Recomputed per tile they cost a dozen v_cmp next to C / 2 MFMAs of 64 cycles
    int fh4 = 4 * fh;
    asm volatile("" : "+v"(fh4));
    // channels this lane owns in register group (j, g4): 32 j + 8 g4 + 4 fh .. + cnt
    float old[NT][4][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) old[j][g4][q] = 0.f;
        if (!p.accum) continue;                           // (wave-uniform) y += : read what is there, before the MFMAs
        const int n0 = j * 32 + 8 * g4 + fh4, cnt = p.N - n0;
        if (!live || cnt <= 0) continue;
        if (p.st16 && cnt >= 4) {
          const f32x4_t u = *reinterpret_cast<const f32x4_t*>(vox + j * 32 + 8 * g4);
#pragma unroll
          for (int q = 0; q < 4; ++q) old[j][g4][q] = u[q];
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) if (q < cnt) old[j][g4][q] = vox[j * 32 + 8 * g4 + q];
        }
      }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      f32x16_t acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j][g][q], xf[g][q], acc, 0, 0, 0);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        if (j * 32 + 8 * g4 >= p.N) continue;            // (wave-uniform) zero-padded channel groups
        const int n0 = j * 32 + 8 * g4 + fh4, cnt = p.N - n0;
        f32x4_t o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          o[q] = acc[g4 * 4 + q] + bv[j][g4][q] + old[j][g4][q];
          if (do_stats) {
            const float r = (live && q < cnt) ? o[q] : 0.f;
            st_s[j][g4][q] += r; st_q[j][g4][q] = fmaf(r, r, st_q[j][g4][q]);
          }
        }
        if (!live || cnt <= 0) continue;                 // foreign lanes (channels >= N) are never written
        if (p.st16 && cnt >= 4) *reinterpret_cast<f32x4_t*>(vox + j * 32 + 8 * g4) = o;
        else {
#pragma unroll
          for (int q = 0; q < 4; ++q) if (q < cnt) vox[j * 32 + 8 * g4 + q] = o[q];
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) xf[g] = xn[g];
  }
  // ---- fused statistics: lanes -> wave -> block -> partial (same scheme as conv_mfma_pw_k) ----
  if (p.stats) {
    __shared__ float red[4 * 64 * 2];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float a = st_s[j][g4][q], c = st_q[j][g4][q];
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
          const int n = j * 32 + 8 * g4 + 4 * fh + q;
          if (fr == 0) { red[(wid * 64 + n) * 2] = a; red[(wid * 64 + n) * 2 + 1] = c; }
        }
    __syncthreads();
    if (tid < NT * 32 && tid < p.N) {
      double a = 0.0, c = 0.0;
      for (int w = 0; w < 4; ++w) { a += (double)red[(w * 64 + tid) * 2]; c += (double)red[(w * 64 + tid) * 2 + 1]; }
      const int g = p.stats_inst ? b : 0;
      stat_add(p.stats, p.stats_inst ? p.stats_inst : 1, p.N, g, tid, a, c);
    }
  }
}

// blocks the chip holds at once of this instance (CUs x resident blocks per CU), asked once per instance and process on the
// device current at that instance's first launch: the project's flows launch eagerly before they capture a graph (the two
// queries are no stream operations, but a first launch inside a capture would make them there), and the GPUs of a node are
// alike.  The grid, and with it the fp32 summation order of the fused statistics, follows the runtime's occupancy answer.
template <auto KERNEL> static long pw_f32_block_cap() {
  static const long cap = [] {
    int dev = 0, cus = 0, nb = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)KERNEL, 256, 0) != hipSuccess || nb < 1) nb = 1;
    return (long)cus * nb;
  }();
  return cap;
}
template <auto KERNEL> static dim3 pw_f32_grid(long V, int B) {
  long cap = pw_f32_block_cap<KERNEL>() / B, nb = ((V + 31) / 32 + 3) / 4;
  if (cap < 1) cap = 1;
  if (nb > cap) nb = cap;
  return dim3((unsigned)nb, (unsigned)B);
}

// conv_mfma_pw_k's scope restated for 4-byte elements, less the class that did not beat its old kernel (profiles/
// pointwise_f32.txt): C >= 48 -> N = 32 where conv_mfma_gather_k<32, 0, float> takes the problem (C % 16 == 0).
// The widest instances (C > 40 with N > 32) keep part of their state in accumulation registers (one wave per SIMD, no
// scratch); the step does not contain them
bool conv_pw_f32_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  return d->ksize == 1 && d->stride == 1 && x->dtype == COMA_F32 && y->dtype == COMA_F32 && x->C >= 8 && x->C <= 64 && x->C % 8 == 0 &&
         y->C >= 4 && y->C <= 64 && !(x->C >= 48 && x->C % 16 == 0 && y->C == 32) && x->ld % 4 == 0 && x->sb % 4 == 0 && (!x->data || aligned16(x->data)) &&
         t_vox(x) >= 4096 && (long)t_vox(x) * x->ld < (1L << 31) && (long)t_vox(y) * y->ld < (1L << 31);
}

int conv_pw_f32(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                hipStream_t s, double2* stats, int stats_inst, int* stats_chunks, int accum) {
  COMA_CHECK(conv_pw_f32_ok(d, x, y), "conv_pw_f32: problem not in the pointwise kernel's scope");
  COMA_CHECK(aligned16(wk) && aligned16(x->data), "conv_pw_f32: operands must be 16-byte aligned");
  PwF32P q;
  q.x = (const float*)x->data; q.ldx = (int)x->ld; q.sbx = x->sb; q.V = t_vox(x); q.C = x->C;
  q.y = (float*)y->data; q.ldy = (int)y->ld; q.sby = y->sb; q.N = y->C;
  q.w = (const float*)wk; q.wsb = d->per_sample_w ? (long)y->C * x->C : 0;
  q.bias = bias; q.bsb = d->per_sample_w ? y->C : 0;
  q.st16 = y->ld % 4 == 0 && y->sb % 4 == 0 && aligned16(y->data);
  q.stats = nullptr; q.stats_inst = stats_inst; q.accum = accum;
  if (stats) { q.stats = stats; *stats_chunks = 1; }
  const int g = x->C / 8, nt = (y->C + 31) / 32;
  coma_set_kernel_tag("conv_pw_f32_k<%d, %d>", g, nt);
#define PWF(G_, N_) hipLaunchKernelGGL((conv_pw_f32_k<G_, N_>), (pw_f32_grid<conv_pw_f32_k<G_, N_>>(q.V, x->B)), dim3(256), 0, s, q)
#define PWF_G(G_) case G_: if (nt == 1) PWF(G_, 1); else PWF(G_, 2); break
  switch (g) {
    PWF_G(1); PWF_G(2); PWF_G(3); PWF_G(4); PWF_G(5); PWF_G(6); PWF_G(7);
    default: if (nt == 1) PWF(8, 1); else PWF(8, 2); break;
  }
#undef PWF_G
#undef PWF
  COMA_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================
// conv_pw_f32_wgrad_k<TN, TC, TV> -- weight gradient dw[n][c] = sum_v dy[v][n] x[v][c]: the VOXELS along K of the exact fp32
// MFMA (2 per instruction), rows = dy channels, columns = x channels, TN x TC <= 4 stationary 32 x 32 accumulator tiles.
// Both operands come from global memory with 16-byte loads into a voxel-major LDS tile of TV voxels ([TV][C] then [TV][N],
// dense: a staged piece's LDS address is 16 x its index) and are read back 4 bytes per lane -- lane (fr, fh) of K step s
// reads channel fr of voxel 2 s + fh: the transposition conv_f32_wgrad16_k / conv_thin16f_wgrad_k use.  The four waves
// take a quarter of the tile's voxels each.  Two LDS tiles: the next tile's global loads are issued before this tile's
// MFMAs and stored behind them, one barrier per tile.  Lanes past the channel count re-read the last channel: their rows
// / columns are never merged.
// Merge: the four waves add up in LDS, one fp32 atomic per weight into one of `nrep` replicas (wgrad_replica_sum behind
// the kernel).  Blocks are short-lived (a run of tiles_per_block tiles each, several blocks per CU): the kernel runs on
// the side stream beside the data-gradient chain.
// =====================================================================================
struct PwF32WP {
  const float* x; int ldx; long sbx; int C;
  const float* dy; int ldn; long sbn; int N;
  long V, ntiles; int tiles_per_block;
  float* dwk; long wsb;
  int nrep; long rep_stride;
};

#define PW_F32_WGRAD_BLOCKS 2048      // budget of blocks per launch (all samples)

template <int TN, int TC, int TV>
__global__ __launch_bounds__(256) void conv_pw_f32_wgrad_k(PwF32WP p) {
  constexpr int NIT = TV * (TN + TC) * 8 / 256;      // 16-byte staging pieces per thread at the widest channel counts
  constexpr int KST = TV / 8;                        // K steps (2 voxels) per wave and tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 31, fh = lane >> 5;
  const int b = blockIdx.y;
  const float* xb = p.x + (long)b * p.sbx;
  const float* db = p.dy + (long)b * p.sbn;
  const int xp = p.C / 4, dp = p.N / 4, xpieces = TV * xp, pieces = TV * (xp + dp);
  const int tile_bytes = pieces * 16;
  // ---- staging descriptors: piece i < xpieces is x[voxel i / xp][4 (i % xp)..], the rest dy alike ----
  const float* s_ptr[NIT]; int s_v[NIT], s_ld[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + 256 * it;
    const bool isx = i < xpieces;
    const int k = isx ? i : i - xpieces, per = isx ? xp : dp;
    const int vv = k / per, ch = k % per;
    s_v[it] = i < pieces ? vv : (1 << 30);            // (no such piece: never live)
    s_ld[it] = isx ? p.ldx : p.ldn;
    s_ptr[it] = (isx ? xb : db) + (long)vv * s_ld[it] + 4 * ch;
  }
  f32x4_t sreg[NIT];
  auto issue = [&](long tile) __attribute__((always_inline)) {
    const long v0 = tile * TV;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      f32x4_t t = {0.f, 0.f, 0.f, 0.f};                // voxels past the end: zeros in both operands
      if (v0 + s_v[it] < p.V) t = *reinterpret_cast<const f32x4_t*>(s_ptr[it] + v0 * s_ld[it]);
      sreg[it] = t;
    }
  };
  auto store_tile = [&](char* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NIT; ++it)
      if (tid + 256 * it < pieces) *reinterpret_cast<f32x4_t*>(buf + (tid + 256 * it) * 16) = sreg[it];
  };
  // ---- fragment addressing ----
  int a_off[TN], b_off[TC];
  const int vw = wid * (TV / 4) + fh;                  // + 2 s
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) { const int n = 32 * tn + fr; a_off[tn] = (xpieces * 4 + vw * p.N + (n < p.N ? n : p.N - 1)) * 4; }
#pragma unroll
  for (int tc = 0; tc < TC; ++tc) { const int c = 32 * tc + fr; b_off[tc] = (vw * p.C + (c < p.C ? c : p.C - 1)) * 4; }
  const int a_step = 2 * p.N * 4, b_step = 2 * p.C * 4;
  f32x16_t acc[TN][TC];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn)
#pragma unroll
    for (int tc = 0; tc < TC; ++tc)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[tn][tc][e] = 0.f;

  long tile = (long)blockIdx.x * p.tiles_per_block;
  long tile_end = tile + p.tiles_per_block;
  if (tile_end > p.ntiles) tile_end = p.ntiles;
  int cur = 0;
  if (tile < tile_end) {
    issue(tile);
    store_tile(smem);
  }
  __syncthreads();
  for (; tile < tile_end; ++tile) {
    const bool has_next = tile + 1 < tile_end;
    if (has_next) issue(tile + 1);
    const char* buf = smem + cur * tile_bytes;
#pragma unroll
    for (int s = 0; s < KST; ++s) {
      float af[TN], bf[TC];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) af[tn] = *reinterpret_cast<const float*>(buf + a_off[tn] + s * a_step);
#pragma unroll
      for (int tc = 0; tc < TC; ++tc) bf[tc] = *reinterpret_cast<const float*>(buf + b_off[tc] + s * b_step);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tc = 0; tc < TC; ++tc) acc[tn][tc] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[tn], bf[tc], acc[tn][tc], 0, 0, 0);
    }
    if (has_next) store_tile(smem + (cur ^ 1) * tile_bytes);
    __syncthreads();
    cur ^= 1;
  }
  // ---- merge: the four waves' tiles add up in LDS, then one fp32 atomic per weight into this block's replica ----
  float* red = reinterpret_cast<float*>(smem);          // [N][C]
  const int nw = p.N * p.C;
  for (int i = tid; i < nw; i += 256) red[i] = 0.f;
  __syncthreads();
#pragma unroll
  for (int tn = 0; tn < TN; ++tn)
#pragma unroll
    for (int tc = 0; tc < TC; ++tc) {
      const int c = 32 * tc + fr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = 32 * tn + 8 * (e >> 2) + 4 * fh + (e & 3);
        if (n < p.N && c < p.C) atomicAdd(&red[n * p.C + c], acc[tn][tc][e]);
      }
    }
  __syncthreads();
  float* wout = p.dwk + (long)b * p.wsb + (long)(blockIdx.x % (unsigned)p.nrep) * p.rep_stride;
  for (int i = tid; i < nw; i += 256) atomicAdd(wout + i, red[i]);
}

static int pw_f32_wgrad_tv(int tn, int tc) { return tn + tc == 2 ? 128 : 64; }

bool conv_pw_f32_wgrad_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  return d->ksize == 1 && d->stride == 1 && x->dtype == COMA_F32 && dy->dtype == COMA_F32 && x->C >= 4 && x->C <= 64 && x->C % 4 == 0 &&
         dy->C >= 4 && dy->C <= 64 && dy->C % 4 == 0 && x->ld % 4 == 0 && x->sb % 4 == 0 && dy->ld % 4 == 0 && dy->sb % 4 == 0 &&
         (!x->data || aligned16(x->data)) && (!dy->data || aligned16(dy->data)) && t_vox(x) >= 4096 &&
         (long)t_vox(x) * x->ld < (1L << 31) && (long)t_vox(dy) * dy->ld < (1L << 31);
}

int conv_pw_f32_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, void* ws, size_t ws_bytes,
                      hipStream_t s, int zeroed) {
  COMA_CHECK(conv_pw_f32_wgrad_ok(d, x, dy), "conv_pw_f32_wgrad: problem not in the pointwise kernel's scope");
  COMA_CHECK(aligned16(x->data) && aligned16(dy->data), "conv_pw_f32_wgrad: operands must be 16-byte aligned");
  PwF32WP q;
  q.x = (const float*)x->data; q.ldx = (int)x->ld; q.sbx = x->sb; q.C = x->C;
  q.dy = (const float*)dy->data; q.ldn = (int)dy->ld; q.sbn = dy->sb; q.N = dy->C;
  q.V = t_vox(x);
  const int tn = (q.N + 31) / 32, tc = (q.C + 31) / 32, tv = pw_f32_wgrad_tv(tn, tc);
  q.ntiles = (q.V + tv - 1) / tv;
  long gx = PW_F32_WGRAD_BLOCKS / x->B;
  if (gx < 1) gx = 1;
  if (gx > q.ntiles) gx = q.ntiles;
  q.tiles_per_block = (int)((q.ntiles + gx - 1) / gx);
  gx = (q.ntiles + q.tiles_per_block - 1) / q.tiles_per_block;      // (no block without a tile)
  const long wsz1 = (long)q.N * q.C, wsz = wsz1 * (d->per_sample_w ? x->B : 1);
  q.wsb = d->per_sample_w ? wsz1 : 0;
  const WgradRep rep = wgrad_replicas(wsz, dwk, ws, ws_bytes, s, zeroed);
  if (!rep.out) return 2;
  q.dwk = rep.out; q.nrep = rep.nrep; q.rep_stride = rep.rep_stride;
  size_t lds = (size_t)2 * tv * (q.C + q.N) * 4;
  if (lds < (size_t)wsz1 * 4) lds = (size_t)wsz1 * 4;
  const dim3 grid((unsigned)gx, (unsigned)x->B);
  coma_set_kernel_tag("conv_pw_f32_wgrad_k<%d, %d, %d>", tn, tc, tv);
#define PWW(TN_, TC_, TV_) do { set_max_lds<conv_pw_f32_wgrad_k<TN_, TC_, TV_>, 80>(); \
    hipLaunchKernelGGL((conv_pw_f32_wgrad_k<TN_, TC_, TV_>), grid, dim3(256), lds, s, q); } while (0)
  if (tn == 1 && tc == 1) PWW(1, 1, 128);
  else if (tn == 1) PWW(1, 2, 64);
  else if (tc == 1) PWW(2, 1, 64);
  else PWW(2, 2, 64);
#undef PWW
  COMA_LAUNCH_CHECK();
  return wgrad_replicas_done(rep, wsz, dwk, s);
}
