// Weight-gradient kernels on 32 x 32 MFMA tiles for gfx950, any stride: conv_mfma_wgrad_k (bf16) and conv_f32_wgrad_k, with
// wgrad_plan, which chooses their tile, and their launcher.  Cut out of conv_mfma.hip, where they were more than half of
// its compile time; the dispatch (conv_mfma_wgrad) and the other weight-gradient kernels are there.
#include "conv_mfma.h"

// =====================================================================================
// Weight gradient on MFMA:  dwk[b][tap][n][c] = sum_m dy[.][n] * x[.][c]  over the voxels m of
// the M-grid, one operand read densely and the other through a tap-shifted (strided) gather:
//   FORM 0 (nn.Conv3d):          dense = dy[m],  gathered = x[m*stride - pad + tap]
//   FORM 1 (nn.ConvTranspose3d): dense = x[m],   gathered = dy[m*2 - pad + tap]
// A block stages one tile of dense voxels and the matching halo of the gathered tensor in LDS
// as [voxel][channel] images, then every tap re-reads the SAME halo at its shifted address: the
// 27-fold operand reuse happens in LDS, not in L2/HBM.  The GEMM reduction index is the voxel,
// so both MFMA operands are read with ds_read_b64_tr_b16 (4 voxels x 16 channels per 16-lane
// group, delivered channel-per-lane).  The 27 taps are dealt to the 4 waves (7,7,7,6); each wave
// keeps its taps' 32x32 fp32 accumulators in registers across all tiles of the block
// (weight-gradient-stationary) and merges them into dwk with fp32 atomics at the end.
// =====================================================================================
struct WgradP2 {
  const void* dyp; int ldn; long sbn;     // dy  (N channels)
  const void* xp;  int ldc; long sbc;     // x   (C channels)
  int N, C;
  int Mz, My, Mx;      // dense grid
  int Gz, Gy, Gx;      // gathered grid
  int k, stride, pad;
  int lx, ly, lz;      // log2 of the tile dims (tile = 2^lz x 2^ly x 2^lx dense voxels)
  int hz, hy, hx;      // halo dims
  int ntx, nty, ntz;   // tiles per dim
  int tiles_total, tiles_per_block;
  float* dwk; long wsb;
  int cblocks;         // ceil(C / (32*TC))
  int vec_n, vec_c;    // 16-byte loads legal on dy / x
  unsigned m_hx, m_hxy; // magic multipliers: n / hx == umulhi(n, m_hx), n / (hx*hy) == umulhi(n, m_hxy)
  int plain;           // every dwk element is produced by exactly one block: plain stores, no memset, no atomics
  int cp, pg;          // fp32 kernel: gathered channels per tap in an MFMA tile (power of two <= 32), gathered LDS row pitch (bytes)
  int nrep; long rep_stride;   // fp32 kernel, small outputs: blocks merge into one of nrep replicas (summed afterwards)
};

template <int TN, int TC, int FORM, int VEC>
__global__ __launch_bounds__(256, 1) void conv_mfma_wgrad_k(WgradP2 p) {
  constexpr int CDB = 32 * (FORM == 0 ? TN : TC);   // dense-side channels per block
  constexpr int CGB = 32 * (FORM == 0 ? TC : TN);   // gathered-side channels per block
  constexpr int PD = CDB * 2, PG = CGB * 2;         // LDS row pitches (bytes)
  constexpr int MAXT = 7;                           // taps per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int TM = 1 << (p.lx + p.ly + p.lz);
  char* Dt = smem;
  char* Gt = smem + TM * PD;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: tap lists live in SGPRs, tap tests are scalar branches
  const int b = blockIdx.z;
  const int nb = blockIdx.y / p.cblocks, cb = blockIdx.y % p.cblocks;
  const int n0 = nb * 32 * TN, c0 = cb * 32 * TC;
  const bf16_t* dyp16 = static_cast<const bf16_t*>(p.dyp);
  const bf16_t* xp16 = static_cast<const bf16_t*>(p.xp);
  const bf16_t* dense = (FORM == 0 ? dyp16 + (long)b * p.sbn + n0 : xp16 + (long)b * p.sbc + c0);
  const bf16_t* gath = (FORM == 0 ? xp16 + (long)b * p.sbc + c0 : dyp16 + (long)b * p.sbn + n0);
  const int ldd = FORM == 0 ? p.ldn : p.ldc, ldg = FORM == 0 ? p.ldc : p.ldn;
  const int chd = (FORM == 0 ? p.N - n0 : p.C - c0), chg = (FORM == 0 ? p.C - c0 : p.N - n0);   // channels left
  const bool vecd = FORM == 0 ? p.vec_n : p.vec_c, vecg = FORM == 0 ? p.vec_c : p.vec_n;
  const int ntaps = p.k * p.k * p.k;
  const int HV = p.hz * p.hy * p.hx;
  const int tx = 1 << p.lx, ty = 1 << p.ly;

  f32x16_t acc[MAXT][TN][TC];
#pragma unroll
  for (int t = 0; t < MAXT; ++t)
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TC; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][i][j][e] = 0.f;

  // per-wave tap list (wave-uniform; hoisted out of every loop: no integer division inside)
  int tap_w[MAXT], toff_w[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int tap = p.k == 1 ? (t == 0 ? 0 : ntaps) : wid + 4 * t;
    tap_w[t] = tap;
    const int kx = tap % p.k, ky = (tap / p.k) % p.k, kz = tap / (p.k * p.k);
    toff_w[t] = __builtin_amdgcn_readfirstlane(((kz * p.hy + ky) * p.hx + kx) * PG);
  }
  // lane roles for the transposed reads
  const int g16 = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
  const int chan_b = ((g16 & 1) * 16 + 4 * pp) * 2;   // byte offset of this lane's 4 channels in a 32-channel block
  const int vrow = 8 * (g16 >> 1) + q;                // voxel (within a 16-voxel K step) whose row this lane addresses

  const int tile_begin = xcd_remap(blockIdx.x, gridDim.x) * p.tiles_per_block;
  int tile_end = tile_begin + p.tiles_per_block;
  if (tile_end > p.tiles_total) tile_end = p.tiles_total;

  // ---- software pipeline: the next tile's global loads are in flight (registers) while this tile computes ----
  constexpr int MAXP = 20;                      // 16-byte pieces per thread (host guarantees pieces <= 256 * MAXP)
  uint4 sv[MAXP];
  const int ndp = TM * (CDB / 8), ngp = HV * (CGB / 8);
  auto piece_dst = [&](int piece) -> int {
    if (piece < ndp) return (piece / (CDB / 8)) * PD + (piece % (CDB / 8)) * 16;
    const int pg = piece - ndp;
    return TM * PD + (pg / (CGB / 8)) * PG + (pg % (CGB / 8)) * 16;
  };
  auto load_tile = [&](int x0, int y0, int z0) {
    const int bz = z0 * p.stride - p.pad, by = y0 * p.stride - p.pad, bx = x0 * p.stride - p.pad;
#pragma unroll
    for (int u = 0; u < MAXP; ++u) {
      const int piece = tid + 256 * u;
      sv[u] = make_uint4(0, 0, 0, 0);
      if (piece < ndp) {
        const int row = piece / (CDB / 8), ch = piece % (CDB / 8);
        const int vx = row & (tx - 1), vy = (row >> p.lx) & (ty - 1), vz = row >> (p.lx + p.ly);
        const int gz = z0 + vz, gy = y0 + vy, gx = x0 + vx;
        if (gz < p.Mz && gy < p.My && gx < p.Mx && ch * 8 < chd) {
          const bf16_t* src = dense + (unsigned)(((gz * p.My + gy) * p.Mx + gx) * ldd + ch * 8);
          sv[u] = VEC ? *reinterpret_cast<const uint4*>(src) : load8(src, chd - ch * 8, vecd);
        }
      } else if (piece < ndp + ngp) {
        const int pg = piece - ndp;
        const int row = pg / (CGB / 8), ch = pg % (CGB / 8);
        const int q1 = (int)__umulhi((unsigned)row, p.m_hx), hzi = (int)__umulhi((unsigned)row, p.m_hxy);
        const int hxi = row - q1 * p.hx, hyi = q1 - hzi * p.hy;
        const int gz = bz + hzi, gy = by + hyi, gx = bx + hxi;
        if ((unsigned)gz < (unsigned)p.Gz && (unsigned)gy < (unsigned)p.Gy && (unsigned)gx < (unsigned)p.Gx && ch * 8 < chg) {
          const bf16_t* src = gath + (unsigned)(((gz * p.Gy + gy) * p.Gx + gx) * ldg + ch * 8);
          sv[u] = VEC ? *reinterpret_cast<const uint4*>(src) : load8(src, chg - ch * 8, vecg);
        }
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int u = 0; u < MAXP; ++u) {
      const int piece = tid + 256 * u;
      if (piece < ndp + ngp) *reinterpret_cast<uint4*>(smem + piece_dst(piece)) = sv[u];
    }
  };

  int tile = tile_begin, tix = 0, tiy = 0, tiz = 0;
  while (tile < tile_end && !tile_coords(tile, p.ntx, p.nty, p.ntz, tix, tiy, tiz)) ++tile;
  if (tile < tile_end) load_tile(tix << p.lx, tiy << p.ly, tiz << p.lz);
  while (tile < tile_end) {
    int nt = tile + 1, ntix = 0, ntiy = 0, ntiz = 0;
    while (nt < tile_end && !tile_coords(nt, p.ntx, p.nty, p.ntz, ntix, ntiy, ntiz)) ++nt;
    __syncthreads();   // previous tile's reads are done
    store_tile();
    __syncthreads();
    if (nt < tile_end) load_tile(ntix << p.lx, ntiy << p.ly, ntiz << p.lz);
    // ---- MFMA over the tile's voxels, 16 per K step ----
    const int ksteps = TM >> 4;
    for (int ks = 0; ks < ksteps; ++ks) {
      if (p.k == 1 && (ks & 3) != wid) continue;     // 1x1x1: the 4 waves share the single tap by K step
      const int v1 = ks * 16 + vrow, v2 = v1 + 4;
      const int x1 = v1 & (tx - 1), y1 = (v1 >> p.lx) & (ty - 1), z1 = v1 >> (p.lx + p.ly);
      const int x2 = v2 & (tx - 1), y2 = (v2 >> p.lx) & (ty - 1), z2 = v2 >> (p.lx + p.ly);
      const int d1 = v1 * PD + chan_b, d2 = v2 * PD + chan_b;
      const int g1 = ((z1 * p.stride * p.hy + y1 * p.stride) * p.hx + x1 * p.stride) * PG + chan_b;
      const int g2 = ((z2 * p.stride * p.hy + y2 * p.stride) * p.hx + x2 * p.stride) * PG + chan_b;
      constexpr int TD = FORM == 0 ? TN : TC, TG = FORM == 0 ? TC : TN;
      bf16x8_t df[TD];
#pragma unroll
      for (int i = 0; i < TD; ++i) {
        const s4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(Dt + d1 + i * 64));
        const s4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(Dt + d2 + i * 64));
        df[i] = (bf16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int t = 0; t < MAXT; ++t) {
        if (tap_w[t] < ntaps) {
          const int toff = toff_w[t];
          bf16x8_t gf[TG];
#pragma unroll
          for (int j = 0; j < TG; ++j) {
            const s4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(Gt + g1 + toff + j * 64));
            const s4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(Gt + g2 + toff + j * 64));
            gf[j] = (bf16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          }
#pragma unroll
          for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TC; ++j) {
              if (FORM == 0) acc[t][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df[i], gf[j], acc[t][i][j], 0, 0, 0);
              else acc[t][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gf[i], df[j], acc[t][i][j], 0, 0, 0);
            }
        }
      }
    }
    tile = nt; tix = ntix; tiy = ntiy; tiz = ntiz;
  }
  // ---- merge into dwk[b][tap][n][c] ----
  float* wout = p.dwk + (long)b * p.wsb;
  const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int tap = tap_w[t];
    if (tap < ntaps) {
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TC; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int n = n0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
            const int c = c0 + j * 32 + fr;
            if (n < p.N && c < p.C) {
              if (p.plain) wout[((long)tap * p.N + n) * p.C + c] = acc[t][i][j][e];
              else atomicAdd(wout + ((long)tap * p.N + n) * p.C + c, acc[t][i][j][e]);
            }
          }
    }
  }
}

// =====================================================================================
// conv_f32_wgrad_k -- the weight gradient in fp32 mode on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulation).  Same block structure as conv_mfma_wgrad_k (one slab of dwk per block, dense tile + gathered halo staged
// once in LDS as [voxel][channel] fp32 rows, accumulators stationary over the block's tiles), but the MFMA reduces over
// TWO voxels per instruction and takes one fp32 per lane and operand: lane (index = lane & 31, voxel = lane >> 5) reads
// its value with a plain ds_read_b32 -- no transposed reads.  An fp32 MFMA occupies the SIMD for 64 cycles, so the LDS
// reads and the address arithmetic of a voxel pair sit in its shadow; the next pair's fragments are read one step ahead.
//
// The 32 indices of the GATHERED operand are (tap, channel) pairs: with >= 32 gathered channels an MFMA tile is one tap
// x 32 channels (27 tiles); with fewer channels (the 1..16-channel layers of the full-resolution tail) CP = next power
// of two >= C channels of 32 / CP taps share a tile (14, 7, 4, 2 or 1 tiles instead of 27) -- the tap offset is just a
// per-lane constant in the gathered read's address.  The tiles are dealt to min(4, tiles) wave groups; with fewer than
// four tiles the remaining waves split the voxel pairs.  NT = tiles per wave is a template parameter: every wave runs
// NT unconditional MFMAs per pair (a wave with fewer real tiles recomputes one into an accumulator that is never
// stored), so the pipeline has no wave-dependent control flow and hipcc keeps its counted lgkmcnt waits.
// =====================================================================================
template <int FORM, int NT>
__global__ __launch_bounds__(256, 1) void conv_f32_wgrad_k(WgradP2 p) {
  constexpr int PD = 128;                            // dense LDS row pitch (bytes): 32 fp32 channels, zero padded
  constexpr int MAXP = NT == 7 ? 21 : 24;            // 16-byte staging pieces per thread (host guarantees the fit; with 7 tiles
                                                     // per wave = 112 accumulator registers 21 is what fits without spilling)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int TM = 1 << (p.lx + p.ly + p.lz);
  const int PG = p.pg;                               // gathered LDS row pitch (bytes): max(CP, 4) channels
  char* Dt = smem;
  char* Gt = smem + TM * PD;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 31, fh = lane >> 5;
  const int b = blockIdx.z;
  const int nb = blockIdx.y / p.cblocks, cb = blockIdx.y % p.cblocks;
  const int n0 = nb * 32, c0 = cb * 32;
  const float* dyp = reinterpret_cast<const float*>(p.dyp);
  const float* xp = reinterpret_cast<const float*>(p.xp);
  const float* dense = (FORM == 0 ? dyp + (long)b * p.sbn + n0 : xp + (long)b * p.sbc + c0);
  const float* gath = (FORM == 0 ? xp + (long)b * p.sbc + c0 : dyp + (long)b * p.sbn + n0);
  const int ldd = FORM == 0 ? p.ldn : p.ldc, ldg = FORM == 0 ? p.ldc : p.ldn;
  const int chd = (FORM == 0 ? p.N - n0 : p.C - c0), chg = (FORM == 0 ? p.C - c0 : p.N - n0);   // channels left
  const bool vecd = FORM == 0 ? p.vec_n : p.vec_c, vecg = FORM == 0 ? p.vec_c : p.vec_n;
  const int ntaps = p.k * p.k * p.k;
  const int HV = p.hz * p.hy * p.hx;
  const int tx = 1 << p.lx, ty = 1 << p.ly;
  const int CP = p.cp, lcp = 31 - __builtin_clz(CP), TPT = 32 >> lcp;       // channels per tap in a tile, taps per tile
  const int ntiles = (ntaps + TPT - 1) / TPT;
  const int wt = ntiles >= 4 ? 4 : ntiles, ws = 4 / wt;                       // wave groups over tiles x over voxel pairs
  const int tg = wid % wt, ps = wid / wt;

  f32x16_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  // this lane's (tap, channel) in each of the wave's tiles -> byte offset of the gathered read; a lane / tile without a
  // real (tap, channel) reads tap 0 (its column or row of the accumulator is never stored)
  int goff[NT];
  const int gch = fr & (CP - 1);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int i = tg + wt * t;
    const int tap = i * TPT + (fr >> lcp);
    const bool ok = i < ntiles && tap < ntaps && gch < chg;
    const int tp = ok ? tap : 0;
    const int kx = tp % p.k, ky = (tp / p.k) % p.k, kz = tp / (p.k * p.k);
    goff[t] = ((kz * p.hy + ky) * p.hx + kx) * PG + (ok ? gch : 0) * 4;
    // one tap per tile (>= 32 gathered channels): the tap offset is wave-uniform -> a scalar register, the lane's channel
    // offset goes into the common lane term
    if (NT == 7) goff[t] = __builtin_amdgcn_readfirstlane(((kz * p.hy + ky) * p.hx + kx) * PG);
  }

  const int tile_begin = xcd_remap(blockIdx.x, gridDim.x) * p.tiles_per_block;
  int tile_end = tile_begin + p.tiles_per_block;
  if (tile_end > p.tiles_total) tile_end = p.tiles_total;

  // ---- staging: 16-byte pieces (4 channels), the next tile's loads in flight while this tile computes ----
  uint4 sv[MAXP];
  const int gpr = PG >> 4;                            // pieces per gathered row
  const int ndp = TM * 8, ngp = HV * gpr;
  // A staged piece = 4 channels of which 1..4 exist.  Every load of the tile is issued UNCONDITIONALLY from a clamped
  // address and nothing touches its result before store_tile: a conditional load (or a mask applied right away) makes
  // hipcc copy the value after an s_waitcnt vmcnt(0) -- 24 serialised L2 round trips per tile, half the kernel's time.
  // Validity (inside the volume / inside the tensor's channels) travels as one bit per piece and is applied at the LDS
  // store.  The vector / element-wise choice is made ONCE around the whole unrolled loop for the same reason.
  const int lgpr = 31 - __builtin_clz(gpr);           // (gpr = 1, 2, 4 or 8)
  unsigned long long okbits = 0;
#define F32WG_LOAD_LOOP(LD4)                                                                                            \
  _Pragma("unroll") for (int u = 0; u < MAXP; ++u) {                                                                    \
    const int piece = tid + 256 * u;                                                                                    \
    const bool isd = 256 * u < ndp;      /* block-uniform: ndp = 8 TM is a multiple of 256 -> scalar base pointers */     \
    const int pg = piece - ndp;                                                                                         \
    const int row = isd ? piece >> 3 : pg >> lgpr, ch = isd ? piece & 7 : pg & (gpr - 1);                               \
    const int vx = row & (tx - 1), vy = (row >> p.lx) & (ty - 1), vz = row >> (p.lx + p.ly);                            \
    const int q1 = (int)__umulhi((unsigned)row, p.m_hx), hzi = (int)__umulhi((unsigned)row, p.m_hxy);                  \
    const int gz = isd ? z0 + vz : bz + hzi, gy = isd ? y0 + vy : by + (q1 - hzi * p.hy), gx = isd ? x0 + vx : bx + (row - q1 * p.hx); \
    const int Lz = isd ? p.Mz : p.Gz, Ly = isd ? p.My : p.Gy, Lx = isd ? p.Mx : p.Gx;                                  \
    const bool ok = piece < ndp + ngp && (unsigned)gz < (unsigned)Lz && (unsigned)gy < (unsigned)Ly &&                  \
                    (unsigned)gx < (unsigned)Lx && ch * 4 < (isd ? chd : chg);                                          \
    const unsigned off = ok ? (unsigned)(((gz * Ly + gy) * Lx + gx) * (isd ? ldd : ldg) + ch * 4) : 0u;                 \
    const float* src = (isd ? dense : gath) + off;                                                                      \
    const int nvalid = ok ? (isd ? chd : chg) - ch * 4 : 1; (void)nvalid;                                               \
    okbits |= (unsigned long long)ok << u;                                                                              \
    sv[u] = LD4;                                                                                                        \
    if (u % 6 == 5) __builtin_amdgcn_sched_barrier(0);   /* bound the live address temporaries: 6 loads per group */      \
  }
  // (vector loads only: the host sends operands without 16-byte aligned rows to the direct kernel.  A second, element-wise
  //  copy of this unrolled loop took the 7-tile variant to 78 KB -- past the 64 KB instruction cache two CUs share.)
  auto load_next = [&](int x0, int y0, int z0) __attribute__((always_inline)) {
    const int bz = z0 * p.stride - p.pad, by = y0 * p.stride - p.pad, bx = x0 * p.stride - p.pad;
    okbits = 0;
    F32WG_LOAD_LOOP(*reinterpret_cast<const uint4*>(src))
  };
#undef F32WG_LOAD_LOOP
  const bool partd = (chd & 3) != 0 && chd < 32, partg = (chg & 3) != 0 && chg < 32;     // a piece with 1..3 valid channels exists
  auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < MAXP; ++u) {
      const int piece = tid + 256 * u;
      if (piece < ndp + ngp) {
        uint4 v = sv[u];
        if (!((okbits >> u) & 1)) v = make_uint4(0, 0, 0, 0);
        if (partd || partg) {       // (block-uniform) channels past the tensor's own: padding or a neighbour's slice -> zero
          const bool isd = 256 * u < ndp;
          const int ch = isd ? (piece & 7) : ((piece - ndp) & (gpr - 1));
          const int nv = (isd ? chd : chg) - ch * 4;
          if (nv < 4) { v.w = 0; if (nv < 3) v.z = 0; if (nv < 2) v.y = 0; if (nv < 1) v.x = 0; }
        }
        reinterpret_cast<uint4*>(smem)[piece] = v;     // dense rows, then halo rows: contiguous
      }
    }
  };

  // one voxel pair (2 q, 2 q + 1: x neighbours of one row) -> the lane's dense value and its tiles' gathered values
  const int lane_d = fh * PD + fr * 4, lane_g = fh * p.stride * PG + (NT == 7 ? gch * 4 : 0);
  auto rd = [&](int q, float& d, float (&g)[NT]) {
    const int v = 2 * q;
    const int x = v & (tx - 1), y = (v >> p.lx) & (ty - 1), z = v >> (p.lx + p.ly);
    d = *reinterpret_cast<const float*>(Dt + v * PD + lane_d);
    const char* gp = Gt + ((z * p.stride * p.hy + y * p.stride) * p.hx + x * p.stride) * PG + lane_g;
#pragma unroll
    for (int t = 0; t < NT; ++t) g[t] = *reinterpret_cast<const float*>(gp + goff[t]);
  };
  auto mm = [&](float d, const float (&g)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (FORM == 0) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(d, g[t], acc[t], 0, 0, 0);
      else acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[t], d, acc[t], 0, 0, 0);
    }
  };

  const int npairs = TM >> 1;                               // (a multiple of 8)
  int tile = tile_begin, tix = 0, tiy = 0, tiz = 0;
  while (tile < tile_end && !tile_coords(tile, p.ntx, p.nty, p.ntz, tix, tiy, tiz)) ++tile;
  if (tile < tile_end) load_next(tix << p.lx, tiy << p.ly, tiz << p.lz);
  while (tile < tile_end) {
    int nt = tile + 1, ntix = 0, ntiy = 0, ntiz = 0;
    while (nt < tile_end && !tile_coords(nt, p.ntx, p.nty, p.ntz, ntix, ntiy, ntiz)) ++nt;
    __syncthreads();   // previous tile's reads are done
    store_tile();
    __syncthreads();
    if (nt < tile_end) load_next(ntix << p.lx, ntiy << p.ly, ntiz << p.lz);
    float dA, dB, gA[NT], gB[NT];
    // one pair ahead: the next pair's reads go out in one group behind this pair's MFMAs.  Measured alternatives on the
    // 32 -> 32 layer at 128^3 (this order: 79-82 TFLOP/s): a row walk with one v_add per read instead of the (x, y, z)
    // decomposition per pair 62-65; reads strictly alternating with the MFMAs 57-59; hipcc's own order (every read sunk to
    // its MFMA behind lgkmcnt(0)) 70.
    rd(ps, dA, gA);
    for (int q = ps; q < npairs; q += 2 * ws) {
      rd(q + ws, dB, gB);
      __builtin_amdgcn_sched_barrier(0);
      mm(dA, gA);
      __builtin_amdgcn_sched_barrier(0);
      rd(q + 2 * ws < npairs ? q + 2 * ws : ps, dA, gA);        // (the last step re-reads pair `ps`: harmless, keeps the loop uniform)
      __builtin_amdgcn_sched_barrier(0);
      mm(dB, gB);
      __builtin_amdgcn_sched_barrier(0);
    }
    tile = nt; tix = ntix; tiy = ntiy; tiz = ntiz;
  }
  // ---- merge into dwk[b][tap][n][c] ----
  float* wout = p.dwk + (long)b * p.wsb + (long)(blockIdx.x % (unsigned)p.nrep) * p.rep_stride;
  if constexpr (NT == 7) {
    // one tap per tile (both forms): row r of the accumulator is output channel n0 + r, the lane's column is input channel
    // c0 + fr.  One pointer per tile, stepped through the 16 rows (kept compact: the 112 merges of the 7-tile variant
    // with per-element index arithmetic alone were 13 KB of code)
    const int c = c0 + fr;
    const bool full = n0 + 32 <= p.N;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int tap = tg + wt * t;
      if (tap < ntaps && c < p.C) {
        float* pe = wout + ((long)tap * p.N + n0 + 4 * fh) * p.C + c;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          if (full || n0 + (e & 3) + 8 * (e >> 2) + 4 * fh < p.N) {
            if (p.plain) *pe = acc[t][e]; else atomicAdd(pe, acc[t][e]);
          }
          pe += ((e & 3) == 3 ? 5 : 1) * p.C;
        }
      }
    }
  } else {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = (e & 3) + 8 * (e >> 2) + 4 * fh;        // accumulator row of this element; the lane's column is fr
      int tap, n, c;
      if (FORM == 0) {       // rows = dense n, columns = gathered (tap, c)
        const int i = tg + wt * t, tp = i * TPT + (fr >> lcp);
        tap = (i < ntiles && tp < ntaps && gch < chg) ? tp : -1; n = n0 + r; c = c0 + gch;
      } else {               // rows = gathered (tap, n), columns = dense c: the row's (tap, n) is lane-independent
        const int i = tg + wt * t, tp = i * TPT + (r >> lcp), nn = r & (CP - 1);
        tap = (i < ntiles && tp < ntaps && nn < chg) ? tp : -1; n = n0 + nn; c = c0 + fr;
      }
      if (tap >= 0 && n < p.N && c < p.C) {
        if (p.plain) wout[((long)tap * p.N + n) * p.C + c] = acc[t][e];
        else atomicAdd(wout + ((long)tap * p.N + n) * p.C + c, acc[t][e]);
      }
    }
  }
  }
}

static int ilog2_ceil(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

struct WgradPlan { WgradP2 p; int TM; size_t lds; int tn, tc; dim3 grid; bool ok; };

static WgradPlan wgrad_plan(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  WgradPlan pl{};
  pl.ok = false;
  const bool f32 = x->dtype == COMA_F32 && dy->dtype == COMA_F32;
  if (!f32 && (x->dtype != COMA_BF16 || dy->dtype != COMA_BF16)) return pl;
  if (d->ksize != 3 && d->ksize != 1) return pl;
  if ((long)t_vox(x) * x->ld >= (1L << 31) || (long)t_vox(dy) * dy->ld >= (1L << 31)) return pl;
  if (d->form == 1 && d->stride != 2) return pl;
  WgradP2& p = pl.p;
  p.dyp = dy->data; p.ldn = (int)dy->ld; p.sbn = dy->sb;
  p.xp = x->data; p.ldc = (int)x->ld; p.sbc = x->sb;
  p.N = dy->C; p.C = x->C;
  const coma_tensor* dn = d->form == 0 ? dy : x;     // dense
  const coma_tensor* ga = d->form == 0 ? x : dy;     // gathered
  p.Mz = dn->D; p.My = dn->H; p.Mx = dn->W; p.Gz = ga->D; p.Gy = ga->H; p.Gx = ga->W;
  p.k = d->ksize; p.stride = d->stride; p.pad = d->pad;
  const int vq = f32 ? 4 : 8;                        // elements per 16-byte piece
  p.vec_n = dy->ld % vq == 0 && dy->sb % vq == 0 && (!dy->data || aligned16(dy->data));
  p.vec_c = x->ld % vq == 0 && x->sb % vq == 0 && (!x->data || aligned16(x->data));
  pl.tn = (dy->C > 32 && !(x->C > 32 && x->C > dy->C)) ? 2 : 1;
  pl.tc = (pl.tn == 1 && x->C > 32) ? 2 : 1;
  if (f32) pl.tn = pl.tc = 1;
  const int gch = d->form == 0 ? x->C : dy->C;
  // bytes per element, channels per piece, 16-byte staging pieces per thread
  const int esz = f32 ? 4 : 2, ppc = f32 ? 4 : 8, maxp = f32 ? ((gch >= 32 && d->ksize == 3) ? 21 : 24) : 20;
  // fp32 kernel: the gathered operand's 32 MFMA indices are (tap, channel) pairs -- cp channels (a power of two) per tap
  p.cp = 32; p.pg = 128;
  if (f32 && gch < 32) { p.cp = 1; while (p.cp < gch) p.cp <<= 1; p.pg = (p.cp < 4 ? 4 : p.cp) * 4; }
  if (f32 && !(p.vec_n && p.vec_c)) return pl;        // fp32 kernel: 16-byte staging loads only
  // tile: up to 256 dense voxels at stride 1, 64 at stride 2 (the halo grows 8x); shrink until the LDS image
  // and the per-thread register staging budget (20 x 16-byte pieces) fit
  const int cdb = 32 * (d->form == 0 ? pl.tn : pl.tc), cgb = f32 ? p.pg / 4 : 32 * (d->form == 0 ? pl.tc : pl.tn);
  bool fits = false;
  for (int budget = d->stride == 1 ? 8 : 6; budget >= 4 && !fits; --budget) {
    int lx = ilog2_ceil(p.Mx); if (lx > 5) lx = 5;
    if (d->stride == 2 && lx > 4) lx = 4;
    if (lx > budget) lx = budget;
    int rem = budget - lx;
    int ly = ilog2_ceil(p.My); if (ly > (rem + 1) / 2) ly = (rem + 1) / 2;
    rem -= ly;
    int lz = ilog2_ceil(p.Mz); if (lz > rem) lz = rem;
    while (lx + ly + lz < 4) ++lx;     // at least one 16-voxel K step
    p.lx = lx; p.ly = ly; p.lz = lz;
    pl.TM = 1 << (lx + ly + lz);
    p.hz = ((1 << lz) - 1) * p.stride + p.k; p.hy = ((1 << ly) - 1) * p.stride + p.k; p.hx = ((1 << lx) - 1) * p.stride + p.k;
    pl.lds = (size_t)pl.TM * cdb * esz + (size_t)p.hz * p.hy * p.hx * cgb * esz + (f32 ? 1024 : 0);
    fits = pl.lds <= 160 * 1024 && pl.TM * (cdb / ppc) + p.hz * p.hy * p.hx * (cgb / ppc) <= 256 * maxp;
  }
  if (!fits) return pl;
  p.m_hx = (unsigned)((1ull << 32) / (unsigned)p.hx) + 1u;
  p.m_hxy = (unsigned)((1ull << 32) / (unsigned)(p.hx * p.hy)) + 1u;
  p.cblocks = (p.C + 32 * pl.tc - 1) / (32 * pl.tc);
  const int pairs = ((p.N + 32 * pl.tn - 1) / (32 * pl.tn)) * p.cblocks;
  // one block per CU, ONE round (256 blocks): a second round repeats every block's 27 x n x c fp32 atomic merge
  // (32 -> 64 stride 2 at 128^3: 307 -> 254 us; 256 -> 256 at 16^3: 163 -> 107 us)
  // Deepest layers (>= 64 weight tiles, <= 1024 voxels): ONE block per tile and sample.  With per-sample weights (or one sample) every
  // dwk element then has a single producer: plain stores instead of memset + fp32 atomics (512 -> 512 at 8^3: the
  // 28 M atomics of a 2-chunk split cost ~90 of the kernel's 142 us).
  // (measured: at <= 1024 dense voxels a quarter of the CUs busy without atomics beats all of them with; at 4096
  // voxels the single block's MFMA work is the longer pole and the old split wins)
  const bool single = pairs * x->B >= 64 && (long)p.Mz * p.My * p.Mx <= 1024;
  const TileRun r = tile_run(p.Mz, p.My, p.Mx, 1 << p.lx, 1 << p.ly, 1 << p.lz, single ? pairs * x->B : 256, pairs * x->B);
  p.ntx = r.ntx; p.nty = r.nty; p.ntz = r.ntz; p.tiles_total = r.ids_total; p.tiles_per_block = r.ids_per_block;
  const int chunks = r.gx;
  p.plain = chunks == 1 && (d->per_sample_w || x->B == 1);
  if (f32 && p.cp < 8 && d->ksize == 3) p.plain = 0;     // fewer than 4 MFMA tiles: several waves of a block sum the same outputs
  if (f32 && d->ksize == 1) p.plain = 0;                  // 1x1x1: the four waves split the voxel pairs of the single tile
  pl.grid = dim3((unsigned)chunks, (unsigned)pairs, (unsigned)x->B);
  const long taps = (long)d->ksize * d->ksize * d->ksize;
  p.wsb = d->per_sample_w ? taps * p.N * p.C : 0;
  pl.ok = true;
  return pl;
}

bool wgrad_plan_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) { return wgrad_plan(d, x, dy).ok; }

// the launch of conv_mfma_wgrad_k / conv_f32_wgrad_k with the tile wgrad_plan chose
int conv_wgrad_planned(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, void* ws,
                       size_t ws_bytes, hipStream_t s, int zeroed) {
  WgradPlan pl = wgrad_plan(d, x, dy);
  COMA_CHECK(pl.ok, "conv_mfma_wgrad: unsupported problem");
  pl.p.dwk = dwk;
  const long wsz = (long)d->ksize * d->ksize * d->ksize * dy->C * x->C * (d->per_sample_w ? x->B : 1);
  if (!pl.p.plain && !(zeroed & COMA_ZEROED_OUT) && hipMemsetAsync(dwk, 0, sizeof(float) * wsz, s) != hipSuccess) { coma_set_error("wgrad memset failed"); return 2; }
  if (x->dtype == COMA_F32) {
    // small outputs (the 1..16-channel layers): hundreds of blocks merging into a few cache lines serialise in the
    // atomic unit -- they merge into WGRAD_NREP replicas in the workspace, summed by one small kernel (as wgrad2 does)
    // (dwk itself was cleared above where the kernel needs it: COMA_ZEROED_OUT)
    const WgradRep rep = wgrad_replicas(wsz, dwk, ws, ws_bytes, s, zeroed | COMA_ZEROED_OUT, !pl.p.plain);
    if (!rep.out) return 2;
    pl.p.dwk = rep.out; pl.p.nrep = rep.nrep; pl.p.rep_stride = rep.rep_stride;
    const int taps = d->ksize * d->ksize * d->ksize, tpt = 32 / pl.p.cp, ntiles = (taps + tpt - 1) / tpt;
    const int nt = (ntiles + 3) / 4;                  // tiles per wave: 27 -> 7, 14 -> 4, 7 -> 2, <= 4 -> 1
    coma_set_kernel_tag("conv_f32_wgrad_k<%d, %d>", d->form, nt == 1 ? 1 : nt == 2 ? 2 : nt <= 4 ? 4 : 7);
#define F32WL_(F, N_) do { set_max_lds<conv_f32_wgrad_k<F, N_>>(); hipLaunchKernelGGL((conv_f32_wgrad_k<F, N_>), pl.grid, dim3(256), pl.lds, s, pl.p); } while (0)
#define F32WL(F) do { if (nt == 1) F32WL_(F, 1); else if (nt == 2) F32WL_(F, 2); else if (nt <= 4) F32WL_(F, 4); else F32WL_(F, 7); } while (0)
    if (d->form == 0) F32WL(0); else F32WL(1);
#undef F32WL
#undef F32WL_
    COMA_LAUNCH_CHECK();
    return wgrad_replicas_done(rep, wsz, dwk, s);
  }
  const bool vecall = pl.p.vec_n && pl.p.vec_c && dy->C % 8 == 0 && x->C % 8 == 0;
#define WL_(TNV, TCV, F, V_) do { set_max_lds<conv_mfma_wgrad_k<TNV, TCV, F, V_>>(); hipLaunchKernelGGL((conv_mfma_wgrad_k<TNV, TCV, F, V_>), pl.grid, dim3(256), pl.lds, s, pl.p); } while (0)
#define WL(TNV, TCV, F) do { if (vecall) WL_(TNV, TCV, F, 1); else WL_(TNV, TCV, F, 0); } while (0)
  coma_set_kernel_tag("conv_mfma_wgrad_k<%d, %d, %d, %d>", pl.tn, pl.tc, d->form, (int)vecall);
  if (d->form == 0) {
    if (pl.tn == 2) WL(2, 1, 0); else if (pl.tc == 2) WL(1, 2, 0); else WL(1, 1, 0);
  } else {
    if (pl.tn == 2) WL(2, 1, 1); else if (pl.tc == 2) WL(1, 2, 1); else WL(1, 1, 1);
  }
#undef WL
#undef WL_
  COMA_LAUNCH_CHECK();
  return 0;
}
