// conv_mfma_duo_k: the thick stride-1 3x3x3 bf16 kernel as two 4-wave groups per CU, and its weight re-layout.
#include "conv_mfma.h"
#include <type_traits>

// =====================================================================================
// conv_mfma_duo_k -- the thick stride-1 3x3x3 kernel as TWO 4-wave groups per CU that alternate roles every phase.
// conv_mfma_halo2_k runs one 4-wave block per CU, and its phases do not overlap: stamped, the MFMA loop is 55 % of the
// kernel, LDS staging stores 18 %, the epilogue 13 %, barriers and waits 14 % -- the matrix pipe idles 45 % of the time.
// Here a workgroup has 8 waves = 2 groups (each SIMD holds one wave of either group).  In a phase one group runs the 54
// MFMAs of a (tile, 16-channel chunk) step out of ITS halo image while the other group does everything else for its own
// next step: writes the halo chunk it fetched two phases ago into its image, writes its half of the next chunk's weights,
// finishes a completed tile (bias, rounding, statistics, 16-byte stores) and issues the loads of the step after next.  One
// workgroup barrier per phase; the loads stay in flight across barriers (raw s_barrier behind an LDS-only wait).
//   LDS: 2 halo images of 816 rows x 48 B (16 channels + pad: 16 consecutive rows land on 16 distinct 16-byte slots)
//        + 2 weight images of 27 taps x 64 lanes x 16 B in FRAGMENT order (a wave's read is 1 KB contiguous) = 130.5 KB.
//   The two groups walk alternate tiles of the block's run and the same chunk sequence, so a weight image serves both
//   (phases 2s and 2s + 1) while the other one is refilled, half by either group.  C == 32: the two images hold the
//   layer's two chunks for the whole kernel.
//   A wave's two M-tiles are y-neighbours: for a fixed (kz, kx) their three ky taps read four distinct halo rows, so a
//   (kz, kx) group is 4 + 3 fragment reads for 6 MFMAs.
// =====================================================================================
// wk[b][tap][N][C] -> [b][n tile][16-channel chunk][tap][lane = (n & 31) + 32 * ((c >> 3) & 1)][8 channels]: the order in which
// conv_mfma_duo_k holds a weight image in LDS, so that a group's half image is ONE contiguous 13.8 KB run (from the plain
// layout a 16-channel piece is 32 bytes of a 2 C-byte row: at C = 64 the staging group pulled 4x the useful bytes through L1)
__global__ __launch_bounds__(256) void duo_relayout_k(const uint4* __restrict__ src, uint4* __restrict__ dst, int N, int C8, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;      // piece (b, tap, n, c8)
  if (i >= total) return;
  const int c8 = (int)(i % C8);
  long t = i / C8;
  const int n = (int)(t % N); t /= N;
  const int tap = (int)(t % 27);
  const long b = t / 27;
  const int nt = N >> 5, nch = C8 >> 1;
  const long o = ((((b * nt + (n >> 5)) * nch + (c8 >> 1)) * 27 + tap) * 64) + (n & 31) + 32 * (c8 & 1);
  dst[o] = src[i];
}

__device__ __forceinline__ void duo_barrier() {
  // LDS traffic of this wave has landed; buffer loads issued for later phases stay in flight (no vmcnt wait)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// LX = 5: tiles of 2 x 4 x 32 voxels (W >= 32); LX = 4: 2 x 8 x 16 (the 16^3 level: an M-tile is two x-rows of 16 voxels)
template <int STATS, int LX = 5>
__global__ __launch_bounds__(512, 1) void conv_mfma_duo_k(Halo2P p) {
  constexpr int TX = 1 << LX, RY = 32 / TX, TY = 4 * RY, TZ = 2, HX = TX + 2, HY = TY + 2, HZ = TZ + 2, HV = HX * HY * HZ;
  static_assert(HV <= 816, "the halo image is sized for the 2 x 4 x 32 tile");
  constexpr int P = 48, HB = 816 * P, WB = 27 * 64 * 16;
  constexpr int HP = HV * 2, HIT = (HP + 255) / 256;        // halo pieces of a 16-channel chunk; per thread of a group
  constexpr int WH = 27 * 32, WIT = (WH + 255) / 256;       // weight pieces per half image; per thread of a group
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // the wave index through readfirstlane: everything derived from it (group, tile walk, descriptors, role branches) is
  // then provably wave-uniform -- otherwise the compiler wraps every buffer load in a waterfall loop
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), grp = wid >> 2, wq = wid & 3, gt = tid & 255;
  char* const Hl = smem + grp * HB;
  char* const Wl = smem + 2 * HB;
  const int b = blockIdx.z, n0 = blockIdx.y * 32;
  const int fr = lane & 31, fh = lane >> 5;
  const bf16_t* xb = static_cast<const bf16_t*>(p.x) + (long)b * p.sbx;
  const bf16_t* wb = static_cast<const bf16_t*>(p.w) + (long)b * p.wsb;
  bf16_t* yb = static_cast<bf16_t*>(p.y) + (long)b * p.sby;
  const int nch = p.C >> 4;
  const bool w_static = nch <= 2;

  // ---- staging descriptors ----
  // Halo piece `it` of this thread is row (gt >> 1) + 128 it, half gt & 1.  Its halo coordinates and global offset are
  // rebuilt from the FIRST piece's coordinates at every fetch (row + 128 = 3 x-lines + 26: a few adds and compares per
  // piece on the staging wave) instead of living in 14 registers: at two waves per SIMD registers are the scarce thing.
  const int h_row0 = gt >> 1, h_half = gt & 1;
  unsigned h_zyx0 = ((unsigned)(h_row0 / (HX * HY)) << 20) | ((unsigned)((h_row0 / HX) % HY) << 10) | (unsigned)(h_row0 % HX);
  // in-volume test of a halo piece as two packed subtractions (fields of 9 bits under a guard bit each): halo coordinate h
  // of a tile at origin o is inside iff lo <= h <= hi with lo = (o == 0), hi = min(dim - o, 510) per axis
  constexpr unsigned GUARD = (1u << 29) | (1u << 19) | (1u << 9);
  const int h_lds0 = (gt >> 1) * P + (gt & 1) * 16;          // + it * 128 * P
  constexpr unsigned OOB = 0x7fff0000u;
  const int w_half = grp == 1 ? 0 : WH;                       // group 1 fills pieces [0, WH), group 0 [WH, 2 WH)
  // weight piece q = w_half + gt + 256 it = (tap, lane): tap = q >> 6 advances by 4 per `it`, the lane part is a per-thread
  // constant -- its global offset is rebuilt at every fetch (a handful of VALU on the staging wave; registers are the
  // scarce thing at two waves per SIMD)
  const int w_q0 = w_half + gt;
  const bool wf = p.wfrag != nullptr;                         // fragment-ordered weights: piece q of a chunk image sits at q * 16
  const unsigned w_lane_b = wf ? (unsigned)((w_q0 & 63) * 16)
                               : (unsigned)((((n0 + (w_q0 & 31)) * p.C) + ((w_q0 >> 5) & 1) * 8) * 2);
  const int w_lds0 = w_q0 * 16;                               // + it * 4096
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(xb), 0, p.xbytes, 0x00020000);
  const bf16_t* wfb = wf ? static_cast<const bf16_t*>(p.wfrag) + (long)b * p.wfrag_sb + (long)blockIdx.y * (nch * 27 * 512) : wb;
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(wfb), 0, wf ? (unsigned)(nch * 27 * 1024) : p.wbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(xb), 0, 0, 0x00020000);   // reads as zero

  // fragment bases: this wave's M-tiles are rows y0, y0 + 1 of plane zq
  const int zq = wq >> 1, y0w = (wq & 1) * 2;
  // (LX = 4: M-tile j = 2 wq + i is rows 2 (j & 3), 2 (j & 3) + 1 of plane zq; the lane's voxel is (fr >> 4, fr & 15) in it)
  const int a_base = LX == 5 ? ((zq * HY + y0w) * HX + fr) * P + fh * 16
                             : ((zq * HY + y0w * RY + (fr >> LX)) * HX + (fr & (TX - 1))) * P + fh * 16;
  const int w_frag = lane * 16;

  // ---- this group's tile walk ----
  const int id_begin = xcd_remap(blockIdx.x, gridDim.x) * p.ids_per_block;
  int id_end = id_begin + p.ids_per_block;
  if (id_end > p.ids_total) id_end = p.ids_total;
  struct Cur { int valid, cc, tix, tiy, tiz, id; };
  auto first_tile = [&](Cur& c, int from) {        // first valid id >= from with the group's parity relative to id_begin
    c.cc = 0; c.valid = 0; c.tix = c.tiy = c.tiz = 0;
    int id = from;
    while (id < id_end && !tile_coords(id, p.ntx, p.nty, p.ntz, c.tix, c.tiy, c.tiz)) id += 2;
    c.id = id;
    c.valid = id < id_end;
  };
  auto advance = [&](Cur& c) {
    if (!c.valid) return;
    if (c.cc + 1 < nch) { ++c.cc; return; }
    first_tile(c, c.id + 2);
  };
  // tiles of the two groups: count them (the phase count must be the same for every wave of the block)
  int nt0 = 0, nt1 = 0;
  {
    int a, bq, c;
    for (int id = id_begin; id < id_end; ++id)
      if (tile_coords(id, p.ntx, p.nty, p.ntz, a, bq, c)) { if ((id - id_begin) & 1) ++nt1; else ++nt0; }
  }
  const int nsteps = (nt0 > nt1 ? nt0 : nt1) * nch;
  if (nsteps == 0) return;
  const int nphases = 2 * nsteps + 4;                // (a multiple of 4: nch is even) + 1 round: the last tiles are finished in a staging phase

  // (native 4-dword vectors: as HIP uint4 structs the loop-carried pieces were split into scalars, the loads landed in
  // temporaries and the copies into the carried registers put an s_waitcnt vmcnt(0) in front of every barrier)
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  // Halo pieces are fetched for TWO consecutive chunk steps at once (hreg[0]: the even chunk, hreg[1]: the odd one -- the
  // two 32-byte halves of a 64-byte run of every voxel row) and written to LDS one step apart: fetched one step at a time,
  // every 128-byte line went through L1 once per 16-channel chunk (4x the useful bytes at C = 64; staging alone 506 us
  // for 64 -> 32 at 128^3 next to 325 us of matrix phases).
  u32x4_t hreg[2][HIT], wreg[WIT];
  auto load_halo = [&](const Cur& c) {               // c: the even chunk step of a pair
    const int z0 = c.tiz * TZ, y0 = c.tiy * TY, x0 = c.tix * TX;
    const int zb = z0 - 1, yb0 = y0 - 1, xb0 = x0 - 1;
    const unsigned org_b = (unsigned)((((long)(zb * p.H + yb0) * p.W + xb0) * p.ldx + c.cc * 16) * 2);
    const __amdgpu_buffer_rsrc_t rs = c.valid ? rs_x : rs_0;
    const unsigned lo = ((unsigned)(z0 == 0) << 20) | ((unsigned)(y0 == 0) << 10) | (unsigned)(x0 == 0);
    const int hz_ = p.D - z0 < 510 ? p.D - z0 : 510, hy_ = p.H - y0 < 510 ? p.H - y0 : 510, hx_ = p.W - x0 < 510 ? p.W - x0 : 510;
    const unsigned hi = (((unsigned)hz_ << 20) | ((unsigned)hy_ << 10) | (unsigned)hx_) | GUARD;
    asm volatile("" : "+v"(h_zyx0));                 // (keeps the per-piece values out of loop-invariant registers)
    int hz = (int)(h_zyx0 >> 20), hy = (int)((h_zyx0 >> 10) & 1023), hx = (int)(h_zyx0 & 1023);
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
      const unsigned zyx = (gt + 256 * it < HP) ? ((unsigned)hz << 20) | ((unsigned)hy << 10) | (unsigned)hx : 0x1ff7fdffu;   // (invalid: above any limit)
      const bool ok = ((((zyx | GUARD) - lo) & (hi - zyx)) & GUARD) == GUARD;
      const unsigned roff = (unsigned)((((hz * p.H + hy) * p.W + hx) * p.ldx + h_half * 8) * 2);
      const unsigned voff = ok ? org_b + roff : OOB;
      hx += 128 % HX; hy += 128 / HX;                  // the next piece: 128 rows = 3 x-lines + 26 voxels on (LX = 4: 7 + 2)
      if (hx >= HX) { hx -= HX; ++hy; }
      if (hy >= HY) { hy -= HY; ++hz; }
      hreg[0][it] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0);
      hreg[1][it] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + 32u, 0, 0);  // (OOB + 32 is still out of range)
    }
  };
  auto store_halo = [&](auto odd_c) {
    constexpr int odd = decltype(odd_c)::value;
#pragma unroll
    for (int it = 0; it < HIT; ++it)
      if (gt + 256 * it < HP) *reinterpret_cast<u32x4_t*>(Hl + h_lds0 + it * 128 * P) = hreg[odd][it];
  };
  typedef std::integral_constant<int, 0> even_t;
  typedef std::integral_constant<int, 1> odd_t;
  auto load_w = [&](int ws, bool on) {               // this group's half of weight step ws (chunk ws % nch)
    const int c0_b = wf ? (ws % nch) * (27 * 1024) : (ws % nch) * 32;
    const __amdgpu_buffer_rsrc_t rs = on ? rs_w : rs_0;
    const unsigned tap_b = wf ? 1024u : (unsigned)(p.N * p.C * 2);
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const int tap = (w_q0 >> 6) + 4 * it;
      const int wt = p.flip ? 26 - tap : tap;
      const unsigned voff = (gt + 256 * it < WH) ? (unsigned)wt * tap_b + w_lane_b : OOB;
      wreg[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, c0_b, 0);
    }
  };
  auto store_w = [&](int ws) {
    char* dst = Wl + (ws & 1) * WB + w_lds0;
#pragma unroll
    for (int it = 0; it < WIT; ++it)
      if (gt + 256 * it < WH) *reinterpret_cast<u32x4_t*>(dst + it * 4096) = wreg[it];
  };
  auto w_needed = [&](int ws) { return ws < 2 || !w_static; };

  f32x16_t acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  float st_s[4][4], st_q[4][4];
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
    for (int q = 0; q < 4; ++q) { st_s[g4][q] = 0.f; st_q[g4][q] = 0.f; }
  float* const bias_l = reinterpret_cast<float*>(smem + 2 * HB + 2 * WB);      // this block's 32 bias values (read at every tile end)
  if (tid < 32) bias_l[tid] = p.bias ? p.bias[b * p.bsb + n0 + tid] : 0.f;

  // ---- prologue: weight step 0 complete, group 0's first halo in place, the next loads in flight ----
  Cur cC, cB, cA;            // computed last / to be stored next / the next PAIR of chunk steps to fetch (cA.cc even)
  cC.valid = 0; cC.cc = 0; cC.tix = cC.tiy = cC.tiz = 0; cC.id = 0;
  first_tile(cB, id_begin + grp);
  cA = cB;
  auto advance2 = [&](Cur& c) {                      // two chunk steps on (nch is even)
    if (!c.valid) return;
    if (c.cc + 2 < nch) { c.cc += 2; return; }
    first_tile(c, c.id + 2);
  };
  load_halo(cA); advance2(cA);                       // steps 0 and 1
  load_w(0, true);
  store_w(0);
  if (grp == 0) {
    store_halo(even_t{});
    cC = cB; advance(cB);
  }
  load_w(1, w_needed(1));
  duo_barrier();

  // ================= matrix phase: step ph >> 1 of this group =================
  auto matrix_phase = [&](int ph) __attribute__((always_inline)) {
#ifdef COMA_DUO_NO_MFMA          // (diagnostic builds only: profiles/ablate_duo.sh)
      return;
#endif
      if (__builtin_amdgcn_readfirstlane(cC.valid)) {
        // (readfirstlane: the walk's fields may live in VGPRs, and a vector compare turned this into 32 v_cndmask per phase)
        if (__builtin_amdgcn_readfirstlane(cC.cc) == 0) {          // a new tile (zeroed here, in place: zeroing in the epilogue made the compiler keep a second copy)
          asm volatile("" ::: "memory");       // (a real branch: if-converted, this is 32 v_cndmask in every matrix phase)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
        }
        const char* Wc = Wl + ((ph >> 1) & 1) * WB + w_frag;
        // xr: LX = 5 the four halo rows y .. y + 3 the wave's two y-neighbour M-tiles share; LX = 4 rows ky + 2 i of the
        // two M-tiles (each two x-rows high: a tap shift by one row gives different fragments: six reads, rows 0 .. 4)
        constexpr int NXR = LX == 5 ? 4 : 5;
        uint4 wg[2][3], xr[2][NXR];
        auto rdg = [&](int g, int bf) {
          const int kz = g / 3, kx = g % 3;
          const int toff = (kz * HY * HX + kx) * P;
#pragma unroll
          for (int r = 0; r < NXR; ++r) xr[bf][r] = *reinterpret_cast<const uint4*>(Hl + a_base + toff + r * HX * P);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) wg[bf][ky] = *reinterpret_cast<const uint4*>(Wc + (kz * 9 + ky * 3 + kx) * 1024);
        };
        rdg(0, 0);
#pragma unroll
        for (int g = 0; g < 9; ++g) {
          if (g + 1 < 9) rdg(g + 1, (g + 1) & 1);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = mma_piece(wg[g & 1][ky], xr[g & 1][RY * i + ky], acc[i], bf16_t());
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
  };
  // ================= everything else, for this group's NEXT matrix phase =================
  // (two forms, chosen at compile time: EVEN writes the even chunk step of a pair and finishes the tile the previous odd step
  // completed; ODD writes the odd step and fetches the next pair -- a run-time choice put the fetch behind a branch, and
  // loop-carried pieces behind a branch are copied through temporaries with a vmcnt(0) wait)
  auto other_phase = [&](auto odd_c, int ph) __attribute__((always_inline)) {
      constexpr int odd = decltype(odd_c)::value;
#ifdef COMA_DUO_NO_STAGE
      if (cC.valid && cC.cc == nch - 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i) asm volatile("" :: "v"(acc[i]));
      }
      cC = cB; advance(cB);
      return;
#endif
      store_halo(odd_c);                                // (waits for the pieces fetched two or more phases ago)
      const int ws = (ph >> 1) + 1;
      if (w_needed(ws)) store_w(ws);
      // every piece fetched two phases ago has been consumed (or, masked off, may be dropped): say so -- a piece stored under
      // a lane mask or a skipped weight refill stays "in flight" for the waitcnt pass, which then drains vmcnt in front of
      // the next fetch AND at the start of the next matrix phase
      __builtin_amdgcn_s_waitcnt(0x0F70);               // vmcnt(0): free at run time, the pieces are two phases old
      // finish the tile whose last chunk this group computed in the previous phase
      if constexpr (odd == 0) {
#ifdef COMA_DUO_NO_EPI
      if (cC.valid && cC.cc == nch - 1) {          // (diagnostic: the accumulators stay live, nothing is stored)
#pragma unroll
        for (int i = 0; i < 2; ++i) asm volatile("" :: "v"(acc[i]));
      }
#else
      if (cC.valid && cC.cc == nch - 1) {
        const int x0 = cC.tix * TX, y0 = cC.tiy * TY, z0 = cC.tiz * TZ;
        float4 bq[4];                                 // this lane's 16 bias values, four LDS reads in flight together
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) bq[g4] = *reinterpret_cast<const float4*>(bias_l + 8 * g4 + 4 * fh);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int j = wq * 2 + i;
          const int gz = z0 + (j >> 2), gy = y0 + (j & 3) * RY + (fr >> LX), gx = x0 + (fr & (TX - 1));
          const bool valid = gz < p.D && gy < p.H && gx < p.W;
          unsigned pk[4][2];
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            bf16_t o[4];
            const float bv[4] = {bq[g4].x, bq[g4].y, bq[g4].z, bq[g4].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              o[q] = static_cast<bf16_t>(acc[i][g4 * 4 + q] + bv[q]);
              if constexpr (STATS) {
                const float r = valid ? static_cast<float>(o[q]) : 0.f;
                st_s[g4][q] += r; st_q[g4][q] = fmaf(r, r, st_q[g4][q]);
              }
            }
            const uint2 u = *reinterpret_cast<const uint2*>(o);
            pk[g4][0] = u.x; pk[g4][1] = u.y;
          }
          bf16_t* vox = yb + ((long)(gz * p.H + gy) * p.W + gx) * p.ldy + n0 + 8 * fh;
#pragma unroll
          for (int gp = 0; gp < 2; ++gp) {
            const auto r0 = __builtin_amdgcn_permlane32_swap(pk[2 * gp][0], pk[2 * gp + 1][0], false, false);
            const auto r1 = __builtin_amdgcn_permlane32_swap(pk[2 * gp][1], pk[2 * gp + 1][1], false, false);
            if (valid) *reinterpret_cast<uint4*>(vox + 16 * gp) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#endif
      }
      // rotate the walk; behind the odd step of a pair, fetch the next pair
      cC = cB; advance(cB);
      if constexpr (odd == 1) { load_halo(cA); advance2(cA); }
      if (w_needed(ws + 1)) load_w(ws + 1, true);
  };
  // Two straight-line loops, one per role order (NOT one loop with a role branch: the pieces in flight are loop-carried
  // registers, and across a branch the compiler parked the loads in temporaries and copied them behind an s_waitcnt
  // vmcnt(0) -- in front of every barrier).  Both loops execute two barriers per round.
  // Enter the loops with nothing in flight: the waitcnt pass merges the prologue's pending loads (other registers than the
  // loop's) into the loop header state and then waits vmcnt(0) wherever the loop body reuses one of those registers --
  // at the start of every matrix phase.  (The builtin, not inline asm: the pass has to see this wait.)
  __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0) only
  if (grp == 0) {        // (its first halo was written by the prologue: even step in place, the odd one follows)
#pragma unroll 1
    for (int ph = 0; ph < nphases; ph += 4) {
      matrix_phase(ph); duo_barrier(); other_phase(odd_t{}, ph + 1); duo_barrier();
      matrix_phase(ph + 2); duo_barrier(); other_phase(even_t{}, ph + 3); duo_barrier();
    }
  } else {
#pragma unroll 1
    for (int ph = 0; ph < nphases; ph += 4) {
      other_phase(even_t{}, ph); duo_barrier(); matrix_phase(ph + 1); duo_barrier();
      other_phase(odd_t{}, ph + 2); duo_barrier(); matrix_phase(ph + 3); duo_barrier();
    }
  }

  // ---- fused statistics: lanes -> wave -> block (LDS) -> the caller's record ----
  if constexpr (STATS) {
    if (p.stats) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      float* red = reinterpret_cast<float*>(smem);      // [8 waves][32 ch][2]
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float a = st_s[g4][q], c = st_q[g4][q];
#pragma unroll
          for (int o = 16; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
          if (fr == 0) { red[(wid * 32 + 8 * g4 + 4 * fh + q) * 2] = a; red[(wid * 32 + 8 * g4 + 4 * fh + q) * 2 + 1] = c; }
        }
      __syncthreads();
      if (tid < 32 && n0 + tid < p.N) {
        double a = 0.0, c = 0.0;
        for (int w = 0; w < 8; ++w) { a += (double)red[(w * 32 + tid) * 2]; c += (double)red[(w * 32 + tid) * 2 + 1]; }
        const int g = p.stats_inst ? b : 0;
        stat_add(p.stats, p.stats_inst ? p.stats_inst : 1, p.N, g, n0 + tid, a, c);
      }
    }
  }
}

// bytes of scratch conv_mfma_duo_k wants for a fragment-ordered copy of the weights (C >= 64 stride-1 3^3 bf16 layers), else 0
// COMA_NO_DUO=1: conv_mfma_halo2_k everywhere (0); COMA_DUO_C32_ONLY=1: the C == 32 layers only (1); default: all (2)
static int duo_mode() {
  static const int mode = getenv("COMA_NO_DUO") != nullptr ? 0 : getenv("COMA_DUO_C32_ONLY") != nullptr ? 1 : 2;
  return mode;
}
size_t duo_frag_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  if (duo_mode() < 2 || x->dtype != COMA_BF16 || d->ksize != 3 || d->stride != 1 || x->W < 16) return 0;
  if (x->C < 64 || x->C % 16 || y->C % 32) return 0;
  return (size_t)(d->per_sample_w ? x->B : 1) * 27 * y->C * x->C * 2;
}

// does conv_mfma_halo<bf16_t> run this problem on conv_mfma_duo_k with fragment-ordered weights (given 16-byte aligned
// weights)?  Every condition of the dispatch below that does not depend on the weight pointer or the scratch.
bool duo_wide_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  if (duo_frag_bytes(d, x, y) == 0 || x->C <= 32 || x->C % 32) return false;
  const bool vecx = x->ld % 8 == 0 && x->sb % 8 == 0 && aligned16(x->data);
  const bool st16 = y->ld % 8 == 0 && y->sb % 8 == 0 && aligned16(y->data);
  return vecx && st16 && (unsigned long long)t_vox(x) * x->ld * sizeof(bf16_t) < 0x7fff0000ull &&
         x->D <= 510 && x->H <= 510 && x->W <= 510;
}

// two 4-wave groups per CU alternating matrix and staging phases (conv_mfma_duo_k): full 32-channel output tiles with
// 16-byte stores, 16-channel input chunks
// Measured (128^3, batch 2; microbenchmarks, duo / halo2): 32 -> 32 forward 282-315 / 321-339 us.  C >= 64 from the plain
// weight layout was SLOWER (64 -> 32 732-757 / 683-704 us: a 16-channel weight piece is 32 bytes of a 128-byte row and the
// staging group pulled 4x the useful bytes through L1); with the weights re-laid in fragment order by a 4-us launch
// (duo_relayout_k into the caller's scratch, coma_conv_fwd_ws_bytes): 64 -> 32 696 / 691 and 665 / 689 (data gradient),
// 64 -> 64 at 64^3 129 / 144 and 134 / 150, 128 -> 64 270 / 273 and 277 / 297, 256 -> 128 at 32^3 117 / 125 and 126 / 134;
// step 18.09 -> 17.99 ms.  COMA_NO_DUO=1: conv_mfma_halo2_k everywhere; COMA_DUO_C32_ONLY=1: the C == 32 layers only.
bool duo_takes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y, const Halo2P& q, bool thin, bool vec, bool wk_frag,
               const void* ws, size_t ws_bytes, size_t* frag_bytes_out) {
  const bool no_duo = duo_mode() == 0, duo_all = duo_mode() == 2;
  const size_t frag_bytes = duo_frag_bytes(d, x, y);      // C >= 64: scratch for the fragment-ordered copy of the weights
  *frag_bytes_out = frag_bytes;
  const bool wide_ok = duo_all && q.C > 32 && frag_bytes > 0 && (wk_frag || (ws && ws_bytes >= frag_bytes && aligned16(ws)));
  return !no_duo && !thin && vec && (q.C == 32 || wide_ok) && q.N % 32 == 0 && q.st16 &&
         q.D <= 510 && q.H <= 510 && q.W <= 510;
}

// q: the fields conv_mfma_halo<bf16_t> filled for both kernels, statistics request included (a problem duo_takes() accepted);
// lx = 5 / 4: tiles of 2 x 4 x 32 voxels, or 2 x 8 x 16 on the 16-wide grids; nblk_n = 32-channel output blocks
int launch_duo(const coma_conv_desc* d, const coma_tensor* x, Halo2P q, const void* wk, int lx, int nblk_n, size_t frag_bytes, void* ws,
               bool wk_frag, hipStream_t s) {
  if (q.C > 32 && wk_frag) {
    q.wfrag = wk; q.wfrag_sb = d->per_sample_w ? 27L * q.N * q.C : 0;
  } else if (q.C > 32) {
    const long pieces = (long)(frag_bytes / 16);
    hipLaunchKernelGGL(duo_relayout_k, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, (const uint4*)wk, (uint4*)ws, q.N, q.C / 8, pieces);
    COMA_LAUNCH_CHECK();
    q.wfrag = ws; q.wfrag_sb = d->per_sample_w ? 27L * q.N * q.C : 0;
  }
  const TileRun r2 = tile_run(q.D, q.H, q.W, lx == 5 ? 32 : 16, lx == 5 ? 4 : 8, 2, 256, nblk_n * x->B);      // one 512-thread block per CU, once
  q.ids_per_block = r2.ids_per_block;
  const dim3 grid2((unsigned)r2.gx, (unsigned)nblk_n, (unsigned)x->B);
  const size_t lds2 = (size_t)2 * 34 * 6 * 4 * 48 + (size_t)2 * 27 * 64 * 16 + 128;
#define DUO(ST_, LX_) do { set_max_lds<conv_mfma_duo_k<ST_, LX_>>(); hipLaunchKernelGGL((conv_mfma_duo_k<ST_, LX_>), grid2, dim3(512), lds2, s, q); } while (0)
  if (lx == 5) {
    coma_set_kernel_tag("conv_mfma_duo_k<%d, 5>", q.stats ? 1 : 0);
    if (q.stats) DUO(1, 5);
    else DUO(0, 5);
  } else {
    coma_set_kernel_tag("conv_mfma_duo_k<%d, 4>", q.stats ? 1 : 0);
    if (q.stats) DUO(1, 4);
    else DUO(0, 4);
  }
#undef DUO
  COMA_LAUNCH_CHECK();
  return 0;
}
