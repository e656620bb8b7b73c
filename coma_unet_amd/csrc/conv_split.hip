// Split-bf16 convolution kernels for gfx950: fp32 tensors and fp32 kernel-layout weights, products on
// v_mfma_f32_32x32x16_bf16 (coma_conv_desc.algo = 4, 5, 6).
//
// Every fp32 operand a is split when it is STAGED into LDS (once per element, not once per use) into two bf16 values
//     a_hi = bf16(a),   a_lo = bf16(a - float(a_hi))            (both round-to-nearest-even)
// and a product is formed from three MFMAs into one fp32 accumulator
//     a * b  ~=  a_hi * b_hi  +  a_hi * b_lo  +  a_lo * b_hi.
// |a - a_hi - a_lo| <= 2^-16 |a| and |a_lo| <= 2^-8 (1 + 2^-8) |a|, so the dropped terms (a_lo b_lo and the two
// residuals) are below 3.03 * 2^-16 |a||b| < 2^-14 |a||b| per product; a product of two bf16 values is exact in fp32.
// Matrix-pipe cost of 16 channels of K: 3 x 32 cycles, against 8 x 64 cycles of v_mfma_f32_32x32x2_f32.
// Non-finite inputs do not split (inf - inf): an infinite operand yields NaN where the exact kernels yield inf.
//
//   conv_split_halo_k  -- stride-1 3x3x3 forward / data gradient (the problems of conv_mfma_halo2_k<2, 16, 1, 1, float>)
//   conv_split_wgrad_k -- stride-1 3x3x3 weight gradient          (the problems of conv_f32_wgrad16_k<1, 0>)
// and, under algo = 5 (wide split), the stride-2 families:
//   conv_split_tconv_k  -- stride-2 3x3x3 transposed convolution / data gradient of the stride-2 convolutions
//                          (the problems of conv_mfma_tconv_k<float, *>)
//   conv_split_wgrad2_k -- stride-2 and transposed 3x3x3 weight gradient (the problems of conv_f32_wgrad16_k<2, *>)
// and, under algo = 6 (thin split), the few-channel full-resolution families on v_mfma_f32_16x16x32_bf16:
//   conv_split_thin_k       -- stride-1 3x3x3 forward / data gradient, C <= 16 (the problems of conv_thin16f_k)
//   conv_split_thin_wgrad_k -- their weight gradient                           (the problems of conv_thin16f_wgrad_k)
#include "conv_mfma.h"    // s4_t / lds_s4_t, aligned16, conv_f32_*_problem: the fp32 problems the exact kernels take

// 4 fp32 (one 16-byte staging piece) -> 4 bf16 hi + 4 bf16 lo
__device__ __forceinline__ void split4(const uint4& v, uint2& hi, uint2& lo) {
  const float f[4] = {__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
  bf16_t h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = static_cast<bf16_t>(f[j]);
    l[j] = static_cast<bf16_t>(f[j] - static_cast<float>(h[j]));
  }
  hi = *reinterpret_cast<const uint2*>(h);
  lo = *reinterpret_cast<const uint2*>(l);
}

__device__ __forceinline__ f32x16_t mma3(const uint4& a_hi, const uint4& a_lo, const uint4& b_hi, const uint4& b_lo, f32x16_t acc) {
  const bf16x8_t ah = *reinterpret_cast<const bf16x8_t*>(&a_hi), al = *reinterpret_cast<const bf16x8_t*>(&a_lo);
  const bf16x8_t bh = *reinterpret_cast<const bf16x8_t*>(&b_hi), bl = *reinterpret_cast<const bf16x8_t*>(&b_lo);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);     // (small terms first)
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  return acc;
}

// =====================================================================================
// conv_split_halo_k -- the structure of conv_mfma_halo2_k<2, 16, 1, 1, float>: one 4-wave block per CU walks a run of
// 2 x 4 x 32-voxel tiles; per (tile, 16-channel chunk) the 4 x 6 x 34 halo and the chunk's 27 x 32 weight rows sit in LDS,
// the next chunk's pieces are fetched by buffer loads issued between the MFMAs.  An LDS row holds the SAME 64 bytes the
// fp32 kernel keeps (16 fp32 channels), now as [16 bf16 hi][16 bf16 lo]; 80-byte row pitch, so the 16-byte fragment reads
// of 16 consecutive rows land on 16 distinct slots.  A wave's two M-tiles are y-neighbours: for a fixed (kz, kx) their
// three ky taps read four halo rows, so a (kz, kx) group is 8 + 6 fragment reads for 18 MFMAs.
// The MFMA is (weights x voxels): a lane holds 4 x 4 consecutive output channels of one voxel (16-byte fp32 stores).
// =====================================================================================
struct SplitHaloP {
  const float* x; int ldx; long sbx; int D, H, W, C;
  float* y; int ldy; long sby; int N;
  const float* w; long wsb;
  const float* bias; int bsb;
  int flip;
  int ntx, nty, ntz, ids_total, ids_per_block;
  unsigned xbytes, wbytes;   // bytes of one sample of x / of one weight set (buffer descriptors: out-of-range pieces read as zero)
  int st16;                  // output rows allow aligned 16-byte (4-channel) stores
  double2* stats;            // optional fused norm statistics record (stat_add)
  int stats_inst;            // B: groups = the B samples (InstanceNorm), 0: one group (BatchNorm)
};

__global__ __launch_bounds__(256, 1) void conv_split_halo_k(SplitHaloP p) {
  constexpr int CK = 16, TX = 32, TY = 4, TZ = 2, HX = TX + 2, HY = TY + 2, HZ = TZ + 2, HV = HX * HY * HZ;
  constexpr int P = 80;                                  // LDS row pitch (bytes)
  constexpr int HP = HV * 4, HIT = (HP + 255) / 256;     // 16-byte fp32 pieces of a halo chunk, per-thread iterations
  constexpr int WP = 27 * 32 * 4, WIT = (WP + 255) / 256;
  static_assert(WIT + HIT <= 27, "one prefetch piece per tap");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Hl = smem;                                       // [HV][80]
  char* Wl = smem + HV * P;                              // [27 * 32][80]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.z, n0 = blockIdx.y * 32;
  const int fr = lane & 31, fh = lane >> 5;
  const float* xb = p.x + (long)b * p.sbx;
  const float* wb = p.w + (long)b * p.wsb;
  float* yb = p.y + (long)b * p.sby;
  const int nchunks = p.C / CK;

  // ---- staging descriptors (tile independent) ----
  int h_roff[HIT], h_lds[HIT], h_z[HIT], h_y[HIT], h_x[HIT];
#pragma unroll
  for (int it = 0; it < HIT; ++it) {
    const int piece = tid + 256 * it;
    const int row = piece >> 2, ch = piece & 3;
    const int hx = row % HX, hy = (row / HX) % HY, hz = row / (HX * HY);
    h_z[it] = piece < HP ? hz : (1 << 20); h_y[it] = hy; h_x[it] = hx;
    h_roff[it] = ((hz * p.H + hy) * p.W + hx) * p.ldx + ch * 4;
    h_lds[it] = row * P + ch * 8;                        // hi half; lo at + 32
  }
  constexpr unsigned OOB = 0x7fff0000u;
  int w_lds[WIT];
  unsigned w_boff[WIT];
#pragma unroll
  for (int it = 0; it < WIT; ++it) {
    const int piece = tid + 256 * it;
    const int ch = piece & 3, n = (piece >> 2) & 31, t = piece >> 7;
    const int wt = p.flip ? 26 - t : t;
    w_boff[it] = (piece < WP && n0 + n < p.N) ? (unsigned)(((wt * p.N + n0 + n) * p.C + ch * 4) * 4) : OOB;   // + chunk offset at load time
    w_lds[it] = (t * 32 + n) * P + ch * 8;
  }
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, p.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wb), 0, p.wbytes, 0x00020000);
  // fragment read bases: the wave's two M-tiles are rows y, y + 1 of one z plane
  const int a_base = ((((wid * 2) >> 2) * HY + ((wid * 2) & 3)) * HX + fr) * P + fh * 16;
  const int w_base = fr * P + fh * 16;

  uint4 hreg[HIT], wreg[WIT];
  auto load_halo = [&](int z0, int y0, int x0, int c0) {
    const int zb = z0 - 1, yb0 = y0 - 1, xb0 = x0 - 1;
    const unsigned org_b = (unsigned)((((long)(zb * p.H + yb0) * p.W + xb0) * p.ldx + c0) * 4L);   // (mod 2^32: a valid piece's sum is its true offset)
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
      const bool ok = (unsigned)(zb + h_z[it]) < (unsigned)p.D && (unsigned)(yb0 + h_y[it]) < (unsigned)p.H &&
                      (unsigned)(xb0 + h_x[it]) < (unsigned)p.W;
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ok ? org_b + (unsigned)h_roff[it] * 4u : OOB, 0, 0);
      hreg[it] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  };
  auto load_w = [&](int c0) {
#pragma unroll
    for (int it = 0; it < WIT; ++it) {
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_boff[it], c0 * 4, 0);
      wreg[it] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  };
  // the split happens here: one conversion per staged element, two 8-byte LDS stores per piece
  auto store_halo = [&]() {
#pragma unroll
    for (int it = 0; it < HIT; ++it)
      if (tid + 256 * it < HP) {
        uint2 hi, lo;
        split4(hreg[it], hi, lo);
        *reinterpret_cast<uint2*>(Hl + h_lds[it]) = hi;
        *reinterpret_cast<uint2*>(Hl + h_lds[it] + 32) = lo;
      }
  };
  auto store_w = [&]() {
#pragma unroll
    for (int it = 0; it < WIT; ++it)
      if (tid + 256 * it < WP) {
        uint2 hi, lo;
        split4(wreg[it], hi, lo);
        *reinterpret_cast<uint2*>(Wl + w_lds[it]) = hi;
        *reinterpret_cast<uint2*>(Wl + w_lds[it] + 32) = lo;
      }
  };

  const int id_begin = xcd_remap(blockIdx.x, gridDim.x) * p.ids_per_block;
  int id_end = id_begin + p.ids_per_block;
  if (id_end > p.ids_total) id_end = p.ids_total;
  int id = id_begin, tix = 0, tiy = 0, tiz = 0;
  while (id < id_end && !tile_coords(id, p.ntx, p.nty, p.ntz, tix, tiy, tiz)) ++id;
  if (id >= id_end) return;      // padding ids only: nothing to store, nothing to add to the statistics record
  load_halo(tiz * TZ, tiy * TY, tix * TX, 0);
  load_w(0);

  const bool do_stats = p.stats != nullptr;
  float bv[4][4];
  float st_s[4][4], st_q[4][4];     // fused norm statistics of this lane's 16 channels (stored values)
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = n0 + 8 * g4 + 4 * fh + q;
      bv[g4][q] = (p.bias && n < p.N) ? p.bias[b * p.bsb + n] : 0.f;
      st_s[g4][q] = 0.f; st_q[g4][q] = 0.f;
    }

  while (id < id_end) {
    const int x0 = tix * TX, y0 = tiy * TY, z0 = tiz * TZ;
    int nid = id + 1, ntix = 0, ntiy = 0, ntiz = 0;
    while (nid < id_end && !tile_coords(nid, p.ntx, p.nty, p.ntz, ntix, ntiy, ntiz)) ++nid;
    const bool has_next = nid < id_end;

    f32x16_t acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    for (int cc = 0; cc < nchunks; ++cc) {
      __syncthreads();                       // all waves finished reading the previous halo / weights
      store_halo();
      store_w();
      __syncthreads();
      // prefetch while this chunk computes: the next chunk of this tile, or chunk 0 of the next tile; one piece per tap
      // inside the MFMA loop, through descriptors whose range is zero when there is nothing to prefetch
      const bool same_tile = cc + 1 < nchunks;
      const bool pref = same_tile || has_next;
      const int pz = same_tile ? z0 : ntiz * TZ, py = same_tile ? y0 : ntiy * TY, px = same_tile ? x0 : ntix * TX;
      const int pc0 = same_tile ? cc * CK + CK : 0;
      const __amdgpu_buffer_rsrc_t rs_xp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, pref ? p.xbytes : 0, 0x00020000);
      const __amdgpu_buffer_rsrc_t rs_wp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wb), 0, pref ? p.wbytes : 0, 0x00020000);
      const unsigned porg_b = (unsigned)((((long)((pz - 1) * p.H + (py - 1)) * p.W + (px - 1)) * p.ldx + pc0) * 4L);
      auto pref_piece = [&](int t) __attribute__((always_inline)) {
        if (t < WIT) {
          const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs_wp, w_boff[t], pc0 * 4, 0);
          wreg[t] = make_uint4(v[0], v[1], v[2], v[3]);
        }
        const int it = t - WIT;
        if (it >= 0 && it < HIT) {
          const bool ok = (unsigned)(pz - 1 + h_z[it]) < (unsigned)p.D && (unsigned)(py - 1 + h_y[it]) < (unsigned)p.H &&
                          (unsigned)(px - 1 + h_x[it]) < (unsigned)p.W;
          const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs_xp, ok ? porg_b + (unsigned)h_roff[it] * 4u : OOB, 0, 0);
          hreg[it] = make_uint4(v[0], v[1], v[2], v[3]);
        }
      };
      // fragments one (kz, kx) group ahead, in a second register set: [.][.][0] = hi, [.][.][1] = lo
      uint4 wg[2][3][2], xr[2][4][2];
      auto rdg = [&](int g, int bf) __attribute__((always_inline)) {
        const int kz = g / 3, kx = g % 3;
        const int toff = (kz * HY * HX + kx) * P;
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) {
#pragma unroll
          for (int r = 0; r < 4; ++r) xr[bf][r][hl] = *reinterpret_cast<const uint4*>(Hl + a_base + toff + r * HX * P + hl * 32);
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
            wg[bf][ky][hl] = *reinterpret_cast<const uint4*>(Wl + w_base + (kz * 9 + ky * 3 + kx) * 32 * P + hl * 32);
        }
      };
      rdg(0, 0);
#pragma unroll
      for (int g = 0; g < 9; ++g) {
        if (g + 1 < 9) rdg(g + 1, (g + 1) & 1);
        pref_piece(3 * g); pref_piece(3 * g + 1); pref_piece(3 * g + 2);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[i] = mma3(wg[g & 1][ky][0], wg[g & 1][ky][1], xr[g & 1][i + ky][0], xr[g & 1][i + ky][1], acc[i]);
        // 18 MFMAs; the next group's 14 fragment reads and this group's 3 prefetch pieces go BETWEEN them
#define COMA_SGB(mfma, ds, valu, vmem)                                   \
        __builtin_amdgcn_sched_group_barrier(0x008, mfma, 0);            \
        if (ds) __builtin_amdgcn_sched_group_barrier(0x100, ds, 0);      \
        if (valu) __builtin_amdgcn_sched_group_barrier(0x006, valu, 0);  \
        if (vmem) __builtin_amdgcn_sched_group_barrier(0x020, vmem, 0);
        COMA_SGB(1, 1, 4, 0) COMA_SGB(1, 1, 4, 1) COMA_SGB(1, 1, 4, 0) COMA_SGB(1, 1, 4, 0) COMA_SGB(1, 1, 4, 1) COMA_SGB(1, 1, 4, 0)
        COMA_SGB(1, 1, 4, 0) COMA_SGB(1, 1, 4, 1) COMA_SGB(1, 1, 2, 0) COMA_SGB(1, 1, 2, 0) COMA_SGB(1, 1, 2, 0) COMA_SGB(1, 1, 2, 0)
        COMA_SGB(1, 1, 0, 0) COMA_SGB(1, 1, 0, 0) COMA_SGB(1, 0, 0, 0) COMA_SGB(1, 0, 0, 0) COMA_SGB(1, 0, 0, 0) COMA_SGB(1, 0, 0, 0)
#undef COMA_SGB
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- epilogue: lane = one voxel, 4 groups of 4 consecutive channels, one 16-byte store each ----
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int j = wid * 2 + i;
      const int gz = z0 + (j >> 2), gy = y0 + (j & 3), gx = x0 + fr;
      const bool valid = gz < p.D && gy < p.H && gx < p.W;
      float* dst = yb + ((long)(gz * p.H + gy) * p.W + gx) * p.ldy + n0 + 4 * fh;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        if (n0 + 8 * g4 >= p.N) continue;            // (wave-uniform)
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          o[q] = acc[i][g4 * 4 + q] + bv[g4][q];
          if (do_stats) { const float r = valid ? o[q] : 0.f; st_s[g4][q] += r; st_q[g4][q] = fmaf(r, r, st_q[g4][q]); }
        }
        if (valid) {
          if (p.st16 && n0 + 8 * g4 + 4 * fh + 3 < p.N) *reinterpret_cast<float4*>(dst + 8 * g4) = make_float4(o[0], o[1], o[2], o[3]);
          else {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (n0 + 8 * g4 + 4 * fh + q < p.N) dst[8 * g4 + q] = o[q];
          }
        }
      }
    }
    id = nid; tix = ntix; tiy = ntiy; tiz = ntiz;
  }
  // ---- fused statistics: lanes -> wave (butterfly over the 32 voxel lanes) -> block (LDS) -> record ----
  if (do_stats) {
    __syncthreads();                                  // LDS images are dead; reuse the front as a [4 waves][32 ch][2] table
    float* red = reinterpret_cast<float*>(smem);
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
      for (int w = 0; w < 4; ++w) { a += (double)red[(w * 32 + tid) * 2]; c += (double)red[(w * 32 + tid) * 2 + 1]; }
      const int g = p.stats_inst ? b : 0;
      stat_add(p.stats, p.stats_inst ? p.stats_inst : 1, p.N, g, n0 + tid, a, c);
    }
  }
}

bool conv_split_fwd_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  return conv_f32_halo2_problem(d, x, y);
}

int conv_split_fwd(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                   hipStream_t s, double2* stats, int stats_inst, int* stats_chunks) {
  COMA_CHECK(conv_split_fwd_ok(d, x, y), "conv_split: problem not in the split kernel's scope");
  COMA_CHECK(aligned16(x->data) && aligned16(wk), "conv_split: operands must allow 16-byte channel pieces (aligned)");
  SplitHaloP q;
  q.x = (const float*)x->data; q.ldx = (int)x->ld; q.sbx = x->sb; q.D = x->D; q.H = x->H; q.W = x->W; q.C = x->C;
  q.y = (float*)y->data; q.ldy = (int)y->ld; q.sby = y->sb; q.N = y->C;
  q.w = (const float*)wk; q.wsb = d->per_sample_w ? 27L * y->C * x->C : 0;
  q.bias = bias; q.bsb = d->per_sample_w ? y->C : 0;
  q.flip = d->form == 1;
  {   // descriptor ranges (one sample / one weight set), capped below the out-of-range marker 0x7fff0000
    const unsigned long long xb_ = (unsigned long long)t_vox(x) * x->ld * 4, wb_ = 27ull * y->C * x->C * 4;
    COMA_CHECK(wb_ < 0x7fff0000ull, "conv_split: weight set too large for 32-bit buffer offsets");
    q.xbytes = (unsigned)(xb_ < 0x7fff0000ull ? xb_ : 0x7fff0000ull);
    q.wbytes = (unsigned)wb_;
  }
  q.st16 = y->ld % 4 == 0 && y->sb % 4 == 0 && aligned16(y->data);
  const int nblk_n = (q.N + 31) / 32;
  const TileRun r = tile_run(q.D, q.H, q.W, 32, 4, 2, 256, nblk_n * x->B);      // one block per CU, one round
  q.ntx = r.ntx; q.nty = r.nty; q.ntz = r.ntz; q.ids_total = r.ids_total; q.ids_per_block = r.ids_per_block;
  q.stats = nullptr; q.stats_inst = stats_inst;
  if (stats) { q.stats = stats; *stats_chunks = 1; }
  const size_t lds = (size_t)(34 * 6 * 4 + 27 * 32) * 80;
  set_max_lds<conv_split_halo_k>();
  coma_set_kernel_tag("conv_split_halo_k");
  hipLaunchKernelGGL(conv_split_halo_k, dim3((unsigned)r.gx, (unsigned)nblk_n, (unsigned)x->B), dim3(256), lds, s, q);
  COMA_LAUNCH_CHECK();
  return 0;
}

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));      // (native vectors for the staging registers: see conv_mfma_duo_k)

__device__ __forceinline__ void split4(const u32x4_t& v, uint2& hi, uint2& lo) { split4(make_uint4(v[0], v[1], v[2], v[3]), hi, lo); }

// =====================================================================================
// conv_split_tconv_k -- the structure of conv_mfma_tconv_k<float, STATS> (see there for the parity classes and the two
// passes): a coarse 2 x 4 x 32 tile plus a one-voxel high-side halo (495 rows), the 27 (class, tap) pairs walked by halo
// offset, persistent blocks, the next step's 15 fp32 staging pieces fetched inside the MFMA loop.  An LDS row holds the same
// 64 bytes (16 channels), now [16 bf16 hi][16 bf16 lo]: the two 16-byte fragment reads per row that fed four
// v_mfma_f32_32x32x2_f32 feed three v_mfma_f32_32x32x16_bf16, and the 75 KB image keeps its size.
// COMA_ACCUMULATE is kept (the stride-2 data gradients add into the skip connection's gradient).  The norm statistics are
// NOT fused: their 32 accumulators, live across the tile loop next to 128 accumulator and 60 staging registers plus the
// conversion temporaries, spilled 24 registers to scratch; the caller runs the separate statistics pass instead.
// =====================================================================================
struct SplitTconvP {
  const float* x; int ldx; long sbx; int D, H, W, C;     // coarse input
  float* y; int ldy; long sby; int Do, Ho, Wo, N;        // fine output (2 x coarse, or one less, per dimension)
  const float* w; long wsb;                              // [b][27][N][C]
  const float* bias; int bsb;
  int ntx, nty, ntz, ids_total, ids_per_block;
  unsigned xbytes, wbytes;
  int accum;
};

__global__ __launch_bounds__(256, 1) void conv_split_tconv_k(SplitTconvP p) {
  constexpr int CK = 16;
  constexpr int TX = 32, TY = 4, TZ = 2, HX = TX + 1, HY = TY + 1, HZ = TZ + 1, HV = HX * HY * HZ;   // 495 halo rows
  constexpr int P = 80;
  constexpr int HP = HV * 4, HIT = (HP + 255) / 256;   // 1980 halo pieces of 4 fp32 -> 8 per thread
  constexpr int WS = 14, WP = WS * 32 * 4, WIT = WP / 256;   // 14 weight slots = 1792 pieces -> 7 per thread
  static_assert(WP % 256 == 0 && HIT + WIT <= 2 * 13, "at most two prefetch pieces per (class, tap) pair");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Wl = smem;                                     // [14 * 32][80]
  char* Hl = smem + WS * 32 * P;                       // [HV][80]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.z, n0 = blockIdx.y * 32;
  const int fr = lane & 31, fh = lane >> 5;
  const float* xb = p.x + (long)b * p.sbx;
  const float* wb = p.w + (long)b * p.wsb;
  float* yb = p.y + (long)b * p.sby;
  const int nchunks = p.C / CK;
  constexpr unsigned OOB = 0x7fff0000u;

  // ---- staging descriptors (tile independent), as conv_mfma_tconv_k: byte offset of a halo piece relative to the tile
  // origin, its halo coordinates as three 9-bit fields tested against the packed per-tile limits with one subtraction ----
  unsigned h_boff[HIT], h_zyx[HIT];
#pragma unroll
  for (int it = 0; it < HIT; ++it) {
    const int piece = tid + 256 * it;
    const int row = piece >> 2, ch = piece & 3;
    const int hx = row % HX, hy = (row / HX) % HY, hz = row / (HX * HY);
    h_boff[it] = (unsigned)((((hz * p.H + hy) * p.W + hx) * p.ldx + ch * 4) * 4);
    h_zyx[it] = piece < HP ? ((unsigned)hz << 20) | ((unsigned)hy << 10) | (unsigned)hx : 0x1ff00000u;
  }
  const int h_lds0 = (tid >> 2) * P + (tid & 3) * 8;       // hi half of piece `it`: + it * 64 rows; lo at + 32
  constexpr unsigned GUARD = (1u << 29) | (1u << 19) | (1u << 9);
  const int w_s0 = tid >> 7, w_n = (tid >> 2) & 31, w_ch = tid & 3;
  const int w_lds0 = (w_s0 * 32 + w_n) * P + w_ch * 8;
  constexpr int W_LSTEP = 2 * 32 * P;
  unsigned w_row = (unsigned)(((long)(n0 + w_n) * p.C + w_ch * 4) * 4L);
  const unsigned w_tap = (unsigned)((long)p.N * p.C * 4L);                      // bytes between two taps
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, p.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wb), 0, p.wbytes, 0x00020000);

  int a_base[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = wid * 2 + i;
    a_base[i] = (((j >> 2) * HY + (j & 3)) * HX + fr) * P + fh * 16;
  }
  const int w_base = fr * P + fh * 16;

  u32x4_t hreg[HIT], wreg[WIT];
  auto tile_lim = [&](int z0, int y0, int x0) -> unsigned {
    const int lz = p.D - z0 - 1 < 511 ? p.D - z0 - 1 : 511, ly = p.H - y0 - 1 < 511 ? p.H - y0 - 1 : 511, lx = p.W - x0 - 1 < 511 ? p.W - x0 - 1 : 511;
    return ((unsigned)lz << 20) | ((unsigned)ly << 10) | (unsigned)lx | GUARD;
  };
  auto halo_piece = [&](const __amdgpu_buffer_rsrc_t& rs, int it, unsigned lim, unsigned org_b) -> u32x4_t {
    const bool ok = ((lim - h_zyx[it]) & GUARD) == GUARD;
    const unsigned voff = ok ? org_b + h_boff[it] : OOB;
    return __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0);
  };
  auto w_piece = [&](const __amdgpu_buffer_rsrc_t& rs, int it, int grp, int c0_b) -> u32x4_t {
    const int t0 = grp ? TC_TAP[1][2 * it] : TC_TAP[0][2 * it], t1 = grp ? TC_TAP[1][2 * it + 1] : TC_TAP[0][2 * it + 1];
    const int tap = w_s0 ? t1 : t0;
    asm volatile("" : "+v"(w_row));                  // (not hoisted back into loop-invariant registers)
    const unsigned voff = tap < 27 ? w_row + (unsigned)tap * w_tap : OOB;
    return __builtin_amdgcn_raw_buffer_load_b128(rs, voff, c0_b, 0);
  };
  auto tile_org = [&](int z0, int y0, int x0, int c0) -> unsigned {
    return (unsigned)((((long)(z0 * p.H + y0) * p.W + x0) * p.ldx + c0) * 4L);
  };

  const int id_begin = xcd_remap(blockIdx.x, gridDim.x) * p.ids_per_block;
  int id_end = id_begin + p.ids_per_block;
  if (id_end > p.ids_total) id_end = p.ids_total;
  int id = id_begin, tix = 0, tiy = 0, tiz = 0;
  while (id < id_end && !tile_coords(id, p.ntx, p.nty, p.ntz, tix, tiy, tiz)) ++id;
  if (id >= id_end) return;
  {
    const unsigned org = tile_org(tiz * TZ, tiy * TY, tix * TX, 0), lim = tile_lim(tiz * TZ, tiy * TY, tix * TX);
#pragma unroll
    for (int it = 0; it < HIT; ++it) hreg[it] = halo_piece(rs_x, it, lim, org);
#pragma unroll
    for (int it = 0; it < WIT; ++it) wreg[it] = w_piece(rs_w, it, 0, 0);
  }

  const bool accum = p.accum != 0;

  while (id < id_end) {
    const int x0 = tix * TX, y0 = tiy * TY, z0 = tiz * TZ;
    int nid = id + 1, ntix = 0, ntiy = 0, ntiz = 0;
    while (nid < id_end && !tile_coords(nid, p.ntx, p.nty, p.ntz, ntix, ntiy, ntiz)) ++nid;
    const bool has_next = nid < id_end;

#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      f32x16_t acc[4][2];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[c][i][e] = 0.f;

      for (int cc = 0; cc < nchunks; ++cc) {
        __syncthreads();                       // all waves finished reading the previous halo / weights
        // the split happens here: one conversion per staged element, two 8-byte LDS stores per piece
#pragma unroll
        for (int it = 0; it < HIT; ++it)
          if (tid + 256 * it < HP) {
            uint2 hi, lo;
            split4(hreg[it], hi, lo);
            *reinterpret_cast<uint2*>(Hl + h_lds0 + it * 64 * P) = hi;
            *reinterpret_cast<uint2*>(Hl + h_lds0 + it * 64 * P + 32) = lo;
          }
#pragma unroll
        for (int it = 0; it < WIT; ++it) {
          uint2 hi, lo;
          split4(wreg[it], hi, lo);
          *reinterpret_cast<uint2*>(Wl + w_lds0 + it * W_LSTEP) = hi;
          *reinterpret_cast<uint2*>(Wl + w_lds0 + it * W_LSTEP + 32) = lo;
        }
        __syncthreads();
        // what to prefetch while this step computes: the next chunk of this pass, chunk 0 of the tile's second pass, or
        // chunk 0 / pass A of the next tile; through descriptors whose range is zero when there is nothing left (no branch)
        const bool same_pass = cc + 1 < nchunks;
        const bool same_tile = same_pass || grp == 0;
        const bool pref = same_tile || has_next;
        const int pz = same_tile ? z0 : ntiz * TZ, py = same_tile ? y0 : ntiy * TY, px = same_tile ? x0 : ntix * TX;
        const int pc0 = same_pass ? (cc + 1) * CK : 0;
        const int pgrp = same_pass ? grp : 1 - grp;
        const __amdgpu_buffer_rsrc_t rs_xp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, pref ? p.xbytes : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_wp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wb), 0, pref ? p.wbytes : 0, 0x00020000);
        const unsigned porg = tile_org(pz, py, px, pc0), plim = tile_lim(pz, py, px);
        const int pc0_b = pc0 * 4;

        uint4 wv[2][2], xv[2][2][2];           // fragments one pair (weights) / one delta (voxels) ahead: [.][0] = hi, [.][1] = lo
        auto rd_w = [&](int k, int bf) {
#pragma unroll
          for (int hl = 0; hl < 2; ++hl) wv[bf][hl] = *reinterpret_cast<const uint4*>(Wl + w_base + k * 32 * P + hl * 32);
        };
        auto rd_x = [&](int di, int bf) {
          const int doff = ((((di >> 2) & 1) * HY + ((di >> 1) & 1)) * HX + (di & 1)) * P;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int hl = 0; hl < 2; ++hl) xv[bf][i][hl] = *reinterpret_cast<const uint4*>(Hl + a_base[i] + doff + hl * 32);
        };
        rd_x(0, 0);
        rd_w(0, 0);
        constexpr int NPMAX = 14;
#pragma unroll
        for (int k = 0; k < NPMAX; ++k) {
          if (k >= TC_NP[grp]) continue;         // (compile time: grp and k are unrolled)
          const int di = TC_DELTA[grp][k], lc = TC_LCLS[grp][k];
          if (k + 1 < TC_NP[grp]) {
            rd_w(k + 1, (k + 1) & 1);
            if (TC_DELTA[grp][k + 1] != di) rd_x(TC_DELTA[grp][k + 1], TC_DELTA[grp][k + 1] & 1);
          }
          // prefetch pieces: 15 per step over 13 / 14 pairs (one per pair, the last ones two)
          if (k < WIT) wreg[k] = w_piece(rs_wp, k, pgrp, pc0_b);
          else if (k - WIT < HIT) hreg[k - WIT] = halo_piece(rs_xp, k - WIT, plim, porg);
          if (k == TC_NP[grp] - 1) {
#pragma unroll
            for (int r = TC_NP[grp] - WIT; r < HIT; ++r) hreg[r] = halo_piece(rs_xp, r, plim, porg);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[lc][i] = mma3(wv[k & 1][0], wv[k & 1][1], xv[di & 1][i][0], xv[di & 1][i][1], acc[lc][i]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // ---- epilogue of this pass's 4 classes: lane = one coarse voxel of each M-tile, 4 groups of 4 consecutive channels ----
      const bool has_bias = p.bias != nullptr;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int j = wid * 2 + i;
        const int cz = z0 + (j >> 2), cy = y0 + (j & 3), cx = x0 + fr;
        const bool cin = cz < p.D && cy < p.H && cx < p.W;
        const bool vz1 = 2 * cz + 1 < p.Do, vy1 = 2 * cy + 1 < p.Ho, vx1 = 2 * cx + 1 < p.Wo;      // (odd fine sizes: the last odd plane is absent)
        const long vbase = ((long)(2 * cz * p.Ho + 2 * cy) * p.Wo + 2 * cx) * p.ldy + n0;         // fine voxel (2cz, 2cy, 2cx)
#pragma unroll
        for (int lc = 0; lc < 4; ++lc) {
          __builtin_amdgcn_sched_barrier(0);     // one class at a time: interleaved, the 8 unrolled instances spill
          const int cls = TC_CLS[grp][lc];
          const bool valid = cin && (!(cls & 4) || vz1) && (!(cls & 2) || vy1) && (!(cls & 1) || vx1);
          const long voff = vbase + ((long)(((cls >> 2) & 1) * p.Ho + ((cls >> 1) & 1)) * p.Wo + (cls & 1)) * p.ldy;
          float* dst = yb + voff + 4 * fh;
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            float of[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) of[q] = acc[lc][i][g4 * 4 + q];
            if (has_bias) {                        // (uniform)
#pragma unroll
              for (int q = 0; q < 4; ++q) of[q] += p.bias[b * p.bsb + n0 + 8 * g4 + 4 * fh + q];
            }
            float4 old = make_float4(0.f, 0.f, 0.f, 0.f);
            if (accum && valid) old = *reinterpret_cast<const float4*>(dst + 8 * g4);
            const float o[4] = {of[0] + old.x, of[1] + old.y, of[2] + old.z, of[3] + old.w};
            if (valid) *reinterpret_cast<float4*>(dst + 8 * g4) = make_float4(o[0], o[1], o[2], o[3]);
          }
        }
      }
    }
    id = nid; tix = ntix; tiy = ntiy; tiz = ntiz;
  }
}

bool conv_split_tconv_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  return conv_f32_tconv_problem(d, x, y);
}

int conv_split_tconv(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                     hipStream_t s, int accum) {
  COMA_CHECK(conv_split_tconv_ok(d, x, y), "conv_split_tconv: problem not in the split kernel's scope");
  COMA_CHECK(aligned16(x->data) && aligned16(y->data) && aligned16(wk), "conv_split_tconv: operands must be 16-byte aligned");
  SplitTconvP q;
  q.x = (const float*)x->data; q.ldx = (int)x->ld; q.sbx = x->sb; q.D = x->D; q.H = x->H; q.W = x->W; q.C = x->C;
  q.y = (float*)y->data; q.ldy = (int)y->ld; q.sby = y->sb; q.Do = y->D; q.Ho = y->H; q.Wo = y->W; q.N = y->C;
  q.w = (const float*)wk; q.wsb = d->per_sample_w ? 27L * y->C * x->C : 0;
  q.bias = bias; q.bsb = d->per_sample_w ? y->C : 0;
  const unsigned long long wb_ = 27ull * y->C * x->C * 4;
  COMA_CHECK(wb_ < 0x7fff0000ull, "conv_split_tconv: weight set too large for 32-bit buffer offsets");
  q.xbytes = (unsigned)((unsigned long long)t_vox(x) * x->ld * 4);
  q.wbytes = (unsigned)wb_;
  q.accum = accum;
  const int nblk_n = y->C / 32;
  const TileRun r = tile_run(q.D, q.H, q.W, 32, 4, 2, 512, nblk_n * x->B);      // one block per CU, about two rounds
  q.ntx = r.ntx; q.nty = r.nty; q.ntz = r.ntz; q.ids_total = r.ids_total; q.ids_per_block = r.ids_per_block;
  set_max_lds<conv_split_tconv_k>();
  const size_t lds = (size_t)(33 * 5 * 3 + 14 * 32) * 80;
  coma_set_kernel_tag("conv_split_tconv_k");
  hipLaunchKernelGGL(conv_split_tconv_k, dim3((unsigned)r.gx, (unsigned)nblk_n, (unsigned)x->B), dim3(256), lds, s, q);
  COMA_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================
// conv_split_wgrad_k, conv_split_wgrad2_k<FORM> -- the 3x3x3 weight gradients: one body, split_wgrad_body<S, FORM>, behind
// the two entry points.  dwk[b][tap][n][c] += sum_m dy[.][n] * x[.][c], the reduction index is the voxel m of the DENSE
// operand's grid; dense voxel m pairs with GATHERED voxel S m + tap - 1.
// The frame of conv_f32_wgrad16_k<S, FORM> (a block owns a 32 x 32 (n, c) weight tile and a run of dense tiles, 2 x 4 x 32
// voxels at S = 1, 1 x 2 x 32 at S = 2; the dense tile and its gathered region, 4 x 6 x 34 = 816 rows / 3 x 5 x 65 = 975
// rows, are staged by buffer loads, the next tile's pieces in flight while this one computes) with the MFMA body of
// conv_mfma_wgrad_k<1, 1, 0>: both operands are [voxel][32 channels] bf16 images (64-byte rows) read transposed with
// ds_read_b64_tr_b16, the 27 taps are dealt to the 4 waves (7, 7, 7, 6) whose 32 x 32 fp32 accumulators stay in registers
// over the block's tiles and merge into dwk with fp32 atomics at the end.  Each image exists twice (hi, lo): together the
// bytes of the fp32 images of conv_f32_wgrad16_k (134 KB / 133 KB).  The stride lives in the lanes' row addresses.
// FORM 0: convolution (dense dy -> MFMA rows n, gathered x -> columns c); at S = 1 both operands lie on one grid.
// FORM 1: transposed stride-2 convolution (dense x -> columns c, gathered dy -> rows n).
// =====================================================================================
struct SplitWgradP {
  const float* dn; int ldd; long sbd; int Mz, My, Mx;      // dense operand (S = 2: on the coarse grid)
  const float* ga; int ldg; long sbg; int Gz, Gy, Gx;      // gathered operand (S = 2: on the fine grid)
  int N, C;
  unsigned dbytes, gbytes;
  int ntx, nty, ntz, ids_total, ids_per_block, cblocks;
  float* dwk; long wsb;
};

// tile constants shared by the body and its launcher
template <int S> struct SplitWgradTile {
  static constexpr int TX = 32, TY = S == 1 ? 4 : 2, TZ = S == 1 ? 2 : 1, TM = TX * TY * TZ;                     // dense tile
  static constexpr int HX = S * (TX - 1) + 3, HY = S * (TY - 1) + 3, HZ = S * (TZ - 1) + 3, HV = HX * HY * HZ;   // gathered region
  static constexpr int PR = 64;                         // LDS row pitch (bytes): 32 bf16 channels
  static constexpr int LDS = 2 * (HV + TM) * PR;        // four images: gathered hi / lo, dense hi / lo
};

// (p by value: behind a reference the compiler no longer keeps the merge's tap * N * C address terms in scalar registers)
template <int S, int FORM>
__device__ __forceinline__ void split_wgrad_body(const SplitWgradP p) {
  using T = SplitWgradTile<S>;
  constexpr int TX = T::TX, TY = T::TY, TZ = T::TZ, TM = T::TM, HX = T::HX, HY = T::HY, HV = T::HV, PR = T::PR;
  constexpr int HIT = (HV * 8 + 255) / 256, DIT = TM * 8 / 256, NIT = HIT + DIT;      // 16-byte fp32 pieces per thread: 26 + 8 / 31 + 2
  constexpr int MAXT = 7;                               // taps per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Gh = smem;                                      // [HV][64] gathered hi
  char* Gl = Gh + HV * PR;                              //          gathered lo
  char* Dh = Gl + HV * PR;                              // [TM][64] dense hi
  char* Dl = Dh + TM * PR;                              //          dense lo
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z;
  const int n0 = (blockIdx.y / p.cblocks) * 32, c0 = (blockIdx.y % p.cblocks) * 32;
  const int dch0 = FORM == 0 ? n0 : c0, gch0 = FORM == 0 ? c0 : n0;      // channel block of the dense / gathered operand
  const int dchn = FORM == 0 ? p.N : p.C, gchn = FORM == 0 ? p.C : p.N;
  const float* dnb = p.dn + (long)b * p.sbd + dch0;
  const float* gab = p.ga + (long)b * p.sbg + gch0;
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gab), 0, p.gbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dnb), 0, p.dbytes, 0x00020000);
  constexpr unsigned OOB = 0x7fff0000u;

  // staging: piece = tid + 256 it -> (row = piece >> 3, 4-channel piece = tid & 7); gathered positions relative to
  // S * tile origin - 1, dense positions relative to the tile origin - 1.  A piece outside its volume or past the tensor's
  // channels (partial 32-channel block) reads as zero: it never touches the neighbouring slice.
  const int chq = (tid & 7) * 4;
  const unsigned choff = (unsigned)(chq * 4);
  const bool ch_g = gch0 + chq < gchn, ch_d = dch0 + chq < dchn;
  int s_pos[NIT];                                       // packed z | y << 4 | x << 8
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (it < HIT) {
      const int row = (tid + 256 * it) >> 3;
      const int hx = row % HX, hy = (row / HX) % HY, hz = row / (HX * HY);
      s_pos[it] = row < HV ? (hz | (hy << 4) | (hx << 8)) : (15 | (15 << 4) | (1023 << 8));
    } else {
      const int row = (tid + 256 * (it - HIT)) >> 3;
      s_pos[it] = ((row / (TY * 32)) + 1) | ((((row >> 5) % TY) + 1) << 4) | (((row & 31) + 1) << 8);
    }
  }
  uint4 sreg[NIT];
  auto issue_all = [&](int z0, int y0, int x0, const __amdgpu_buffer_rsrc_t& rg, const __amdgpu_buffer_rsrc_t& rd) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int sc = it < HIT ? S : 1;
      const int gz = sc * z0 - 1 + (s_pos[it] & 15), gy = sc * y0 - 1 + ((s_pos[it] >> 4) & 15), gx = sc * x0 - 1 + (s_pos[it] >> 8);
      const bool ok = it < HIT ? ((unsigned)gz < (unsigned)p.Gz && (unsigned)gy < (unsigned)p.Gy && (unsigned)gx < (unsigned)p.Gx && ch_g)
                               : ((unsigned)gz < (unsigned)p.Mz && (unsigned)gy < (unsigned)p.My && (unsigned)gx < (unsigned)p.Mx && ch_d);
      const unsigned off = it < HIT ? (unsigned)(((gz * p.Gy + gy) * p.Gx + gx) * p.ldg) * 4u + choff
                                    : (unsigned)(((gz * p.My + gy) * p.Mx + gx) * p.ldd) * 4u + choff;
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(it < HIT ? rg : rd, ok ? off : OOB, 0, 0);
      sreg[it] = make_uint4(v[0], v[1], v[2], v[3]);
    }
  };
  auto store_tile = [&]() __attribute__((always_inline)) {      // the split: one conversion per staged element
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      uint2 hi, lo;
      split4(sreg[it], hi, lo);
      if (it < HIT) {
        const int piece = tid + 256 * it;
        if ((piece >> 3) < HV) { *reinterpret_cast<uint2*>(Gh + piece * 8) = hi; *reinterpret_cast<uint2*>(Gl + piece * 8) = lo; }
      } else {
        const int piece = tid + 256 * (it - HIT);
        *reinterpret_cast<uint2*>(Dh + piece * 8) = hi; *reinterpret_cast<uint2*>(Dl + piece * 8) = lo;
      }
    }
  };

  f32x16_t acc[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  // per-wave tap list (wave-uniform): tap = wid + 4 t; byte offset of the tap's shift in the gathered image
  int toff_w[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int tap = wid + 4 * t;
    const int kx = tap % 3, ky = (tap / 3) % 3, kz = tap / 9;
    toff_w[t] = __builtin_amdgcn_readfirstlane(((kz * HY + ky) * HX + kx) * PR);
  }
  const bool last_tap = wid + 4 * (MAXT - 1) < 27;      // (wave 3 has six taps)
  // lane roles of the transposed reads (as conv_mfma_wgrad_k): a 16-lane group covers 4 voxels x 16 channels per read
  const int g16 = lane >> 4, li = lane & 15, q4 = li >> 2, pp = li & 3;
  const int chan_b = ((g16 & 1) * 16 + 4 * pp) * 2;     // byte offset of this lane's 4 channels in the 32-channel row
  const int vrow = 8 * (g16 >> 1) + q4;                 // voxel (within a 16-voxel K step) whose row this lane addresses

  const int id_begin = xcd_remap(blockIdx.x, gridDim.x) * p.ids_per_block;
  int id_end = id_begin + p.ids_per_block;
  if (id_end > p.ids_total) id_end = p.ids_total;
  int id = id_begin, tix = 0, tiy = 0, tiz = 0;
  while (id < id_end && !tile_coords(id, p.ntx, p.nty, p.ntz, tix, tiy, tiz)) ++id;
  if (id >= id_end) return;
  issue_all(tiz * TZ, tiy * TY, tix * TX, rs_g, rs_d);
  while (id < id_end) {
    int nid = id + 1, ntix = 0, ntiy = 0, ntiz = 0;
    while (nid < id_end && !tile_coords(nid, p.ntx, p.nty, p.ntz, ntix, ntiy, ntiz)) ++nid;
    const bool has_next = nid < id_end;
    const __amdgpu_buffer_rsrc_t rn_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gab), 0, has_next ? p.gbytes : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rn_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dnb), 0, has_next ? p.dbytes : 0, 0x00020000);
    __syncthreads();
    store_tile();
    __syncthreads();
    issue_all(ntiz * TZ, ntiy * TY, ntix * TX, rn_g, rn_d);
    // TM / 16 K steps of 16 dense voxels (16 steps at S = 1, unrolled by 2; 4 at S = 2, unrolled): step ks = half an x row
    constexpr int KUNROLL = S == 1 ? 2 : TM / 16;
#pragma unroll KUNROLL
    for (int ks = 0; ks < TM / 16; ++ks) {
      const int r = ks >> 1, xh = (ks & 1) * 16 + vrow;                      // dense row (z, y) of the tile, x within it
      const int d1 = (r * 32 + xh) * PR + chan_b;
      const int g1 = (((S * (r / TY)) * HY + S * (r % TY)) * HX + S * xh) * PR + chan_b;   // the same voxel's tap (0, 0, 0) in the gathered image
      auto frag = [&](const char* base, int step) __attribute__((always_inline)) -> uint4 {
        const s4_t u = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(base));
        const s4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(base + step));
        const bf16x8_t f = (bf16x8_t){u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
        return *reinterpret_cast<const uint4*>(&f);
      };
      const uint4 dh = frag(Dh + d1, 4 * PR), dl = frag(Dl + d1, 4 * PR);
#pragma unroll
      for (int t = 0; t < MAXT; ++t) {
        if (t < MAXT - 1 || last_tap) {
          const uint4 gh = frag(Gh + g1 + toff_w[t], 4 * S * PR), gl = frag(Gl + g1 + toff_w[t], 4 * S * PR);
          acc[t] = FORM == 0 ? mma3(dh, dl, gh, gl, acc[t]) : mma3(gh, gl, dh, dl, acc[t]);
        }
      }
    }
    id = nid; tix = ntix; tiy = ntiy; tiz = ntiz;
  }
  // ---- merge into dwk[b][tap][n][c]: MFMA rows = n, columns = c ----
  float* wout = p.dwk + (long)b * p.wsb;
  const int fr = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    const int tap = wid + 4 * t;
    if (tap < 27) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = n0 + (e & 3) + 8 * (e >> 2) + 4 * fh, c = c0 + fr;
        if (n < p.N && c < p.C) atomicAdd(wout + ((long)tap * p.N + n) * p.C + c, acc[t][e]);
      }
    }
  }
}

__global__ __launch_bounds__(256, 1) void conv_split_wgrad_k(SplitWgradP p) { split_wgrad_body<1, 0>(p); }

template <int FORM>
__global__ __launch_bounds__(256, 1) void conv_split_wgrad2_k(SplitWgradP p) { split_wgrad_body<2, FORM>(p); }

// the problems conv_f32_wgrad16_k<1, 0> takes, plus partial 32-channel blocks (C, N multiples of 16)
bool conv_split_wgrad_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  return d->ksize == 3 && d->form == 0 && d->stride == 1 && d->pad == 1 && x->dtype == COMA_F32 && dy->dtype == COMA_F32 &&
         t_same_grid(x, dy) && x->W >= 32 && x->C >= 32 && dy->C >= 32 && x->C % 16 == 0 && dy->C % 16 == 0 &&
         x->ld % 4 == 0 && x->sb % 4 == 0 && dy->ld % 4 == 0 && dy->sb % 4 == 0 &&
         (!x->data || aligned16(x->data)) && (!dy->data || aligned16(dy->data)) &&
         (unsigned long long)t_vox(x) * x->ld * 4 < 0x7fff0000ull && (unsigned long long)t_vox(dy) * dy->ld * 4 < 0x7fff0000ull;
}

bool conv_split_wgrad2_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  const coma_tensor* dn = d->form == 0 ? dy : x;
  const coma_tensor* ga = d->form == 0 ? x : dy;
  // (the dense grid is the coarse one: every gathered row 2 m - 1 + tap of a dense voxel m is tested against the fine grid)
  return conv_f32_wgrad16s2_problem(d, x, dy) && d->pad == 1 && dn->B == ga->B &&
         ga->D <= 2 * dn->D && ga->H <= 2 * dn->H && ga->W <= 2 * dn->W;
}

template <int S, auto KERNEL>
static int launch_split_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, hipStream_t s, int zeroed) {
  using T = SplitWgradTile<S>;
  const coma_tensor* dn = d->form == 0 ? dy : x;
  const coma_tensor* ga = d->form == 0 ? x : dy;
  SplitWgradP q;
  q.dn = (const float*)dn->data; q.ldd = (int)dn->ld; q.sbd = dn->sb; q.Mz = dn->D; q.My = dn->H; q.Mx = dn->W;
  q.ga = (const float*)ga->data; q.ldg = (int)ga->ld; q.sbg = ga->sb; q.Gz = ga->D; q.Gy = ga->H; q.Gx = ga->W;
  q.N = dy->C; q.C = x->C;
  // (descriptor ranges are measured from the block's channel offset; the voxel and channel tests keep every piece inside)
  q.dbytes = (unsigned)((unsigned long long)t_vox(dn) * dn->ld * 4);
  q.gbytes = (unsigned)((unsigned long long)t_vox(ga) * ga->ld * 4);
  q.cblocks = (q.C + 31) / 32;
  const int pairs = q.cblocks * ((q.N + 31) / 32);
  // one block per CU, one round: a second round repeats the atomic merge
  const TileRun r = tile_run(q.Mz, q.My, q.Mx, T::TX, T::TY, T::TZ, 256, pairs * x->B);
  q.ntx = r.ntx; q.nty = r.nty; q.ntz = r.ntz; q.ids_total = r.ids_total; q.ids_per_block = r.ids_per_block;
  const long wsz1 = 27L * q.N * q.C, wsz = wsz1 * (d->per_sample_w ? x->B : 1);
  q.wsb = d->per_sample_w ? wsz1 : 0;
  q.dwk = dwk;
  if (!(zeroed & COMA_ZEROED_OUT) && hipMemsetAsync(dwk, 0, sizeof(float) * wsz, s) != hipSuccess) { coma_set_error("wgrad memset failed"); return 2; }
  set_max_lds<KERNEL>();
  if (S == 1) coma_set_kernel_tag("conv_split_wgrad_k");
  else coma_set_kernel_tag("conv_split_wgrad2_k<%d>", d->form);
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)r.gx, (unsigned)pairs, (unsigned)x->B), dim3(256), (size_t)T::LDS, s, q);
  COMA_LAUNCH_CHECK();
  return 0;
}

int conv_split_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, hipStream_t s, int zeroed) {
  COMA_CHECK(conv_split_wgrad_ok(d, x, dy), "conv_split_wgrad: problem not in the split kernel's scope");
  return launch_split_wgrad<1, conv_split_wgrad_k>(d, x, dy, dwk, s, zeroed);
}

int conv_split_wgrad2(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, hipStream_t s, int zeroed) {
  COMA_CHECK(conv_split_wgrad2_ok(d, x, dy), "conv_split_wgrad2: problem not in the split kernel's scope");
  return d->form == 0 ? launch_split_wgrad<2, conv_split_wgrad2_k<0>>(d, x, dy, dwk, s, zeroed)
                      : launch_split_wgrad<2, conv_split_wgrad2_k<1>>(d, x, dy, dwk, s, zeroed);
}

// =====================================================================================
// Thin split (algo = 6): the few-channel full-resolution layers (C <= 16 and N <= 16, or C <= 8 and N <= 32; W >= 32) -- the
// problems of conv_thin16f_k / conv_thin16f_wgrad_k -- on v_mfma_f32_16x16x32_bf16.
//
// conv_split_thin_k<CP, NB> -- forward / data gradient (`flip`), the structure of conv_thin16_k: the taps packed along K
// (K = 32 = 2 taps x 16 channels at CP = 16: 14 steps; 4 taps x 8 channels at CP = 8: 7 steps), 2 x 4 x 32-voxel tiles, four
// voxel groups of 16 per wave, persistent blocks, two per CU; staging by buffer loads (zero fill outside the volume), the next
// tile's pieces issued one per step inside the MFMA loop, channels that are not the tensor's masked before the split.
// The halo is TWO planes (hi, lo), each [816 rows][CP bf16] with the bf16 kernel's unpadded 32- / 16-byte row pitch, so a
// 16-lane group's 16-byte fragment reads cover consecutive rows (conflict-free); one interleaved [hi][lo] row of 64 bytes
// would put the group's lanes 64 bytes apart (4-way).  The weights sit in LDS as hi / lo FRAGMENTS in lane order
// ([step][block][64 lanes][16 bytes], 27 x 16 NB x CP x 4 bytes in all, the fp32 twin's byte count): one conflict-free 16-byte
// read per step, block and plane, shared by the wave's four voxel groups; in registers they would be 2 x 56 VGPRs next to
// 64 of voxel fragments and 52 of staging pieces.  Epilogue and fused statistics as conv_thin16f_k.
// =====================================================================================
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

struct SplitThinP {
  const float* x; int ldx; long sbx; int D, H, W, C;
  float* y; int ldy; long sby; int N;
  const float* w; long wsb;
  const float* bias; int bsb;
  int flip;
  unsigned xbytes;
  int ntx, nty, ntz, ids_total, ids_per_block;
  int st16;            // output rows allow aligned 16-byte (4-channel) stores
  double2* stats; int stats_inst;
};

template <int CP, int NB> struct SplitThinTile {
  static constexpr int HV = 34 * 6 * 4;
  static constexpr int TPM = 32 / CP, NM = (27 + TPM - 1) / TPM;      // taps per MFMA, MFMA steps per voxel group
  static constexpr int PLANE = HV * CP * 2;                           // one halo plane (bytes)
  static constexpr int WPLANE = NM * NB * 64 * 16;                    // one weight-fragment plane (bytes)
  static constexpr int LDS = 2 * PLANE + 2 * WPLANE;
};

template <int CP, int NB>      // CP = padded input channels per tap (16 or 8), NB = 16-channel output blocks (1 or 2)
__global__ __launch_bounds__(256, 2) void conv_split_thin_k(SplitThinP p) {
  using T = SplitThinTile<CP, NB>;
  constexpr int TX = 32, TY = 4, TZ = 2, HX = TX + 2, HY = TY + 2, HV = T::HV;
  constexpr int TPM = T::TPM, NM = T::NM;
  constexpr int P = CP * 2;                       // row pitch of a halo plane (bytes)
  constexpr int PCH = CP / 4;                     // 16-byte fp32 pieces per halo row
  constexpr int HP = HV * PCH, HIT = (HP + 255) / 256;
  static_assert(HIT <= NM, "one staging piece per MFMA step");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Hh = smem;                                // [HV][CP] bf16 hi
  char* Hl = smem + T::PLANE;                     //          lo
  char* Wh = smem + 2 * T::PLANE;                 // [NM][NB][64][8] bf16 hi
  char* Wl = Wh + T::WPLANE;                      //                 lo
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z;
  const int lv = lane & 15, lg = lane >> 4;       // voxel within the group / k group (A, B) = row group (D)
  const float* xb = p.x + (long)b * p.sbx;
  const float* wb = p.w + (long)b * p.wsb;
  float* yb = p.y + (long)b * p.sby;

  // ---- weights -> LDS fragments: lane (n = lv, k group lg) of step m holds w[tap][nb * 16 + n][8 channels] of its tap ----
  for (int e = tid; e < NM * NB * 512; e += 256) {
    const int j = e & 7, ln = (e >> 3) & 63, nb = (e >> 9) % NB, m = (e >> 9) / NB;
    const int flv = ln & 15, flg = ln >> 4;
    const int tap = m * TPM + (CP == 16 ? flg >> 1 : flg), c = (CP == 16 ? 8 * (flg & 1) : 0) + j, n = nb * 16 + flv;
    const int wt = p.flip ? 26 - tap : tap;
    const bool ok = tap < 27 && n < p.N && c < p.C;
    const float v = ok ? wb[((long)wt * p.N + n) * p.C + c] : 0.f;
    const bf16_t h = static_cast<bf16_t>(v);
    reinterpret_cast<bf16_t*>(Wh)[e] = h;
    reinterpret_cast<bf16_t*>(Wl)[e] = static_cast<bf16_t>(v - static_cast<float>(h));
  }
  // ---- B-fragment bases: this wave's first voxel group, this lane's voxel, its tap in step m, its channel half ----
  const int tsub = CP == 16 ? lg >> 1 : lg, cofs = CP == 16 ? 8 * (lg & 1) : 0;
  const int gz = wid >> 1, gy0 = 2 * (wid & 1);
  int abase[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const int tap = m * TPM + tsub < 27 ? m * TPM + tsub : 0;       // (padding taps have zero weights: read tap 0)
    const int kx = tap % 3, ky = (tap / 3) % 3, kz = tap / 9;
    abase[m] = (((gz + kz) * HY + gy0 + ky) * HX + lv + kx) * P + cofs * 2;
  }
  const int wfrag = lane * 16;                    // + (m * NB + nb) * 1024
  // ---- staging descriptors: piece = tid + 256 it -> halo row piece / PCH, 4-channel quarter piece % PCH (a per-thread
  // constant); the piece's 8 bytes of either plane sit at piece * 8 ----
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, p.xbytes, 0x00020000);
  constexpr unsigned OOB = 0x7fff0000u;
  int h_pos[HIT];                                 // hz | hy << 8 | hx << 16
  unsigned h_boff[HIT];
#pragma unroll
  for (int it = 0; it < HIT; ++it) {
    const int piece = tid + 256 * it;
    const int row = piece / PCH, ch = piece % PCH;
    const int hx = row % HX, hy = (row / HX) % HY, hz = row / (HX * HY);
    h_pos[it] = piece < HP ? (hz | (hy << 8) | (hx << 16)) : (255 | (255 << 8) | (4095 << 16));
    h_boff[it] = (unsigned)((((hz * p.H + hy) * p.W + hx) * p.ldx + ch * 4) * 4);
  }
  const int nval = p.C - 4 * (tid % PCH);
  const uint4 hmask = make_uint4(nval > 0 ? ~0u : 0u, nval > 1 ? ~0u : 0u, nval > 2 ? ~0u : 0u, nval > 3 ? ~0u : 0u);
  uint4 hreg[HIT];
  auto issue = [&](int it, int z0, int y0, int x0, const __amdgpu_buffer_rsrc_t& rs) __attribute__((always_inline)) {
    const bool ok = (unsigned)(z0 - 1 + (h_pos[it] & 255)) < (unsigned)p.D && (unsigned)(y0 - 1 + ((h_pos[it] >> 8) & 255)) < (unsigned)p.H &&
                    (unsigned)(x0 - 1 + (h_pos[it] >> 16)) < (unsigned)p.W;
    const unsigned org_b = (unsigned)((((long)((z0 - 1) * p.H + (y0 - 1)) * p.W + (x0 - 1)) * p.ldx) * 4);   // (mod 2^32: a valid piece's sum is its true offset)
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? org_b + h_boff[it] : OOB, 0, 0);
    hreg[it] = make_uint4(v[0], v[1], v[2], v[3]);
  };
  // the split happens here: one conversion per staged element, one 8-byte store per piece and plane
  auto store_halo = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < HIT; ++it)
      if (tid + 256 * it < HP) {
        uint4 v = hreg[it];
        v.x &= hmask.x; v.y &= hmask.y; v.z &= hmask.z; v.w &= hmask.w;
        uint2 hi, lo;
        split4(v, hi, lo);
        *reinterpret_cast<uint2*>(Hh + (tid + 256 * it) * 8) = hi;
        *reinterpret_cast<uint2*>(Hl + (tid + 256 * it) * 8) = lo;
      }
  };

  const int id_begin = xcd_remap(blockIdx.x, gridDim.x) * p.ids_per_block;
  int id_end = id_begin + p.ids_per_block;
  if (id_end > p.ids_total) id_end = p.ids_total;
  int id = id_begin, tix = 0, tiy = 0, tiz = 0;
  while (id < id_end && !tile_coords(id, p.ntx, p.nty, p.ntz, tix, tiy, tiz)) ++id;
  const bool do_stats = p.stats != nullptr;
  float st_s[NB][4], st_q[NB][4], bv[NB][4];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = nb * 16 + 4 * lg + j;
      st_s[nb][j] = 0.f; st_q[nb][j] = 0.f;
      bv[nb][j] = (p.bias && n < p.N) ? p.bias[b * p.bsb + n] : 0.f;
    }
  if (id < id_end) {
#pragma unroll
    for (int it = 0; it < HIT; ++it) issue(it, tiz * TZ, tiy * TY, tix * TX, rs_x);
  }
  while (id < id_end) {
    const int x0 = tix * TX, y0 = tiy * TY, z0 = tiz * TZ;
    int nid = id + 1, ntix = 0, ntiy = 0, ntiz = 0;
    while (nid < id_end && !tile_coords(nid, p.ntx, p.nty, p.ntz, ntix, ntiy, ntiz)) ++nid;
    const bool has_next = nid < id_end;
    // nothing to prefetch after the last tile: a zero-range descriptor makes every piece read as zero (no branch in the loop)
    const __amdgpu_buffer_rsrc_t rs_n = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, has_next ? p.xbytes : 0, 0x00020000);
    __syncthreads();                       // the previous tile's fragment reads are done (first tile: the weight image is complete)
    store_halo();
    __syncthreads();
    f32x4_t acc[4][NB];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[q][nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // fragments one step ahead: the four voxel groups' rows and the step's weights, hi and lo
    uint4 xh[2][4], xl[2][4], wh[2][NB], wl[2][NB];
    auto rd = [&](int m, int bf) __attribute__((always_inline)) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int off = abase[m] + ((q >> 1) * HX + (q & 1) * 16) * P;
        xh[bf][q] = *reinterpret_cast<const uint4*>(Hh + off);
        xl[bf][q] = *reinterpret_cast<const uint4*>(Hl + off);
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        wh[bf][nb] = *reinterpret_cast<const uint4*>(Wh + wfrag + (m * NB + nb) * 1024);
        wl[bf][nb] = *reinterpret_cast<const uint4*>(Wl + wfrag + (m * NB + nb) * 1024);
      }
    };
    rd(0, 0);
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      if (m + 1 < NM) rd(m + 1, (m + 1) & 1);
      if (m < HIT) issue(m, ntiz * TZ, ntiy * TY, ntix * TX, rs_n);      // one staging piece of the next tile per step
      __builtin_amdgcn_sched_barrier(0);
      // lo x hi, hi x lo, hi x hi (small terms first); the 4 NB accumulators of a term are independent
#pragma unroll
      for (int term = 0; term < 3; ++term)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const uint4& a = term == 0 ? wl[m & 1][nb] : wh[m & 1][nb];
            const uint4& f = term == 1 ? xl[m & 1][q] : xh[m & 1][q];
            acc[q][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&a), *reinterpret_cast<const bf16x8_t*>(&f),
                                                                 acc[q][nb], 0, 0, 0);
          }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- epilogue: lane = voxel lv of group q, output channels nb * 16 + 4 lg + 0..3 ----
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int vz = z0 + gz, vy = y0 + gy0 + (q >> 1), vx = x0 + (q & 1) * 16 + lv;
      const bool valid = vz < p.D && vy < p.H && vx < p.W;
      float* vox = yb + ((long)(vz * p.H + vy) * p.W + vx) * p.ldy;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int n = nb * 16 + 4 * lg;
        if (n >= p.N) continue;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = acc[q][nb][j] + bv[nb][j];
          if (do_stats) { const float r = valid ? o[j] : 0.f; st_s[nb][j] += r; st_q[nb][j] = fmaf(r, r, st_q[nb][j]); }
        }
        if (valid) {
          if (p.st16 && n + 3 < p.N) *reinterpret_cast<float4*>(vox + n) = make_float4(o[0], o[1], o[2], o[3]);
          else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < p.N) vox[n + j] = o[j];
          }
        }
      }
    }
    id = nid; tix = ntix; tiy = ntiy; tiz = ntiz;
  }
  // ---- fused statistics (as conv_thin16f_k): the 16 voxel lanes of a row group -> wave -> block (LDS) -> record ----
  if (do_stats) {
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);          // [4 waves][32 ch][2]
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float a = st_s[nb][j], c = st_q[nb][j];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
        if (lv == 0) { red[(wid * 32 + nb * 16 + 4 * lg + j) * 2] = a; red[(wid * 32 + nb * 16 + 4 * lg + j) * 2 + 1] = c; }
      }
    __syncthreads();
    if (tid < NB * 16 && tid < p.N) {
      double a = 0.0, c = 0.0;
      for (int w = 0; w < 4; ++w) { a += (double)red[(w * 32 + tid) * 2]; c += (double)red[(w * 32 + tid) * 2 + 1]; }
      const int g = p.stats_inst ? b : 0;
      stat_add(p.stats, p.stats_inst ? p.stats_inst : 1, p.N, g, tid, a, c);
    }
  }
}

bool conv_split_thin_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  return conv_f32_thin_problem(d, x, y);
}

int conv_split_thin(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                    hipStream_t s, double2* stats, int stats_inst, int* stats_chunks) {
  COMA_CHECK(conv_split_thin_ok(d, x, y), "conv_split_thin: problem not in the split kernel's scope");
  SplitThinP q;
  q.x = (const float*)x->data; q.ldx = (int)x->ld; q.sbx = x->sb; q.D = x->D; q.H = x->H; q.W = x->W; q.C = x->C;
  q.y = (float*)y->data; q.ldy = (int)y->ld; q.sby = y->sb; q.N = y->C;
  q.w = (const float*)wk; q.wsb = d->per_sample_w ? 27L * y->C * x->C : 0;
  q.bias = bias; q.bsb = d->per_sample_w ? y->C : 0;
  q.flip = d->form == 1;
  q.xbytes = (unsigned)((unsigned long long)t_vox(x) * x->ld * 4);
  q.st16 = y->ld % 4 == 0 && y->sb % 4 == 0 && aligned16(y->data);
  const TileRun r = tile_run(q.D, q.H, q.W, 32, 4, 2, 512, x->B);      // two blocks per CU, one round
  q.ntx = r.ntx; q.nty = r.nty; q.ntz = r.ntz; q.ids_total = r.ids_total; q.ids_per_block = r.ids_per_block;
  q.stats = nullptr; q.stats_inst = stats_inst;
  if (stats) { q.stats = stats; *stats_chunks = 1; }
  const dim3 grid((unsigned)r.gx, 1, (unsigned)x->B);
  const int cp = q.C > 8 ? 16 : 8, nb = q.N > 16 ? 2 : 1;      // (C <= 4 runs the CP = 8 variant)
  coma_set_kernel_tag("conv_split_thin_k<%d, %d>", cp, nb);
#define SPLIT_THIN(CP_, NB_) do { set_max_lds<conv_split_thin_k<CP_, NB_>, 80>(); \
    hipLaunchKernelGGL((conv_split_thin_k<CP_, NB_>), grid, dim3(256), (size_t)(SplitThinTile<CP_, NB_>::LDS), s, q); } while (0)
  if (cp == 16) SPLIT_THIN(16, 1);
  else if (nb == 2) SPLIT_THIN(8, 2);
  else SPLIT_THIN(8, 1);
#undef SPLIT_THIN
  COMA_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================
// conv_split_thin_wgrad_k<CP, NB> -- weight gradient of the same layers, the structure of conv_thin16_wgrad_k: the VOXELS
// along K (32 per MFMA), rows = 16 output channels from the dense dy tile, columns = 16 = TPM taps x CP channels from the x
// halo (27 column tiles at CP = 16, 14 at CP = 8), both operands voxel-major in LDS and read transposed with
// ds_read_b64_tr_b16, all column tiles' accumulators stationary over the block's tiles.  Four images: x hi / lo
// ([816 + 2][CP] bf16) and dy hi / lo ([256][16 NB] bf16), split once when staged.  Merge as the exact kernel: the four
// waves add up in LDS, one fp32 atomic per weight into one of `nrep` replicas, wgrad_replica_sum behind the kernel.
// CP = 16: 108 accumulator + 68 staging + 64 fragment registers: one block per CU (as conv_thin16f_wgrad_k<16, 1>); so is
// <8, 2> (112 + 60 + 64: at two blocks per CU it spilled 55 registers).
// =====================================================================================
struct SplitThinWP {
  const float* x; int ldx; long sbx; int D, H, W, C;
  const float* dy; int ldn; long sbn; int N;
  unsigned xbytes, dbytes;
  int ntx, nty, ntz, ids_total, ids_per_block;
  float* dwk; long wsb;
  int nrep; long rep_stride;
};

template <int CP, int NB> struct SplitThinWTile {
  static constexpr int HV = 34 * 6 * 4, TM = 256;
  static constexpr int TPM = 16 / CP, NM = (27 + TPM - 1) / TPM;
  static constexpr int XPL = (HV + 2) * CP * 2, DPL = TM * NB * 16 * 2;      // one x / dy plane (bytes)
  static constexpr int IMG = 2 * XPL + 2 * DPL, RED = NM * NB * 256 * 4;
  static constexpr int LDS = IMG > RED ? IMG : RED;
};

template <int CP, int NB>
__global__ __launch_bounds__(256, CP == 16 || NB == 2 ? 1 : 2) void conv_split_thin_wgrad_k(SplitThinWP p) {
  using T = SplitThinWTile<CP, NB>;
  constexpr int TX = 32, TY = 4, TZ = 2, HX = TX + 2, HY = TY + 2, HV = T::HV, TM = T::TM;
  constexpr int TPM = T::TPM, NM = T::NM;
  constexpr int ND = NB * 16;                        // bf16 per dense dy row
  constexpr int PX = CP * 2, PD = ND * 2;            // row pitches of a plane (bytes)
  constexpr int PCH = CP / 4, DCH = ND / 4;          // 16-byte fp32 pieces per halo / dense row
  constexpr int HP = HV * PCH, DP = TM * DCH, HIT = (HP + 255) / 256, DIT = DP / 256, NIT = HIT + DIT;
  constexpr int RING = CP == 16 || NB == 2 ? 8 : 4;  // B fragment pairs in flight
  constexpr int NPAIR = 2 * NM;
  static_assert(NIT <= NPAIR, "one staging piece per MFMA step");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Xh = smem;                                   // [HV + 2][CP] bf16 hi
  char* Xl = smem + T::XPL;                          //              lo
  char* Dh = smem + 2 * T::XPL;                      // [TM][ND] bf16 hi
  char* Dl = Dh + T::DPL;                            //               lo
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z;
  const int lv = lane & 15, lg = lane >> 4;
  const float* xb = p.x + (long)b * p.sbx;
  const float* db = p.dy + (long)b * p.sbn;
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, p.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(db), 0, p.dbytes, 0x00020000);
  constexpr unsigned OOB = 0x7fff0000u;

  // ---- staging descriptors: pieces 0..HIT-1 = x halo, HIT.. = dense dy; positions relative to the tile origin - 1, packed
  // z | y << 4 | x << 8; a piece's 8 bytes of either plane sit at piece * 8 ----
  int s_pos[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (it < HIT) {
      const int row = (tid + 256 * it) / PCH;
      const int hx = row % HX, hy = (row / HX) % HY, hz = row / (HX * HY);
      s_pos[it] = row < HV ? (hz | (hy << 4) | (hx << 8)) : (15 | (15 << 4) | (4095 << 8));
    } else {
      const int row = (tid + 256 * (it - HIT)) / DCH;
      s_pos[it] = ((row >> 7) + 1) | ((((row >> 5) & 3) + 1) << 4) | (((row & 31) + 1) << 8);
    }
  }
  const unsigned xoffb = (unsigned)((tid % PCH) * 16), doffb = (unsigned)((tid % DCH) * 16);
  const int xval = p.C - 4 * (tid % PCH), dval = p.N - 4 * (tid % DCH);
  const uint4 xmask = make_uint4(xval > 0 ? ~0u : 0u, xval > 1 ? ~0u : 0u, xval > 2 ? ~0u : 0u, xval > 3 ? ~0u : 0u);
  const uint4 dmask = make_uint4(dval > 0 ? ~0u : 0u, dval > 1 ? ~0u : 0u, dval > 2 ? ~0u : 0u, dval > 3 ? ~0u : 0u);
  uint4 sreg[NIT];
  auto issue = [&](int it, int z0, int y0, int x0, const __amdgpu_buffer_rsrc_t& rx, const __amdgpu_buffer_rsrc_t& rd) __attribute__((always_inline)) {
    const int gz = z0 - 1 + (s_pos[it] & 15), gy = y0 - 1 + ((s_pos[it] >> 4) & 15), gx = x0 - 1 + (s_pos[it] >> 8);
    const bool ok = (unsigned)gz < (unsigned)p.D && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
    const unsigned off = (unsigned)(((gz * p.H + gy) * p.W + gx) * (it < HIT ? p.ldx : p.ldn)) * 4u + (it < HIT ? xoffb : doffb);
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(it < HIT ? rx : rd, ok ? off : OOB, 0, 0);
    sreg[it] = make_uint4(v[0], v[1], v[2], v[3]);
  };
  auto store_tile = [&]() __attribute__((always_inline)) {      // the split: one conversion per staged element
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      uint4 v = sreg[it];
      uint2 hi, lo;
      if (it < HIT) {
        v.x &= xmask.x; v.y &= xmask.y; v.z &= xmask.z; v.w &= xmask.w;
        split4(v, hi, lo);
        const int piece = tid + 256 * it;
        if (piece < HP) { *reinterpret_cast<uint2*>(Xh + piece * 8) = hi; *reinterpret_cast<uint2*>(Xl + piece * 8) = lo; }
      } else {
        v.x &= dmask.x; v.y &= dmask.y; v.z &= dmask.z; v.w &= dmask.w;
        split4(v, hi, lo);
        const int piece = tid + 256 * (it - HIT);
        *reinterpret_cast<uint2*>(Dh + piece * 8) = hi; *reinterpret_cast<uint2*>(Dl + piece * 8) = lo;
      }
    }
  };

  // ---- transposed-read addressing (as conv_thin16_wgrad_k): lane 4q+p of group lg supplies voxel x = 4 lg + q (+16 for the
  // second read), columns 4p.. ----
  const int gz = wid >> 1, gy0 = 2 * (wid & 1);
  const int q4 = lv >> 2, p4 = lv & 3;
  const int vx = 4 * lg + q4;
  const int d_addr = ((gz * 4 + gy0) * 32 + vx) * PD + 8 * p4;                                   // + row step s * 32 * PD, + 16 * PD second read, + nb * 32 bytes
  const int sub = (4 * p4) / CP, cin = (4 * p4) % CP;
  const int x_addr = ((gz * HY + gy0) * HX + vx) * PX + cin * 2;                                 // + s * HX * PX, + 16 * PX second read, + tap offset
  int toff[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const int t = TPM == 1 ? m : (m * TPM + sub < 27 ? m * TPM + sub : 0);    // (padding taps read tap 0: their columns are never stored)
    toff[m] = (((t / 9) * HY + (t / 3) % 3) * HX + t % 3) * PX;
  }
  f32x4_t acc[NM][NB];
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[m][nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int id_begin = xcd_remap(blockIdx.x, gridDim.x) * p.ids_per_block;
  int id_end = id_begin + p.ids_per_block;
  if (id_end > p.ids_total) id_end = p.ids_total;
  int id = id_begin, tix = 0, tiy = 0, tiz = 0;
  while (id < id_end && !tile_coords(id, p.ntx, p.nty, p.ntz, tix, tiy, tiz)) ++id;
  if (id < id_end) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) issue(it, tiz * TZ, tiy * TY, tix * TX, rs_x, rs_d);
  }
  while (id < id_end) {
    int nid = id + 1, ntix = 0, ntiy = 0, ntiz = 0;
    while (nid < id_end && !tile_coords(nid, p.ntx, p.nty, p.ntz, ntix, ntiy, ntiz)) ++nid;
    const bool has_next = nid < id_end;
    const __amdgpu_buffer_rsrc_t rn_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, has_next ? p.xbytes : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rn_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(db), 0, has_next ? p.dbytes : 0, 0x00020000);
    __syncthreads();
    store_tile();
    __syncthreads();
    // the sequence of (row step s, column tile m) pairs is unrolled; B fragments (hi and lo) run RING pairs ahead
    auto frag = [&](const char* src, int step) __attribute__((always_inline)) -> bf16x8_t {
      const s4_t u = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(src));
      const s4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(src + step));
      return (bf16x8_t){u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
    };
    bf16x8_t bh[RING], bl[RING], ah[2][NB], al[2][NB];
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        ah[s_][nb] = frag(Dh + d_addr + s_ * 32 * PD + nb * 32, 16 * PD);
        al[s_][nb] = frag(Dl + d_addr + s_ * 32 * PD + nb * 32, 16 * PD);
      }
#pragma unroll
    for (int pi = 0; pi < RING && pi < NPAIR; ++pi) {
      const int xo = x_addr + (pi / NM) * HX * PX + toff[pi % NM];
      bh[pi] = frag(Xh + xo, 16 * PX); bl[pi] = frag(Xl + xo, 16 * PX);
    }
#pragma unroll
    for (int pi = 0; pi < NPAIR; ++pi) {
      const int s_ = pi / NM, m = pi % NM;
      const bf16x8_t ch = bh[pi % RING], cl = bl[pi % RING];
      if (pi + RING < NPAIR) {
        const int xo = x_addr + ((pi + RING) / NM) * HX * PX + toff[(pi + RING) % NM];
        bh[pi % RING] = frag(Xh + xo, 16 * PX); bl[pi % RING] = frag(Xl + xo, 16 * PX);
      }
      if (pi < NIT) issue(pi, ntiz * TZ, ntiy * TY, ntix * TX, rn_x, rn_d);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int term = 0; term < 3; ++term)      // lo x hi, hi x lo, hi x hi
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          acc[m][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(term == 0 ? al[s_][nb] : ah[s_][nb], term == 1 ? cl : ch, acc[m][nb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    id = nid; tix = ntix; tiy = ntiy; tiz = ntiz;
  }
  // ---- merge (as conv_thin16f_wgrad_k): the four waves' tiles add up in LDS, then one fp32 atomic per weight into this
  // block's replica ----
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);                     // [NM][NB][16 n][16 col]
  for (int i = tid; i < NM * NB * 256; i += 256) red[i] = 0.f;
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&red[((m * NB + nb) * 16 + 4 * lg + j) * 16 + lv], acc[m][nb][j]);
  __syncthreads();
  float* wout = p.dwk + (long)b * p.wsb + (long)(blockIdx.x % (unsigned)p.nrep) * p.rep_stride;
  for (int i = tid; i < NM * NB * 256; i += 256) {
    const int col = i & 15, row = (i >> 4) & 15, nb = (i >> 8) % NB, m = i / (256 * NB);
    const int tap = m * TPM + col / CP, c = col % CP, n = nb * 16 + row;
    if (tap < 27 && n < p.N && c < p.C) atomicAdd(wout + ((long)tap * p.N + n) * p.C + c, red[i]);
  }
}

bool conv_split_thin_wgrad_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  return conv_f32_thin_wgrad_problem(d, x, dy);
}

int conv_split_thin_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, void* ws, size_t ws_bytes,
                          hipStream_t s, int zeroed) {
  COMA_CHECK(conv_split_thin_wgrad_ok(d, x, dy), "conv_split_thin_wgrad: problem not in the split kernel's scope");
  SplitThinWP q;
  q.x = (const float*)x->data; q.ldx = (int)x->ld; q.sbx = x->sb; q.D = x->D; q.H = x->H; q.W = x->W; q.C = x->C;
  q.dy = (const float*)dy->data; q.ldn = (int)dy->ld; q.sbn = dy->sb; q.N = dy->C;
  q.xbytes = (unsigned)((unsigned long long)t_vox(x) * x->ld * 4);
  q.dbytes = (unsigned)((unsigned long long)t_vox(dy) * dy->ld * 4);
  const int cp = q.C > 8 ? 16 : 8, nb = q.N > 16 ? 2 : 1;
  const TileRun r = tile_run(q.D, q.H, q.W, 32, 4, 2, cp == 16 || nb == 2 ? 256 : 512, x->B);      // <16, 1>, <8, 2>: one block per CU
  q.ntx = r.ntx; q.nty = r.nty; q.ntz = r.ntz; q.ids_total = r.ids_total; q.ids_per_block = r.ids_per_block;
  const long wsz1 = 27L * q.N * q.C, wsz = wsz1 * (d->per_sample_w ? x->B : 1);
  q.wsb = d->per_sample_w ? wsz1 : 0;
  const WgradRep rep = wgrad_replicas(wsz, dwk, ws, ws_bytes, s, zeroed);
  if (!rep.out) return 2;
  q.dwk = rep.out; q.nrep = rep.nrep; q.rep_stride = rep.rep_stride;
  const dim3 grid((unsigned)r.gx, 1, (unsigned)x->B);
  coma_set_kernel_tag("conv_split_thin_wgrad_k<%d, %d>", cp, nb);
#define SPLIT_THINW(CP_, NB_) do { set_max_lds<conv_split_thin_wgrad_k<CP_, NB_>, 80>(); \
    hipLaunchKernelGGL((conv_split_thin_wgrad_k<CP_, NB_>), grid, dim3(256), (size_t)(SplitThinWTile<CP_, NB_>::LDS), s, q); } while (0)
  if (cp == 16) SPLIT_THINW(16, 1);
  else if (nb == 2) SPLIT_THINW(8, 2);
  else SPLIT_THINW(8, 1);
#undef SPLIT_THINW
  COMA_LAUNCH_CHECK();
  return wgrad_replicas_done(rep, wsz, dwk, s);
}
