// Gradient-difference loss (DESIGN.md section 4 "Gradient-difference loss"): an edge term on forward differences.  Per sample b,
// axis a in {z, y, x} and every voxel v whose neighbour v + e_a is inside the volume (a "pair"):
//   gp = pred[v + e_a] - pred[v],  gg = gt[v + e_a] - gt[v],  t = |gp| - |gg| (mode 0, "abs") | gp - gg (mode 1, "signed")
//   phi(t) = |t| (alpha 1) | t^2 (alpha 2),   m_a(v) = 1 (no mask) | [roi[v] != 0 and roi[v + e_a] != 0]
//   N_a = sum m_a,  S_a = sum m_a phi(t),  loss_b = sum_a s_a (N_a > 0 ? S_a / N_a : 0),  coef[b][a] = N_a > 0 ? s_a / N_a : 0
//   psi_a(v) = m_a(v) phi'(t) chi,  phi' = sign(t) | 2 t,  chi = sign(gp) (abs) | 1 (signed),  sign(0) = 0
//   dpred[v] = gout[b] sum_a coef[b][a] (psi_a(v - e_a) - psi_a(v))                       (psi = 0 where the pair does not exist)
// A block owns an 8 x 8 x 32 tile (smooth.hip's).  It stages the tile and its one-voxel halo (forward: the + side, backward:
// both sides) of pred and gt into LDS as fp32, and the mask bit as a byte, every voxel fetched once per block: rows that are
// contiguous and 16-byte aligned by 16-byte loads (4 fp32 / 8 bf16), anything else element by element.  Both ways leave the
// same values in LDS and everything after reads LDS only, so the two paths give the same bits.  A lane owns four consecutive
// x of one row.  All arithmetic on the staged values is fp64 (differences of fp32 values: the sign decisions are exact), and
// the result is rounded once: the block's record, loss / coef in the finalise, a dpred voxel at its store.
// No atomics, every output has one writer, every sum a fixed order: bitwise repeatable; no host read: capture-safe.
#include "common.h"
#include <math.h>

enum { GD_ABS = 0, GD_SIGNED = 1 };
enum { GD_TZ = 8, GD_TY = COMA_SMOOTH_TILE_Y, GD_TX = COMA_SMOOTH_TILE_X, GD_ROW = 40, GD_X0 = 4,   // LDS row: x0 - 1 at 3, the tile at 4 .. 35, x0 + 32 at 36
       GD_STAGE = 4, GD_REC = 6 };                                                             // loads in flight per lane; doubles per record {S_z, S_y, S_x, N_z, N_y, N_x}
static_assert(GD_TX == 32 && GD_TY == 8, "the compute loops decode (z, y, quad) with shifts for an 8 x 8 x 32 tile");

struct GdP {
  const void* pred; int64_t sbp, ldp; const void* gt; int64_t sbg; const float* roi; int64_t sbr;
  int D, H, W, ntx, nty, ntiles;
  int vp, vg, vr;                   // 16-byte staging of pred / gt / roi
  int mode, alpha;
  double* rec;                      // forward: [B][ntiles][GD_REC]
  const float* gout; const float* coef; void* dp; int64_t sbd, ldd; int vd;
};

__device__ __forceinline__ double gd_sgn(double x) { return (double)((x > 0.0) - (x < 0.0)); }
// the pair (v, v + e): values at v (p0, g0) and at v + e (p1, g1)
__device__ __forceinline__ double gd_t(int mode, double p0, double p1, double g0, double g1) {
  const double gp = p1 - p0, gg = g1 - g0;
  return mode == GD_ABS ? fabs(gp) - fabs(gg) : gp - gg;
}
__device__ __forceinline__ double gd_phi(int mode, int alpha, double p0, double p1, double g0, double g1) {
  const double t = gd_t(mode, p0, p1, g0, g1);
  return alpha == 1 ? fabs(t) : t * t;
}
__device__ __forceinline__ double gd_psi(int mode, int alpha, double p0, double p1, double g0, double g1) {
  const double t = gd_t(mode, p0, p1, g0, g1);
  const double d = alpha == 1 ? gd_sgn(t) : 2.0 * t;
  return mode == GD_ABS ? d * gd_sgn(p1 - p0) : d;
}

__device__ __forceinline__ void gd_put4(float* d, const float* v) { vec_io<float, 4>::store(d, v); }
__device__ __forceinline__ void gd_put4(unsigned char* d, const float* v) {
  *reinterpret_cast<uint32_t*>(d) = (v[0] != 0.f ? 1u : 0u) | (v[1] != 0.f ? 1u << 8 : 0u) | (v[2] != 0.f ? 1u << 16 : 0u) | (v[3] != 0.f ? 1u << 24 : 0u);
}
__device__ __forceinline__ void gd_put1(float* d, float v) { *d = v; }
__device__ __forceinline__ void gd_put1(unsigned char* d, float v) { *d = v != 0.f ? 1 : 0; }

// Whole block calls this.  dst[(iz * RY + iy) * GD_ROW + GD_X0 + lx] = src at (z0 - HLO + iz, y0 - HLO + iy, x0 + lx), lx in
// -HLO .. 32, zero outside the volume.  Every load is unconditional from a clamped address (loads behind a branch are not
// issued back to back) and GD_STAGE of them are in flight per lane before the first LDS write.
template <typename T, typename DT, int HLO>
__device__ __forceinline__ void gd_stage(DT* dst, const T* src, int64_t ld, int vec, int D, int H, int W, int z0, int y0, int x0) {
  constexpr int RY = GD_TY + HLO + 1, NR = (GD_TZ + HLO + 1) * RY, VEC = 16 / (int)sizeof(T), NU = GD_TX / VEC, NX = GD_TX + HLO + 1;
  const int tid = threadIdx.x;
  auto row = [&](int r, bool& ok) -> int64_t {
    const int iz = r / RY, iy = r - iz * RY;
    int gz = z0 - HLO + iz, gy = y0 - HLO + iy;
    ok = gz >= 0 && gz < D && gy >= 0 && gy < H;
    gz = min(max(gz, 0), D - 1); gy = min(max(gy, 0), H - 1);
    return ((int64_t)gz * H + gy) * W;
  };
  if (vec) {                        // (host: voxel pitch 1, W % VEC == 0, 16-byte aligned sample bases: a chunk is all in or all out)
    for (int u0 = tid; u0 < NR * NU; u0 += 256 * GD_STAGE) {
      float v[GD_STAGE][VEC];
#pragma unroll
      for (int s = 0; s < GD_STAGE; ++s) {
        const int u = min(u0 + 256 * s, NR * NU - 1), r = u / NU, c = u - r * NU;
        bool ok;
        const int64_t base = row(r, ok);
        const int gx = x0 + c * VEC;
        vec_io<T, VEC>::load(src + base + min(gx, W - VEC), v[s]);
        if (!ok || gx >= W) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) v[s][k] = 0.f;
        }
      }
#pragma unroll
      for (int s = 0; s < GD_STAGE; ++s) {
        const int u = u0 + 256 * s, r = u / NU, c = u - r * NU;
        if (u < NR * NU) {
#pragma unroll
          for (int k = 0; k < VEC; k += 4) gd_put4(dst + r * GD_ROW + GD_X0 + c * VEC + k, v[s] + k);
        }
      }
    }
    for (int i = tid; i < NR * (HLO + 1); i += 256) {          // the halo columns x0 + 32 and, with HLO, x0 - 1
      const int r = i / (HLO + 1), lx = (HLO && i - r * (HLO + 1) == 0) ? -1 : GD_TX;
      bool ok;
      const int64_t base = row(r, ok);
      const int gx = x0 + lx;
      const float v = ld_f(src + base + min(max(gx, 0), W - 1));
      gd_put1(dst + r * GD_ROW + GD_X0 + lx, ok && gx >= 0 && gx < W ? v : 0.f);
    }
  } else {
    for (int e0 = tid; e0 < NR * NX; e0 += 256 * GD_STAGE) {
      float v[GD_STAGE];
#pragma unroll
      for (int s = 0; s < GD_STAGE; ++s) {
        const int e = min(e0 + 256 * s, NR * NX - 1), r = e / NX, gx = x0 - HLO + (e - r * NX);
        bool ok;
        const int64_t base = row(r, ok);
        v[s] = ld_f(src + (base + min(max(gx, 0), W - 1)) * ld);
        if (!ok || gx < 0 || gx >= W) v[s] = 0.f;
      }
#pragma unroll
      for (int s = 0; s < GD_STAGE; ++s) {
        const int e = e0 + 256 * s, r = e / NX;
        if (e < NR * NX) gd_put1(dst + r * GD_ROW + GD_X0 - HLO + (e - r * NX), v[s]);
      }
    }
  }
}

__device__ __forceinline__ void gd_tile(const GdP& p, int& z0, int& y0, int& x0) {
  int t = blockIdx.x;
  const int tx = t % p.ntx; t /= p.ntx;
  x0 = tx * GD_TX; y0 = (t % p.nty) * GD_TY; z0 = (t / p.nty) * GD_TZ;
}

// four values of a row from LDS (o: the lane's first column, 16-byte aligned)
__device__ __forceinline__ void gd_ld4(const float* s, int o, float* v) { vec_io<float, 4>::load(s + o, v); }
__device__ __forceinline__ void gd_ld4(const unsigned char* s, int o, bool* v) {
  const uint32_t u = *reinterpret_cast<const uint32_t*>(s + o);
  v[0] = u & 1u; v[1] = (u >> 8) & 1u; v[2] = (u >> 16) & 1u; v[3] = (u >> 24) & 1u;
}

// rec[(b * ntiles + tile) * GD_REC + k]: the tile's {S_z, S_y, S_x, N_z, N_y, N_x} (N = 0 without a mask: closed form later)
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void grad_diff_fwd_k(const GdP p) {
  constexpr int RY = GD_TY + 1, NR = (GD_TZ + 1) * RY;
  __shared__ __attribute__((aligned(16))) float sp[NR * GD_ROW];
  __shared__ __attribute__((aligned(16))) float sg[NR * GD_ROW];
  __shared__ __attribute__((aligned(16))) unsigned char sm[MASK ? NR * GD_ROW : 16];
  __shared__ double red[4][GD_REC];
  const int tid = threadIdx.x, b = blockIdx.y;
  int z0, y0, x0;
  gd_tile(p, z0, y0, x0);
  gd_stage<T, float, 0>(sp, reinterpret_cast<const T*>(p.pred) + b * p.sbp, p.ldp, p.vp, p.D, p.H, p.W, z0, y0, x0);
  gd_stage<T, float, 0>(sg, reinterpret_cast<const T*>(p.gt) + b * p.sbg, 1, p.vg, p.D, p.H, p.W, z0, y0, x0);
  if (MASK) gd_stage<float, unsigned char, 0>(sm, p.roi + b * p.sbr, 1, p.vr, p.D, p.H, p.W, z0, y0, x0);
  __syncthreads();

  double S[3] = {0.0, 0.0, 0.0};
  int N[3] = {0, 0, 0};
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int i = tid + 256 * it, q = i & 7, y = (i >> 3) & 7, z = i >> 6;
    const int gz = z0 + z, gy = y0 + y, gx = x0 + 4 * q;
    if (gz >= p.D || gy >= p.H || gx >= p.W) continue;
    const int o = (z * RY + y) * GD_ROW + GD_X0 + 4 * q;
    float pc[5], pz[4], py[4], gc[5], gzv[4], gyv[4];
    gd_ld4(sp, o, pc); pc[4] = sp[o + 4]; gd_ld4(sp, o + RY * GD_ROW, pz); gd_ld4(sp, o + GD_ROW, py);
    gd_ld4(sg, o, gc); gc[4] = sg[o + 4]; gd_ld4(sg, o + RY * GD_ROW, gzv); gd_ld4(sg, o + GD_ROW, gyv);
    bool mc[5] = {true, true, true, true, true}, mz[4] = {true, true, true, true}, my[4] = {true, true, true, true};
    if (MASK) { gd_ld4(sm, o, mc); mc[4] = sm[o + 4] != 0; gd_ld4(sm, o + RY * GD_ROW, mz); gd_ld4(sm, o + GD_ROW, my); }
    const bool ez = gz + 1 < p.D, ey = gy + 1 < p.H;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (gx + j >= p.W || !mc[j]) continue;
      if (ez && mz[j]) { S[0] += gd_phi(p.mode, p.alpha, pc[j], pz[j], gc[j], gzv[j]); N[0] += 1; }
      if (ey && my[j]) { S[1] += gd_phi(p.mode, p.alpha, pc[j], py[j], gc[j], gyv[j]); N[1] += 1; }
      if (gx + j + 1 < p.W && mc[j + 1]) { S[2] += gd_phi(p.mode, p.alpha, pc[j], pc[j + 1], gc[j], gc[j + 1]); N[2] += 1; }
    }
  }
  // the block's sums in a fixed order: a butterfly over each wave's lanes, then the four waves in order
  double r[GD_REC] = {S[0], S[1], S[2], (double)N[0], (double)N[1], (double)N[2]};
#pragma unroll
  for (int k = 0; k < GD_REC; ++k) {
    if (!MASK && k >= 3) continue;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r[k] += __shfl_xor(r[k], o, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < GD_REC; ++k) red[tid >> 6][k] = r[k];
  }
  __syncthreads();
  if (tid < GD_REC)
    p.rec[((int64_t)b * p.ntiles + blockIdx.x) * GD_REC + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one wave per sample: lane l adds the records l, l + 64, ... in order, then a butterfly over the lanes
__global__ __launch_bounds__(64) void grad_diff_finalize_k(const double* rec, int ntiles, int masked, int D, int H, int W,
                                                           float w0, float w1, float w2, float* loss, float* coef) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double s[GD_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lane; i < ntiles; i += 64) {
#pragma unroll
    for (int k = 0; k < GD_REC; ++k) s[k] += rec[((int64_t)b * ntiles + i) * GD_REC + k];
  }
#pragma unroll
  for (int k = 0; k < GD_REC; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
  }
  if (lane != 0) return;
  const double w[3] = {(double)w0, (double)w1, (double)w2};
  const double n[3] = {masked ? s[3] : (double)(D - 1) * H * W, masked ? s[4] : (double)D * (H - 1) * W,
                       masked ? s[5] : (double)D * H * (W - 1)};
  double l = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {     // an axis of length 1, or without a counted pair: 0, never NaN
    const bool live = n[a] > 0.0;
    if (live) l += w[a] * (s[a] / n[a]);
    coef[b * 3 + a] = live ? (float)(w[a] / n[a]) : 0.f;
  }
  loss[b] = (float)l;
}

// dpred[v] = gout[b] sum_a coef[b][a] (psi_a(v - e_a) - psi_a(v)); every voxel of the tile is assigned by one lane
template <typename T, bool MASK>
__global__ __launch_bounds__(256) void grad_diff_bwd_k(const GdP p) {
  constexpr int RY = GD_TY + 2, NR = (GD_TZ + 2) * RY, SZ = RY * GD_ROW, SY = GD_ROW;
  __shared__ __attribute__((aligned(16))) float sp[NR * GD_ROW];
  __shared__ __attribute__((aligned(16))) float sg[NR * GD_ROW];
  __shared__ __attribute__((aligned(16))) unsigned char sm[MASK ? NR * GD_ROW : 16];
  const int tid = threadIdx.x, b = blockIdx.y;
  int z0, y0, x0;
  gd_tile(p, z0, y0, x0);
  gd_stage<T, float, 1>(sp, reinterpret_cast<const T*>(p.pred) + b * p.sbp, p.ldp, p.vp, p.D, p.H, p.W, z0, y0, x0);
  gd_stage<T, float, 1>(sg, reinterpret_cast<const T*>(p.gt) + b * p.sbg, 1, p.vg, p.D, p.H, p.W, z0, y0, x0);
  if (MASK) gd_stage<float, unsigned char, 1>(sm, p.roi + b * p.sbr, 1, p.vr, p.D, p.H, p.W, z0, y0, x0);
  __syncthreads();

  const double go = (double)p.gout[b];
  const double cz = go * (double)p.coef[b * 3], cy = go * (double)p.coef[b * 3 + 1], cx = go * (double)p.coef[b * 3 + 2];
  T* ob = reinterpret_cast<T*>(p.dp) + b * p.sbd;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int i = tid + 256 * it, q = i & 7, y = (i >> 3) & 7, z = i >> 6;
    const int gz = z0 + z, gy = y0 + y, gx = x0 + 4 * q;
    if (gz >= p.D || gy >= p.H || gx >= p.W) continue;
    const int o = ((z + 1) * RY + (y + 1)) * GD_ROW + GD_X0 + 4 * q;
    float pc[6], pzl[4], pzh[4], pyl[4], pyh[4], gc[6], gzl[4], gzh[4], gyl[4], gyh[4];   // pc / gc: x - 1, the four, x + 4
    gd_ld4(sp, o, pc + 1); pc[0] = sp[o - 1]; pc[5] = sp[o + 4];
    gd_ld4(sp, o - SZ, pzl); gd_ld4(sp, o + SZ, pzh); gd_ld4(sp, o - SY, pyl); gd_ld4(sp, o + SY, pyh);
    gd_ld4(sg, o, gc + 1); gc[0] = sg[o - 1]; gc[5] = sg[o + 4];
    gd_ld4(sg, o - SZ, gzl); gd_ld4(sg, o + SZ, gzh); gd_ld4(sg, o - SY, gyl); gd_ld4(sg, o + SY, gyh);
    bool mc[6] = {true, true, true, true, true, true}, mzl[4] = {true, true, true, true}, mzh[4] = {true, true, true, true},
         myl[4] = {true, true, true, true}, myh[4] = {true, true, true, true};
    if (MASK) {
      gd_ld4(sm, o, mc + 1); mc[0] = sm[o - 1] != 0; mc[5] = sm[o + 4] != 0;
      gd_ld4(sm, o - SZ, mzl); gd_ld4(sm, o + SZ, mzh); gd_ld4(sm, o - SY, myl); gd_ld4(sm, o + SY, myh);
    }
    const bool zl = gz >= 1, zh = gz + 1 < p.D, yl = gy >= 1, yh = gy + 1 < p.H;
    // psi_x of the five pairs (x - 1 + k, x + k), k = 0 .. 4: neighbouring voxels of the lane share them
    double px[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int xa = gx - 1 + k;
      px[k] = (xa >= 0 && xa + 1 < p.W && mc[k] && mc[k + 1]) ? gd_psi(p.mode, p.alpha, pc[k], pc[k + 1], gc[k], gc[k + 1]) : 0.0;
    }
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float pv = pc[j + 1], gv = gc[j + 1];
      const bool mv = mc[j + 1];
      const double zlo = (zl && mv && mzl[j]) ? gd_psi(p.mode, p.alpha, pzl[j], pv, gzl[j], gv) : 0.0;
      const double zhi = (zh && mv && mzh[j]) ? gd_psi(p.mode, p.alpha, pv, pzh[j], gv, gzh[j]) : 0.0;
      const double ylo = (yl && mv && myl[j]) ? gd_psi(p.mode, p.alpha, pyl[j], pv, gyl[j], gv) : 0.0;
      const double yhi = (yh && mv && myh[j]) ? gd_psi(p.mode, p.alpha, pv, pyh[j], gv, gyh[j]) : 0.0;
      out[j] = (float)((cz * (zlo - zhi) + cy * (ylo - yhi)) + cx * (px[j] - px[j + 1]));
    }
    const int64_t v = ((int64_t)gz * p.H + gy) * p.W + gx;
    if (p.vd) vec_io<T, 4>::store(ob + v, out);      // (host: voxel pitch 1, W % 4 == 0: the quad is inside)
    else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (gx + j < p.W) st_f(ob + (v + j) * p.ldd, out[j]);
    }
  }
}

static int64_t gd_ntiles(const coma_tensor* t, int* ntx, int* nty) {
  const int64_t nx = (t->W + GD_TX - 1) / GD_TX, ny = (t->H + GD_TY - 1) / GD_TY, nz = (t->D + GD_TZ - 1) / GD_TZ;
  if (ntx) *ntx = (int)nx;
  if (nty) *nty = (int)ny;
  return nx * ny * nz;
}
// rows of n-element chunks: voxel pitch 1, W and the sample stride multiples of n, base on an n-element boundary
static bool gd_vec(const coma_tensor* t, int n) {
  return t->ld == 1 && t->W % n == 0 && t->sb % n == 0 && ((uintptr_t)t->data % (n * esize(t->dtype))) == 0;
}
static int gd_check(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, int mode, int alpha, const char* who) {
  COMA_CHECK(pred && gt && pred->data && gt->data, "%s: null argument", who);
  COMA_CHECK(pred->B > 0 && pred->D > 0 && pred->H > 0 && pred->W > 0 && pred->B <= 65535, "%s: bad shape (%d, %d, %d, %d)", who,
             pred->B, pred->D, pred->H, pred->W);
  COMA_CHECK(pred->C == 1 && gt->C == 1 && t_same_grid(pred, gt), "%s: pred / gt must be single-channel volumes of equal shape", who);
  COMA_CHECK((pred->dtype == COMA_F32 || pred->dtype == COMA_BF16) && pred->dtype == gt->dtype, "%s: pred / gt dtype mismatch", who);
  COMA_CHECK(gt->ld == 1 && pred->ld >= 1, "%s: gt must have voxel pitch 1", who);
  if (roi) {
    COMA_CHECK(roi->data && roi->C == 1 && t_same_grid(pred, roi), "%s: roi must be a single-channel volume of pred's shape", who);
    COMA_CHECK(roi->dtype == COMA_F32 && roi->ld == 1, "%s: roi must be fp32 of voxel pitch 1", who);
  }
  COMA_CHECK(mode == GD_ABS || mode == GD_SIGNED, "%s: mode=%d out of range 0..1", who, mode);
  COMA_CHECK(alpha == 1 || alpha == 2, "%s: alpha=%d out of range 1..2", who, alpha);
  COMA_CHECK(gd_ntiles(pred, nullptr, nullptr) <= 2147483647LL, "%s: volume too large for one launch", who);
  return 0;
}
static GdP gd_params(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, int mode, int alpha) {
  GdP p{};
  p.pred = pred->data; p.sbp = pred->sb; p.ldp = pred->ld; p.gt = gt->data; p.sbg = gt->sb;
  p.roi = roi ? (const float*)roi->data : nullptr; p.sbr = roi ? roi->sb : 0;
  p.D = pred->D; p.H = pred->H; p.W = pred->W;
  p.ntiles = (int)gd_ntiles(pred, &p.ntx, &p.nty);
  const int n = 16 / esize(pred->dtype);
  p.vp = gd_vec(pred, n); p.vg = gd_vec(gt, n); p.vr = roi ? gd_vec(roi, 4) : 0;
  p.mode = mode; p.alpha = alpha;
  return p;
}

extern "C" size_t coma_grad_diff_ws_bytes(const coma_tensor* pred) {
  return (size_t)pred->B * (size_t)gd_ntiles(pred, nullptr, nullptr) * GD_REC * sizeof(double);
}

extern "C" int coma_grad_diff_fwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, int32_t mode, int32_t alpha,
                                  const float* axis_w, float* loss, float* coef, void* ws, size_t ws_bytes, void* stream) {
  if (gd_check(pred, gt, roi, mode, alpha, "grad_diff_fwd")) return 1;
  COMA_CHECK(axis_w && loss && coef, "grad_diff_fwd: null argument");
  for (int a = 0; a < 3; ++a)
    COMA_CHECK(axis_w[a] >= 0.f && isfinite(axis_w[a]), "grad_diff_fwd: axis weight %d = %g must be finite and >= 0", a, (double)axis_w[a]);
  COMA_CHECK(ws, "grad_diff_fwd: no workspace");
  COMA_CHECK(ws_bytes >= coma_grad_diff_ws_bytes(pred), "grad_diff_fwd: workspace too small");
  GdP p = gd_params(pred, gt, roi, mode, alpha);
  p.rec = (double*)ws;
  const dim3 grid((unsigned)p.ntiles, (unsigned)pred->B);
  hipStream_t s = (hipStream_t)stream;
#define LK(T) do { if (roi) hipLaunchKernelGGL((grad_diff_fwd_k<T, true>), grid, dim3(256), 0, s, p); \
                   else hipLaunchKernelGGL((grad_diff_fwd_k<T, false>), grid, dim3(256), 0, s, p); } while (0)
  if (pred->dtype == COMA_F32) LK(float); else LK(bf16_t);
#undef LK
  COMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_diff_finalize_k, dim3(pred->B), dim3(64), 0, s, (const double*)ws, p.ntiles, roi ? 1 : 0, p.D, p.H, p.W,
                     axis_w[0], axis_w[1], axis_w[2], loss, coef);
  COMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int coma_grad_diff_bwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, int32_t mode, int32_t alpha,
                                  const float* gout, const float* coef, const coma_tensor* dpred, void* stream) {
  if (gd_check(pred, gt, roi, mode, alpha, "grad_diff_bwd")) return 1;
  COMA_CHECK(gout && coef && dpred && dpred->data, "grad_diff_bwd: null argument");
  COMA_CHECK(dpred->C == 1 && t_same_grid(pred, dpred) && dpred->dtype == pred->dtype && dpred->ld >= 1,
             "grad_diff_bwd: dpred must be a single-channel volume of pred's shape and dtype");
  GdP p = gd_params(pred, gt, roi, mode, alpha);
  p.gout = gout; p.coef = coef; p.dp = dpred->data; p.sbd = dpred->sb; p.ldd = dpred->ld; p.vd = gd_vec(dpred, 4);
  const dim3 grid((unsigned)p.ntiles, (unsigned)pred->B);
  hipStream_t s = (hipStream_t)stream;
#define LB(T) do { if (roi) hipLaunchKernelGGL((grad_diff_bwd_k<T, true>), grid, dim3(256), 0, s, p); \
                   else hipLaunchKernelGGL((grad_diff_bwd_k<T, false>), grid, dim3(256), 0, s, p); } while (0)
  if (pred->dtype == COMA_F32) LB(float); else LB(bf16_t);
#undef LB
  COMA_LAUNCH_CHECK();
  return 0;
}
