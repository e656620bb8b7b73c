// On-device 3-D augmentation (DESIGN.md section 4 "Augmentation"): ONE launch warps the MRI, the tau target and the ROI
// label volume of every sample of a batch by the same per-sample transform.  Output voxel o = (z, y, x) of sample b reads
//   s = A_b (z, y, x, 1)^T + u_b(o)            A_b: 3 x 4, output voxel index -> source voxel index, (z, y, x) order
// where u_b is the trilinear (align-corners) interpolation of an optional control grid of displacements in voxels.
//   roi_out = roi[floor(s + 0.5)] (0 outside), tau_out = trilinear(tau, s) (corners outside the volume contribute 0),
//   mri_out = scale * f(trilinear(mri, s)) + shift + sigma * n(seed, b, voxel), then 0 where roi_out == 0.
// n is Philox4x32-10 + Box-Muller on (seed, voxel index, b): a pure function of its arguments, nothing to go stale.
// A block is a compact 4 x 8 x 32 tile of OUTPUT voxels (one wave = one 8 x 32 slab); a lane owns four consecutive x:
// under a small rotation the tile's source footprint is a compact box, so the 17 gathers of a voxel hit lines its
// neighbours use too, and the three outputs leave in 16-byte stores.  No atomics, no scratch, 6 KB of LDS.
#include "common.h"

#define AUG_TX 32
#define AUG_TY 8
#define AUG_TZ 4
#define AUG_MAXG 8

struct AugP {
  const float* mri; const float* tau; const float* roi;
  float* mri_out; float* tau_out; float* roi_out;
  int D, H, W;
  int ntx, nty;
  const float* params;              // (B, COMA_AUG_NPARAM)
  const float* disp;                // (B, 3, gz, gy, gx) or nullptr
  int gz, gy, gx;
  float rz, ry, rx;                 // (g - 1) / (size - 1) per axis: output index -> control-grid coordinate
  uint32_t k0, k1;                  // the two halves of the seed
};

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
}

// standard normal of (key, voxel index, sample): Philox4x32-10 on counter (index low, index high, b, 0); Box-Muller on
// the top 24 bits of words 0 and 1, so that both uniforms are exact in fp32: u1 in (0, 1], u2 in [0, 1)
__device__ __forceinline__ float aug_normal(uint32_t k0, uint32_t k1, int64_t idx, int b) {
  uint32_t c[4] = {(uint32_t)idx, (uint32_t)((uint64_t)idx >> 32), (uint32_t)b, 0u};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const float u1 = (float)((c[0] >> 8) + 1u) * 5.9604644775390625e-8f;      // 2^-24
  const float u2 = (float)(c[1] >> 8) * 5.9604644775390625e-8f;
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// floor of a source coordinate, its fraction and which of the two corners lie inside [0, size); i0 is clamped so that
// an index built from it always stays inside the volume, whatever the coordinate (NaN and infinities included)
__device__ __forceinline__ void aug_axis(float s, int size, int& i0, float& f, bool& in0, bool& in1) {
  const float fl = floorf(s);
  f = s - fl;
  const float top = (float)(size - 1);
  in0 = fl >= 0.f && fl <= top;
  in1 = fl >= -1.f && fl <= top - 1.f;
  i0 = (int)fminf(fmaxf(fl, -1.f), top);          // NaN -> -1: both corners out
}

template <bool VEC>
__global__ __launch_bounds__(256) void augment_warp_k(AugP p) {
  __shared__ float sd[3 * AUG_MAXG * AUG_MAXG * AUG_MAXG];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const bool elastic = p.disp != nullptr;
  const int gvol = p.gz * p.gy * p.gx;
  if (elastic) {
    const float* dg = p.disp + (int64_t)b * 3 * gvol;
    for (int i = tid; i < 3 * gvol; i += 256) sd[i] = dg[i];
    __syncthreads();
  }
  int t = blockIdx.x;
  const int tx = t % p.ntx; t /= p.ntx;
  const int ty = t % p.nty; const int tz = t / p.nty;
  const int x0 = tx * AUG_TX + (tid % 8) * 4, y = ty * AUG_TY + (tid / 8) % 8, z = tz * AUG_TZ + tid / 64;
  if (x0 >= p.W || y >= p.H || z >= p.D) return;             // (after the only barrier)
  const float* pr = p.params + (int64_t)b * COMA_AUG_NPARAM;
  float A[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) A[i] = pr[i];
  const float mscale = pr[12], mshift = pr[13], mgamma = pr[14], sigma = pr[15];
  const int64_t V = (int64_t)p.D * p.H * p.W;
  const float* mri = p.mri + b * V;
  const float* tau = p.tau + b * V;
  const float* roi = p.roi + b * V;
  const int64_t row = ((int64_t)z * p.H + y) * p.W;
  const float fz = (float)z, fy = (float)y;

  // control-grid cell and weights of this row (z, y): shared by the four x outputs
  int cz0 = 0, cy0 = 0;
  float wz = 0.f, wy = 0.f;
  if (elastic) {
    const float cz = fz * p.rz, cy = fy * p.ry;
    cz0 = min((int)cz, p.gz - 2); wz = cz - (float)cz0;
    cy0 = min((int)cy, p.gy - 2); wy = cy - (float)cy0;
  }

  float om[4], ot[4], orr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j;
    om[j] = ot[j] = orr[j] = 0.f;
    if (!VEC && x >= p.W) continue;
    const float fx = (float)x;
    float sz = fmaf(A[0], fz, fmaf(A[1], fy, fmaf(A[2], fx, A[3])));
    float sy = fmaf(A[4], fz, fmaf(A[5], fy, fmaf(A[6], fx, A[7])));
    float sx = fmaf(A[8], fz, fmaf(A[9], fy, fmaf(A[10], fx, A[11])));
    if (elastic) {
      const float cx = fx * p.rx;
      const int cx0 = min((int)cx, p.gx - 2);
      const float wx = cx - (float)cx0;
      float u[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* g = sd + c * gvol + (cz0 * p.gy + cy0) * p.gx + cx0;
        const int sy_ = p.gx, sz_ = p.gy * p.gx;
        const float a00 = fmaf(wx, g[1] - g[0], g[0]), a01 = fmaf(wx, g[sy_ + 1] - g[sy_], g[sy_]);
        const float a10 = fmaf(wx, g[sz_ + 1] - g[sz_], g[sz_]), a11 = fmaf(wx, g[sz_ + sy_ + 1] - g[sz_ + sy_], g[sz_ + sy_]);
        const float a0 = fmaf(wy, a01 - a00, a00), a1 = fmaf(wy, a11 - a10, a10);
        u[c] = fmaf(wz, a1 - a0, a0);
      }
      sz += u[0]; sy += u[1]; sx += u[2];
    }
    // ROI: nearest, rounding half up like nn_index of metrics.hip
    float lab = 0.f;
    {
      const float nz = floorf(sz + 0.5f), ny = floorf(sy + 0.5f), nx = floorf(sx + 0.5f);
      if (nz >= 0.f && nz <= (float)(p.D - 1) && ny >= 0.f && ny <= (float)(p.H - 1) && nx >= 0.f && nx <= (float)(p.W - 1))
        lab = roi[((int64_t)(int)nz * p.H + (int)ny) * p.W + (int)nx];
    }
    orr[j] = lab;
    int iz, iy, ix;
    float tz_, ty_, tx_;
    bool z0in, z1in, y0in, y1in, x0in, x1in;
    aug_axis(sz, p.D, iz, tz_, z0in, z1in);
    aug_axis(sy, p.H, iy, ty_, y0in, y1in);
    aug_axis(sx, p.W, ix, tx_, x0in, x1in);
    const float wzc[2] = {1.f - tz_, tz_}, wyc[2] = {1.f - ty_, ty_}, wxc[2] = {1.f - tx_, tx_};
    const bool zin[2] = {z0in, z1in}, yin[2] = {y0in, y1in}, xin[2] = {x0in, x1in};
    const bool fg = lab != 0.f;               // the MRI is 0 wherever the warped ROI is: its eight gathers are skipped there
    float m = 0.f, tv = 0.f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          if (zin[dz] && yin[dy] && xin[dx]) {
            const int64_t v = ((int64_t)(iz + dz) * p.H + (iy + dy)) * p.W + (ix + dx);
            const float w = wzc[dz] * wyc[dy] * wxc[dx];
            tv = fmaf(w, tau[v], tv);
            if (fg) m = fmaf(w, mri[v], m);
          }
        }
    ot[j] = tv;
    if (fg) {
      if (mgamma != 1.f) m = powf(fmaxf(m, 0.f), mgamma);
      m = fmaf(mscale, m, mshift);
      if (sigma != 0.f) m = fmaf(sigma, aug_normal(p.k0, p.k1, row + x, b), m);
      om[j] = m;
    }
  }
  float* mo = p.mri_out + b * V + row + x0;
  float* to = p.tau_out + b * V + row + x0;
  float* ro = p.roi_out + b * V + row + x0;
  if (VEC) {
    vec_io<float, 4>::store(mo, om); vec_io<float, 4>::store(to, ot); vec_io<float, 4>::store(ro, orr);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < p.W) { mo[j] = om[j]; to[j] = ot[j]; ro[j] = orr[j]; }
  }
}

static inline bool aug_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

extern "C" int coma_augment_warp(const float* mri, const float* tau, const float* roi, float* mri_out, float* tau_out,
                                 float* roi_out, int32_t B, int32_t D, int32_t H, int32_t W, const float* params,
                                 const float* disp, int32_t gz, int32_t gy, int32_t gx, uint64_t seed, void* stream) {
  COMA_CHECK(mri && tau && roi && mri_out && tau_out && roi_out && params, "augment_warp: null argument");
  COMA_CHECK(B > 0 && D > 0 && H > 0 && W > 0 && B <= 65535, "augment_warp: bad shape (%d, %d, %d, %d)", B, D, H, W);
  const int64_t ntx = (W + AUG_TX - 1) / AUG_TX, nty = (H + AUG_TY - 1) / AUG_TY, ntz = (D + AUG_TZ - 1) / AUG_TZ;
  COMA_CHECK(ntx * nty * ntz <= 2147483647LL, "augment_warp: volume too large for one launch");
  const size_t bytes = (size_t)B * D * H * W * sizeof(float);
  const void* ins[3] = {mri, tau, roi};
  void* outs[3] = {mri_out, tau_out, roi_out};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      COMA_CHECK(!aug_overlap(outs[i], ins[j], bytes), "augment_warp: an output overlaps an input (the warp gathers: not in place)");
    for (int j = i + 1; j < 3; ++j)
      COMA_CHECK(!aug_overlap(outs[i], outs[j], bytes), "augment_warp: two outputs overlap");
  }
  AugP p;
  p.mri = mri; p.tau = tau; p.roi = roi; p.mri_out = mri_out; p.tau_out = tau_out; p.roi_out = roi_out;
  p.D = D; p.H = H; p.W = W; p.ntx = (int)ntx; p.nty = (int)nty;
  p.params = params; p.disp = disp; p.gz = p.gy = p.gx = 2; p.rz = p.ry = p.rx = 0.f;
  if (disp) {
    COMA_CHECK(gz >= 2 && gy >= 2 && gx >= 2, "augment_warp: control grid (%d, %d, %d) needs >= 2 points per axis", gz, gy, gx);
    COMA_CHECK(gz <= AUG_MAXG && gy <= AUG_MAXG && gx <= AUG_MAXG, "augment_warp: control grid (%d, %d, %d) exceeds %d points per axis",
               gz, gy, gx, AUG_MAXG);
    p.gz = gz; p.gy = gy; p.gx = gx;
    p.rz = D > 1 ? (float)((double)(gz - 1) / (D - 1)) : 0.f;
    p.ry = H > 1 ? (float)((double)(gy - 1) / (H - 1)) : 0.f;
    p.rx = W > 1 ? (float)((double)(gx - 1) / (W - 1)) : 0.f;
  }
  p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32);
  const bool vec = W % 4 == 0 && (((uintptr_t)mri_out | (uintptr_t)tau_out | (uintptr_t)roi_out) & 15) == 0;
  dim3 grid((unsigned)(ntx * nty * ntz), (unsigned)B);
  if (vec) hipLaunchKernelGGL(augment_warp_k<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(augment_warp_k<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
  COMA_LAUNCH_CHECK();
  return 0;
}
