// Gaussian smoothing of the tau target (DESIGN.md section 4 "Target smoothing"): ONE launch filters a contiguous fp32
// (B, D, H, W) batch with a separable filter whose taps are given per axis, zero padding or edge replication.
// A block owns a TZ x 8 x 32 tile of OUTPUT voxels.  Its halo, widened only along the axes that are filtered, is staged
// once into LDS; the passes run there in the order x, y, z, ping-ponging between two buffers, and the last active pass
// stores to global memory.  A lane owns four consecutive x of one row in every pass (16-byte LDS reads, 16-byte stores
// where W and the alignment allow).  Every output voxel has one owner: no atomics, bitwise repeatable.
// Arithmetic contract (include/coma_unet.h): per pass s = 0, then s = fmaf(w[k], v[k], s) for k ascending; s is an fp32
// value in LDS before the next pass reads it.
// With a fused source the halo is staged THROUGH the input pipeline's nearest-neighbour index map (resample.h) from the raw
// volume: the staged values are the ones coma_resample_nearest would have written, so the result is bit for bit the
// two-step one without the intermediate volume.
#include "common.h"
#include "resample.h"

#define SM_TX COMA_SMOOTH_TILE_X
#define SM_TY COMA_SMOOTH_TILE_Y
#define SM_MAXN (2 * COMA_SMOOTH_MAX_RADIUS + 1)
#define SM_STAGE 8                   // staging loads a lane keeps in flight
static_assert(SM_TX == 32 && SM_TY == 8, "the pass loops decode (row, quad) with shifts for an 8 x 32 tile face");

struct SmoothP {
  const float* in;                  // (B, D, H, W), or nullptr with a fused source
  float* out;                       // (B, D, H, W)
  int D, H, W;
  int ntx, nty;
  int nz, ny, nx;                   // taps per axis (odd), 0: the axis is skipped
  int last;                         // the last active axis (0 x, 1 y, 2 z; -1: none), whose pass stores to global memory
  int nearest, vec;
  float w[3][SM_MAXN];              // z, y, x
  const float* src; int Dz, Hy, Wx; // fused source: raw (B, Dz, Hy, Wx) volumes ...
  double qz, qy, qx;                // ... new_spacing / old_spacing per axis ...
  float default_value; int nan_to_num;
};

// one pass along an axis for four x-adjacent outputs: v is read through `at(k)`, a float4 of the four columns at tap k
template <int RMAX, int AXIS, typename At>
__device__ __forceinline__ void sm_chain(const SmoothP& p, int n, float (&s)[4], At at) {
  s[0] = s[1] = s[2] = s[3] = 0.f;
#pragma unroll
  for (int k = 0; k < 2 * RMAX + 1; ++k)
    if (k < n) {
      const float4 v = at(k);
      const float w = p.w[AXIS][k];
      s[0] = fmaf(w, v.x, s[0]); s[1] = fmaf(w, v.y, s[1]); s[2] = fmaf(w, v.z, s[2]); s[3] = fmaf(w, v.w, s[3]);
    }
}

// RMAX: the largest radius this instantiation has LDS for; TZ: tile depth; ZH: the z axis has a halo; SRC: fused source
template <int RMAX, int TZ, bool ZH, bool SRC>
__global__ __launch_bounds__(256) void gauss_smooth_k(SmoothP p) {
  constexpr int TX = SM_TX, TY = SM_TY;
  constexpr int AZ = ZH ? TZ + 2 * RMAX : TZ, AY = TY + 2 * RMAX, AXS = TX + 2 * RMAX;
  static_assert(AXS % 4 == 0, "a staged row is padded to 16 bytes");
  __shared__ __attribute__((aligned(16))) float bufA[AZ * AY * AXS];     // the halo; later the y pass's output
  __shared__ __attribute__((aligned(16))) float bufB[AZ * AY * TX];      // the x pass's output
  const int tid = threadIdx.x, b = blockIdx.y;
  int t = blockIdx.x;
  const int tx = t % p.ntx; t /= p.ntx;
  const int ty = t % p.nty; const int tz = t / p.nty;
  const int x0 = tx * TX, y0 = ty * TY, z0 = tz * TZ;
  const int rz = ZH ? p.nz >> 1 : 0, ry = p.ny >> 1, rx = p.nx >> 1;
  const int eZ = TZ + 2 * rz, eY = TY + 2 * ry;                // staged extents; a skipped axis has no halo
  const int xs = TX + ((2 * rx + 3) & ~3);                     // staged row stride: TX + 2 rx, rounded up to 16 bytes
  const int64_t V = (int64_t)p.D * p.H * p.W;

  // ---- stage the halo: element e of [eZ][eY][xs] per lane, SM_STAGE loads in flight per lane before the first LDS write
  //      (one load per trip left every block waiting out a full memory latency per 256 elements) ----------------------
  {
    const int total = eZ * eY * xs;
    // e / xs and r / eY through a reciprocal: e < 2^15 and the quotient of (e + 0.5) is at least 0.5 / 48 away from an
    // integer, far beyond the rounding of the product
    const float inv_xs = 1.f / (float)xs, inv_ey = 1.f / (float)eY;
    auto fetch = [&](int e) -> float {
      const int r = (int)(((float)e + 0.5f) * inv_xs), lx = e - r * xs;
      const int iz = (int)(((float)r + 0.5f) * inv_ey), iy = r - iz * eY;
      int gz = z0 - rz + iz, gy = y0 - ry + iy, gx = x0 - rx + lx;
      // the load itself is unconditional, from a clamped address, and its value is dropped where it does not apply: loads
      // behind a branch would not be issued back to back
      const bool keep = p.nearest || (gz >= 0 && gz < p.D && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W);
      gz = min(max(gz, 0), p.D - 1); gy = min(max(gy, 0), p.H - 1); gx = min(max(gx, 0), p.W - 1);
      float v;
      if (SRC) {
        const int sz = nn_index(gz, p.qz, p.Dz), sy = nn_index(gy, p.qy, p.Hy), sx = nn_index(gx, p.qx, p.Wx);
        v = p.src[(((int64_t)b * p.Dz + max(sz, 0)) * p.Hy + max(sy, 0)) * p.Wx + max(sx, 0)];
        if (sx < 0 || sy < 0 || sz < 0) v = p.default_value;
        if (p.nan_to_num) v = nan_to_num_f(v);
      } else {
        v = p.in[b * V + ((int64_t)gz * p.H + gy) * p.W + gx];
      }
      return keep ? v : 0.f;
    };
    for (int e0 = tid; e0 < total; e0 += 256 * SM_STAGE) {
      float v[SM_STAGE];
#pragma unroll
      for (int u = 0; u < SM_STAGE; ++u) v[u] = fetch(min(e0 + 256 * u, total - 1));
#pragma unroll
      for (int u = 0; u < SM_STAGE; ++u)
        if (e0 + 256 * u < total) bufA[e0 + 256 * u] = v[u];
    }
  }
  __syncthreads();

  float* out = p.out + b * V;
  // the four outputs of lane-quad q in row (z, y) of the tile leave for global memory
  auto store = [&](int z, int y, int q, const float (&s)[4]) {
    const int gz = z0 + z, gy = y0 + y, gx = x0 + 4 * q;
    if (gz >= p.D || gy >= p.H || gx >= p.W) return;
    float* o = out + ((int64_t)gz * p.H + gy) * p.W + gx;
    if (p.vec) vec_io<float, 4>::store(o, s);
    else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (gx + j < p.W) o[j] = s[j];
    }
  };

  const float* cur = bufA;          // [eZ][eY][xs]; from the x pass on [.][.][TX]
  if (p.nx > 0) {                   // ---- x pass: rows eZ * eY, eight quads each ----
    for (int i = tid; i < eZ * eY * 8; i += 256) {
      const int q = i & 7, r = i >> 3;
      const float* a = bufA + r * xs + 4 * q;
      float v[4 + 2 * RMAX];
#pragma unroll
      for (int j = 0; j < (4 + 2 * RMAX) / 4; ++j) {
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * j < 4 + 2 * rx) u = *reinterpret_cast<const float4*>(a + 4 * j);
        v[4 * j] = u.x; v[4 * j + 1] = u.y; v[4 * j + 2] = u.z; v[4 * j + 3] = u.w;
      }
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 2 * RMAX + 1; ++k)
        if (k < p.nx) {
#pragma unroll
          for (int j = 0; j < 4; ++j) s[j] = fmaf(p.w[2][k], v[j + k], s[j]);
        }
      if (p.last == 0) store(r >> 3, r & 7, q, s);            // (no later pass: eZ = TZ, eY = TY)
      else vec_io<float, 4>::store(bufB + r * TX + 4 * q, s);
    }
    if (p.last == 0) return;
    __syncthreads();
    cur = bufB;
  }
  if (p.ny > 0) {                   // ---- y pass: eZ planes of TY x 8 quads ----
    float* dst = cur == bufA ? bufB : bufA;
    for (int i = tid; i < eZ * TY * 8; i += 256) {
      const int q = i & 7, y = (i >> 3) & 7, z = i >> 6;
      const float* a = cur + (z * eY + y) * TX + 4 * q;
      float s[4];
      sm_chain<RMAX, 1>(p, p.ny, s, [&](int k) { return *reinterpret_cast<const float4*>(a + k * TX); });
      if (p.last == 1) store(z, y, q, s);
      else vec_io<float, 4>::store(dst + (z * TY + y) * TX + 4 * q, s);
    }
    if (p.last == 1) return;
    __syncthreads();
    cur = dst;
  }
  // ---- z pass, or the plain copy when no axis is filtered: [eZ][TY][TX] -> global ----
  for (int i = tid; i < TZ * TY * 8; i += 256) {
    const int q = i & 7, y = (i >> 3) & 7, z = i >> 6;
    const float* a = cur + (z * TY + y) * TX + 4 * q;
    float s[4];
    if (p.nz > 0) sm_chain<RMAX, 0>(p, p.nz, s, [&](int k) { return *reinterpret_cast<const float4*>(a + k * TY * TX); });
    else vec_io<float, 4>::load(a, s);
    store(z, y, q, s);
  }
}

static inline bool sm_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

template <int RMAX, int TZ, bool ZH>
static void sm_launch(const SmoothP& p, bool fused, dim3 grid, hipStream_t s) {
  if (fused) hipLaunchKernelGGL((gauss_smooth_k<RMAX, TZ, ZH, true>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((gauss_smooth_k<RMAX, TZ, ZH, false>), grid, dim3(256), 0, s, p);
}

extern "C" void coma_gauss_smooth3d_tile(int32_t radius, int32_t z_filtered, int32_t* tz, int32_t* ty, int32_t* tx) {
  *tz = radius > COMA_SMOOTH_SMALL_RADIUS && z_filtered ? COMA_SMOOTH_TILE_Z / 2 : COMA_SMOOTH_TILE_Z;
  *ty = COMA_SMOOTH_TILE_Y; *tx = COMA_SMOOTH_TILE_X;
}

extern "C" int coma_gauss_smooth3d(const float* in, float* out, int32_t B, int32_t D, int32_t H, int32_t W, const float* taps_z,
                                   int32_t nz, const float* taps_y, int32_t ny, const float* taps_x, int32_t nx, int32_t boundary,
                                   const float* src, int32_t Dz, int32_t Hy, int32_t Wx, double sp_z, double sp_y, double sp_x,
                                   double nsp_z, double nsp_y, double nsp_x, float default_value, int32_t nan_to_num, void* stream) {
  COMA_CHECK(out && ((in != nullptr) != (src != nullptr)), "gauss_smooth3d: an output and exactly one of `in` and `src` expected");
  COMA_CHECK(B > 0 && D > 0 && H > 0 && W > 0 && B <= 65535, "gauss_smooth3d: bad shape (%d, %d, %d, %d)", B, D, H, W);
  COMA_CHECK(boundary == COMA_SMOOTH_ZEROS || boundary == COMA_SMOOTH_NEAREST, "gauss_smooth3d: unknown boundary mode %d", boundary);
  const float* taps[3] = {taps_z, taps_y, taps_x};
  int n[3] = {taps_z ? nz : 0, taps_y ? ny : 0, taps_x ? nx : 0};
  int rmax = 0, last = -1;
  for (int a = 0; a < 3; ++a) {
    COMA_CHECK(n[a] >= 0 && (n[a] == 0 || n[a] % 2 == 1), "gauss_smooth3d: axis %d has %d taps (an odd count, or 0 to skip the axis)", a, n[a]);
    COMA_CHECK(n[a] <= SM_MAXN, "gauss_smooth3d: axis %d has radius %d > %d", a, n[a] / 2, COMA_SMOOTH_MAX_RADIUS);
    if (n[a] / 2 > rmax) rmax = n[a] / 2;
  }
  if (n[0] > 0) last = 2; else if (n[1] > 0) last = 1; else if (n[2] > 0) last = 0;
  const size_t bytes = (size_t)B * D * H * W * sizeof(float);
  if (in) COMA_CHECK(!sm_overlap(in, bytes, out, bytes), "gauss_smooth3d: input and output overlap (the filter gathers: not in place)");
  if (src) {
    COMA_CHECK(Dz > 0 && Hy > 0 && Wx > 0, "gauss_smooth3d: bad source shape (%d, %d, %d)", Dz, Hy, Wx);
    COMA_CHECK(sp_z > 0 && sp_y > 0 && sp_x > 0 && nsp_z > 0 && nsp_y > 0 && nsp_x > 0, "gauss_smooth3d: spacings must be positive");
    COMA_CHECK(!sm_overlap(src, (size_t)B * Dz * Hy * Wx * sizeof(float), out, bytes), "gauss_smooth3d: source and output overlap");
  }
  const bool zh = n[0] > 1;
  int32_t tz, ty, tx;
  coma_gauss_smooth3d_tile(rmax, zh, &tz, &ty, &tx);
  const int64_t ntx = (W + tx - 1) / tx, nty = (H + ty - 1) / ty, ntz = (D + tz - 1) / tz;
  COMA_CHECK(ntx * nty * ntz <= 2147483647LL, "gauss_smooth3d: volume too large for one launch");
  SmoothP p;
  p.in = in; p.out = out; p.D = D; p.H = H; p.W = W; p.ntx = (int)ntx; p.nty = (int)nty;
  p.nz = n[0]; p.ny = n[1]; p.nx = n[2]; p.last = last;
  p.nearest = boundary == COMA_SMOOTH_NEAREST;
  p.vec = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
  for (int a = 0; a < 3; ++a)
    for (int k = 0; k < SM_MAXN; ++k) p.w[a][k] = k < n[a] ? taps[a][k] : 0.f;
  p.src = src; p.Dz = Dz; p.Hy = Hy; p.Wx = Wx;
  p.qz = p.qy = p.qx = 1.0;
  if (src) { p.qz = nsp_z / sp_z; p.qy = nsp_y / sp_y; p.qx = nsp_x / sp_x; }
  p.default_value = default_value; p.nan_to_num = nan_to_num;
  const dim3 grid((unsigned)(ntx * nty * ntz), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (rmax <= COMA_SMOOTH_SMALL_RADIUS) {
    if (zh) sm_launch<COMA_SMOOTH_SMALL_RADIUS, COMA_SMOOTH_TILE_Z, true>(p, src != nullptr, grid, s);
    else sm_launch<COMA_SMOOTH_SMALL_RADIUS, COMA_SMOOTH_TILE_Z, false>(p, src != nullptr, grid, s);
  } else {
    if (zh) sm_launch<COMA_SMOOTH_MAX_RADIUS, COMA_SMOOTH_TILE_Z / 2, true>(p, src != nullptr, grid, s);
    else sm_launch<COMA_SMOOTH_MAX_RADIUS, COMA_SMOOTH_TILE_Z, false>(p, src != nullptr, grid, s);
  }
  COMA_LAUNCH_CHECK();
  return 0;
}
