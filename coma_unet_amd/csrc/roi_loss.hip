// ROI-weighted voxel losses (the reference's criterions.py:28-122 RoiRRMSE / RoiRSE, and the plain weighted MSE): every
// voxel's squared error is weighted by the ROI weight of its label.  Per sample b with V voxels, w_v = roi_w[slot of the
// label] or `bg` for a label outside the table, d_v = p_v - g_v, N = sum w d^2:
//   kind 0 WMSE   D = sum w                                     loss = N / D         coef = 2 / D
//   kind 1 RSE    D = sum g^2 - 2 m sum g + V m^2, m = sum(w g) / V   loss = N / D   coef = 2 / D
//   kind 2 RRMSE  D = sum w g^2                                 loss = sqrt(N / D)   coef = 1 / (D loss)
// (RSE's D is sum (g - m)^2: the reference's UNWEIGHTED denominator about its weighted "mean" m = mean(w g), :109-112.)
// d loss / d p_v = coef w_v d_v.  Forward: one grid-stride launch keeps fp64 per-thread sums of the terms its kind needs and
// writes one record per block; a one-wave finalise adds the records in fixed order (no atomics, bitwise repeatable).
// Backward: one streaming launch that rebuilds w_v from the label table.  No clamps: D = 0, or N = 0 under RRMSE, give
// inf / nan by IEEE arithmetic as the reference's autograd does.
#include "common.h"

enum { RWL_WMSE = 0, RWL_RSE = 1, RWL_RRMSE = 2 };
enum { RWL_BLOCKS = 512, RWL_PER_BLOCK = 256 * 8, RWL_REC = 4 };      // grid cap, voxels per block below it, doubles per record

template <int KIND> struct rwl_ns { static constexpr int n = KIND == RWL_RSE ? 4 : 2; };

struct RwlP { const void* pred; int64_t sbp, ldp; const void* gt; int64_t sbg; const float* roi; int64_t sbr;
              const int32_t* ids; const float* w; int n_roi; float bg; int64_t V;
              double* partial; const float* gout; const float* coef; void* dp; int64_t sbd, ldd; };

// whole block calls this: ids / weights / label table into LDS
__device__ __forceinline__ void rwl_tables(const RwlP& p, int32_t* ids, float* w, signed char* lut) {
  if (threadIdx.x < p.n_roi) { ids[threadIdx.x] = p.ids[threadIdx.x]; w[threadIdx.x] = p.w[threadIdx.x]; }
  __syncthreads();
  roi_lut_build(lut, ids, p.n_roi);
}
__device__ __forceinline__ float rwl_weight(const signed char* lut, const int32_t* ids, const float* w, int n, float bg, float label) {
  const int slot = roi_lut_slot(lut, ids, n, label);
  return slot >= 0 ? w[slot] : bg;
}

// s: {N, sum w | sum g^2 | sum w g^2, -, - | sum g, sum w g}
template <int KIND>
__device__ __forceinline__ void rwl_acc(double* s, float w, float pv, float gv) {
  const float d = pv - gv;
  const double wd = (double)w, gd = (double)gv;
  s[0] += wd * ((double)d * (double)d);
  if (KIND == RWL_WMSE) s[1] += wd;
  if (KIND == RWL_RSE) { s[1] += gd * gd; s[2] += gd; s[3] += wd * gd; }
  if (KIND == RWL_RRMSE) s[1] += wd * (gd * gd);
}

// partial[(b * nblk + blk) * RWL_REC + k], k < rwl_ns<KIND>::n
template <typename T, int KIND, int VEC>
__global__ __launch_bounds__(256) void roi_wloss_partial_k(const RwlP p) {
  constexpr int NS = rwl_ns<KIND>::n;
  __shared__ int32_t ids[64];
  __shared__ float w[64];
  __shared__ signed char lut[COMA_ROI_LUT];
  __shared__ double sh[4][NS];
  rwl_tables(p, ids, w, lut);
  const int b = blockIdx.y;
  const T* pb = reinterpret_cast<const T*>(p.pred) + b * p.sbp;
  const T* gb = reinterpret_cast<const T*>(p.gt) + b * p.sbg;
  const float* rb = p.roi + b * p.sbr;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  if (VEC == 4) {       // (host: voxel pitch 1, 16-byte / 8-byte aligned sample bases)
    const int64_t nq = p.V >> 2;
    for (int64_t q = t0; q < nq; q += step) {
      float pv[4], gv[4], rv[4];
      vec_io<T, 4>::load(pb + 4 * q, pv);
      vec_io<T, 4>::load(gb + 4 * q, gv);
      vec_io<float, 4>::load(rb + 4 * q, rv);
#pragma unroll
      for (int j = 0; j < 4; ++j) rwl_acc<KIND>(s, rwl_weight(lut, ids, w, p.n_roi, p.bg, rv[j]), pv[j], gv[j]);
    }
    const int64_t v = 4 * nq + t0;       // the V % 4 tail voxels
    if (v < p.V) rwl_acc<KIND>(s, rwl_weight(lut, ids, w, p.n_roi, p.bg, rb[v]), ld_f(pb + v), ld_f(gb + v));
  } else {
    for (int64_t v = t0; v < p.V; v += step)
      rwl_acc<KIND>(s, rwl_weight(lut, ids, w, p.n_roi, p.bg, rb[v]), ld_f(pb + v * p.ldp), ld_f(gb + v));
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < NS)
    p.partial[((int64_t)b * gridDim.x + blockIdx.x) * RWL_REC + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// one 64-lane wave per sample: lane-strided sums of the block records in fixed order, then a butterfly
template <int KIND>
__global__ __launch_bounds__(64) void roi_wloss_finalize_k(const double* partial, int nblk, int64_t V, float* loss, float* coef) {
  constexpr int NS = rwl_ns<KIND>::n;
  const int b = blockIdx.x, lane = threadIdx.x;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = 0.0;
  for (int i = lane; i < nblk; i += 64) {
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] += partial[((int64_t)b * nblk + i) * RWL_REC + k];
  }
#pragma unroll
  for (int k = 0; k < NS; ++k)
    for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
  if (lane != 0) return;
  double D, l, c;
  if (KIND == RWL_RSE) {
    const double m = s[3] / (double)V;          // the reference's mean(mask * gt)
    D = (s[1] - 2.0 * m * s[2]) + (double)V * m * m;
  } else {
    D = s[1];
  }
  if (KIND == RWL_RRMSE) { l = sqrt(s[0] / D); c = 1.0 / (D * l); }
  else { l = s[0] / D; c = 2.0 / D; }
  loss[b] = (float)l;
  coef[b] = (float)c;
}

// dp_v = ((gout_b coef_b) w_v) d_v, the same per-voxel arithmetic on both paths
template <typename T, int VEC>
__global__ __launch_bounds__(256) void roi_wloss_bwd_k(const RwlP p) {
  __shared__ int32_t ids[64];
  __shared__ float w[64];
  __shared__ signed char lut[COMA_ROI_LUT];
  rwl_tables(p, ids, w, lut);
  const int b = blockIdx.y;
  const T* pb = reinterpret_cast<const T*>(p.pred) + b * p.sbp;
  const T* gb = reinterpret_cast<const T*>(p.gt) + b * p.sbg;
  const float* rb = p.roi + b * p.sbr;
  T* ob = reinterpret_cast<T*>(p.dp) + b * p.sbd;
  const float scale = p.gout[b] * p.coef[b];
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (VEC == 4) {
    const int64_t nq = p.V >> 2;
    for (int64_t q = t0; q < nq; q += step) {
      float pv[4], gv[4], rv[4], o[4];
      vec_io<T, 4>::load(pb + 4 * q, pv);
      vec_io<T, 4>::load(gb + 4 * q, gv);
      vec_io<float, 4>::load(rb + 4 * q, rv);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (scale * rwl_weight(lut, ids, w, p.n_roi, p.bg, rv[j])) * (pv[j] - gv[j]);
      vec_io<T, 4>::store(ob + 4 * q, o);
    }
    const int64_t v = 4 * nq + t0;
    if (v < p.V) st_f(ob + v, (scale * rwl_weight(lut, ids, w, p.n_roi, p.bg, rb[v])) * (ld_f(pb + v) - ld_f(gb + v)));
  } else {
    for (int64_t v = t0; v < p.V; v += step)
      st_f(ob + v * p.ldd, (scale * rwl_weight(lut, ids, w, p.n_roi, p.bg, rb[v])) * (ld_f(pb + v * p.ldp) - ld_f(gb + v)));
  }
}

static int rwl_blocks(int64_t V) {
  int64_t nb = (V + RWL_PER_BLOCK - 1) / RWL_PER_BLOCK;
  if (nb > RWL_BLOCKS) nb = RWL_BLOCKS;
  return (int)(nb < 1 ? 1 : nb);
}
// 4 voxels per lane: voxel pitch 1, sample stride a multiple of 4, base on a 4-element boundary
static bool rwl_vec4(const coma_tensor* t) {
  return t->ld == 1 && t->sb % 4 == 0 && ((uintptr_t)t->data % (4 * esize(t->dtype))) == 0;
}
static int rwl_check(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, const int32_t* ids, const float* w,
                     int n_roi, const char* who) {
  COMA_CHECK(pred && gt && roi && pred->data && gt->data && roi->data && ids && w, "%s: null argument", who);
  COMA_CHECK(n_roi >= 1 && n_roi <= 64, "%s: n_roi=%d out of range 1..64", who, n_roi);
  COMA_CHECK(t_same_grid(pred, gt) && t_same_grid(pred, roi) && pred->C == 1 && gt->C == 1 && roi->C == 1,
             "%s: pred / gt / roi must be single-channel volumes of equal shape", who);
  COMA_CHECK((pred->dtype == COMA_F32 || pred->dtype == COMA_BF16) && pred->dtype == gt->dtype, "%s: pred / gt dtype mismatch", who);
  COMA_CHECK(roi->dtype == COMA_F32 && roi->ld == 1 && gt->ld == 1, "%s: roi must be fp32, roi and gt of voxel pitch 1", who);
  return 0;
}
static RwlP rwl_params(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, const int32_t* ids, const float* w,
                       int n_roi, float bg) {
  RwlP p{};
  p.pred = pred->data; p.sbp = pred->sb; p.ldp = pred->ld; p.gt = gt->data; p.sbg = gt->sb;
  p.roi = (const float*)roi->data; p.sbr = roi->sb; p.ids = ids; p.w = w; p.n_roi = n_roi; p.bg = bg; p.V = t_vox(pred);
  return p;
}

extern "C" size_t coma_roi_wloss_ws_bytes(const coma_tensor* pred) {
  return (size_t)pred->B * RWL_BLOCKS * RWL_REC * sizeof(double);
}

extern "C" int coma_roi_wloss_fwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, const int32_t* roi_ids,
                                  const float* roi_w, int32_t n_roi, float bg_weight, int32_t kind, float* loss, float* coef,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (rwl_check(pred, gt, roi, roi_ids, roi_w, n_roi, "roi_wloss_fwd")) return 1;
  COMA_CHECK(loss && coef && ws, "roi_wloss_fwd: null argument");
  COMA_CHECK(kind >= 0 && kind <= 2, "roi_wloss_fwd: kind=%d out of range 0..2", kind);
  COMA_CHECK(ws_bytes >= coma_roi_wloss_ws_bytes(pred), "roi_wloss_fwd: workspace too small");
  RwlP p = rwl_params(pred, gt, roi, roi_ids, roi_w, n_roi, bg_weight);
  p.partial = (double*)ws;
  const int nblk = rwl_blocks(p.V);
  const bool v4 = rwl_vec4(pred) && rwl_vec4(gt) && rwl_vec4(roi);
  dim3 grid(nblk, pred->B);
  hipStream_t s = (hipStream_t)stream;
#define LK(T, K) do { if (v4) hipLaunchKernelGGL((roi_wloss_partial_k<T, K, 4>), grid, dim3(256), 0, s, p); \
                      else hipLaunchKernelGGL((roi_wloss_partial_k<T, K, 1>), grid, dim3(256), 0, s, p); } while (0)
#define LT(T) do { if (kind == RWL_WMSE) LK(T, RWL_WMSE); else if (kind == RWL_RSE) LK(T, RWL_RSE); else LK(T, RWL_RRMSE); } while (0)
  if (pred->dtype == COMA_F32) LT(float); else LT(bf16_t);
#undef LT
#undef LK
  COMA_LAUNCH_CHECK();
#define LF(K) hipLaunchKernelGGL(roi_wloss_finalize_k<K>, dim3(pred->B), dim3(64), 0, s, (const double*)ws, nblk, p.V, loss, coef)
  if (kind == RWL_WMSE) LF(RWL_WMSE); else if (kind == RWL_RSE) LF(RWL_RSE); else LF(RWL_RRMSE);
#undef LF
  COMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int coma_roi_wloss_bwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, const int32_t* roi_ids,
                                  const float* roi_w, int32_t n_roi, float bg_weight, const float* gout, const float* coef,
                                  const coma_tensor* dpred, void* stream) {
  if (rwl_check(pred, gt, roi, roi_ids, roi_w, n_roi, "roi_wloss_bwd")) return 1;
  COMA_CHECK(gout && coef && dpred && dpred->data, "roi_wloss_bwd: null argument");
  COMA_CHECK(t_same_grid(pred, dpred) && dpred->C == 1 && dpred->dtype == pred->dtype, "roi_wloss_bwd: dpred shape/dtype mismatch");
  RwlP p = rwl_params(pred, gt, roi, roi_ids, roi_w, n_roi, bg_weight);
  p.gout = gout; p.coef = coef; p.dp = dpred->data; p.sbd = dpred->sb; p.ldd = dpred->ld;
  const bool v4 = rwl_vec4(pred) && rwl_vec4(gt) && rwl_vec4(roi) && rwl_vec4(dpred);
  int64_t nb = ((v4 ? (p.V + 3) / 4 : p.V) + 255) / 256;
  if (nb > 8192) nb = 8192;
  dim3 grid((unsigned)(nb < 1 ? 1 : nb), pred->B);
  hipStream_t s = (hipStream_t)stream;
#define LB(T) do { if (v4) hipLaunchKernelGGL((roi_wloss_bwd_k<T, 4>), grid, dim3(256), 0, s, p); \
                   else hipLaunchKernelGGL((roi_wloss_bwd_k<T, 1>), grid, dim3(256), 0, s, p); } while (0)
  if (pred->dtype == COMA_F32) LB(float); else LB(bf16_t);
#undef LB
  COMA_LAUNCH_CHECK();
  return 0;
}
