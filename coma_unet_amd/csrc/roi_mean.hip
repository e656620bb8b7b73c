// ROI-mean (per-region SUVR) loss: a loss on the regional means the validation loop reports (RoiCorrMetric, attn_unet_data_
// parallel.py:49-60).  Per sample b and table slot r (id_r, w_r): n_r = #{v: label_v == id_r}, d_r = mean_r(pred) - mean_r(gt),
//   loss_b = sum_{r: n_r > 0} w_r phi(d_r) / sum_{r: n_r > 0} w_r,   phi = d^2 (kind 0) | |d| (kind 1) | huber_delta(d) (kind 2)
//   d loss_b / d pred_v = coef[b][r(v)],   coef[b][r] = w_r phi'(d_r) / (n_r sum w)       (0 for a voxel in no region)
// A sample with no present region, or sum w = 0, has loss 0 and coef 0 (never NaN: the augmentation can push a region out).
//
// Forward: one label-segmented reduction.  Every wave handles 256 consecutive voxels per trip, 4 consecutive ones per lane
// (the same voxels on the 16-byte path and on the scalar path, so both add in the same order).  A lane first adds its own
// voxels of one slot; labels come in runs along x, so a segmented inclusive scan over the lanes (6 shuffle steps, whatever the
// labels are) leaves every run's sums in its last lane; those few lanes are then read one after the other (v_readlane) and
// lane r, which OWNS slot r of its wave, adds what belongs to r to accumulators it keeps in registers for the whole kernel.
// The block adds its four waves in fixed order into one record of n_roi x {count, sum pred, sum gt}; a one-block finalise adds
// the records in fixed order.  No atomics anywhere and no LDS read-modify-write: the order of every addition is fixed by the
// labels and the grid, so the result is bitwise repeatable.  The work per trip grows with the number of runs among a wave's
// 256 voxels (a handful on a parcellation, 256 on independent random labels); correctness does not depend on it.
// Backward: one streaming launch that reads only the labels.
#include "common.h"
#include <math.h>

enum { RM_MSE = 0, RM_L1 = 1, RM_HUBER = 2 };
enum { RM_BLOCKS = 512, RM_PER_BLOCK = 256 * 8, RM_WAVE_VOX = 256, RM_SLOTS = 64, RM_REC = 3 * RM_SLOTS,   // doubles per block record [k][slot]
       RM_FIN_THREADS = 1024, RM_FIN_PARTS = 16, RM_BWD_BLOCKS = 8192 };

struct RmP { const void* pred; int64_t sbp, ldp; const void* gt; int64_t sbg; const float* roi; int64_t sbr;
             const int32_t* ids; int n_roi; int64_t V; double* partial;
             const float* gout; const float* coef; void* dp; int64_t sbd, ldd; };

// whole block calls this: ids / label table into LDS
__device__ __forceinline__ void rm_tables(const RmP& p, int32_t* ids, signed char* lut) {
  if (threadIdx.x < p.n_roi) ids[threadIdx.x] = p.ids[threadIdx.x];
  __syncthreads();
  roi_lut_build(lut, ids, p.n_roi);
}

__device__ __forceinline__ double rm_readlane(double x, int k) {      // k wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), k), __builtin_amdgcn_readlane(__double2loint(x), k));
}

// lane r's running sums of slot r over everything its wave has seen
struct RmAcc { int c; double sp, sg; };

// Whole wave calls this (every lane active): one value per lane, (c, sp, sg) of slot s (s < 0: nothing).
__device__ __forceinline__ void rm_wave_add(int s, int c, double sp, double sg, RmAcc& acc) {
  const int lane = threadIdx.x & 63;
  // runs of equal slots over consecutive lanes: segmented inclusive scan, a run's last lane ends up with the run's sums
  const int prev = __shfl_up(s, 1, 64);                             // (every cross-lane step outside any lane-dependent branch)
  int f = (lane == 0 || prev != s) ? 1 : 0;                         // head of a run
  const int next_head = __shfl_down(f, 1, 64);
  const bool tail = lane == 63 || next_head != 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int c2 = __shfl_up(c, d, 64), f2 = __shfl_up(f, d, 64);
    const double sp2 = __shfl_up(sp, d, 64), sg2 = __shfl_up(sg, d, 64);
    if (lane >= d && !f) { c += c2; sp += sp2; sg += sg2; f = f2; }
  }
  // the runs' last lanes, in lane order: lane r takes what belongs to slot r (s < n_roi <= 64: roi_lut_slot's range)
  unsigned long long pend = __ballot(tail && s >= 0);
  while (pend) {
    const int k = __builtin_amdgcn_readfirstlane(__ffsll((long long)pend) - 1);
    pend &= pend - 1;
    const int ks = __builtin_amdgcn_readlane(s, k), kc = __builtin_amdgcn_readlane(c, k);
    const double ksp = rm_readlane(sp, k), ksg = rm_readlane(sg, k);
    if (lane == ks) { acc.c += kc; acc.sp += ksp; acc.sg += ksg; }
  }
}

// Whole wave calls this.  slot[j] < 0: nothing to add (no region, or past the volume).  One pass per distinct slot among a
// lane's own 4 voxels (one, but for the lanes a run ends in).
__device__ __forceinline__ void rm_trip(const int slot[4], const float pv[4], const float gv[4], RmAcc& acc) {
  unsigned todo = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) todo |= (slot[j] >= 0 ? 1u : 0u) << j;
  while (__ballot(todo != 0)) {
    const int mine = (todo & 1u) ? slot[0] : (todo & 2u) ? slot[1] : (todo & 4u) ? slot[2] : (todo & 8u) ? slot[3] : -1;
    int c = 0;
    double sp = 0.0, sg = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (((todo >> j) & 1u) && slot[j] == mine) { c += 1; sp += (double)pv[j]; sg += (double)gv[j]; todo &= ~(1u << j); }
    rm_wave_add(mine, c, sp, sg, acc);
  }
}

// partial[(b * nblk + blk) * RM_REC + k * RM_SLOTS + r], k: {count, sum pred, sum gt}, r < n_roi
template <typename T, int VEC>
__global__ __launch_bounds__(256) void roi_mean_partial_k(const RmP p) {
  __shared__ int32_t ids[64];
  __shared__ signed char lut[COMA_ROI_LUT];
  __shared__ double bins[4][RM_REC];
  rm_tables(p, ids, lut);
  const int b = blockIdx.y;
  const T* pb = reinterpret_cast<const T*>(p.pred) + b * p.sbp;
  const T* gb = reinterpret_cast<const T*>(p.gt) + b * p.sbg;
  const float* rb = p.roi + b * p.sbr;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RmAcc acc = {0, 0.0, 0.0};
  // wave-uniform loop: every lane of a wave makes the same trips, so the cross-lane steps see all 64 lanes
  const int64_t step = (int64_t)gridDim.x * 4 * RM_WAVE_VOX;
  for (int64_t c0 = ((int64_t)blockIdx.x * 4 + wave) * RM_WAVE_VOX; c0 < p.V; c0 += step) {
    float pv[4], gv[4], rv[4];
    int slot[4];
    const int64_t v = c0 + 4 * lane;
    if (VEC == 4 && v + 3 < p.V) {      // (host: voxel pitch 1, 16-byte / 8-byte aligned sample bases)
      vec_io<T, 4>::load(pb + v, pv);
      vec_io<T, 4>::load(gb + v, gv);
      vec_io<float, 4>::load(rb + v, rv);
#pragma unroll
      for (int j = 0; j < 4; ++j) slot[j] = roi_lut_slot(lut, ids, p.n_roi, rv[j]);
    } else {                            // the scalar path; on the 16-byte path the group that holds the V % 4 tail voxels
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = v + j < p.V;
        pv[j] = in ? ld_f(pb + (v + j) * p.ldp) : 0.f;
        gv[j] = in ? ld_f(gb + v + j) : 0.f;
        slot[j] = in ? roi_lut_slot(lut, ids, p.n_roi, rb[v + j]) : -1;
      }
    }
    rm_trip(slot, pv, gv, acc);
  }
  bins[wave][lane] = (double)acc.c;
  bins[wave][RM_SLOTS + lane] = acc.sp;
  bins[wave][2 * RM_SLOTS + lane] = acc.sg;
  __syncthreads();
  if (threadIdx.x < RM_REC && (threadIdx.x & (RM_SLOTS - 1)) < p.n_roi) {
    const int i = threadIdx.x;
    p.partial[((int64_t)b * gridDim.x + blockIdx.x) * RM_REC + i] = ((bins[0][i] + bins[1][i]) + bins[2][i]) + bins[3][i];
  }
}

// Whole block (RM_FIN_THREADS) calls this: thread (part, r) adds slot r of the records part, part + 16, ... in order, then the
// parts are added in order.  -> tot[k][r], r < 64 (zeros for r >= n_roi)
__device__ __forceinline__ void rm_sum_records(const double* partial, int nblk, int n_roi, double (*sh)[3][RM_SLOTS],
                                               double (*tot)[RM_SLOTS]) {
  const int r = threadIdx.x & 63, part = threadIdx.x >> 6;
  double s[3] = {0.0, 0.0, 0.0};
  if (r < n_roi) {
#pragma unroll 4
    for (int i = part; i < nblk; i += RM_FIN_PARTS) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] += partial[((int64_t)blockIdx.x * nblk + i) * RM_REC + k * RM_SLOTS + r];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) sh[part][k][r] = s[k];
  __syncthreads();
  if (threadIdx.x < 3 * RM_SLOTS) {
    const int k = threadIdx.x >> 6;
    double t = sh[0][k][r];
#pragma unroll
    for (int q = 1; q < RM_FIN_PARTS; ++q) t += sh[q][k][r];
    tot[k][r] = t;
  }
  __syncthreads();
}

// one block per sample: stats[b][r] = {n, sum pred, sum gt}
__global__ __launch_bounds__(RM_FIN_THREADS) void roi_mean_stats_k(const double* partial, int nblk, int n_roi, double* stats) {
  __shared__ double sh[RM_FIN_PARTS][3][RM_SLOTS];
  __shared__ double tot[3][RM_SLOTS];
  rm_sum_records(partial, nblk, n_roi, sh, tot);
  if (threadIdx.x < n_roi) {
#pragma unroll
    for (int k = 0; k < 3; ++k) stats[((int64_t)blockIdx.x * n_roi + threadIdx.x) * 3 + k] = tot[k][threadIdx.x];
  }
}

// one block per sample: loss[b], coef[b][r]
__global__ __launch_bounds__(RM_FIN_THREADS) void roi_mean_finalize_k(const double* partial, int nblk, const float* w, int n_roi,
                                                                      int kind, double delta, float* loss, float* coef) {
  __shared__ double sh[RM_FIN_PARTS][3][RM_SLOTS];
  __shared__ double tot[3][RM_SLOTS];
  rm_sum_records(partial, nblk, n_roi, sh, tot);
  if (threadIdx.x >= RM_SLOTS) return;            // one wave from here on
  const int r = threadIdx.x;
  const double n = tot[0][r];
  const bool present = r < n_roi && n > 0.0;
  double num = 0.0, den = 0.0, g = 0.0;           // w phi(d), w, w phi'(d) / n
  if (present) {
    const double wr = (double)w[r];
    const double d = tot[1][r] / n - tot[2][r] / n;
    const double a = fabs(d), sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    double phi, dphi;
    if (kind == RM_MSE) { phi = d * d; dphi = 2.0 * d; }
    else if (kind == RM_L1) { phi = a; dphi = sgn; }
    else if (a < delta) { phi = 0.5 * d * d; dphi = d; }
    else { phi = delta * (a - 0.5 * delta); dphi = delta * sgn; }
    num = wr * phi; den = wr; g = wr * dphi / n;
  }
  for (int o = 32; o > 0; o >>= 1) { num += __shfl_xor(num, o, 64); den += __shfl_xor(den, o, 64); }
  const bool live = den != 0.0;                   // no present region, or weights that cancel: loss and gradient exactly 0
  if (r == 0) loss[blockIdx.x] = live ? (float)(num / den) : 0.f;
  if (r < n_roi) coef[(int64_t)blockIdx.x * n_roi + r] = live ? (float)(g / den) : 0.f;
}

// dp_v = gout_b coef[b][slot of the label], 0 in no region; every voxel has one writer
template <typename T, int VEC>
__global__ __launch_bounds__(256) void roi_mean_bwd_k(const RmP p) {
  __shared__ int32_t ids[64];
  __shared__ float cf[64];
  __shared__ signed char lut[COMA_ROI_LUT];
  const int b = blockIdx.y;
  if (threadIdx.x < p.n_roi) cf[threadIdx.x] = p.gout[b] * p.coef[(int64_t)b * p.n_roi + threadIdx.x];
  rm_tables(p, ids, lut);
  const float* rb = p.roi + b * p.sbr;
  T* ob = reinterpret_cast<T*>(p.dp) + b * p.sbd;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (VEC == 4) {
    const int64_t nq = p.V >> 2;
    for (int64_t q = t0; q < nq; q += step) {
      float rv[4], o[4];
      vec_io<float, 4>::load(rb + 4 * q, rv);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int s = roi_lut_slot(lut, ids, p.n_roi, rv[j]); o[j] = s >= 0 ? cf[s] : 0.f; }
      vec_io<T, 4>::store(ob + 4 * q, o);
    }
    const int64_t v = 4 * nq + t0;       // the V % 4 tail voxels
    if (v < p.V) { const int s = roi_lut_slot(lut, ids, p.n_roi, rb[v]); st_f(ob + v, s >= 0 ? cf[s] : 0.f); }
  } else {
    for (int64_t v = t0; v < p.V; v += step) {
      const int s = roi_lut_slot(lut, ids, p.n_roi, rb[v]);
      st_f(ob + v * p.ldd, s >= 0 ? cf[s] : 0.f);
    }
  }
}

static int rm_blocks(int64_t V) {
  int64_t nb = (V + RM_PER_BLOCK - 1) / RM_PER_BLOCK;
  if (nb > RM_BLOCKS) nb = RM_BLOCKS;
  return (int)(nb < 1 ? 1 : nb);
}
// 4 voxels per lane: voxel pitch 1, sample stride a multiple of 4, base on a 4-element boundary
static bool rm_vec4(const coma_tensor* t) {
  return t->ld == 1 && t->sb % 4 == 0 && ((uintptr_t)t->data % (4 * esize(t->dtype))) == 0;
}
static int rm_check(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, const int32_t* ids, int n_roi,
                    const char* who) {
  COMA_CHECK(pred && gt && roi && pred->data && gt->data && roi->data && ids, "%s: null argument", who);
  COMA_CHECK(n_roi >= 1 && n_roi <= 64, "%s: n_roi=%d out of range 1..64", who, n_roi);
  COMA_CHECK(t_same_grid(pred, gt) && t_same_grid(pred, roi) && pred->C == 1 && gt->C == 1 && roi->C == 1,
             "%s: pred / gt / roi must be single-channel volumes of equal shape", who);
  COMA_CHECK((pred->dtype == COMA_F32 || pred->dtype == COMA_BF16) && pred->dtype == gt->dtype, "%s: pred / gt dtype mismatch", who);
  COMA_CHECK(roi->dtype == COMA_F32 && roi->ld == 1 && gt->ld == 1, "%s: roi must be fp32, roi and gt of voxel pitch 1", who);
  return 0;
}

extern "C" size_t coma_roi_mean_ws_bytes(const coma_tensor* pred) {
  return (size_t)pred->B * RM_BLOCKS * RM_REC * sizeof(double);
}

// the partial launch shared by the loss and the statistics; -> blocks per sample
static int rm_partial(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, const int32_t* ids, int n_roi, void* ws,
                      hipStream_t s) {
  RmP p{};
  p.pred = pred->data; p.sbp = pred->sb; p.ldp = pred->ld; p.gt = gt->data; p.sbg = gt->sb;
  p.roi = (const float*)roi->data; p.sbr = roi->sb; p.ids = ids; p.n_roi = n_roi; p.V = t_vox(pred);
  p.partial = (double*)ws;
  const int nblk = rm_blocks(p.V);
  const bool v4 = rm_vec4(pred) && rm_vec4(gt) && rm_vec4(roi);
  dim3 grid(nblk, pred->B);
#define LK(T) do { if (v4) hipLaunchKernelGGL((roi_mean_partial_k<T, 4>), grid, dim3(256), 0, s, p); \
                   else hipLaunchKernelGGL((roi_mean_partial_k<T, 1>), grid, dim3(256), 0, s, p); } while (0)
  if (pred->dtype == COMA_F32) LK(float); else LK(bf16_t);
#undef LK
  return nblk;
}

extern "C" int coma_roi_mean_fwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, const int32_t* roi_ids,
                                 const float* roi_w, int32_t n_roi, int32_t kind, float delta, float* loss, float* coef,
                                 void* ws, size_t ws_bytes, void* stream) {
  if (rm_check(pred, gt, roi, roi_ids, n_roi, "roi_mean_fwd")) return 1;
  COMA_CHECK(roi_w && loss && coef && ws, "roi_mean_fwd: null argument");
  COMA_CHECK(kind >= 0 && kind <= 2, "roi_mean_fwd: kind=%d out of range 0..2", kind);
  COMA_CHECK(kind != RM_HUBER || (delta > 0.f && isfinite(delta)), "roi_mean_fwd: huber delta=%g must be positive and finite", (double)delta);
  COMA_CHECK(ws_bytes >= coma_roi_mean_ws_bytes(pred), "roi_mean_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nblk = rm_partial(pred, gt, roi, roi_ids, n_roi, ws, s);
  COMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(roi_mean_finalize_k, dim3(pred->B), dim3(RM_FIN_THREADS), 0, s, (const double*)ws, nblk, roi_w, (int)n_roi,
                     (int)kind, (double)delta, loss, coef);
  COMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int coma_roi_region_stats(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, const int32_t* roi_ids,
                                     int32_t n_roi, double* stats, void* ws, size_t ws_bytes, void* stream) {
  if (rm_check(pred, gt, roi, roi_ids, n_roi, "roi_region_stats")) return 1;
  COMA_CHECK(stats && ws, "roi_region_stats: null argument");
  COMA_CHECK(ws_bytes >= coma_roi_mean_ws_bytes(pred), "roi_region_stats: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nblk = rm_partial(pred, gt, roi, roi_ids, n_roi, ws, s);
  COMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(roi_mean_stats_k, dim3(pred->B), dim3(RM_FIN_THREADS), 0, s, (const double*)ws, nblk, (int)n_roi, stats);
  COMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int coma_roi_mean_bwd(const coma_tensor* roi, const int32_t* roi_ids, int32_t n_roi, const float* gout, const float* coef,
                                 const coma_tensor* dpred, void* stream) {
  COMA_CHECK(roi && roi->data && roi_ids && gout && coef && dpred && dpred->data, "roi_mean_bwd: null argument");
  COMA_CHECK(n_roi >= 1 && n_roi <= 64, "roi_mean_bwd: n_roi=%d out of range 1..64", n_roi);
  COMA_CHECK(t_same_grid(roi, dpred) && roi->C == 1 && dpred->C == 1, "roi_mean_bwd: roi / dpred must be single-channel volumes of equal shape");
  COMA_CHECK(roi->dtype == COMA_F32 && roi->ld == 1, "roi_mean_bwd: roi must be fp32 of voxel pitch 1");
  COMA_CHECK(dpred->dtype == COMA_F32 || dpred->dtype == COMA_BF16, "roi_mean_bwd: dpred must be fp32 or bf16");
  RmP p{};
  p.roi = (const float*)roi->data; p.sbr = roi->sb; p.ids = roi_ids; p.n_roi = n_roi; p.V = t_vox(roi);
  p.gout = gout; p.coef = coef; p.dp = dpred->data; p.sbd = dpred->sb; p.ldd = dpred->ld;
  const bool v4 = rm_vec4(roi) && rm_vec4(dpred);
  int64_t nb = ((v4 ? (p.V + 3) / 4 : p.V) + 255) / 256;
  if (nb > RM_BWD_BLOCKS) nb = RM_BWD_BLOCKS;
  dim3 grid((unsigned)(nb < 1 ? 1 : nb), roi->B);
  hipStream_t s = (hipStream_t)stream;
#define LB(T) do { if (v4) hipLaunchKernelGGL((roi_mean_bwd_k<T, 4>), grid, dim3(256), 0, s, p); \
                   else hipLaunchKernelGGL((roi_mean_bwd_k<T, 1>), grid, dim3(256), 0, s, p); } while (0)
  if (dpred->dtype == COMA_F32) LB(float); else LB(bf16_t);
#undef LB
  COMA_LAUNCH_CHECK();
  return 0;
}
