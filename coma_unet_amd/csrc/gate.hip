// The attention gate between its 1x1x1 convolutions and its output, fused (MONAI AttentionBlock as used by
// attn_unet_data_parallel.py:139-150):
//
//     g1 = BN_g(W_g g)   x1 = BN_x(W_x x)   s = relu(g1 + x1)   psi = sigmoid(BN_psi(w_psi . s + b_psi))   att = x * psi
//
// W_g / W_x stay MFMA convolutions with their BatchNorm statistics out of the epilogue (conv_mfma.hip); everything behind
// them is HBM-bound element-wise work that used to be eight launches forward (2 x BN apply, add-relu, psi dot product,
// psi statistics + finalise, sigmoid-BN apply, multiply) and fourteen backward, each re-reading what the previous one
// wrote.  Here: TWO launches forward, THREE backward.
//   gate_mid_fwd_k    g1raw, x1raw -> s (saved for backward), psi_raw, {sum, sumsq}(psi_raw)        1.5 F reads... per voxel
//   gate_apply_fwd_k  x, psi_raw   -> psi (saved), att = x * psi (written into the concat slice)
//   gate_apply_bwd_k  x, psi, psi_raw, d(att) -> dx (= or +=), dz = d(psi) psi (1 - psi), BN_psi backward sums
//   gate_mid_bwd_partial_k / _apply_k: dz -> d(psi_raw) -> ds -> relu mask -> the two BatchNorm backwards at once (they
//   share d(s)), d(w_psi) and every parameter gradient; only dg1raw / dx1raw are written.
// All BatchNorms are training-mode with statistics records (norm_common.h); R = B * V elements per channel.
//
// EVAL mode (inference): every BatchNorm is a known affine map the host folds once into fp32 tables, so the gate is one pass
//     att = x * sigmoid(a_p * (w_psi . relu(scale_g * g1raw + scale_x * x1raw + shift)) + b_p)
//   gate_eval_fwd_k   g1raw, x1raw, x -> att (, psi): ONE launch behind the W_g / W_x convolutions instead of six
//   gate_eval_mfma_k  g, x -> att (, psi): both 1x1x1 convolutions on the bf16 MFMA included; s, g1, x1, psi_raw never exist
#include "norm_common.h"
#include "conv_tiles.h"   // bf16x8_t / f32x16_t

struct GateMidP {
  const void* g1; int64_t ldg, sbg;
  const void* x1; int64_t ldx, sbx;
  void* s; int64_t lds_, sbs;
  void* pr; int64_t ldp, sbp;          // psi_raw [B][V][1]
  const void* dz; int64_t lddz, sbdz;  // backward: d(BN_psi output pre-sigmoid ... ) see gate_apply_bwd_k
  void* dg1; int64_t lddg, sbdg;
  void* dx1; int64_t lddx, sbdx;
  int64_t V; int B, F, cv;
  NormStat stg, stx, stp;              // statistics of g1raw, x1raw, psi_raw
  const float *gam_g, *bet_g, *gam_x, *bet_x, *gam_p, *bet_p;
  const float* w; const float* bias;   // psi convolution: w[F], bias[1] or NULL
  double* psums; int64_t prs;          // forward: zeroed record of psi_raw [rep][1][1][2]
  const double* pbs; int64_t pbrs;     // backward: BN_psi backward sums [rep][1][1][3]
  double* rec; int64_t rrs;            // backward: zeroed record [rep][F][4] = {sum d, sum d ghat, sum d xhat, sum dpr s}
  float *rm_g, *rv_g, *rm_x, *rv_x; float momentum;
  float *dgam_g, *dbet_g, *dgam_x, *dbet_x, *dw, *dgam_p, *dbet_p;
};

// BatchNorm3d(train) running statistics from a record (one block calls this)
__device__ __forceinline__ void bn_running_update(const NormStat& st, int C, float* rm, float* rv, float momentum) {
  if (!rm) return;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const double m = rec_get(st.sums, st.rs, 2 * c) / st.R;
    double var = rec_get(st.sums, st.rs, 2 * c + 1) / st.R - m * m;
    if (var < 0.0) var = 0.0;
    const double unb = st.R > 1.0 ? var * st.R / (st.R - 1.0) : var;
    rm[c] = (1.f - momentum) * rm[c] + momentum * (float)m;
    rv[c] = (1.f - momentum) * rv[c] + momentum * (float)unb;
  }
}

#define GATE_TAB 512      // F <= 512 (the model: 16 .. 128)

template <typename T, int VEC>
__global__ __launch_bounds__(256) void gate_mid_fwd_k(GateMidP p) {
  __shared__ float t_scg[GATE_TAB], t_scx[GATE_TAB], t_sh[GATE_TAB], t_w[GATE_TAB];
  __shared__ double red[2][4];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int c = tid; c < p.F; c += 256) {
    float mg, rg, mx, rx;
    norm_mr(p.stg, c, mg, rg); norm_mr(p.stx, c, mx, rx);
    const float sg = rg * p.gam_g[c], sx = rx * p.gam_x[c];
    t_scg[c] = sg; t_scx[c] = sx;
    t_sh[c] = (p.bet_g[c] - mg * sg) + (p.bet_x[c] - mx * sx);
    t_w[c] = p.w[c];
  }
  if (blockIdx.x == 0 && b == 0) {
    bn_running_update(p.stg, p.F, p.rm_g, p.rv_g, p.momentum);
    bn_running_update(p.stx, p.F, p.rm_x, p.rv_x, p.momentum);
  }
  __syncthreads();
  const int cv = p.cv;                                   // lanes per voxel: a power of two <= 64
  const int c0 = (tid % cv) * VEC;
  float scg[VEC], scx[VEC], sh[VEC], w[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { scg[j] = t_scg[c0 + j]; scx[j] = t_scx[c0 + j]; sh[j] = t_sh[c0 + j]; w[j] = t_w[c0 + j]; }
  const float bias = p.bias ? *p.bias : 0.f;
  const T* gb = reinterpret_cast<const T*>(p.g1) + (int64_t)b * p.sbg;
  const T* xb = reinterpret_cast<const T*>(p.x1) + (int64_t)b * p.sbx;
  T* sb = reinterpret_cast<T*>(p.s) + (int64_t)b * p.sbs;
  T* pb = reinterpret_cast<T*>(p.pr) + (int64_t)b * p.sbp;
  const int vpb = 256 / cv;                              // voxels per block step
  float fs = 0.f, fq = 0.f;
  double ds = 0.0, dq = 0.0;
  int cnt = 0;
  const int64_t vstep = (int64_t)gridDim.x * vpb;
  int64_t v = (int64_t)blockIdx.x * vpb + tid / cv;
  constexpr int U = 2;
  auto one = [&](int64_t vv, const float* gv, const float* xv, bool live) {
    float sv[VEC], dot = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float t = fmaf(gv[j], scg[j], fmaf(xv[j], scx[j], sh[j]));
      sv[j] = t > 0.f ? t : 0.f;
    }
    if (live) vec_io<T, VEC>::store(sb + vv * p.lds_ + c0, sv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      // the product the stand-alone psi convolution would form: the STORED (rounded) s times w
      float sr[1]; T tmp = static_cast<T>(sv[j]); sr[0] = static_cast<float>(tmp);
      dot = fmaf(sr[0], w[j], dot);
    }
    for (int o = cv >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (live && c0 == 0) {
      const T q = static_cast<T>(dot + bias);
      pb[vv * p.ldp] = q;
      const float r = static_cast<float>(q);
      fs += r; fq = fmaf(r, r, fq);
    }
  };
  for (; v < p.V; v += U * vstep) {                      // (the shuffles need whole waves: every lane runs every trip)
    float gv[U][VEC], xv[U][VEC];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t vv = v + u * vstep;
      live[u] = vv < p.V;
      const int64_t va = live[u] ? vv : v;
      vec_io<T, VEC>::load(gb + va * p.ldg + c0, gv[u]);
      vec_io<T, VEC>::load(xb + va * p.ldx + c0, xv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(v + u * vstep, gv[u], xv[u], live[u]);
    if (++cnt == 8) { ds += (double)fs; dq += (double)fq; fs = 0.f; fq = 0.f; cnt = 0; }
  }
  ds += (double)fs; dq += (double)fq;
  // block reduction of the two psi_raw sums (only the lanes with c0 == 0 hold any) -> one atomic pair per block
  ds = wave_sum(ds); dq = wave_sum(dq);
  if ((tid & 63) == 0) { red[0][tid >> 6] = ds; red[1][tid >> 6] = dq; }
  __syncthreads();
  if (tid < 2) {
    const double t = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    add_f64(p.psums + (int64_t)(blockIdx.x & (COMA_STAT_REPLICAS - 1)) * p.prs + tid, t);
  }
}

struct GateApplyP {
  const void* x; int64_t ldx, sbx;
  const void* pr; int64_t ldp, sbp;        // psi_raw
  void* psi; int64_t ldq, sbq;             // psi (forward: out; backward: in)
  void* att; int64_t lda, sba;             // forward: x * psi
  const void* dout; int64_t ldo, sbo;      // backward: d(att)
  void* dx; int64_t lddx, sbdx; int acc;   // backward: dx (=) or (+=) dout * psi
  void* dz; int64_t lddz, sbdz;            // backward: dz [B][V][1]
  int64_t V; int B, C, cv;
  NormStat stp; const float *gam_p, *bet_p;
  float *rm_p, *rv_p; float momentum;
  double* pbs; int64_t pbrs;               // backward: zeroed record [rep][1][1][3]
};

template <typename T, int VEC>
__global__ __launch_bounds__(256) void gate_apply_fwd_k(GateApplyP p) {
  const int b = blockIdx.y, tid = threadIdx.x;
  float mu, rs; norm_mr(p.stp, 0, mu, rs);
  const float sc = rs * p.gam_p[0], sh = p.bet_p[0] - mu * sc;
  if (blockIdx.x == 0 && b == 0) bn_running_update(p.stp, 1, p.rm_p, p.rv_p, p.momentum);
  const int cv = p.cv, c0 = (tid % cv) * VEC;
  const T* xb = reinterpret_cast<const T*>(p.x) + (int64_t)b * p.sbx;
  const T* rb = reinterpret_cast<const T*>(p.pr) + (int64_t)b * p.sbp;
  T* qb = reinterpret_cast<T*>(p.psi) + (int64_t)b * p.sbq;
  T* ab = reinterpret_cast<T*>(p.att) + (int64_t)b * p.sba;
  const int64_t total = p.V * cv, stride = (int64_t)gridDim.x * 256;
  constexpr int U = 4;
  int64_t e = (int64_t)blockIdx.x * 256 + tid;
  for (; e + (U - 1) * stride < total; e += U * stride) {
    float xv[U][VEC], pr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = (e + u * stride) / cv;
      vec_io<T, VEC>::load(xb + v * p.ldx + c0, xv[u]);
      pr[u] = ld_f(rb + v * p.ldp);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = (e + u * stride) / cv;
      const T q = static_cast<T>(1.f / (1.f + expf(-fmaf(pr[u], sc, sh))));
      const float ps = static_cast<float>(q);            // the stored psi (what the stand-alone multiply would read)
      if (c0 == 0) qb[v * p.ldq] = q;
      float ov[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) ov[j] = xv[u][j] * ps;
      vec_io<T, VEC>::store(ab + v * p.lda + c0, ov);
    }
  }
  for (; e < total; e += stride) {
    const int64_t v = e / cv;
    float xv[VEC], ov[VEC];
    vec_io<T, VEC>::load(xb + v * p.ldx + c0, xv);
    const T q = static_cast<T>(1.f / (1.f + expf(-fmaf(ld_f(rb + v * p.ldp), sc, sh))));
    const float ps = static_cast<float>(q);
    if (c0 == 0) qb[v * p.ldq] = q;
#pragma unroll
    for (int j = 0; j < VEC; ++j) ov[j] = xv[j] * ps;
    vec_io<T, VEC>::store(ab + v * p.lda + c0, ov);
  }
}

// d(att) -> dx (=|+=) d(att) * psi;  dpsi = sum_c d(att) x;  dz = dpsi * psi (1 - psi) (the gradient at the sigmoid's
// input = BN_psi's output);  BN_psi backward sums {sum dz, sum dz psihat}
template <typename T, int VEC>
__global__ __launch_bounds__(256) void gate_apply_bwd_k(GateApplyP p) {
  __shared__ double red[2][4];
  const int b = blockIdx.y, tid = threadIdx.x;
  float mu, rs; norm_mr(p.stp, 0, mu, rs);
  const int cv = p.cv, c0 = (tid % cv) * VEC;
  const T* xb = reinterpret_cast<const T*>(p.x) + (int64_t)b * p.sbx;
  const T* rb = reinterpret_cast<const T*>(p.pr) + (int64_t)b * p.sbp;
  const T* qb = reinterpret_cast<const T*>(p.psi) + (int64_t)b * p.sbq;
  const T* gb = reinterpret_cast<const T*>(p.dout) + (int64_t)b * p.sbo;
  T* dxb = reinterpret_cast<T*>(p.dx) + (int64_t)b * p.sbdx;
  T* dzb = reinterpret_cast<T*>(p.dz) + (int64_t)b * p.sbdz;
  const int vpb = 256 / cv;
  const int64_t vstep = (int64_t)gridDim.x * vpb;
  float f1 = 0.f, f2 = 0.f;
  double s1 = 0.0, s2 = 0.0;
  int cnt = 0;
  constexpr int U = 2;
  for (int64_t v = (int64_t)blockIdx.x * vpb + tid / cv; v < p.V; v += U * vstep) {
    float xv[U][VEC], gv[U][VEC], ov[U][VEC], ps[U], pr[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t vv = v + u * vstep;
      live[u] = vv < p.V;
      const int64_t va = live[u] ? vv : v;
      vec_io<T, VEC>::load(xb + va * p.ldx + c0, xv[u]);
      vec_io<T, VEC>::load(gb + va * p.ldo + c0, gv[u]);
      if (p.acc) vec_io<T, VEC>::load(dxb + va * p.lddx + c0, ov[u]);
      ps[u] = ld_f(qb + va * p.ldq); pr[u] = ld_f(rb + va * p.ldp);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t vv = v + u * vstep;
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < VEC; ++j) { dot = fmaf(xv[u][j], gv[u][j], dot); ov[u][j] = (p.acc ? ov[u][j] : 0.f) + gv[u][j] * ps[u]; }
      if (live[u]) vec_io<T, VEC>::store(dxb + vv * p.lddx + c0, ov[u]);
      for (int o = cv >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
      if (live[u] && c0 == 0) {
        const T q = static_cast<T>(dot * ps[u] * (1.f - ps[u]));
        dzb[vv * p.lddz] = q;
        const float dz = static_cast<float>(q);
        f1 += dz; f2 = fmaf(dz, (pr[u] - mu) * rs, f2);
      }
    }
    if (++cnt == 8) { s1 += (double)f1; s2 += (double)f2; f1 = 0.f; f2 = 0.f; cnt = 0; }
  }
  s1 += (double)f1; s2 += (double)f2;
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = s2; }
  __syncthreads();
  if (tid < 2) {
    const double t = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    add_f64(p.pbs + (int64_t)(blockIdx.x & (COMA_STAT_REPLICAS - 1)) * p.pbrs + tid, t);
  }
}

// ---- backward of the middle: per-channel sums {sum d, sum d ghat, sum d xhat, sum dpr s}, d = dpr * w * [s > 0],
// dpr = d(psi_raw) = gamma_psi rstd_psi (dz - mean(dz) - psihat mean(dz psihat)) ----
template <typename T, int VEC>
__global__ __launch_bounds__(256) void gate_mid_bwd_partial_k(RowsP rp, GateMidP p) {
  __shared__ double sh[256][4 * VEC];
  __shared__ float t_mg[GATE_TAB], t_rg[GATE_TAB], t_mx[GATE_TAB], t_rx[GATE_TAB], t_w[GATE_TAB];
  const int tid = threadIdx.x, tx = tid % rp.cvp, ty = tid / rp.cvp;
  for (int c = tid; c < p.F; c += 256) {
    norm_mr(p.stg, c, t_mg[c], t_rg[c]); norm_mr(p.stx, c, t_mx[c], t_rx[c]);
    t_w[c] = p.w[c];
  }
  float mp, rsp; norm_mr(p.stp, 0, mp, rsp);
  const float cp = p.gam_p[0] * rsp;
  const float m1 = (float)(rec_get(p.pbs, p.pbrs, 0) / p.stp.R), m2 = (float)(rec_get(p.pbs, p.pbrs, 1) / p.stp.R);
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rp.ch;
  const int64_t r1 = r0 + rp.ch < rp.R ? r0 + rp.ch : rp.R;
  double acc[4 * VEC];
#pragma unroll
  for (int j = 0; j < 4 * VEC; ++j) acc[j] = 0.0;
  if (tx < rp.cv) {
    const T* gb = reinterpret_cast<const T*>(p.g1);
    const T* xb = reinterpret_cast<const T*>(p.x1);
    const T* sb = reinterpret_cast<const T*>(p.s);
    const T* zb = reinterpret_cast<const T*>(p.dz);
    const T* rb = reinterpret_cast<const T*>(p.pr);
    float mg[VEC], rg[VEC], mx[VEC], rx[VEC], w[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int c = tx * VEC + j;
      mg[j] = t_mg[c]; rg[j] = t_rg[c]; mx[j] = t_mx[c]; rx[j] = t_rx[c]; w[j] = t_w[c];
    }
    constexpr int BURST = 4;
    RowWalk wk(rp, r0 + ty);
    while (wk.r < r1) {
      float gv[BURST][VEC], xv[BURST][VEC], sv[BURST][VEC], dz[BURST], pr[BURST];
      bool ok[BURST];
      int64_t og = wk.off(rp, 0, p.ldg, p.sbg), ox = wk.off(rp, 0, p.ldx, p.sbx), os = wk.off(rp, 0, p.lds_, p.sbs),
              oz = wk.off(rp, 0, p.lddz, p.sbdz), opr = wk.off(rp, 0, p.ldp, p.sbp);
#pragma unroll
      for (int u = 0; u < BURST; ++u) {
        ok[u] = wk.r < r1;
        if (ok[u]) { og = wk.off(rp, 0, p.ldg, p.sbg); ox = wk.off(rp, 0, p.ldx, p.sbx); os = wk.off(rp, 0, p.lds_, p.sbs);
                     oz = wk.off(rp, 0, p.lddz, p.sbdz); opr = wk.off(rp, 0, p.ldp, p.sbp); }
        vec_io<T, VEC>::load(gb + og + tx * VEC, gv[u]);
        vec_io<T, VEC>::load(xb + ox + tx * VEC, xv[u]);
        vec_io<T, VEC>::load(sb + os + tx * VEC, sv[u]);
        dz[u] = ld_f(zb + oz); pr[u] = ld_f(rb + opr);
        wk.step(rp);
      }
      float f[4 * VEC];
#pragma unroll
      for (int j = 0; j < 4 * VEC; ++j) f[j] = 0.f;
#pragma unroll
      for (int u = 0; u < BURST; ++u) {
        const float dpr = ok[u] ? cp * (dz[u] - m1 - (pr[u] - mp) * rsp * m2) : 0.f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float d = sv[u][j] > 0.f ? dpr * w[j] : 0.f;
          f[4 * j] += d;
          f[4 * j + 1] = fmaf(d, (gv[u][j] - mg[j]) * rg[j], f[4 * j + 1]);
          f[4 * j + 2] = fmaf(d, (xv[u][j] - mx[j]) * rx[j], f[4 * j + 2]);
          f[4 * j + 3] = fmaf(dpr, sv[u][j], f[4 * j + 3]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4 * VEC; ++j) acc[j] += (double)f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4 * VEC; ++j) sh[tid][j] = acc[j];
  __syncthreads();
  for (int off = rp.ry >> 1; off > 0; off >>= 1) {
    if (ty < off) {
#pragma unroll
      for (int j = 0; j < 4 * VEC; ++j) sh[tid][j] += sh[tid + off * rp.cvp][j];
    }
    __syncthreads();
  }
  rec_add(p.rec, p.rrs, 0, &sh[0][0], p.F * 4);          // row 0 of the tree = a contiguous [F][4] image
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void gate_mid_bwd_apply_k(GateMidP p) {
  __shared__ float t_mg[GATE_TAB], t_rg[GATE_TAB], t_mx[GATE_TAB], t_rx[GATE_TAB], t_w[GATE_TAB];
  __shared__ float t_a[GATE_TAB], t_bg[GATE_TAB], t_bx[GATE_TAB], t_cg[GATE_TAB], t_cx[GATE_TAB];
  const int b = blockIdx.y, tid = threadIdx.x;
  const bool first = blockIdx.x == 0 && b == 0;
  for (int c = tid; c < p.F; c += 256) {
    norm_mr(p.stg, c, t_mg[c], t_rg[c]); norm_mr(p.stx, c, t_mx[c], t_rx[c]);
    t_w[c] = p.w[c];
    const double a = rec_get(p.rec, p.rrs, 4 * c), bg = rec_get(p.rec, p.rrs, 4 * c + 1), bx = rec_get(p.rec, p.rrs, 4 * c + 2);
    t_a[c] = (float)(a / p.stg.R); t_bg[c] = (float)(bg / p.stg.R); t_bx[c] = (float)(bx / p.stg.R);
    t_cg[c] = t_rg[c] * p.gam_g[c]; t_cx[c] = t_rx[c] * p.gam_x[c];
    if (first) {
      if (p.dgam_g) p.dgam_g[c] = (float)bg;
      if (p.dbet_g) p.dbet_g[c] = (float)a;
      if (p.dgam_x) p.dgam_x[c] = (float)bx;
      if (p.dbet_x) p.dbet_x[c] = (float)a;
      if (p.dw) p.dw[c] = (float)rec_get(p.rec, p.rrs, 4 * c + 3);
    }
  }
  if (first && tid == 0) {
    if (p.dbet_p) p.dbet_p[0] = (float)rec_get(p.pbs, p.pbrs, 0);
    if (p.dgam_p) p.dgam_p[0] = (float)rec_get(p.pbs, p.pbrs, 1);
  }
  float mp, rsp; norm_mr(p.stp, 0, mp, rsp);
  const float cp = p.gam_p[0] * rsp;
  const float m1 = (float)(rec_get(p.pbs, p.pbrs, 0) / p.stp.R), m2 = (float)(rec_get(p.pbs, p.pbrs, 1) / p.stp.R);
  __syncthreads();
  const int cv = p.cv, c0 = (tid % cv) * VEC;
  float mg[VEC], rg[VEC], mx[VEC], rx[VEC], w[VEC], a[VEC], bg[VEC], bx[VEC], cg[VEC], cx[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int c = c0 + j;
    mg[j] = t_mg[c]; rg[j] = t_rg[c]; mx[j] = t_mx[c]; rx[j] = t_rx[c]; w[j] = t_w[c];
    a[j] = t_a[c]; bg[j] = t_bg[c]; bx[j] = t_bx[c]; cg[j] = t_cg[c]; cx[j] = t_cx[c];
  }
  const T* gb = reinterpret_cast<const T*>(p.g1) + (int64_t)b * p.sbg;
  const T* xb = reinterpret_cast<const T*>(p.x1) + (int64_t)b * p.sbx;
  const T* sb = reinterpret_cast<const T*>(p.s) + (int64_t)b * p.sbs;
  const T* zb = reinterpret_cast<const T*>(p.dz) + (int64_t)b * p.sbdz;
  const T* rb = reinterpret_cast<const T*>(p.pr) + (int64_t)b * p.sbp;
  T* dgb = reinterpret_cast<T*>(p.dg1) + (int64_t)b * p.sbdg;
  T* dxb = reinterpret_cast<T*>(p.dx1) + (int64_t)b * p.sbdx;
  const int64_t total = p.V * cv, stride = (int64_t)gridDim.x * 256;
  constexpr int U = 2;
  auto one = [&](int64_t v, const float* gv, const float* xv, const float* sv, float dz, float pr) {
    const float dpr = cp * (dz - m1 - (pr - mp) * rsp * m2);
    float og[VEC], ox[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float d = sv[j] > 0.f ? dpr * w[j] : 0.f;
      og[j] = cg[j] * (d - a[j] - (gv[j] - mg[j]) * rg[j] * bg[j]);
      ox[j] = cx[j] * (d - a[j] - (xv[j] - mx[j]) * rx[j] * bx[j]);
    }
    vec_io<T, VEC>::store(dgb + v * p.lddg + c0, og);
    vec_io<T, VEC>::store(dxb + v * p.lddx + c0, ox);
  };
  int64_t e = (int64_t)blockIdx.x * 256 + tid;
  for (; e + (U - 1) * stride < total; e += U * stride) {
    float gv[U][VEC], xv[U][VEC], sv[U][VEC], dz[U], pr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = (e + u * stride) / cv;
      vec_io<T, VEC>::load(gb + v * p.ldg + c0, gv[u]);
      vec_io<T, VEC>::load(xb + v * p.ldx + c0, xv[u]);
      vec_io<T, VEC>::load(sb + v * p.lds_ + c0, sv[u]);
      dz[u] = ld_f(zb + v * p.lddz); pr[u] = ld_f(rb + v * p.ldp);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one((e + u * stride) / cv, gv[u], xv[u], sv[u], dz[u], pr[u]);
  }
  for (; e < total; e += stride) {
    const int64_t v = e / cv;
    float gv[VEC], xv[VEC], sv[VEC];
    vec_io<T, VEC>::load(gb + v * p.ldg + c0, gv);
    vec_io<T, VEC>::load(xb + v * p.ldx + c0, xv);
    vec_io<T, VEC>::load(sb + v * p.lds_ + c0, sv);
    one(v, gv, xv, sv, ld_f(zb + v * p.lddz), ld_f(rb + v * p.ldp));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static NormStat bn_stat(const double* sums, int C, double R, float eps) {
  NormStat st;
  st.sums = sums; st.rs = COMA_NORM_RECORD_DOUBLES(1, C, 2); st.R = R; st.eps = eps; st.mean = st.rstd = nullptr;
  return st;
}
static int pow2_le64(int v) { return v >= 1 && v <= 64 && (v & (v - 1)) == 0; }
static unsigned gate_blocks(int64_t items, int per_block, int cap) {
  int64_t nb = (items + per_block - 1) / per_block;
  if (nb > cap) nb = cap;
  return (unsigned)(nb < 1 ? 1 : nb);
}
// vector width all of the given [.., F] tensors allow (8 bf16 / 4 fp32 elements = 16 bytes, else 4, else 1)
static int gate_vec(const coma_tensor* const* ts, int n, int want) {
  int v = want;
  for (int i = 0; i < n; ++i) { const int t = t_vec(ts[i], want); if (t < v) v = t; }
  return v;
}
#define GATE_DISPATCH(KERNEL, DT, VEC, GRID, ...)                                                              \
  do {                                                                                                         \
    if ((DT) == COMA_F32) { if ((VEC) == 4) hipLaunchKernelGGL((KERNEL<float, 4>), GRID, dim3(256), 0, s, __VA_ARGS__);      \
                            else hipLaunchKernelGGL((KERNEL<float, 1>), GRID, dim3(256), 0, s, __VA_ARGS__); }               \
    else { if ((VEC) == 8) hipLaunchKernelGGL((KERNEL<bf16_t, 8>), GRID, dim3(256), 0, s, __VA_ARGS__);                     \
           else if ((VEC) == 4) hipLaunchKernelGGL((KERNEL<bf16_t, 4>), GRID, dim3(256), 0, s, __VA_ARGS__);                 \
           else hipLaunchKernelGGL((KERNEL<bf16_t, 1>), GRID, dim3(256), 0, s, __VA_ARGS__); }                               \
  } while (0)

static int gate_pick_vec(int dtype, const coma_tensor* const* ts, int n, int F, int max_lanes) {
  int vec = gate_vec(ts, n, dtype == COMA_BF16 ? 8 : 4);
  if (dtype == COMA_F32 && vec == 8) vec = 4;
  if (vec == 2) vec = 1;
  // lanes per voxel must be a power of two <= 64 (wave shuffles): widen nothing, but fall back to narrower vectors never
  // makes it worse -- F / vec too large means an unsupported F
  while (vec > 1 && !pow2_le64(F / vec)) vec = vec == 8 ? 4 : 1;
  (void)max_lanes;
  return vec;
}

extern "C" int coma_gate_mid_fwd(const coma_tensor* g1, const coma_tensor* x1, const double* sums_g, float eps_g,
                                 const float* gamma_g, const float* beta_g, const double* sums_x, float eps_x,
                                 const float* gamma_x, const float* beta_x, const float* w_psi, const float* b_psi,
                                 float* rmean_g, float* rvar_g, float* rmean_x, float* rvar_x, float momentum,
                                 const coma_tensor* s_out, const coma_tensor* psi_raw, double* sums_psi, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  COMA_CHECK(g1 && x1 && s_out && psi_raw && g1->data && x1->data && s_out->data && psi_raw->data && sums_g && sums_x && sums_psi &&
             gamma_g && beta_g && gamma_x && beta_x && w_psi, "gate_mid_fwd: null argument");
  COMA_CHECK(t_same_grid(g1, x1) && t_same_grid(g1, s_out) && t_same_grid(g1, psi_raw) && g1->C == x1->C && g1->C == s_out->C &&
             psi_raw->C == 1 && g1->dtype == x1->dtype && g1->dtype == s_out->dtype && g1->dtype == psi_raw->dtype,
             "gate_mid_fwd: shape/dtype mismatch");
  const int F = g1->C;
  COMA_CHECK(F <= GATE_TAB, "gate_mid_fwd: F=%d too large", F);
  const coma_tensor* ts[3] = {g1, x1, s_out};
  const int vec = gate_pick_vec(g1->dtype, ts, 3, F, 64);
  COMA_CHECK(pow2_le64(F / vec), "gate_mid_fwd: F=%d unsupported (F / vector width must be a power of two <= 64)", F);
  GateMidP p{};
  p.g1 = g1->data; p.ldg = g1->ld; p.sbg = g1->sb; p.x1 = x1->data; p.ldx = x1->ld; p.sbx = x1->sb;
  p.s = s_out->data; p.lds_ = s_out->ld; p.sbs = s_out->sb; p.pr = psi_raw->data; p.ldp = psi_raw->ld; p.sbp = psi_raw->sb;
  p.V = t_vox(g1); p.B = g1->B; p.F = F; p.cv = F / vec;
  const double R = (double)p.V * g1->B;
  p.stg = bn_stat(sums_g, F, R, eps_g); p.stx = bn_stat(sums_x, F, R, eps_x);
  p.gam_g = gamma_g; p.bet_g = beta_g; p.gam_x = gamma_x; p.bet_x = beta_x; p.w = w_psi; p.bias = b_psi;
  p.psums = sums_psi; p.prs = COMA_NORM_RECORD_DOUBLES(1, 1, 2);
  p.rm_g = rmean_g; p.rv_g = rvar_g; p.rm_x = rmean_x; p.rv_x = rvar_x; p.momentum = momentum;
  const int vpb = 256 / p.cv;
  int cap = 1024 / g1->B; if (cap < 1) cap = 1;
  dim3 grid(gate_blocks(p.V, vpb * 2, cap), g1->B);
  GATE_DISPATCH(gate_mid_fwd_k, g1->dtype, vec, grid, p);
  COMA_LAUNCH_CHECK();
  return 0;
}

static int gate_apply_setup(GateApplyP& p, const coma_tensor* x, const coma_tensor* psi_raw, const coma_tensor* psi,
                            const double* sums_psi, float eps, const float* gamma_p, const float* beta_p) {
  p.x = x->data; p.ldx = x->ld; p.sbx = x->sb; p.pr = psi_raw->data; p.ldp = psi_raw->ld; p.sbp = psi_raw->sb;
  p.psi = psi->data; p.ldq = psi->ld; p.sbq = psi->sb;
  p.V = t_vox(x); p.B = x->B; p.C = x->C;
  p.stp = bn_stat(sums_psi, 1, (double)p.V * x->B, eps);
  p.gam_p = gamma_p; p.bet_p = beta_p;
  return 0;
}

extern "C" int coma_gate_apply_fwd(const coma_tensor* x, const coma_tensor* psi_raw, const double* sums_psi, float eps,
                                   const float* gamma_psi, const float* beta_psi, float* rmean_psi, float* rvar_psi,
                                   float momentum, const coma_tensor* psi, const coma_tensor* att, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  COMA_CHECK(x && psi_raw && psi && att && x->data && psi_raw->data && psi->data && att->data && sums_psi && gamma_psi && beta_psi,
             "gate_apply_fwd: null argument");
  COMA_CHECK(t_same_grid(x, psi_raw) && t_same_grid(x, psi) && t_same_grid(x, att) && psi_raw->C == 1 && psi->C == 1 &&
             x->C == att->C && x->dtype == psi_raw->dtype && x->dtype == psi->dtype && x->dtype == att->dtype,
             "gate_apply_fwd: shape/dtype mismatch");
  const coma_tensor* ts[2] = {x, att};
  const int vec = gate_pick_vec(x->dtype, ts, 2, x->C, 64);
  COMA_CHECK(pow2_le64(x->C / vec), "gate_apply_fwd: C=%d unsupported", x->C);
  GateApplyP p{};
  gate_apply_setup(p, x, psi_raw, psi, sums_psi, eps, gamma_psi, beta_psi);
  p.cv = x->C / vec;
  p.att = att->data; p.lda = att->ld; p.sba = att->sb;
  p.rm_p = rmean_psi; p.rv_p = rvar_psi; p.momentum = momentum;
  dim3 grid(gate_blocks(p.V * p.cv, 256 * 4, 4096), x->B);
  GATE_DISPATCH(gate_apply_fwd_k, x->dtype, vec, grid, p);
  COMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int coma_gate_apply_bwd(const coma_tensor* x, const coma_tensor* psi, const coma_tensor* psi_raw,
                                   const coma_tensor* dout, const double* sums_psi, float eps, const float* gamma_psi,
                                   const float* beta_psi, const coma_tensor* dx, int32_t accumulate_dx,
                                   const coma_tensor* dz, double* bsums_psi, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  COMA_CHECK(x && psi && psi_raw && dout && dx && dz && x->data && psi->data && psi_raw->data && dout->data && dx->data &&
             dz->data && sums_psi && bsums_psi && gamma_psi, "gate_apply_bwd: null argument");
  COMA_CHECK(t_same_grid(x, psi) && t_same_grid(x, psi_raw) && t_same_grid(x, dout) && t_same_grid(x, dx) && t_same_grid(x, dz) &&
             psi->C == 1 && psi_raw->C == 1 && dz->C == 1 && x->C == dout->C && x->C == dx->C && x->dtype == dout->dtype &&
             x->dtype == dx->dtype && x->dtype == dz->dtype && x->dtype == psi->dtype, "gate_apply_bwd: shape/dtype mismatch");
  const coma_tensor* ts[3] = {x, dout, dx};
  const int vec = gate_pick_vec(x->dtype, ts, 3, x->C, 64);
  COMA_CHECK(pow2_le64(x->C / vec), "gate_apply_bwd: C=%d unsupported", x->C);
  GateApplyP p{};
  gate_apply_setup(p, x, psi_raw, psi, sums_psi, eps, gamma_psi, beta_psi);
  p.cv = x->C / vec;
  p.dout = dout->data; p.ldo = dout->ld; p.sbo = dout->sb;
  p.dx = dx->data; p.lddx = dx->ld; p.sbdx = dx->sb; p.acc = accumulate_dx;
  p.dz = dz->data; p.lddz = dz->ld; p.sbdz = dz->sb;
  p.pbs = bsums_psi; p.pbrs = COMA_NORM_RECORD_DOUBLES(1, 1, 3);
  int cap = 1024 / x->B; if (cap < 1) cap = 1;
  dim3 grid(gate_blocks(p.V, (256 / p.cv) * 2, cap), x->B);
  GATE_DISPATCH(gate_apply_bwd_k, x->dtype, vec, grid, p);
  COMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int coma_gate_mid_bwd(const coma_tensor* dz, const coma_tensor* psi_raw, const coma_tensor* s_in,
                                 const coma_tensor* g1, const coma_tensor* x1, const double* sums_psi, float eps_psi,
                                 const float* gamma_psi, const double* bsums_psi, const double* sums_g, float eps_g,
                                 const float* gamma_g, const double* sums_x, float eps_x, const float* gamma_x,
                                 const float* w_psi, double* rec, const coma_tensor* dg1, const coma_tensor* dx1,
                                 float* dgamma_g, float* dbeta_g, float* dgamma_x, float* dbeta_x, float* dw_psi,
                                 float* dgamma_psi, float* dbeta_psi, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  COMA_CHECK(dz && psi_raw && s_in && g1 && x1 && dg1 && dx1 && dz->data && psi_raw->data && s_in->data && g1->data && x1->data &&
             dg1->data && dx1->data && sums_psi && bsums_psi && sums_g && sums_x && gamma_psi && gamma_g && gamma_x && w_psi && rec,
             "gate_mid_bwd: null argument");
  COMA_CHECK(t_same_grid(g1, x1) && t_same_grid(g1, s_in) && t_same_grid(g1, dz) && t_same_grid(g1, psi_raw) && t_same_grid(g1, dg1) &&
             t_same_grid(g1, dx1) && g1->C == x1->C && g1->C == s_in->C && g1->C == dg1->C && g1->C == dx1->C && dz->C == 1 &&
             psi_raw->C == 1 && g1->dtype == x1->dtype && g1->dtype == s_in->dtype && g1->dtype == dz->dtype &&
             g1->dtype == dg1->dtype && g1->dtype == dx1->dtype && g1->dtype == psi_raw->dtype, "gate_mid_bwd: shape/dtype mismatch");
  const int F = g1->C;
  COMA_CHECK(F <= GATE_TAB, "gate_mid_bwd: F=%d too large", F);
  GateMidP p{};
  p.g1 = g1->data; p.ldg = g1->ld; p.sbg = g1->sb; p.x1 = x1->data; p.ldx = x1->ld; p.sbx = x1->sb;
  p.s = s_in->data; p.lds_ = s_in->ld; p.sbs = s_in->sb; p.pr = psi_raw->data; p.ldp = psi_raw->ld; p.sbp = psi_raw->sb;
  p.dz = dz->data; p.lddz = dz->ld; p.sbdz = dz->sb;
  p.dg1 = dg1->data; p.lddg = dg1->ld; p.sbdg = dg1->sb; p.dx1 = dx1->data; p.lddx = dx1->ld; p.sbdx = dx1->sb;
  p.V = t_vox(g1); p.B = g1->B; p.F = F;
  const double R = (double)p.V * g1->B;
  p.stg = bn_stat(sums_g, F, R, eps_g); p.stx = bn_stat(sums_x, F, R, eps_x); p.stp = bn_stat(sums_psi, 1, R, eps_psi);
  p.gam_g = gamma_g; p.gam_x = gamma_x; p.gam_p = gamma_psi; p.w = w_psi;
  p.pbs = bsums_psi; p.pbrs = COMA_NORM_RECORD_DOUBLES(1, 1, 3);
  p.rec = rec; p.rrs = COMA_NORM_RECORD_DOUBLES(1, F, 4);
  p.dgam_g = dgamma_g; p.dbet_g = dbeta_g; p.dgam_x = dgamma_x; p.dbet_x = dbeta_x; p.dw = dw_psi;
  p.dgam_p = dgamma_psi; p.dbet_p = dbeta_psi;
  // pass 1: per-channel sums (row walk of the statistics kernels, 4-wide: 16 fp64 accumulators per lane)
  {
    const coma_tensor* ts[3] = {g1, x1, s_in};
    const int pv = gate_vec(ts, 3, 4) >= 4 ? 4 : 1;
    RowsP rp = make_rows(g1, COMA_NORM_BATCH, pv);
    COMA_CHECK(rp.cv <= 256, "gate_mid_bwd: F=%d too large", F);
    dim3 pg(rp.nchunks, 1);
    if (g1->dtype == COMA_F32) { if (pv == 4) hipLaunchKernelGGL((gate_mid_bwd_partial_k<float, 4>), pg, dim3(256), 0, s, rp, p);
                                 else hipLaunchKernelGGL((gate_mid_bwd_partial_k<float, 1>), pg, dim3(256), 0, s, rp, p); }
    else { if (pv == 4) hipLaunchKernelGGL((gate_mid_bwd_partial_k<bf16_t, 4>), pg, dim3(256), 0, s, rp, p);
           else hipLaunchKernelGGL((gate_mid_bwd_partial_k<bf16_t, 1>), pg, dim3(256), 0, s, rp, p); }
    COMA_LAUNCH_CHECK();
  }
  // pass 2: dg1raw, dx1raw + the parameter gradients
  const coma_tensor* ts[5] = {g1, x1, s_in, dg1, dx1};
  const int vec = gate_pick_vec(g1->dtype, ts, 5, F, 64);
  COMA_CHECK(pow2_le64(F / vec), "gate_mid_bwd: F=%d unsupported", F);
  p.cv = F / vec;
  dim3 grid(gate_blocks(p.V * p.cv, 256 * 2, 4096), g1->B);
  GATE_DISPATCH(gate_mid_bwd_apply_k, g1->dtype, vec, grid, p);
  COMA_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Eval-mode gate.  The tables are folded by the host (coma_unet_amd/inference.py: fold_gate).
struct GateEvalP {
  const void* x; int64_t ldx, sbx;         // [B][V][C]
  const void* g1; int64_t ldg, sbg;        // element-wise: g1raw [B][V][F];  MFMA: g [B][V][C]
  const void* x1; int64_t ldx1, sbx1;      // element-wise: x1raw [B][V][F]
  void* att; int64_t lda, sba;             // [B][V][C], possibly a channel slice
  void* psi; int64_t ldq, sbq;             // [B][V][1] or NULL
  int64_t V; int B, C, F, cv;
  const float *scg, *scx, *sh, *w, *ab;    // scale_g[F], scale_x[F], shift[F], w_psi[F], {a_p, b_p}
  const void *wg, *wx;                     // MFMA: folded bf16 weights [32][C], zero rows beyond F
};

// The pass of a gate whose BatchNorms are affine maps, behind the block's folded LDS tables (scale_g, scale_x, shift, w_psi)
// and {a_p, b_p}: shared by the eval gate and the frozen gate's forward.
// `cv` = max(C, F) / VEC lanes per voxel; the lanes with c0 < F form the dot product, those with c0 < C the multiply
template <typename T, int VEC>
__device__ __forceinline__ void gate_affine_fwd(const GateEvalP& p, const float* t_scg, const float* t_scx, const float* t_sh,
                                                const float* t_w, const float pa, const float pb) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int cv = p.cv;                                   // a power of two <= 64
  const int c0 = (tid % cv) * VEC;
  const bool in_f = c0 < p.F, in_c = c0 < p.C;           // (F and C are multiples of VEC)
  float scg[VEC], scx[VEC], sh[VEC], w[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    scg[j] = in_f ? t_scg[c0 + j] : 0.f; scx[j] = in_f ? t_scx[c0 + j] : 0.f;
    sh[j] = in_f ? t_sh[c0 + j] : 0.f; w[j] = in_f ? t_w[c0 + j] : 0.f;
  }
  const T* gb = reinterpret_cast<const T*>(p.g1) + (int64_t)b * p.sbg;
  const T* x1b = reinterpret_cast<const T*>(p.x1) + (int64_t)b * p.sbx1;
  const T* xb = reinterpret_cast<const T*>(p.x) + (int64_t)b * p.sbx;
  T* ab = reinterpret_cast<T*>(p.att) + (int64_t)b * p.sba;
  T* qb = p.psi ? reinterpret_cast<T*>(p.psi) + (int64_t)b * p.sbq : nullptr;
  const int vpb = 256 / cv;                              // voxels per block step
  const int64_t vstep = (int64_t)gridDim.x * vpb;
  constexpr int U = 2;
  for (int64_t v = (int64_t)blockIdx.x * vpb + tid / cv; v < p.V; v += U * vstep) {   // (whole waves run every trip: shuffles)
    float gv[U][VEC], x1v[U][VEC], xv[U][VEC];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t vv = v + u * vstep;
      live[u] = vv < p.V;
      const int64_t va = live[u] ? vv : v;
#pragma unroll
      for (int j = 0; j < VEC; ++j) { gv[u][j] = 0.f; x1v[u][j] = 0.f; xv[u][j] = 0.f; }
      if (in_f) { vec_io<T, VEC>::load(gb + va * p.ldg + c0, gv[u]); vec_io<T, VEC>::load(x1b + va * p.ldx1 + c0, x1v[u]); }
      if (in_c) vec_io<T, VEC>::load(xb + va * p.ldx + c0, xv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t vv = v + u * vstep;
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float t = fmaf(gv[u][j], scg[j], fmaf(x1v[u][j], scx[j], sh[j]));
        dot = fmaf(t > 0.f ? t : 0.f, w[j], dot);
      }
      for (int o = cv >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
      const T q = static_cast<T>(1.f / (1.f + expf(-fmaf(dot, pa, pb))));
      const float ps = static_cast<float>(q);            // the stored psi, as the training kernels multiply with
      if (live[u]) {
        if (qb && c0 == 0) qb[vv * p.ldq] = q;
        if (in_c) {
          float ov[VEC];
#pragma unroll
          for (int j = 0; j < VEC; ++j) ov[j] = xv[u][j] * ps;
          vec_io<T, VEC>::store(ab + vv * p.lda + c0, ov);
        }
      }
    }
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void gate_eval_fwd_k(GateEvalP p) {
  __shared__ float t_scg[GATE_TAB], t_scx[GATE_TAB], t_sh[GATE_TAB], t_w[GATE_TAB];
  for (int c = threadIdx.x; c < p.F; c += 256) { t_scg[c] = p.scg[c]; t_scx[c] = p.scx[c]; t_sh[c] = p.sh[c]; t_w[c] = p.w[c]; }
  __syncthreads();
  gate_affine_fwd<T, VEC>(p, t_scg, t_scx, t_sh, t_w, p.ab[0], p.ab[1]);
}

// The whole gate in one launch, modelled on conv_mfma_pw_k (conv_mfma.hip): no LDS; the folded weights diag(scale) W of both
// convolutions stay in registers as MFMA A fragments; a wave owns 32 voxels, lane (fr = lane & 31, fh = lane >> 5) streams
// the 16-byte chunks [16 ks + 8 fh, + 8) of voxel fr of g and of x into the B operand, and both products land in ONE
// accumulator (2 KS MFMAs).  The lane then holds rows 8 g4 + 4 fh + q (g4, q < 4) of its voxel's column: shift, ReLU and
// the w_psi product over those 16 rows, one exchange with lane ^ 32 for the other 16, sigmoid -- and att = x * psi from
// the x fragments it still holds (the two half-waves together own all C = 16 KS channels of the voxel), 16-byte stores.
// The host pads the folded weights ([32][C]) and the shift / w_psi tables ([32]) with zero rows beyond F: relu(0 + 0) * 0,
// those rows contribute exactly nothing and the kernel needs no F.
template <int KS>
__global__ __launch_bounds__(256) void gate_eval_mfma_k(GateEvalP p) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int b = blockIdx.y;
  const bf16_t* gb = reinterpret_cast<const bf16_t*>(p.g1) + (int64_t)b * p.sbg;
  const bf16_t* xb = reinterpret_cast<const bf16_t*>(p.x) + (int64_t)b * p.sbx;
  bf16_t* ab = reinterpret_cast<bf16_t*>(p.att) + (int64_t)b * p.sba;
  bf16_t* qb = p.psi ? reinterpret_cast<bf16_t*>(p.psi) + (int64_t)b * p.sbq : nullptr;
  const bf16_t* wg = reinterpret_cast<const bf16_t*>(p.wg);
  const bf16_t* wx = reinterpret_cast<const bf16_t*>(p.wx);
  bf16x8_t wgf[KS], wxf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int c = ks * 16 + fh * 8;                      // < C = 16 KS
    const uint4 a = *reinterpret_cast<const uint4*>(wg + fr * p.C + c);
    const uint4 c4 = *reinterpret_cast<const uint4*>(wx + fr * p.C + c);
    wgf[ks] = *reinterpret_cast<const bf16x8_t*>(&a);
    wxf[ks] = *reinterpret_cast<const bf16x8_t*>(&c4);
  }
  float sh[16], w[16];
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = 8 * g4 + 4 * fh + q;
      sh[g4 * 4 + q] = p.sh[n];
      w[g4 * 4 + q] = p.w[n];
    }
  const float pa = p.ab[0], pb = p.ab[1];
  const int64_t mtiles = (p.V + 31) / 32;
  for (int64_t mt = (int64_t)blockIdx.x * 4 + wid; mt < mtiles; mt += (int64_t)gridDim.x * 4) {
    const int64_t v = mt * 32 + fr;
    const bool live = v < p.V;
    uint4 gq[KS], xq[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = ks * 16 + fh * 8;
      gq[ks] = make_uint4(0, 0, 0, 0); xq[ks] = make_uint4(0, 0, 0, 0);
      if (live) {
        gq[ks] = *reinterpret_cast<const uint4*>(gb + v * p.ldg + c);
        xq[ks] = *reinterpret_cast<const uint4*>(xb + v * p.ldx + c);
      }
    }
    f32x16_t acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wgf[ks], *reinterpret_cast<const bf16x8_t*>(&gq[ks]), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wxf[ks], *reinterpret_cast<const bf16x8_t*>(&xq[ks]), acc, 0, 0, 0);
    }
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float t = acc[e] + sh[e];
      dot = fmaf(t > 0.f ? t : 0.f, w[e], dot);
    }
    dot += __shfl_xor(dot, 32, 64);                      // (every lane of the wave is here: `live` only masks memory)
    const bf16_t q = static_cast<bf16_t>(1.f / (1.f + expf(-fmaf(dot, pa, pb))));
    const float ps = static_cast<float>(q);
    if (live) {
      if (qb && fh == 0) qb[v * p.ldq] = q;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const unsigned u[4] = {xq[ks].x, xq[ks].y, xq[ks].z, xq[ks].w};
        bf16_t o[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[2 * j] = static_cast<bf16_t>(__uint_as_float(u[j] << 16) * ps);
          o[2 * j + 1] = static_cast<bf16_t>(__uint_as_float(u[j] & 0xffff0000u) * ps);
        }
        *reinterpret_cast<uint4*>(ab + v * p.lda + ks * 16 + fh * 8) = *reinterpret_cast<const uint4*>(o);
      }
    }
  }
}

static int gate_eval_common(GateEvalP& p, const coma_tensor* x, const coma_tensor* psi, const coma_tensor* att) {
  p.x = x->data; p.ldx = x->ld; p.sbx = x->sb;
  p.att = att->data; p.lda = att->ld; p.sba = att->sb;
  p.psi = nullptr; p.ldq = 0; p.sbq = 0;
  if (psi) { p.psi = psi->data; p.ldq = psi->ld; p.sbq = psi->sb; }
  p.V = t_vox(x); p.B = x->B; p.C = x->C;
  return 0;
}

extern "C" int coma_gate_eval_fwd(const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw, const float* scale_g,
                                  const float* scale_x, const float* shift, const float* w_psi, const float* psi_ab,
                                  const coma_tensor* psi, const coma_tensor* att, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  COMA_CHECK(x && g1raw && x1raw && att && x->data && g1raw->data && x1raw->data && att->data && scale_g && scale_x && shift &&
             w_psi && psi_ab && (!psi || psi->data), "gate_eval_fwd: null argument");
  COMA_CHECK(t_same_grid(x, g1raw) && t_same_grid(x, x1raw) && t_same_grid(x, att) && (!psi || (t_same_grid(x, psi) && psi->C == 1)) &&
             g1raw->C == x1raw->C && x->C == att->C && x->dtype == g1raw->dtype && x->dtype == x1raw->dtype &&
             x->dtype == att->dtype && (!psi || psi->dtype == x->dtype), "gate_eval_fwd: shape/dtype mismatch");
  const int F = g1raw->C, C = x->C;
  COMA_CHECK(F >= 1 && F <= GATE_TAB, "gate_eval_fwd: F=%d too large", F);
  const coma_tensor* ts[4] = {x, g1raw, x1raw, att};
  const int m = C > F ? C : F;
  int vec = gate_vec(ts, 4, x->dtype == COMA_BF16 ? 8 : 4);
  if (vec == 2) vec = 1;
  while (vec > 1 && !pow2_le64(m / vec)) vec = vec == 8 ? 4 : 1;
  COMA_CHECK(C % vec == 0 && F % vec == 0 && pow2_le64(m / vec),
             "gate_eval_fwd: C=%d F=%d unsupported (max(C, F) / vector width must be a power of two <= 64)", C, F);
  GateEvalP p{};
  gate_eval_common(p, x, psi, att);
  p.g1 = g1raw->data; p.ldg = g1raw->ld; p.sbg = g1raw->sb; p.x1 = x1raw->data; p.ldx1 = x1raw->ld; p.sbx1 = x1raw->sb;
  p.F = F; p.cv = m / vec;
  p.scg = scale_g; p.scx = scale_x; p.sh = shift; p.w = w_psi; p.ab = psi_ab;
  int cap = 2048 / x->B; if (cap < 1) cap = 1;
  dim3 grid(gate_blocks(p.V, (256 / p.cv) * 2, cap), x->B);
  GATE_DISPATCH(gate_eval_fwd_k, x->dtype, vec, grid, p);
  COMA_LAUNCH_CHECK();
  return 0;
}

static bool gate_al16(const coma_tensor* t) { return t->ld % 8 == 0 && t->sb % 8 == 0 && (!t->data || ((uintptr_t)t->data & 15) == 0); }

extern "C" int coma_gate_eval_mfma_ok(const coma_tensor* g, const coma_tensor* x, int32_t F) {
  if (!g || !x) return 0;
  return g->dtype == COMA_BF16 && x->dtype == COMA_BF16 && t_same_grid(g, x) && g->C == x->C && x->C % 16 == 0 && x->C >= 16 &&
         x->C <= 64 && F >= 1 && F <= 32 && gate_al16(g) && gate_al16(x) ? 1 : 0;
}

// one grid pass covers GATE_EVAL_MFMA_BLOCKS blocks x 4 waves x 32 voxels per sample (conv_mfma_pw_k's cap)
#define GATE_EVAL_MFMA_BLOCKS 2048
extern "C" int coma_gate_eval_mfma(const coma_tensor* g, const coma_tensor* x, const void* wg_folded, const void* wx_folded,
                                   const float* shift, const float* w_psi, const float* psi_ab, const coma_tensor* psi,
                                   const coma_tensor* att, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  COMA_CHECK(g && x && att && g->data && x->data && att->data && wg_folded && wx_folded && shift && w_psi && psi_ab &&
             (!psi || psi->data), "gate_eval_mfma: null argument");
  COMA_CHECK(t_same_grid(x, att) && x->C == att->C && att->dtype == COMA_BF16 &&
             (!psi || (t_same_grid(x, psi) && psi->C == 1 && psi->dtype == COMA_BF16)), "gate_eval_mfma: shape/dtype mismatch");
  COMA_CHECK(coma_gate_eval_mfma_ok(g, x, 32) && gate_al16(att), "gate_eval_mfma: unsupported problem (ask coma_gate_eval_mfma_ok)");
  COMA_CHECK((((uintptr_t)wg_folded | (uintptr_t)wx_folded) & 15) == 0, "gate_eval_mfma: folded weights must be 16-byte aligned");
  GateEvalP p{};
  gate_eval_common(p, x, psi, att);
  p.g1 = g->data; p.ldg = g->ld; p.sbg = g->sb;
  p.F = 32; p.wg = wg_folded; p.wx = wx_folded; p.sh = shift; p.w = w_psi; p.ab = psi_ab;
  int64_t nb = ((p.V + 31) / 32 + 3) / 4;
  if (nb > GATE_EVAL_MFMA_BLOCKS) nb = GATE_EVAL_MFMA_BLOCKS;
  dim3 grid((unsigned)nb, (unsigned)x->B);
  const int ks = x->C / 16;
  if (ks == 1) hipLaunchKernelGGL((gate_eval_mfma_k<1>), grid, dim3(256), 0, s, p);
  else if (ks == 2) hipLaunchKernelGGL((gate_eval_mfma_k<2>), grid, dim3(256), 0, s, p);
  else if (ks == 3) hipLaunchKernelGGL((gate_eval_mfma_k<3>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((gate_eval_mfma_k<4>), grid, dim3(256), 0, s, p);
  COMA_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// FROZEN gate: a train-mode model whose three gate BatchNorms normalise with their running statistics.  Each is a known
// affine map (m = running_mean, r = rsqrt(running_var + eps): the caller's fp32 tables), so forward is the eval pass and
// backward needs no statistics of its own gradients:
//     t = gam_g ghat + bet_g + gam_x x1hat + bet_x     s = relu(t)     pr = w_psi . s + b_psi
//     zhat = (pr - m_p) r_p     psi = sigmoid(gam_p zhat + bet_p)      att = x psi
//   gate_frozen_fwd_k   g1raw, x1raw, x -> att, psi.  s is NOT saved: the backward reads g1raw / x1raw anyway (ghat and
//                       x1hat for dgamma_g / dgamma_x) and t, s, pr come out of them in registers.
//   gate_frozen_bwd_k   x, psi, d(att), g1raw, x1raw -> dx (= or +=), dg1raw, dx1raw and the block's sums
//                       {sum d, sum d ghat, sum d x1hat, sum dpr s}[F], {sum dzp, sum dzp zhat} into a replica record
//   gate_frozen_finalize_k   record -> the eight parameter gradients and d(b_psi) (one block)
struct GateFrozenP {
  GateEvalP e;                             // x, g1raw, x1raw, att (forward), psi, V, B, C, F, cv
  const float *mean_g, *rstd_g, *gam_g, *bet_g, *mean_x, *rstd_x, *gam_x, *bet_x, *mean_p, *rstd_p, *gam_p, *bet_p;
  const float *w, *bias;                   // psi convolution: w[F], bias[1] or NULL
  const void* dout; int64_t ldo, sbo;      // backward: d(att)
  void* dx; int64_t lddx, sbdx; int acc;   // dx (=) or (+=) d(att) psi
  void* dg1; int64_t lddg, sbdg;
  void* dx1; int64_t lddx1, sbdx1;
  double* rec; int64_t rrs;                // zeroed record [rep][F + 1][4]: [c][4] as above, [F][0..1] the two psi sums
  float *dgam_g, *dbet_g, *dgam_x, *dbet_x, *dw, *db, *dgam_p, *dbet_p;
};

// the block's folded tables (whole block; ends with a barrier)
__device__ __forceinline__ void gate_frozen_fold(const GateFrozenP& p, float* t_scg, float* t_scx, float* t_sh, float* t_w) {
  for (int c = threadIdx.x; c < p.e.F; c += 256) {
    const float sg = p.rstd_g[c] * p.gam_g[c], sx = p.rstd_x[c] * p.gam_x[c];
    t_scg[c] = sg; t_scx[c] = sx;
    t_sh[c] = (p.bet_g[c] - p.mean_g[c] * sg) + (p.bet_x[c] - p.mean_x[c] * sx);
    t_w[c] = p.w[c];
  }
  __syncthreads();
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void gate_frozen_fwd_k(GateFrozenP p) {
  __shared__ float t_scg[GATE_TAB], t_scx[GATE_TAB], t_sh[GATE_TAB], t_w[GATE_TAB];
  gate_frozen_fold(p, t_scg, t_scx, t_sh, t_w);
  // gam_p zhat + bet_p = a_p dot + b_p with a_p = gam_p r_p, b_p = a_p (b_psi - m_p) + bet_p
  const float pa = p.gam_p[0] * p.rstd_p[0];
  const float pb = fmaf(pa, (p.bias ? *p.bias : 0.f) - p.mean_p[0], p.bet_p[0]);
  gate_affine_fwd<T, VEC>(p.e, t_scg, t_scx, t_sh, t_w, pa, pb);
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void gate_frozen_bwd_k(GateFrozenP p) {
  __shared__ float t_scg[GATE_TAB], t_scx[GATE_TAB], t_sh[GATE_TAB], t_w[GATE_TAB];
  __shared__ double sh[256][4 * VEC];
  __shared__ double red[2][4];
  gate_frozen_fold(p, t_scg, t_scx, t_sh, t_w);
  const int b = blockIdx.y, tid = threadIdx.x;
  const int cv = p.e.cv;                                 // lanes per voxel: a power of two <= 64
  const int c0 = (tid % cv) * VEC;
  const bool in_f = c0 < p.e.F, in_c = c0 < p.e.C;       // (F and C are multiples of VEC)
  float scg[VEC], scx[VEC], shf[VEC], w[VEC], mg[VEC], rg[VEC], mx[VEC], rx[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    scg[j] = in_f ? t_scg[c0 + j] : 0.f; scx[j] = in_f ? t_scx[c0 + j] : 0.f;
    shf[j] = in_f ? t_sh[c0 + j] : 0.f; w[j] = in_f ? t_w[c0 + j] : 0.f;
    mg[j] = in_f ? p.mean_g[c0 + j] : 0.f; rg[j] = in_f ? p.rstd_g[c0 + j] : 0.f;
    mx[j] = in_f ? p.mean_x[c0 + j] : 0.f; rx[j] = in_f ? p.rstd_x[c0 + j] : 0.f;
  }
  const float rp = p.rstd_p[0], cp = p.gam_p[0] * rp;
  const float zb = ((p.bias ? *p.bias : 0.f) - p.mean_p[0]) * rp;            // zhat = dot r_p + zb
  const T* gb = reinterpret_cast<const T*>(p.e.g1) + (int64_t)b * p.e.sbg;
  const T* x1b = reinterpret_cast<const T*>(p.e.x1) + (int64_t)b * p.e.sbx1;
  const T* xb = reinterpret_cast<const T*>(p.e.x) + (int64_t)b * p.e.sbx;
  const T* qb = reinterpret_cast<const T*>(p.e.psi) + (int64_t)b * p.e.sbq;
  const T* ob = reinterpret_cast<const T*>(p.dout) + (int64_t)b * p.sbo;
  T* dxb = reinterpret_cast<T*>(p.dx) + (int64_t)b * p.sbdx;
  T* dgb = reinterpret_cast<T*>(p.dg1) + (int64_t)b * p.sbdg;
  T* dx1b = reinterpret_cast<T*>(p.dx1) + (int64_t)b * p.sbdx1;
  const int vpb = 256 / cv;                              // voxels per block step
  const int64_t vstep = (int64_t)gridDim.x * vpb;
  float f[4 * VEC], f1 = 0.f, f2 = 0.f;
  double acc[4 * VEC], s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int j = 0; j < 4 * VEC; ++j) { f[j] = 0.f; acc[j] = 0.0; }
  int cnt = 0;
  constexpr int U = 2;
  for (int64_t v = (int64_t)blockIdx.x * vpb + tid / cv; v < p.e.V; v += U * vstep) {   // (whole waves run every trip: shuffles)
    float gv[U][VEC], x1v[U][VEC], xv[U][VEC], dv[U][VEC], ov[U][VEC], ps[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t vv = v + u * vstep;
      live[u] = vv < p.e.V;
      const int64_t va = live[u] ? vv : v;
#pragma unroll
      for (int j = 0; j < VEC; ++j) { gv[u][j] = 0.f; x1v[u][j] = 0.f; xv[u][j] = 0.f; dv[u][j] = 0.f; ov[u][j] = 0.f; }
      if (in_f) { vec_io<T, VEC>::load(gb + va * p.e.ldg + c0, gv[u]); vec_io<T, VEC>::load(x1b + va * p.e.ldx1 + c0, x1v[u]); }
      if (in_c) {
        vec_io<T, VEC>::load(xb + va * p.e.ldx + c0, xv[u]);
        vec_io<T, VEC>::load(ob + va * p.ldo + c0, dv[u]);
        if (p.acc) vec_io<T, VEC>::load(dxb + va * p.lddx + c0, ov[u]);
      }
      ps[u] = ld_f(qb + va * p.e.ldq);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t vv = v + u * vstep;
      float tv[VEC], dot_s = 0.f, dot_x = 0.f;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        tv[j] = fmaf(gv[u][j], scg[j], fmaf(x1v[u][j], scx[j], shf[j]));
        dot_s = fmaf(tv[j] > 0.f ? tv[j] : 0.f, w[j], dot_s);
        dot_x = fmaf(xv[u][j], dv[u][j], dot_x);
        ov[u][j] += dv[u][j] * ps[u];
      }
      if (live[u] && in_c) vec_io<T, VEC>::store(dxb + vv * p.lddx + c0, ov[u]);
      for (int o = cv >> 1; o > 0; o >>= 1) { dot_s += __shfl_xor(dot_s, o, 64); dot_x += __shfl_xor(dot_x, o, 64); }
      const float dzp = live[u] ? dot_x * ps[u] * (1.f - ps[u]) : 0.f;
      const float dpr = dzp * cp;
      if (c0 == 0) { f1 += dzp; f2 = fmaf(dzp, fmaf(dot_s, rp, zb), f2); }
      float og[VEC], ox[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float d = tv[j] > 0.f ? dpr * w[j] : 0.f;
        og[j] = d * scg[j]; ox[j] = d * scx[j];
        f[4 * j] += d;
        f[4 * j + 1] = fmaf(d, (gv[u][j] - mg[j]) * rg[j], f[4 * j + 1]);
        f[4 * j + 2] = fmaf(d, (x1v[u][j] - mx[j]) * rx[j], f[4 * j + 2]);
        f[4 * j + 3] = fmaf(dpr, tv[j] > 0.f ? tv[j] : 0.f, f[4 * j + 3]);
      }
      if (live[u] && in_f) {
        vec_io<T, VEC>::store(dgb + vv * p.lddg + c0, og);
        vec_io<T, VEC>::store(dx1b + vv * p.lddx1 + c0, ox);
      }
    }
    if (++cnt == 8) {                                    // fp32 partial sums over 16 voxels, folded into fp64
#pragma unroll
      for (int j = 0; j < 4 * VEC; ++j) { acc[j] += (double)f[j]; f[j] = 0.f; }
      s1 += (double)f1; s2 += (double)f2; f1 = 0.f; f2 = 0.f; cnt = 0;
    }
  }
#pragma unroll
  for (int j = 0; j < 4 * VEC; ++j) sh[tid][j] = acc[j] + (double)f[j];
  s1 += (double)f1; s2 += (double)f2;
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = s2; }
  __syncthreads();
  for (int off = vpb >> 1; off > 0; off >>= 1) {         // tree over the block's voxel slots (tid = slot * cv + lane)
    if (tid / cv < off) {
#pragma unroll
      for (int j = 0; j < 4 * VEC; ++j) sh[tid][j] += sh[tid + off * cv][j];
    }
    __syncthreads();
  }
  // slot 0 of the tree = a contiguous [max(C, F)][4] image; its first F rows are the record's
  rec_add(p.rec, p.rrs, 0, &sh[0][0], p.e.F * 4);
  if (tid < 2) {
    const double t = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    add_f64(p.rec + (int64_t)(blockIdx.x & (COMA_STAT_REPLICAS - 1)) * p.rrs + 4 * p.e.F + tid, t);
  }
}

__global__ __launch_bounds__(256) void gate_frozen_finalize_k(GateFrozenP p) {
  for (int c = threadIdx.x; c < p.e.F; c += 256) {
    const double a = rec_get(p.rec, p.rrs, 4 * c);
    if (p.dbet_g) p.dbet_g[c] = (float)a;
    if (p.dbet_x) p.dbet_x[c] = (float)a;
    if (p.dgam_g) p.dgam_g[c] = (float)rec_get(p.rec, p.rrs, 4 * c + 1);
    if (p.dgam_x) p.dgam_x[c] = (float)rec_get(p.rec, p.rrs, 4 * c + 2);
    if (p.dw) p.dw[c] = (float)rec_get(p.rec, p.rrs, 4 * c + 3);
  }
  if (threadIdx.x == 0) {
    const double sz = rec_get(p.rec, p.rrs, 4 * p.e.F);
    if (p.dbet_p) p.dbet_p[0] = (float)sz;
    if (p.dgam_p) p.dgam_p[0] = (float)rec_get(p.rec, p.rrs, 4 * p.e.F + 1);
    if (p.db) p.db[0] = (float)(sz * (double)(p.gam_p[0] * p.rstd_p[0]));      // sum dpr = gam_p r_p sum dzp
  }
}

// vector width and lanes per voxel of the frozen gate kernels over the given tensors (0: outside the envelope)
static int gate_frozen_vec(int dtype, const coma_tensor* const* ts, int n, int C, int F, int want) {
  const int m = C > F ? C : F;
  int vec = gate_vec(ts, n, want);
  if (vec == 2) vec = 1;
  while (vec > 1 && !pow2_le64(m / vec)) vec = vec == 8 ? 4 : 1;
  (void)dtype;
  return (C % vec == 0 && F % vec == 0 && pow2_le64(m / vec) && F >= 1 && F <= GATE_TAB) ? vec : 0;
}

static int gate_frozen_common(GateFrozenP& p, const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw,
                              const coma_tensor* psi, const float* const* bn_g, const float* const* bn_x,
                              const float* const* bn_p, const float* w_psi, const float* b_psi) {
  p.e.x = x->data; p.e.ldx = x->ld; p.e.sbx = x->sb;
  p.e.g1 = g1raw->data; p.e.ldg = g1raw->ld; p.e.sbg = g1raw->sb;
  p.e.x1 = x1raw->data; p.e.ldx1 = x1raw->ld; p.e.sbx1 = x1raw->sb;
  p.e.psi = psi->data; p.e.ldq = psi->ld; p.e.sbq = psi->sb;
  p.e.V = t_vox(x); p.e.B = x->B; p.e.C = x->C; p.e.F = g1raw->C;
  p.mean_g = bn_g[0]; p.rstd_g = bn_g[1]; p.gam_g = bn_g[2]; p.bet_g = bn_g[3];
  p.mean_x = bn_x[0]; p.rstd_x = bn_x[1]; p.gam_x = bn_x[2]; p.bet_x = bn_x[3];
  p.mean_p = bn_p[0]; p.rstd_p = bn_p[1]; p.gam_p = bn_p[2]; p.bet_p = bn_p[3];
  p.w = w_psi; p.bias = b_psi;
  return 0;
}

static bool gate_frozen_tables_ok(const float* const* bn) { return bn && bn[0] && bn[1] && bn[2] && bn[3]; }

extern "C" int coma_gate_frozen_ok(const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw,
                                   const coma_tensor* att) {
  if (!x || !g1raw || !x1raw || !att) return 0;
  if (!(t_same_grid(x, g1raw) && t_same_grid(x, x1raw) && t_same_grid(x, att) && g1raw->C == x1raw->C && x->C == att->C &&
        x->dtype == g1raw->dtype && x->dtype == x1raw->dtype && x->dtype == att->dtype)) return 0;
  const coma_tensor* ts[4] = {x, g1raw, x1raw, att};
  // the backward runs 4 wide at most (its gradients come in buffers of the same alignment as these)
  return gate_frozen_vec(x->dtype, ts, 4, x->C, g1raw->C, 4) > 0 ? 1 : 0;
}

extern "C" int coma_gate_frozen_fwd(const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw,
                                    const float* const* bn_g, const float* const* bn_x, const float* const* bn_p,
                                    const float* w_psi, const float* b_psi, const coma_tensor* psi, const coma_tensor* att,
                                    void* stream) {
  hipStream_t s = (hipStream_t)stream;
  COMA_CHECK(x && g1raw && x1raw && psi && att && x->data && g1raw->data && x1raw->data && psi->data && att->data && w_psi &&
             gate_frozen_tables_ok(bn_g) && gate_frozen_tables_ok(bn_x) && gate_frozen_tables_ok(bn_p), "gate_frozen_fwd: null argument");
  COMA_CHECK(t_same_grid(x, g1raw) && t_same_grid(x, x1raw) && t_same_grid(x, att) && t_same_grid(x, psi) && psi->C == 1 &&
             g1raw->C == x1raw->C && x->C == att->C && x->dtype == g1raw->dtype && x->dtype == x1raw->dtype &&
             x->dtype == att->dtype && psi->dtype == x->dtype, "gate_frozen_fwd: shape/dtype mismatch");
  const coma_tensor* ts[4] = {x, g1raw, x1raw, att};
  const int vec = gate_frozen_vec(x->dtype, ts, 4, x->C, g1raw->C, x->dtype == COMA_BF16 ? 8 : 4);
  COMA_CHECK(vec > 0, "gate_frozen_fwd: C=%d F=%d unsupported (max(C, F) / vector width must be a power of two <= 64)", x->C, g1raw->C);
  GateFrozenP p{};
  gate_frozen_common(p, x, g1raw, x1raw, psi, bn_g, bn_x, bn_p, w_psi, b_psi);
  p.e.att = att->data; p.e.lda = att->ld; p.e.sba = att->sb;
  p.e.cv = (x->C > g1raw->C ? x->C : g1raw->C) / vec;
  int cap = 2048 / x->B; if (cap < 1) cap = 1;
  dim3 grid(gate_blocks(p.e.V, (256 / p.e.cv) * 2, cap), x->B);
  GATE_DISPATCH(gate_frozen_fwd_k, x->dtype, vec, grid, p);
  COMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int coma_gate_frozen_bwd(const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw,
                                    const coma_tensor* psi, const coma_tensor* datt, const float* const* bn_g,
                                    const float* const* bn_x, const float* const* bn_p, const float* w_psi, const float* b_psi,
                                    const coma_tensor* dx, int32_t accumulate_dx, const coma_tensor* dg1raw,
                                    const coma_tensor* dx1raw, double* rec, float* dgamma_g, float* dbeta_g, float* dgamma_x,
                                    float* dbeta_x, float* dw_psi, float* db_psi, float* dgamma_psi, float* dbeta_psi,
                                    void* stream) {
  hipStream_t s = (hipStream_t)stream;
  COMA_CHECK(x && g1raw && x1raw && psi && datt && dx && dg1raw && dx1raw && x->data && g1raw->data && x1raw->data && psi->data &&
             datt->data && dx->data && dg1raw->data && dx1raw->data && w_psi && rec && gate_frozen_tables_ok(bn_g) &&
             gate_frozen_tables_ok(bn_x) && gate_frozen_tables_ok(bn_p), "gate_frozen_bwd: null argument");
  COMA_CHECK(t_same_grid(x, g1raw) && t_same_grid(x, x1raw) && t_same_grid(x, psi) && t_same_grid(x, datt) && t_same_grid(x, dx) &&
             t_same_grid(x, dg1raw) && t_same_grid(x, dx1raw) && psi->C == 1 && g1raw->C == x1raw->C && g1raw->C == dg1raw->C &&
             g1raw->C == dx1raw->C && x->C == datt->C && x->C == dx->C, "gate_frozen_bwd: shape mismatch");
  COMA_CHECK(x->dtype == g1raw->dtype && x->dtype == x1raw->dtype && x->dtype == psi->dtype && x->dtype == datt->dtype &&
             x->dtype == dx->dtype && x->dtype == dg1raw->dtype && x->dtype == dx1raw->dtype, "gate_frozen_bwd: dtype mismatch");
  const coma_tensor* ts[7] = {x, g1raw, x1raw, datt, dx, dg1raw, dx1raw};
  // 4 wide at most: 16 fp64 + 16 fp32 accumulators per lane beside five tensors in flight (8 wide would spill)
  const int vec = gate_frozen_vec(x->dtype, ts, 7, x->C, g1raw->C, 4);
  COMA_CHECK(vec > 0, "gate_frozen_bwd: C=%d F=%d unsupported (max(C, F) / vector width must be a power of two <= 64)", x->C, g1raw->C);
  GateFrozenP p{};
  gate_frozen_common(p, x, g1raw, x1raw, psi, bn_g, bn_x, bn_p, w_psi, b_psi);
  p.e.cv = (x->C > g1raw->C ? x->C : g1raw->C) / vec;
  p.dout = datt->data; p.ldo = datt->ld; p.sbo = datt->sb;
  p.dx = dx->data; p.lddx = dx->ld; p.sbdx = dx->sb; p.acc = accumulate_dx;
  p.dg1 = dg1raw->data; p.lddg = dg1raw->ld; p.sbdg = dg1raw->sb;
  p.dx1 = dx1raw->data; p.lddx1 = dx1raw->ld; p.sbdx1 = dx1raw->sb;
  p.rec = rec; p.rrs = COMA_NORM_RECORD_DOUBLES(1, g1raw->C + 1, 4);
  p.dgam_g = dgamma_g; p.dbet_g = dbeta_g; p.dgam_x = dgamma_x; p.dbet_x = dbeta_x; p.dw = dw_psi; p.db = db_psi;
  p.dgam_p = dgamma_psi; p.dbet_p = dbeta_psi;
  int cap = 2048 / x->B; if (cap < 1) cap = 1;
  dim3 grid(gate_blocks(p.e.V, (256 / p.e.cv) * 2, cap), x->B);
  if (x->dtype == COMA_F32) { if (vec == 4) hipLaunchKernelGGL((gate_frozen_bwd_k<float, 4>), grid, dim3(256), 0, s, p);
                              else hipLaunchKernelGGL((gate_frozen_bwd_k<float, 1>), grid, dim3(256), 0, s, p); }
  else { if (vec == 4) hipLaunchKernelGGL((gate_frozen_bwd_k<bf16_t, 4>), grid, dim3(256), 0, s, p);
         else hipLaunchKernelGGL((gate_frozen_bwd_k<bf16_t, 1>), grid, dim3(256), 0, s, p); }
  COMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(gate_frozen_finalize_k, dim3(1), dim3(256), 0, s, p);
  COMA_LAUNCH_CHECK();
  return 0;
}
