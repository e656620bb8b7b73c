// C-ABI entry points that dispatch between kernel families, plus error reporting.
#include "conv_mfma.h"
#include <string.h>

static thread_local char g_err[512] = "";

void coma_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static thread_local char g_ktag[160] = "";

void coma_set_kernel_tag(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_ktag, sizeof(g_ktag), fmt, ap);
  va_end(ap);
}

extern "C" const char* coma_last_kernel(void) { return g_ktag; }
extern "C" int coma_abi_version(void) { return COMA_ABI_VERSION; }
extern "C" const char* coma_last_error(void) { return g_err; }

// conv_direct.hip
int conv_check(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int conv_direct_fwd(const coma_conv_desc* d, const coma_tensor* x, const float* wk, const float* bias,
                    const coma_tensor* y, hipStream_t s);
int conv_direct_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, hipStream_t s, int zeroed);
// conv_point1.hip
bool conv_point1_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int conv_point1_fwd(const coma_conv_desc* d, const coma_tensor* x, const float* wk, const float* bias, const coma_tensor* y,
                    hipStream_t s);
int conv_point1_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, hipStream_t s, int zeroed);
// norm.hip
int colsum(const coma_tensor* x, int per_sample, float* out, void* ws, size_t ws_bytes, hipStream_t s);
// conv_mfma.hip: conv_mfma.h
// conv_split.hip (algo 4: fp32 tensors, two-term bf16 split on the bf16 matrix pipe)
bool conv_split_fwd_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int conv_split_fwd(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                   hipStream_t s, double2* stats, int stats_inst, int* stats_chunks);
bool conv_split_wgrad_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
int conv_split_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, hipStream_t s, int zeroed);
// (algo 5, wide split: algo 4 plus the stride-2 transposed / data-gradient kernel and the stride-2 weight gradients)
bool conv_split_tconv_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int conv_split_tconv(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                     hipStream_t s, int accum);
bool conv_split_wgrad2_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
int conv_split_wgrad2(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, hipStream_t s, int zeroed);
// (algo 6, thin split: algo 5 plus the few-channel full-resolution layers, forward / data gradient and weight gradient)
bool conv_split_thin_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int conv_split_thin(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                    hipStream_t s, double2* stats, int stats_inst, int* stats_chunks);
bool conv_split_thin_wgrad_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
int conv_split_thin_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, void* ws, size_t ws_bytes,
                          hipStream_t s, int zeroed);

// (algo 7, pointwise: algo 6 plus the 1x1x1 fp32 layers with several channels on both sides on the exact fp32 MFMA:
// conv_pw_f32.hip, declared in conv_mfma.h.  These problems resolve to 3 -- fp32 kernel-layout weights)
static bool thin_on(const coma_conv_desc* d) { return d->algo == 6 || d->algo == 7; }
static bool pw_fwd(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) { return d->algo == 7 && conv_pw_f32_ok(d, x, y); }
static bool pw_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) { return d->algo == 7 && conv_pw_f32_wgrad_ok(d, x, dy); }

// the split kernel of a problem that resolved to 4: stride 1 under algo 4 to 7, the stride-2 families under algo 5 to 7,
// the thin layers under algo 6 and 7 only (the three scopes are disjoint)
static int split_fwd(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                     hipStream_t s, double2* stats, int stats_inst, int* stats_chunks, int accum) {
  if (conv_split_fwd_ok(d, x, y)) return conv_split_fwd(d, x, wk, bias, y, s, stats, stats_inst, stats_chunks);
  if (thin_on(d) && conv_split_thin_ok(d, x, y)) return conv_split_thin(d, x, wk, bias, y, s, stats, stats_inst, stats_chunks);
  return conv_split_tconv(d, x, wk, bias, y, s, accum);      // (statistics not fused: *stats_chunks stays 0, the caller runs the separate pass)
}

extern "C" int coma_conv_pick_algo(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  if (d->algo == 1) return 1;
  if (conv_point1_ok(d, x, y)) return 1;            // one channel on a side: streaming dot / scale kernels (fp32 weights)
  if (d->algo == 4 && conv_split_fwd_ok(d, x, y)) return 4;   // split: the thick stride-1 3^3 fp32 layers; every other problem as algo 0
  if (d->algo == 5 && (conv_split_fwd_ok(d, x, y) || conv_split_tconv_ok(d, x, y))) return 4;   // wide split: + stride-2 transposed / data gradient
  if (thin_on(d) && (conv_split_fwd_ok(d, x, y) || conv_split_tconv_ok(d, x, y) || conv_split_thin_ok(d, x, y))) return 4;   // thin split: + C <= 16 at W >= 32
  if (pw_fwd(d, x, y)) return 3;                    // pointwise: the 1x1x1 fp32 layers on conv_pw_f32_k (ksize 1: none of the split scopes)
  if (conv_mfma_supported(d, x, y)) return 2;       // bf16 tensors: MFMA wherever the shape allows
  if (conv_f32mfma_supported(d, x, y)) return 3;    // fp32 tensors: fp32 MFMA wherever the shape allows
  return 1;
}

extern "C" int coma_conv_accumulate_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  const int algo = coma_conv_pick_algo(d, x, y);
  if (pw_fwd(d, x, y)) return 1;
  return algo >= 2 && conv_mfma_accumulate_ok(d, x, y) ? 1 : 0;
}

extern "C" size_t coma_conv_fwd_ws_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  if (pw_fwd(d, x, y)) return 0;
  return coma_conv_pick_algo(d, x, y) >= 2 ? conv_mfma_fwd_ws_bytes(d, x, y) : 0;
}

extern "C" size_t coma_conv_wk_frag_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y) {
  if (!d || !x || !y) return 0;
  return coma_conv_pick_algo(d, x, y) == 2 ? conv_mfma_wk_frag_bytes(d, x, y) : 0;
}

extern "C" int coma_conv_fwd(const coma_conv_desc* d, const coma_tensor* x, const void* wk, int32_t wk_dtype,
                             const float* bias, const coma_tensor* y, void* stream) {
  return coma_conv_fwd_ws(d, x, wk, wk_dtype, bias, y, nullptr, 0, 0, stream);
}

extern "C" int coma_conv_fwd_ws(const coma_conv_desc* d, const coma_tensor* x, const void* wk, int32_t wk_dtype,
                                const float* bias, const coma_tensor* y, void* ws, size_t ws_bytes, int32_t zeroed,
                                void* stream) {
  if (int rc = conv_check(d, x, y)) return rc;
  COMA_CHECK(wk, "conv_fwd: null weights");
  const int wz = (zeroed & COMA_ZEROED_WS) ? 1 : 0, accum = (zeroed & COMA_ACCUMULATE) ? 1 : 0;
  COMA_CHECK(!accum || coma_conv_accumulate_ok(d, x, y), "conv_fwd: COMA_ACCUMULATE is not supported for this problem (ask coma_conv_accumulate_ok)");
  hipStream_t s = (hipStream_t)stream;
  const int algo = coma_conv_pick_algo(d, x, y);
  if (zeroed & COMA_WK_FRAG) {
    COMA_CHECK(algo == 2 && wk_dtype == COMA_BF16 && !accum, "conv_fwd: COMA_WK_FRAG needs a bf16 MFMA problem (ask coma_conv_wk_frag_bytes)");
    return conv_mfma_fwd(d, x, wk, bias, y, s, nullptr, 0, nullptr, nullptr, 0, 0, 0, 1);
  }
  if (algo == 2) {
    COMA_CHECK(wk_dtype == COMA_BF16, "conv_fwd: MFMA path needs bf16 kernel-layout weights");
    COMA_CHECK(conv_mfma_supported(d, x, y), "conv_fwd: shape not supported by the MFMA path (C=%d N=%d dtype=%d)",
               x->C, y->C, x->dtype);
    return conv_mfma_fwd(d, x, wk, bias, y, s, nullptr, 0, nullptr, ws, ws_bytes, wz, accum);
  }
  COMA_CHECK(wk_dtype == COMA_F32, "conv_fwd: fp32 tensors need fp32 kernel-layout weights");
  if (algo == 4) return split_fwd(d, x, wk, bias, y, s, nullptr, 0, nullptr, accum);
  if (pw_fwd(d, x, y)) return conv_pw_f32(d, x, wk, bias, y, s, nullptr, 0, nullptr, accum);
  if (algo == 3) return conv_mfma_fwd(d, x, wk, bias, y, s, nullptr, 0, nullptr, ws, ws_bytes, wz, accum);
  if (conv_point1_ok(d, x, y)) return conv_point1_fwd(d, x, (const float*)wk, bias, y, s);
  return conv_direct_fwd(d, x, (const float*)wk, bias, y, s);
}

extern "C" int coma_conv_wgrad_algo(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  if (d->algo == 1 || conv_point1_ok(d, x, dy)) return 1;
  if (d->algo == 4 && conv_split_wgrad_ok(d, x, dy)) return 4;
  if (d->algo == 5 && (conv_split_wgrad_ok(d, x, dy) || conv_split_wgrad2_ok(d, x, dy))) return 4;
  if (thin_on(d) && (conv_split_wgrad_ok(d, x, dy) || conv_split_wgrad2_ok(d, x, dy) || conv_split_thin_wgrad_ok(d, x, dy))) return 4;
  if (pw_wgrad(d, x, dy)) return 3;
  if (!conv_mfma_wgrad_supported(d, x, dy)) return 1;
  return x->dtype == COMA_BF16 ? 2 : 3;
}

// conv forward + the statistics of the following BatchNorm(train)/InstanceNorm in one pass where the kernel family
// supports it (the epilogue ADDS its {sum, sumsq} to the caller's zeroed fp64 record `sums[G][C][2]`), otherwise conv
// followed by the stand-alone statistics pass (which adds to the same record).
extern "C" int coma_conv_fwd_norm_stats(const coma_conv_desc* d, const coma_tensor* x, const void* wk, int32_t wk_dtype,
                                        const float* bias, const coma_tensor* y, int32_t mode, double* sums, void* ws,
                                        size_t ws_bytes, int32_t zeroed, void* stream) {
  if (int rc = conv_check(d, x, y)) return rc;
  COMA_CHECK(wk && sums, "conv_fwd_norm_stats: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int algo_ = coma_conv_pick_algo(d, x, y);
  const int wk_frag = (zeroed & COMA_WK_FRAG) ? 1 : 0;
  COMA_CHECK(!wk_frag || (algo_ == 2 && wk_dtype == COMA_BF16), "conv_fwd_norm_stats: COMA_WK_FRAG needs a bf16 MFMA problem (ask coma_conv_wk_frag_bytes)");
  if ((algo_ == 2 && wk_dtype == COMA_BF16) || (algo_ >= 3 && wk_dtype == COMA_F32)) {
    int fused = 0;
    const int inst = mode == COMA_NORM_INSTANCE ? y->B : 0;      // (the kernels' group count; 0 = one BatchNorm group)
    if (pw_fwd(d, x, y)) {
      if (int rc = conv_pw_f32(d, x, wk, bias, y, s, (double2*)sums, inst, &fused, 0)) return rc;
    } else if (algo_ == 4) {
      if (int rc = split_fwd(d, x, wk, bias, y, s, (double2*)sums, inst, &fused, 0)) return rc;
    } else if (int rc = conv_mfma_fwd(d, x, wk, bias, y, s, (double2*)sums, inst, &fused, ws, ws_bytes, (zeroed & COMA_ZEROED_WS) ? 1 : 0, 0, wk_frag)) return rc;
    if (fused) return 0;
  } else {
    if (int rc = coma_conv_fwd(d, x, wk, wk_dtype, bias, y, stream)) return rc;
  }
  return coma_norm_stats(y, mode, sums, stream);
}

extern "C" size_t coma_conv_wgrad_ws_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  size_t a = coma_norm_ws_bytes(dy);
  size_t b = conv_mfma_wgrad_supported(d, x, dy) ? conv_mfma_wgrad_ws_bytes(d, x, dy) : 0;
  return a > b ? a : b;
}

// the part of coma_conv_wgrad_ws_bytes() the weight-gradient kernels merge into with atomics (their replica scratch): what
// a caller with a pre-zeroed arena hands over as `ws` together with COMA_ZEROED_WS (0: nothing of ws needs to be zero)
extern "C" size_t coma_conv_wgrad_zs_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  if (conv_point1_ok(d, x, dy) || coma_conv_wgrad_algo(d, x, dy) < 2) return 0;
  return conv_mfma_wgrad_ws_bytes(d, x, dy);
}

extern "C" int coma_conv_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk,
                               float* dbias, void* ws, size_t ws_bytes, int32_t zeroed, void* stream) {
  if (int rc = conv_check(d, x, dy)) return rc;
  COMA_CHECK(dwk, "conv_wgrad: null dwk");
  hipStream_t s = (hipStream_t)stream;
  if (dbias) {
    // (the column sums write their partial rows into ws: a pre-zeroed ws is no longer zero afterwards)
    COMA_CHECK(ws && ws_bytes >= coma_norm_ws_bytes(dy), "conv_wgrad: workspace too small for the bias gradient");
    if (int rc = colsum(dy, d->per_sample_w, dbias, ws, ws_bytes, s)) return rc;
    zeroed &= ~COMA_ZEROED_WS;
  }
  if (conv_point1_ok(d, x, dy)) return conv_point1_wgrad(d, x, dy, dwk, s, zeroed);
  const int algo = coma_conv_wgrad_algo(d, x, dy);
  if (algo == 4) {
    if (conv_split_wgrad_ok(d, x, dy)) return conv_split_wgrad(d, x, dy, dwk, s, zeroed);
    if (thin_on(d) && conv_split_thin_wgrad_ok(d, x, dy)) return conv_split_thin_wgrad(d, x, dy, dwk, ws, ws_bytes, s, zeroed);      // (merges into the replica scratch, as algo 0)
    return conv_split_wgrad2(d, x, dy, dwk, s, zeroed);
  }
  if (pw_wgrad(d, x, dy)) return conv_pw_f32_wgrad(d, x, dy, dwk, ws, ws_bytes, s, zeroed);      // (merges into the replica scratch, as algo 0)
  if (algo >= 2) return conv_mfma_wgrad(d, x, dy, dwk, ws, ws_bytes, s, zeroed);
  return conv_direct_wgrad(d, x, dy, dwk, s, zeroed);
}
