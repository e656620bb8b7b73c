// What conv_mfma.hip and conv_wgrad.hip share, and the convolution entry points api.hip and conv_split.hip call.
#pragma once
#include "common.h"
#include "conv_tiles.h"   // bf16x8_t / f32x16_t, stat_add, xcd_remap, tile_coords, tile_run, set_max_lds
#include <stdlib.h>

// 8 channels starting at `ptr`, of which `nvalid` exist; `vec` = 16-byte access is legal here: the base is 16-byte
// aligned and the voxel pitch is a multiple of 8 channels, so the 8-channel piece lies inside the voxel's row even when
// fewer than 8 of its channels belong to this tensor (a channel slice of a wider, padded buffer) -- those are masked off.
__device__ __forceinline__ uint4 load8(const bf16_t* ptr, int nvalid, bool vec) {
  if (vec) {
    uint4 v = *reinterpret_cast<const uint4*>(ptr);
    if (nvalid < 8) {
      auto m = [&](int j) -> unsigned { const int k = nvalid - 2 * j; return k >= 2 ? 0xffffffffu : (k == 1 ? 0xffffu : 0u); };
      v.x &= m(0); v.y &= m(1); v.z &= m(2); v.w &= m(3);
    }
    return v;
  }
  unsigned short e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = j < nvalid ? reinterpret_cast<const unsigned short*>(ptr)[j] : (unsigned short)0;
  return make_uint4(e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16), e[4] | ((unsigned)e[5] << 16),
                    e[6] | ((unsigned)e[7] << 16));
}

// The same piece WITHOUT the mask when the vector access is legal: a prefetch must not consume its data (the mask would
// put an s_waitcnt vmcnt(0) behind every load and serialise a tile's 13 loads); apply mask8() when the piece is stored.
__device__ __forceinline__ uint4 load8_raw(const bf16_t* ptr, int nvalid, bool vec) {
  if (vec) return *reinterpret_cast<const uint4*>(ptr);
  return load8(ptr, nvalid, false);
}
__device__ __forceinline__ uint4 mask8(int nvalid) {
  auto m = [&](int j) -> unsigned { const int k = nvalid - 2 * j; return k >= 2 ? 0xffffffffu : (k == 1 ? 0xffffu : 0u); };
  return make_uint4(m(0), m(1), m(2), m(3));
}

typedef __attribute__((ext_vector_type(4))) short s4_t;
typedef __attribute__((address_space(3))) s4_t lds_s4_t;

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- conv_mfma.hip ----
bool conv_mfma_supported(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
bool conv_f32mfma_supported(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int conv_mfma_fwd(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias,
                  const coma_tensor* y, hipStream_t s, double2* stats = nullptr, int stats_inst = 0,
                  int* stats_chunks = nullptr, void* ws = nullptr, size_t ws_bytes = 0, int ws_zeroed = 0, int accum = 0,
                  int wk_frag = 0);
size_t conv_mfma_wk_frag_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
bool conv_mfma_accumulate_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
size_t conv_mfma_fwd_ws_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
bool conv_mfma_wgrad_supported(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
size_t conv_mfma_wgrad_ws_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
int conv_mfma_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, void* ws,
                    size_t ws_bytes, hipStream_t s, int zeroed);
// the fp32 problems of conv_mfma_halo2_k<2, 16, 1, 1, float> / conv_mfma_tconv_k<float, *> / conv_f32_wgrad16_k<2, *>
bool conv_f32_halo2_problem(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
bool conv_f32_tconv_problem(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
bool conv_f32_wgrad16s2_problem(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
// the fp32 problems of conv_thin16f_k / conv_thin16f_wgrad_k
bool conv_f32_thin_problem(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
bool conv_f32_thin_wgrad_problem(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);

// ---- conv_pw_f32.hip (algo 7, pointwise: the 1x1x1 fp32 layers with several channels on both sides, exact fp32 MFMA) ----
bool conv_pw_f32_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int conv_pw_f32(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                hipStream_t s, double2* stats, int stats_inst, int* stats_chunks, int accum);
bool conv_pw_f32_wgrad_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
int conv_pw_f32_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, void* ws, size_t ws_bytes,
                      hipStream_t s, int zeroed);

// ---- between conv_mfma.hip and conv_wgrad.hip only ----
// Small weight tensors (the 1..16-channel layers, 1x1x1 gates): a thousand blocks merging into a few cache lines
// serialise in the L2 atomic unit (1 -> 32 channels at 128^3: 520 us, of which ~400 us were atomics).  Their blocks
// merge into WGRAD_NREP replicas in the workspace instead, summed by one tiny kernel.
#define WGRAD_NREP 64
#define WGRAD_REP_MAX_ELEMS 16384
static inline long wgrad_out_elems(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  return (long)d->ksize * d->ksize * d->ksize * dy->C * x->C * (d->per_sample_w ? x->B : 1);
}
// (hidden: not part of the library's symbol table)
#pragma GCC visibility push(hidden)
bool wgrad_plan_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
int conv_wgrad_planned(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, void* ws,
                       size_t ws_bytes, hipStream_t s, int zeroed);
int wgrad_replica_sum(const float* rep, long wsz, float* dwk, hipStream_t s);      // (conv_mfma.hip)
#pragma GCC visibility pop
