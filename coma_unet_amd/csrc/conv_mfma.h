// What conv_mfma.hip and the files cut out of it (conv_duo.hip, conv_tconv.hip, conv_wgrad.hip) share, and the convolution
// entry points api.hip and conv_split.hip call.
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

// Everything below crosses a file boundary inside the library only (hidden: not part of its symbol table).
#pragma GCC visibility push(hidden)
// ---- between conv_mfma.hip (conv_mfma_halo2_k; conv_mfma_halo<T> fills the fields the two kernels share) and conv_duo.hip ----
struct Halo2P {
  const void* x; int ldx; long sbx; int D, H, W, C;
  void* y; int ldy; long sby; int N;
  const void* w; long wsb;
  const float* bias; int bsb;
  int flip, vecx, vecw;
  int ntx, nty, ntz, ids_total, ids_per_block;
  unsigned xbytes, wbytes;   // bytes of one sample of x / of one weight set (buffer descriptors: out-of-range pieces read as zero)
  int st8;             // output rows allow aligned 8-byte (4-channel) stores
  int st16;            // ... and aligned 16-byte (8-channel) stores
  double2* stats;      // optional: per-block {sum, sumsq} of the stored outputs, [chunk][G][N]
  int stats_inst;      // B: groups = the B samples (InstanceNorm), 0: one group (BatchNorm)
  const void* wfrag;   // conv_mfma_duo_k, C >= 64: the weights re-laid in fragment order (duo_relayout_k), else null
  long wfrag_sb;       // ... elements between two samples' weight sets
};
size_t duo_frag_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
bool duo_wide_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
// q: the common fields of conv_mfma_halo<bf16_t>; thin / vec / lx as there
bool duo_takes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y, const Halo2P& q, bool thin, bool vec, bool wk_frag,
               const void* ws, size_t ws_bytes, size_t* frag_bytes_out);
int launch_duo(const coma_conv_desc* d, const coma_tensor* x, Halo2P q, const void* wk, int lx, int nblk_n, size_t frag_bytes, void* ws,
               bool wk_frag, hipStream_t s);

// ---- conv_tconv.hip ----
bool tconv_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
template <typename T>
int conv_mfma_tconv(const coma_conv_desc* d, const coma_tensor* x, const void* wk, const float* bias, const coma_tensor* y,
                    hipStream_t s, double2* stats, int stats_inst, int* stats_chunks, int accum);

// ---- conv_wgrad.hip ----
bool wgrad_plan_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
int conv_wgrad_planned(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy, float* dwk, void* ws,
                       size_t ws_bytes, hipStream_t s, int zeroed);

// ---- the weight-gradient launchers whose blocks merge with atomics ----
// Small weight tensors (the 1..16-channel layers, 1x1x1 gates): a thousand blocks merging into a few cache lines
// serialise in the L2 atomic unit (1 -> 32 channels at 128^3: 520 us, of which ~400 us were atomics).  Their blocks
// merge into WGRAD_NREP replicas in the workspace instead, summed by one tiny kernel.
#define WGRAD_NREP 64
#define WGRAD_REP_MAX_ELEMS 16384
static inline long wgrad_out_elems(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy) {
  return (long)d->ksize * d->ksize * d->ksize * dy->C * x->C * (d->per_sample_w ? x->B : 1);
}
int wgrad_replica_sum(const float* rep, long wsz, float* dwk, hipStream_t s);      // (conv_mfma.hip)
// Where a launcher's blocks merge their wsz outputs: WGRAD_NREP replicas in ws when the output is small, the workspace is
// there and `allow`, else dwk itself; cleared here unless `zeroed` says the caller did (COMA_ZEROED_WS / COMA_ZEROED_OUT).
// out == nullptr: the memset failed (error set; return 2).  After the kernel: wgrad_replicas_done().
struct WgradRep { float* out; int nrep; long rep_stride; };
static inline WgradRep wgrad_replicas(long wsz, float* dwk, void* ws, size_t ws_bytes, hipStream_t s, int zeroed, bool allow = true) {
  const bool replicas = allow && wsz <= WGRAD_REP_MAX_ELEMS && ws && ws_bytes >= sizeof(float) * wsz * WGRAD_NREP;
  WgradRep r = {replicas ? (float*)ws : dwk, replicas ? WGRAD_NREP : 1, replicas ? wsz : 0};
  if (!(zeroed & (replicas ? COMA_ZEROED_WS : COMA_ZEROED_OUT)) && hipMemsetAsync(r.out, 0, sizeof(float) * wsz * r.nrep, s) != hipSuccess) { coma_set_error("wgrad memset failed"); r.out = nullptr; }
  return r;
}
static inline int wgrad_replicas_done(const WgradRep& r, long wsz, float* dwk, hipStream_t s) {
  return r.nrep > 1 ? wgrad_replica_sum(r.out, wsz, dwk, s) : 0;
}
#pragma GCC visibility pop
