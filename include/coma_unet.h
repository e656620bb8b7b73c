/*
 * coma_unet.h -- C ABI of the MI355X (gfx950) CoMA-UNet training hot path.
 *
 * Drop-in boundary.  The reference (mborhi/CoMA-UNet) is pure Python: its hot
 * path is the nn.Module / criterion surface of
 *   attn_unet_data_parallel.py:503-693  (ContrastiveAttentionUNET_DP)
 *   attn_unet_data_parallel.py:779-912  (train_dp step body)
 *   criterions.py:124-211,485-644       (RoiMSE, GenerativeContrastiveLoss, RnC)
 * and it has no FFI of its own; every conv / norm / activation there is a
 * cuDNN/ATen kernel that PyTorch dispatches.  This library is what replaces
 * those dispatches: one entry point per row of SURVEY.md section 2.1.  The
 * Python host (coma_unet_amd/) mirrors the reference's module surface and calls
 * these functions through ctypes with raw device pointers.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless the name ends in _host.
 *  - Activations are channels-last volumes "NDHWC": element (b, z, y, x, c) of
 *    a coma_tensor t lives at  data + b*sb + ((z*H + y)*W + x)*ld + c  (in
 *    elements of t.dtype).  ld >= C lets a tensor be a channel slice of a wider
 *    buffer, which is how torch.cat((att, fromlower), dim=1)
 *    (attn_unet_data_parallel.py:229,651,654) is done without a copy.
 *  - Parameters, statistics and weight gradients are fp32.
 *  - No function allocates, synchronises or keeps global state.  `stream` is a
 *    hipStream_t passed as void*.  Return value 0 = ok, otherwise an error code;
 *    coma_last_error() returns a thread-local message.
 *  - Process-wide switches, read once from the environment, all for A/B measurements
 *    of one build: COMA_NO_DUO, COMA_DUO_C32_ONLY, COMA_NO_TCONV, COMA_THIN16 (kernel
 *    dispatch of the convolutions), COMA_WPREP_BWD_OLD, COMA_WPREP_BWD_SPLIT (form of
 *    the expert scatter).  The Python host has its own, among
 *    them COMA_PREP_AHEAD and COMA_PREP_BATCH (batched weight preparation).
 *  - Workspaces are caller-provided; the *_ws_bytes query says how much.
 */
#ifndef COMA_UNET_H
#define COMA_UNET_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 2): coma_conv_pick_algo / coma_conv_wgrad_algo may answer 3 (fp32 MFMA), algo 0 routes fp32 tensors to the
 * fp32 MFMA kernels and one-channel 1x1x1 layers to conv_point1 (fp32 kernel-layout weights) before the bf16 MFMA path;
 * new exports coma_last_kernel, coma_comm_*, coma_allreduce/reduce_scatter/allgather/broadcast.
 * 3 (round 3): normalisation statistics travel as caller-zeroed fp64 records (coma_norm_stats / coma_norm_act_fwd /
 * coma_norm_act_bwd / coma_conv_fwd_norm_stats: no mean / rstd tensors, no finalise launches); `zeroed` arguments on
 * coma_conv_fwd_ws / coma_conv_fwd_norm_stats / coma_conv_wgrad / coma_weight_prep_bwd. */
#define COMA_ABI_VERSION 3

enum { COMA_F32 = 0, COMA_BF16 = 1 };

/* `zeroed` argument of the entry points that merge partial results with atomics (weight gradients, split-K partial
 * tiles, routing gradients): what the caller guarantees to be all zeros on entry -- the callee then skips its own
 * memset.  A training step keeps ONE zeroed arena and hands out slices of it (~60 memset launches per step gone).
 * COMA_ZEROED_OUT: the output the call accumulates into (dwk / dr); COMA_ZEROED_WS: the first *_ws_bytes() bytes of
 * `ws`, which must then be private to this call (the callee leaves them dirty).  0 = the callee zeroes what it needs. */
enum { COMA_ZEROED_OUT = 1, COMA_ZEROED_WS = 2,
       /* coma_conv_fwd_ws only: y += conv(x) instead of y = conv(x) -- a data gradient added to the gradient another
        * consumer of the same activation has already written (no separate accumulation pass); valid where
        * coma_conv_accumulate_ok() answers 1 (the gather / pointwise kernel families)                                */
       COMA_ACCUMULATE = 4,
       /* coma_conv_fwd_ws / coma_conv_fwd_norm_stats: `wk` is already in the fragment order of the wide two-group kernel
        * (coma_weight_prep_batch wrote it so; layout: coma_conv_wk_frag_bytes) -- no re-layout launch, no scratch for it.
        * Only where coma_conv_wk_frag_bytes() answers non-zero: any other problem returns an error and runs nothing. */
       COMA_WK_FRAG = 8 };

/* activation after a normalisation (MONAI ADN "A" slot) */
enum {
  COMA_ACT_NONE = 0,
  COMA_ACT_RELU = 1,        /* attentionunet.ConvBlock / UpConv                         */
  COMA_ACT_PRELU = 2,       /* MONAI Convolution default, one shared slope             */
  COMA_ACT_LEAKY = 3,       /* StackedFusionConvLayers, attn_unet_data_parallel.py:487 */
  COMA_ACT_SIGMOID = 4,     /* AttentionBlock.psi                                       */
  COMA_ACT_PRELU_RELU = 5   /* final_pred_head PReLU followed by final_act ReLU (:654-656) */
};

enum { COMA_NORM_BATCH = 0, COMA_NORM_INSTANCE = 1 };

typedef struct coma_tensor {
  void*   data;
  int32_t dtype;          /* COMA_F32 | COMA_BF16 */
  int32_t B, D, H, W, C;
  int64_t ld;             /* elements between consecutive voxels (>= C)   */
  int64_t sb;             /* elements between consecutive samples          */
} coma_tensor;

/* Gather form of a (transposed) convolution with a cubic kernel.
 *   form 0 ("conv"):   in = out*stride - pad + tap       nn.Conv3d forward,
 *                                                         ConvTranspose3d data-gradient
 *   form 1 ("tconv"):  in = (out + pad - tap)/stride     nn.ConvTranspose3d forward,
 *                       (only when divisible)             Conv3d data-gradient
 * Kernel-layout weights are wk[b][tap][n][c] (c fastest), tap = (kz*k + ky)*k + kx. */
typedef struct coma_conv_desc {
  int32_t ksize;          /* 1 or 3 */
  int32_t stride;         /* 1 or 2 */
  int32_t pad;            /* 0 or 1 */
  int32_t form;           /* 0 conv, 1 tconv */
  int32_t per_sample_w;   /* 1: wk/bias have a leading B dim (CondConv) */
  int32_t algo;           /* 0 auto: MFMA wherever the shape allows (bf16 tensors: v_mfma_f32_32x32x16_bf16; fp32 tensors:
                             v_mfma_f32_32x32x2_f32, exact fp32), otherwise the direct kernels;
                             1 force the direct VALU fp32 kernels; 2 = 0 (kept for callers of ABI 1);
                             4 split: fp32 tensors and fp32 kernel-layout weights, but the thick stride-1 3x3x3 layers at
                             W >= 32 (forward, data gradient, weight gradient) form every product from a two-term bf16
                             split of both operands on v_mfma_f32_32x32x16_bf16 (three MFMAs, fp32 accumulation: error
                             below 2^-14 |a||b| per product); coma_conv_pick_algo / coma_conv_wgrad_algo answer 4 there.
                             Every other problem, and bf16 tensors, resolve exactly as algo 0 does.
                             5 wide split: everything algo 4 resolves to the split kernels, plus the stride-2 3x3x3
                             families with a coarse W >= 32 on fp32 tensors: the transposed convolution (form 1, stride 2:
                             forward of the up-convolutions and data gradient of the stride-2 convolutions, per-sample or
                             shared weights, COMA_ACCUMULATE and the fused statistics kept) and the stride-2 / transposed
                             weight gradients.  coma_conv_pick_algo / coma_conv_wgrad_algo answer 4 there too (the host's
                             weight preparation is the same: fp32 kernel-layout weights); coma_conv_accumulate_ok and
                             coma_conv_fwd_ws_bytes answer what they answer under algo 0.  Every other problem, and bf16
                             tensors, resolve exactly as algo 0 does.
                             6 thin split: everything algo 5 resolves to the split kernels, plus the few-channel stride-1
                             3x3x3 layers at W >= 32 on fp32 tensors (C <= 16 and N <= 16, or C <= 8 and N <= 32: forward,
                             data gradient and weight gradient, per-sample or shared weights, fused statistics kept) on
                             v_mfma_f32_16x16x32_bf16 with the same two-term split.  coma_conv_pick_algo /
                             coma_conv_wgrad_algo answer 4 there too (fp32 kernel-layout weights); coma_conv_accumulate_ok,
                             coma_conv_fwd_ws_bytes and coma_conv_wgrad_ws_bytes answer what they answer under algo 0 (the
                             weight gradient merges into the same replica scratch and honours COMA_ZEROED_WS).  Every other
                             problem, and bf16 tensors, resolve exactly as algo 0 does.
                             7 pointwise: everything algo 6 resolves as algo 6 does, plus the 1x1x1 stride-1 layers with
                             several channels on both sides on fp32 tensors, at >= 4096 voxels per sample, on kernels of
                             their own on v_mfma_f32_32x32x2_f32 (exact fp32, no split): forward / data gradient for
                             8 <= C <= 64, C % 8 == 0, 4 <= N <= 64 (not C = 48 or 64 with N = 32), per-sample or shared weights,
                             COMA_ACCUMULATE and the fused statistics implemented; weight gradient for both channel counts
                             in 4..64 and multiples of 4.  coma_conv_pick_algo / coma_conv_wgrad_algo answer 3 there (fp32
                             kernel-layout weights); for such a forward problem coma_conv_accumulate_ok answers 1 and
                             coma_conv_fwd_ws_bytes 0; the weight gradient merges into the replica scratch
                             coma_conv_wgrad_ws_bytes / _zs_bytes name and honours COMA_ZEROED_WS / COMA_ZEROED_OUT.  Every
                             other problem, and bf16 tensors, resolve exactly as algo 6 does. */
} coma_conv_desc;

int         coma_abi_version(void);
const char* coma_last_error(void);
/* name of the convolution kernel variant the calling thread's most recent coma_conv_* call launched, spelled as
 * rocprofv3 prints it (e.g. "conv_mfma_halo2_k<2, 32, 1, 1>"): lets a host-side timer attribute its per-launch HIP-event
 * durations to the kernel names of a rocprofv3 --kernel-trace of the same command. */
const char* coma_last_kernel(void);

/* ---- CondConv expert mixing + weight re-layout  (replaces CondConv.CondConvolution's
 *      per-sample kernel synthesis, call sites attn_unet_data_parallel.py:126,285-306) ----
 * master: fp32 [E][..] with element (e, n, c, tap) at e*se + n*sn + c*sc + tap
 * r: fp32 [Bw][E] routing weights, or NULL (=> Bw = 1, E = 1, plain re-layout/cast)
 * out: [Bw][taps][N][C] in out_dtype                                              */
int coma_weight_prep(const float* master, const float* r, int32_t E, int32_t Bw,
                     int32_t N, int32_t C, int32_t taps, int64_t se, int64_t sn, int64_t sc,
                     void* out, int32_t out_dtype, void* stream);
/* 27-tap masters, both kernel layouts from one pass over the experts: master [E][A][B][27]
 * -> out_ab [Bw][27][A][B] and/or out_ba [Bw][27][B][A] (either may be NULL), each fp32 or bf16. */
int coma_weight_prep_pair(const float* master, const float* r, int32_t E, int32_t Bw, int32_t A,
                          int32_t B, void* out_ab, int32_t dtype_ab, void* out_ba, int32_t dtype_ba,
                          void* stream);
/* dwk: fp32 [Bw][taps][N][C]  ->  dmaster (=, fp32, master layout), dr [Bw][E] (=, fp32; accumulated with
 * atomics: zeroed here unless `zeroed` has COMA_ZEROED_OUT, i.e. the caller hands over a dr that is already zero) */
int coma_weight_prep_bwd(const float* dwk, const float* master, const float* r, int32_t E,
                         int32_t Bw, int32_t N, int32_t C, int32_t taps, int64_t se,
                         int64_t sn, int64_t sc, float* dmaster, float* dr, int32_t zeroed, void* stream);

/* Every mix of a forward pass in one launch (per layer the mixes are launch- and latency-bound).  `items` is a HOST array,
 * one item per layer, read during the call: the table travels by value in the kernel arguments (chunked into several
 * launches beyond a few dozen items), so the device pointers are the ones valid at call time -- as with the per-layer entry
 * points, also inside a captured graph.  master [E][A][B][taps] fp32, taps 27 or 1; r [Bw][E] or NULL (E = 1);
 * out[0] [Bw][taps][A][B], out[1] [Bw][taps][B][A] (the two kernel layouts: forward and data gradient, which is which
 * follows from `transposed`, informative here), each NULL or of dtype[i]; out[2] is reserved and must be NULL.  With bit i of
 * `frag` set, out[i] takes the fragment order the wide two-group convolution kernel stages from instead (27 taps, bf16,
 * 16-byte aligned, n % 32 == 0 and c % 16 == 0 for its [n][c] = [A][B] or [B][A]; layout: coma_conv_wk_frag_bytes): the
 * same values, permuted.  The arithmetic per output element is that of coma_weight_prep_pair / coma_weight_prep: the
 * results are bit-identical to the per-layer calls.                                                                 */
typedef struct coma_wprep_item {
  const float* master;
  const float* r;
  int32_t E, Bw, A, B, taps, transposed;
  void*   out[3];
  int32_t dtype[3];
  int32_t frag;           /* bit i: out[i] (i < 2) is written in fragment order (see below) */
} coma_wprep_item;
int coma_weight_prep_batch(const coma_wprep_item* items /* host */, int32_t n, void* stream);

/* ---- CondConv routing (call sites attn_unet_data_parallel.py:285-306):
 *      r[b][e] = sigmoid(cov[b] . Wr[e] + br[e]);  bias_mix[b][n] = sum_e r[b][e] * bias_e[e][n]
 * cov fp32 [B][NC], Wr [E][NC], br [E], bias_e [E][N] (or NULL with bias_mix NULL); B*E <= 64.   */
int coma_routing_fwd(const float* cov, int32_t B, int32_t NC, const float* Wr, const float* br,
                     int32_t E, const float* bias_e, int32_t N, float* r, float* bias_mix,
                     void* stream);
/* coma_routing_fwd for every conditional layer of a forward pass in one launch; `items`: HOST array (see
 * coma_weight_prep_batch).  r and bias_mix are bit-identical to the per-layer call's.                           */
typedef struct coma_routing_item {
  const float* cov; const float* Wr; const float* br; const float* bias_e;
  float* r; float* bias_mix;
  int32_t B, NC, E, N;
} coma_routing_item;
int coma_routing_fwd_batch(const coma_routing_item* items /* host */, int32_t n, void* stream);
/* dr_w [B][E] (gradient reaching r through the mixed weights, or NULL), dbias_mix [B][N] (or
 * NULL)  ->  dWr [E][NC], dbr [E], dbias_e [E][N] (or NULL); all written with "=".             */
int coma_routing_bwd(const float* cov, int32_t B, int32_t NC, const float* r, int32_t E,
                     const float* bias_e, int32_t N, const float* dr_w, const float* dbias_mix,
                     float* dWr, float* dbr, float* dbias_e, void* stream);

/* ---- convolution (nn.Conv3d / nn.ConvTranspose3d and their data-gradients) ---- */
/* which kernel family d->algo resolves to for this problem: 1 direct (wants fp32 wk), 2 bf16 MFMA
 * (wants bf16 wk), 3 fp32 MFMA (fp32 tensors, wants fp32 wk), 4 split-bf16 MFMA (algo 4, 5 and 6 only; fp32
 * tensors, wants fp32 wk: the split is done inside the library).  The host prepares the kernel-layout
 * weights accordingly.  coma_conv_wgrad_algo answers the same question for the weight gradient.   */
int coma_conv_pick_algo(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int coma_conv_fwd(const coma_conv_desc* d, const coma_tensor* x, const void* wk,
                  int32_t wk_dtype, const float* bias, const coma_tensor* y, void* stream);
/* coma_conv_fwd with a scratch buffer: layers with fewer output tiles than CUs (8^3 / 16^3 grids, 256-512 channels)
 * split their K loop (taps x channel chunks) over more blocks, merge fp32 partials in `ws` and convert once.
 * ws_bytes >= coma_conv_fwd_ws_bytes(...) enables it; a smaller or NULL ws runs the unsplit kernel.          */
size_t coma_conv_fwd_ws_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int coma_conv_accumulate_ok(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
/* Non-zero (the size of the weights in bytes) when this problem runs on the wide two-group kernel, which stages its weights
 * from FRAGMENT order: bf16 wk[b][n / 32][c / 16][tap][lane = (n & 31) + 32 * ((c >> 3) & 1)][c & 7] instead of
 * wk[b][tap][n][c].  A caller that prepares them in that order passes COMA_WK_FRAG; with plain weights the library
 * re-lays them into the workspace itself (coma_conv_fwd_ws_bytes).  0: the plain layout is wanted.                  */
size_t coma_conv_wk_frag_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* y);
int coma_conv_fwd_ws(const coma_conv_desc* d, const coma_tensor* x, const void* wk, int32_t wk_dtype,
                     const float* bias, const coma_tensor* y, void* ws, size_t ws_bytes, int32_t zeroed, void* stream);
/* conv forward + statistics of the BatchNorm(train)/InstanceNorm that follows it (MONAI Convolution =
 * conv -> ADN): the conv epilogue ADDS its {sum, sumsq} to `sums` where the kernel supports it, so the conv
 * output is not re-read; otherwise coma_norm_stats runs behind the conv.  `sums`: see coma_norm_stats.       */
int coma_conv_fwd_norm_stats(const coma_conv_desc* d, const coma_tensor* x, const void* wk, int32_t wk_dtype,
                             const float* bias, const coma_tensor* y, int32_t mode, double* sums,
                             void* ws, size_t ws_bytes, int32_t zeroed, void* stream);
/* dwk[b][tap][n][c] (=) sum_m dy[m][n] * x[pos(m,tap)][c]; fp32; batch-summed when
 * !per_sample_w.  dbias[b][n] (=) sum_m dy[m][n] (may be NULL).                     */
int coma_conv_wgrad_algo(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
size_t coma_conv_wgrad_ws_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
/* the part of it that must be ZERO for the kernels' atomic merges (0 = none): with COMA_ZEROED_WS and dbias == NULL a
 * caller may pass a private pre-zeroed buffer of just this size as `ws`                                          */
size_t coma_conv_wgrad_zs_bytes(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy);
/* What coma_conv_wgrad does with `ws` follows from ws_bytes alone (tests/test_conv_ws_gpu.py): with dbias != NULL it needs
 * ws_bytes >= coma_norm_ws_bytes(dy) -- less is an error and nothing is written -- writes the bias gradient's partial rows
 * there first and then ignores COMA_ZEROED_WS; the blocks merge into replicas in the first coma_conv_wgrad_zs_bytes() bytes
 * only when that is non-zero and ws_bytes is at least as large, otherwise (a smaller or NULL ws) into dwk itself.
 * COMA_ZEROED_WS speaks about the replica bytes, COMA_ZEROED_OUT about dwk: each spares the memset of the branch that
 * merges there.  Nothing beyond the bytes named here is touched.                                                      */
int coma_conv_wgrad(const coma_conv_desc* d, const coma_tensor* x, const coma_tensor* dy,
                    float* dwk, float* dbias, void* ws, size_t ws_bytes, int32_t zeroed, void* stream);

/* ---- BatchNorm3d (train) / InstanceNorm3d + activation  (MONAI ADN "N","A") ---- */
size_t coma_norm_ws_bytes(const coma_tensor* x);   /* scratch of coma_spatial_mean / the conv bias gradient */
/* Training statistics are fp64 records sums[COMA_STAT_REPLICAS][G][C][2] = {sum x, sum x^2}, G = 1 (batch) or B
 * (instance), replica stride COMA_NORM_RECORD_DOUBLES(G, C, 2), that the CALLER hands over ZEROED and the producers add
 * to with fp64 atomics (a block picks a replica by its index: short queues at the memory-side atomic units); every
 * consumer below sums the replicas and derives mean = sum / R and rstd = 1 / sqrt(sumsq / R - mean^2 + eps) itself
 * (R = voxels per group): there is no finalise launch and no (mean, rstd) tensor on the training path.             */
#define COMA_STAT_REPLICAS 8
/* doubles in ONE replica of a record with k values per (group, channel), rounded up to a 64-byte line */
#define COMA_NORM_RECORD_DOUBLES(G, C, k) ((((int64_t)(G) * (C) * (k)) + 7) & ~(int64_t)7)
int coma_norm_stats(const coma_tensor* x, int32_t mode, double* sums, void* stream);
/* y = act((x - mean)*rstd*gamma + beta); gamma/beta may be NULL; slope: device fp32[1].  Statistics: `sums`
 * (training) or, when sums == NULL, fp32 mean/rstd [G][C] (eval-mode BatchNorm: running statistics).
 * running_mean/var (BatchNorm training, may be NULL): r = (1-momentum)*r + momentum*stat, unbiased variance.  */
int coma_norm_act_fwd(const coma_tensor* x, int32_t mode, const double* sums, float eps, const float* mean,
                      const float* rstd, const float* gamma, const float* beta, int32_t act, const float* slope,
                      float* running_mean, float* running_var, float momentum, const coma_tensor* y, void* stream);
/* dx (=); dgamma/dbeta [C] (=); dslope [1] (=); any of the three may be NULL.  bsums: fp64
 * [COMA_STAT_REPLICAS][G][C][3] (replica stride COMA_NORM_RECORD_DOUBLES(G, C, 3)), ZEROED by the caller: the
 * backward's own partial sums {sum dz, sum dz*xhat, sum dy*dact/dslope}.                                         */
int coma_norm_act_bwd(const coma_tensor* x, const coma_tensor* dy, int32_t mode, const double* sums, float eps,
                      const float* gamma, const float* beta, int32_t act, const float* slope,
                      const coma_tensor* dx, float* dgamma, float* dbeta, float* dslope, double* bsums, void* stream);
/* Backward through a FROZEN BatchNorm3d (+ activation): a train-mode model that normalises with the running statistics.
 * With m = running_mean and r = rsqrt(running_var + eps) handed in as the fp32 tables mean / rstd [C] (the form
 * coma_norm_act_fwd takes when sums == NULL; that call is the forward):
 *     xhat = (x - m) r        z = gamma xhat + beta        y = act(z)
 *     dz = dy act'(z)         dx (=) dz gamma r
 *     dgamma (=) sum dz xhat  dbeta (=) sum dz             dslope (=) sum dy dact/dslope
 * No statistics of dy are needed: one streaming pass over (x, dy) (16 bytes per lane on bf16 without, 8 with the
 * sums), plus one one-block finalise launch when any of dgamma / dbeta / dslope is wanted (each may be NULL).  bsums: ZEROED fp64 record [COMA_STAT_REPLICAS][3][C], replica
 * stride COMA_NORM_RECORD_DOUBLES(1, C, 3); may be NULL when no parameter gradient is wanted (the pass then touches no
 * record).  gamma / beta may both be NULL.  The running statistics are not written.                                  */
int coma_norm_act_bwd_frozen(const coma_tensor* x, const coma_tensor* dy, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, int32_t act, const float* slope,
                             const coma_tensor* dx, float* dgamma, float* dbeta, float* dslope, double* bsums,
                             void* stream);

/* ---- attention gate pieces (MONAI AttentionBlock, attn_unet_data_parallel.py:139-150) ---- */
/* out = relu(a + b);  da (=) db (=) dout * [out > 0] */
int coma_add_relu_fwd(const coma_tensor* a, const coma_tensor* b, const coma_tensor* out, void* stream);
int coma_add_relu_bwd(const coma_tensor* out, const coma_tensor* dout, const coma_tensor* da, void* stream);
/* out[v][c] = x[v][c] * psi[v]   (psi has C == 1) */
int coma_gate_mul_fwd(const coma_tensor* x, const coma_tensor* psi, const coma_tensor* out, void* stream);
int coma_gate_mul_bwd(const coma_tensor* x, const coma_tensor* psi, const coma_tensor* dout,
                      const coma_tensor* dx, int32_t accumulate_dx, const coma_tensor* dpsi, void* stream);

/* ---- the attention gate behind its W_g / W_x convolutions, fused (csrc/gate.hip; attn_unet_data_parallel.py:139-150):
 *      s = relu(BN_g(g1raw) + BN_x(x1raw));  psi_raw = w_psi . s + b_psi;  psi = sigmoid(BN_psi(psi_raw));  att = x * psi
 * All three BatchNorms in training mode on statistics records (coma_norm_stats; G = 1): sums_g / sums_x come out of the
 * W_g / W_x convolutions (coma_conv_fwd_norm_stats), sums_psi is a ZEROED record this call fills.  s and psi_raw are
 * written for the backward.  running_* may be NULL.                                                                    */
int coma_gate_mid_fwd(const coma_tensor* g1raw, const coma_tensor* x1raw, const double* sums_g, float eps_g,
                      const float* gamma_g, const float* beta_g, const double* sums_x, float eps_x,
                      const float* gamma_x, const float* beta_x, const float* w_psi, const float* b_psi,
                      float* rmean_g, float* rvar_g, float* rmean_x, float* rvar_x, float momentum,
                      const coma_tensor* s_out, const coma_tensor* psi_raw, double* sums_psi, void* stream);
/* psi = sigmoid(BN_psi(psi_raw)) (written: [B][V][1]) and att = x * psi (e.g. a channel slice of the concat buffer) */
int coma_gate_apply_fwd(const coma_tensor* x, const coma_tensor* psi_raw, const double* sums_psi, float eps,
                        const float* gamma_psi, const float* beta_psi, float* rmean_psi, float* rvar_psi,
                        float momentum, const coma_tensor* psi, const coma_tensor* att, void* stream);
/* dx (= or +=) d(att) * psi;  dz[v] = (sum_c d(att) x) psi (1 - psi);  bsums_psi: ZEROED record, k = 3            */
int coma_gate_apply_bwd(const coma_tensor* x, const coma_tensor* psi, const coma_tensor* psi_raw,
                        const coma_tensor* dout, const double* sums_psi, float eps, const float* gamma_psi,
                        const float* beta_psi, const coma_tensor* dx, int32_t accumulate_dx,
                        const coma_tensor* dz, double* bsums_psi, void* stream);
/* dz -> d(psi_raw) -> ds -> relu mask -> both BatchNorm backwards: dg1raw, dx1raw (=) and every parameter gradient (=;
 * any may be NULL).  rec: ZEROED scratch record [COMA_STAT_REPLICAS][COMA_NORM_RECORD_DOUBLES(1, F, 4)].            */
int coma_gate_mid_bwd(const coma_tensor* dz, const coma_tensor* psi_raw, const coma_tensor* s_in,
                      const coma_tensor* g1raw, const coma_tensor* x1raw, const double* sums_psi, float eps_psi,
                      const float* gamma_psi, const double* bsums_psi, const double* sums_g, float eps_g,
                      const float* gamma_g, const double* sums_x, float eps_x, const float* gamma_x,
                      const float* w_psi, double* rec, const coma_tensor* dg1raw, const coma_tensor* dx1raw,
                      float* dgamma_g, float* dbeta_g, float* dgamma_x, float* dbeta_x, float* dw_psi,
                      float* dgamma_psi, float* dbeta_psi, void* stream);

/* ---- the attention gate with every BatchNorm in EVAL mode: each is a known affine map, so the gate is one pass
 *      att = x * psi,   psi = sigmoid(a_p * (w_psi . relu(scale_g * g1raw + scale_x * x1raw + shift)) + b_p)
 * The caller folds the running statistics ONCE into fp32 device tables: scale_g[F] = gamma_g * rstd_g, scale_x[F],
 * shift[F] (both betas, both means, both convolution biases when g1raw / x1raw are bias-free products), w_psi[F] and
 * psi_ab[2] = {a_p, b_p} = {gamma_p rstd_p, a_p b_psi + beta_p - a_p mean_p}.  psi ([B][V][1]) may be NULL; att may be a
 * channel slice of a wider buffer.  Nothing is saved: there is no backward.                                          */
/* behind the W_g / W_x convolutions: g1raw, x1raw have F channels; x, att have C.  Any dtype, F and C the training gate
 * kernels take (max(C, F) / vector width a power of two <= 64, F <= 512).                                          */
int coma_gate_eval_fwd(const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw, const float* scale_g,
                       const float* scale_x, const float* shift, const float* w_psi, const float* psi_ab,
                       const coma_tensor* psi, const coma_tensor* att, void* stream);
/* ---- the attention gate with every BatchNorm FROZEN (a train-mode model on running statistics), behind the W_g / W_x
 * convolutions, which run plain (with their biases, no statistics epilogue).  Per BatchNorm a table of four device
 * pointers bn[4] = {mean, rstd, gamma, beta} (fp32; F entries for g and x, one for psi) with m = running_mean and
 * r = rsqrt(running_var + eps) made once by the caller -- nothing is re-folded on the device between steps:
 *     t = gamma_g ghat + beta_g + gamma_x x1hat + beta_x     s = relu(t)     pr = w_psi . s + b_psi
 *     zhat = (pr - m_p) r_p     psi = sigmoid(gamma_p zhat + beta_p)         att = x psi
 * backward:
 *     dx (= or +=) datt psi     dpsi = sum_c datt x     dzp = dpsi psi (1 - psi)
 *     dgamma_p = sum dzp zhat   dbeta_p = sum dzp       dpr = dzp gamma_p r_p     db_psi = sum dpr
 *     dw_f = sum dpr s_f        d_f = dpr w_f [t_f > 0]
 *     dg1raw_f = d_f gamma_g,f r_g,f        dx1raw_f = d_f gamma_x,f r_x,f
 *     dgamma_g,f = sum d_f ghat_f           dbeta_g,f = sum d_f      (and the same for x)
 * Forward: one launch; writes psi ([B][V][1], read again by the backward) and att (may be a channel slice).  s is not
 * saved: the backward reads g1raw / x1raw anyway (ghat, x1hat) and recomputes t, s and pr in registers.
 * Backward: one pass over the voxels + a one-block finalise launch.  dx may accumulate (accumulate_dx) into a shared
 * gradient buffer; datt may be a channel slice.  rec: ZEROED fp64 record
 * [COMA_STAT_REPLICAS][COMA_NORM_RECORD_DOUBLES(1, F + 1, 4)].  Parameter gradients (=); any may be NULL; b_psi may be NULL.
 * Envelope (coma_gate_frozen_ok): one dtype, C and F multiples of the vector width (4, or 1 for unaligned tensors) and
 * max(C, F) / width a power of two <= 64, F <= 512 -- what the training gate kernels take.                          */
int coma_gate_frozen_ok(const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw, const coma_tensor* att);
int coma_gate_frozen_fwd(const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw,
                         const float* const* bn_g, const float* const* bn_x, const float* const* bn_psi,
                         const float* w_psi, const float* b_psi, const coma_tensor* psi, const coma_tensor* att,
                         void* stream);
int coma_gate_frozen_bwd(const coma_tensor* x, const coma_tensor* g1raw, const coma_tensor* x1raw,
                         const coma_tensor* psi, const coma_tensor* datt, const float* const* bn_g,
                         const float* const* bn_x, const float* const* bn_psi, const float* w_psi, const float* b_psi,
                         const coma_tensor* dx, int32_t accumulate_dx, const coma_tensor* dg1raw,
                         const coma_tensor* dx1raw, double* rec, float* dgamma_g, float* dbeta_g, float* dgamma_x,
                         float* dbeta_x, float* dw_psi, float* db_psi, float* dgamma_psi, float* dbeta_psi,
                         void* stream);
/* The whole gate INCLUDING both 1x1x1 convolutions in one launch (bf16 MFMA, no intermediate ever in memory):
 * wg_folded / wx_folded are bf16 [32][C] = diag(scale_g) W_g, diag(scale_x) W_x with ZERO rows beyond F, and shift / w_psi
 * here have 32 entries, zero beyond F (shift carries the biases): the padded rows contribute exactly nothing.
 * coma_gate_eval_mfma_ok answers 1 where this form runs: bf16 g and x on one grid with C % 16 == 0, 16 <= C <= 64,
 * 1 <= F <= 32, 16-byte aligned data and pitches; 0 otherwise (then use coma_gate_eval_fwd behind the convolutions). */
int coma_gate_eval_mfma_ok(const coma_tensor* g, const coma_tensor* x, int32_t F);
int coma_gate_eval_mfma(const coma_tensor* g, const coma_tensor* x, const void* wg_folded, const void* wx_folded,
                        const float* shift, const float* w_psi, const float* psi_ab, const coma_tensor* psi,
                        const coma_tensor* att, void* stream);

/* ---- generic strided element-wise helpers ---- */
/* dst = a (+ b).  b may be NULL.  a/b with B == 1 broadcast over dst's batch. */
int coma_add(const coma_tensor* a, const coma_tensor* b, const coma_tensor* dst, void* stream);
/* dst = dtype_of_dst(src): same grid and channels, any pitches, fp32 <-> bf16 (input staging into padded buffers) */
int coma_cast_copy(const coma_tensor* src, const coma_tensor* dst, void* stream);
/* base[off, off + len) = 0 for each of the n (off, len) int64 rows (elements) of the device table `ranges`; max_len = the
 * longest row (sizes the grid).  One launch for the sparse zero_grad of a flat gradient buffer.                         */
int coma_zero_ranges(float* base, const int64_t* ranges, int32_t n, int64_t max_len, void* stream);
/* dst[0] (=) sum_b src[b]  (gradient of a batch-broadcast parameter) */
int coma_batch_sum(const coma_tensor* src, const coma_tensor* dst, void* stream);
/* per-sample, per-channel mean over voxels -> fp32 [B][C] (AdaptiveAvgPool3d(1)) */
int coma_spatial_mean(const coma_tensor* x, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- ROI prior painting + prompt select (attn_unet_data_parallel.py:630-651) ----
 * roi: fp32 labels (C==1); x: the MRI (C==1); prior: fp32 [B][n_roi][2] (loc,std);
 * roi_ids: int32 [n_roi]; abeta: fp32 [B]; prompts: fp32, shape (1,D,H,W,1).
 * out3: (B,D,H,W,3) = cat(prompt_sel, saliency, suvr)  with the x < 1e-4 zeroing.   */
int coma_roi_paint_fwd(const coma_tensor* roi, const coma_tensor* x, const float* prior,
                       const int32_t* roi_ids, int32_t n_roi, const float* abeta,
                       const float* pos_prompt, const float* neg_prompt,
                       const coma_tensor* out3, void* stream);
/* dpos/dneg (+=, fp32 volumes): channel 0 of dout3 routed by abeta */
int coma_roi_paint_bwd(const coma_tensor* dout3, const float* abeta, float* dpos, float* dneg, void* stream);

/* ---- losses (criterions.py:181-211 RoiMSE voxel_wise=False; L1 = the MAE metric,
 *      attn_unet_data_parallel.py:1215) ----
 * loss[b] = mean_vox(mask_b) * mean_vox((pred_b - gt_b)^2), mask = weight LUT of roi */
size_t coma_loss_ws_bytes(const coma_tensor* pred);
int coma_roi_mse_fwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi,
                     const int32_t* roi_ids, const float* roi_w, int32_t n_roi,
                     float* loss, float* mask_mean, void* ws, size_t ws_bytes, void* stream);
/* dpred (=) gout[b] * mask_mean[b] * 2 (pred - gt) / V */
int coma_roi_mse_bwd(const coma_tensor* pred, const coma_tensor* gt, const float* gout,
                     const float* mask_mean, const coma_tensor* dpred, void* stream);
int coma_l1_fwd(const coma_tensor* pred, const coma_tensor* gt, float* loss, void* ws, size_t ws_bytes, void* stream);
int coma_l1_bwd(const coma_tensor* pred, const coma_tensor* gt, const float* gout,
                const coma_tensor* dpred, void* stream);

/* ---- ROI-weighted voxel losses (criterions.py:28-122 RoiRRMSE / RoiRSE and the plain weighted MSE; csrc/roi_loss.hip) ----
 * w_v = roi_w[slot of the voxel's label], bg_weight for a label outside roi_ids; d = pred - gt; N = sum_v w d^2
 *   kind 0 WMSE   D = sum w                                               loss = N / D        coef = 2 / D
 *   kind 1 RSE    D = sum g^2 - 2 m sum g + V m^2,  m = sum(w g) / V      loss = N / D        coef = 2 / D
 *   kind 2 RRMSE  D = sum w g^2                                           loss = sqrt(N / D)  coef = 1 / (D loss)
 * (RSE's D = sum (g - m)^2 is the reference's unweighted denominator about its weighted "mean", :109-112.)
 * loss, coef: B floats.  No clamps: D = 0, or N = 0 under RRMSE, give inf / nan by IEEE arithmetic.
 * pred / gt / dpred: one dtype (fp32 or bf16), C = 1; gt and roi (fp32) of voxel pitch 1.  No atomics, no host read. */
size_t coma_roi_wloss_ws_bytes(const coma_tensor* pred);
int coma_roi_wloss_fwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi,
                       const int32_t* roi_ids, const float* roi_w, int32_t n_roi, float bg_weight, int32_t kind,
                       float* loss, float* coef, void* ws, size_t ws_bytes, void* stream);
/* dpred (=) gout[b] * coef[b] * w_v * (pred - gt); the target gets no gradient */
int coma_roi_wloss_bwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi,
                       const int32_t* roi_ids, const float* roi_w, int32_t n_roi, float bg_weight,
                       const float* gout, const float* coef, const coma_tensor* dpred, void* stream);

/* ---- ROI-mean (per-region SUVR) loss (csrc/roi_mean.hip): a loss on the regional means.  Per sample and table slot r,
 * n_r = #{v: label_v == roi_ids[r]} (roi_lut_slot's rules: exact integer labels, the first of a duplicated id wins),
 * d_r = mean_r(pred) - mean_r(gt);
 *   loss = sum_{r: n_r > 0} w_r phi(d_r) / sum_{r: n_r > 0} w_r,   phi: kind 0 d^2 | kind 1 |d| | kind 2 huber(d; delta)
 *   coef[b][r] = w_r phi'(d_r) / (n_r sum w)    (0 for an absent region; phi'(0) = 0 for kind 1)
 * No present region, or sum w = 0: loss 0 and coef 0.  loss: B floats; coef: B x n_roi floats.  pred / gt: one dtype (fp32
 * or bf16), C = 1; gt and roi (fp32) of voxel pitch 1.  A label-segmented reduction without atomics: bitwise repeatable. */
size_t coma_roi_mean_ws_bytes(const coma_tensor* pred);
int coma_roi_mean_fwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi,
                      const int32_t* roi_ids, const float* roi_w, int32_t n_roi, int32_t kind, float delta,
                      float* loss, float* coef, void* ws, size_t ws_bytes, void* stream);
/* dpred (=) gout[b] * coef[b][slot of the voxel's label], 0 for a voxel in no region; dpred fp32 or bf16, any voxel pitch */
int coma_roi_mean_bwd(const coma_tensor* roi, const int32_t* roi_ids, int32_t n_roi, const float* gout, const float* coef,
                      const coma_tensor* dpred, void* stream);
/* stats: fp64 [B][n_roi][3] = {n_r, sum_r pred, sum_r gt}, by the same reduction (ws: coma_roi_mean_ws_bytes) */
int coma_roi_region_stats(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi,
                          const int32_t* roi_ids, int32_t n_roi, double* stats, void* ws, size_t ws_bytes, void* stream);

/* ---- gradient-difference loss (csrc/grad_diff.hip): an edge term on forward differences.  Per sample, axis a in {z, y, x}
 * and every voxel v whose neighbour v + e_a is inside the volume:
 *   gp = pred[v + e_a] - pred[v], gg = gt[v + e_a] - gt[v], t = |gp| - |gg| (mode 0, "abs") | gp - gg (mode 1, "signed")
 *   phi(t) = |t| (alpha 1) | t^2 (alpha 2);  m_a(v) = 1 (roi NULL) | [roi[v] != 0 and roi[v + e_a] != 0]
 *   loss = sum_a axis_w[a] S_a / N_a,  S_a = sum_v m_a phi(t),  N_a = sum_v m_a  (an axis with N_a = 0 contributes 0)
 *   coef[b][a] = axis_w[a] / N_a  (0 if N_a = 0);  sign(0) = 0 in every derivative
 * axis_w: three HOST floats (z, y, x), finite and >= 0, read at the call.  loss: B floats; coef: B x 3 floats (device).
 * pred: fp32 or bf16, C = 1, any voxel pitch; gt: pred's dtype, voxel pitch 1; roi: fp32, voxel pitch 1, or NULL.
 * One pass over 8 x 8 x 32 tiles staged in LDS, fp64 arithmetic on the staged values, one fp64 record per tile in ws, a
 * fixed-order finalise: no atomics, no host read, bitwise repeatable, the same bits from 16-byte and element-wise staging. */
size_t coma_grad_diff_ws_bytes(const coma_tensor* pred);
int coma_grad_diff_fwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, int32_t mode, int32_t alpha,
                       const float* axis_w, float* loss, float* coef, void* ws, size_t ws_bytes, void* stream);
/* dpred[v] (=) gout[b] * sum_a coef[b][a] * (psi_a(v - e_a) - psi_a(v)), psi_a(v) = m_a(v) phi'(t) chi, chi = sign(gp) (abs)
 * | 1 (signed), 0 where the pair does not exist.  dpred: pred's dtype, any voxel pitch; every voxel is assigned once. */
int coma_grad_diff_bwd(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi, int32_t mode, int32_t alpha,
                       const float* gout, const float* coef, const coma_tensor* dpred, void* stream);

/* ---- evaluation statistics: one pass over (pred, gt, roi) giving, per sample and per
 *      bin (n_roi ROIs + the whole volume), the sums behind calc_roi_metrics (attn_unet_data_parallel.py:1361-1397),
 *      the global MAE/MAPE/RSE/RRMSE of contrastive_test (:1214-1231) and RoiCorrMetric (:49-60).
 *      stats: fp64 [B][n_roi+1][8] = {count, sum|d|, sum d^2, sum g, sum g^2, sum p, sum|d/g| (non-NaN), #non-NaN} ---- */
int coma_eval_stats(const coma_tensor* pred, const coma_tensor* gt, const coma_tensor* roi,
                    const int32_t* roi_ids, int32_t n_roi, double* stats, void* stream);

/* ---- AdamW over a flat fp32 buffer (torch.optim.AdamW defaults,
 *      attn_unet_data_parallel.py:736): p,g,m,v length n; step counted from 1.  When step_dev is
 *      non-NULL the step count is read from that device int32 instead (hipGraph replay). ---- */
int coma_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
               float beta2, float eps, float weight_decay, int32_t step, const int32_t* step_dev,
               void* stream);

/* ---- gradient accumulation and global-norm clipping on the same flat buffers (FusedAdamW(grad_acc_batch,
 *      max_grad_norm)).  Both calls are deterministic (no atomics; every sum runs in one fixed order).
 * coma_grad_accum: one micro-batch's gradient g (length n) into the window's accumulator.  count_dev (device int32) =
 *   micro-batches already in the window, read ON THE DEVICE: 0 -> acc = g (acc is not read), else acc += g (one fp32
 *   rounding), so that one captured graph serves every micro-batch of a window.  acc == NULL: norm-only form, g is read
 *   and nothing but `partials` is written.  partials (device fp64, room for 1024; NULL: no norm wanted): block b stores
 *   (plain store) its fp64 sum of x^2 over the values it handled (the new acc, or g in the norm-only form) to
 *   partials[b].  The grid is at most 1024 blocks of 256 threads; *blocks_out (host int32, may be NULL) receives the
 *   number launched = the number of live partials -- the slots behind them are neither written here nor to be read.
 *   n == 0: no launch, *blocks_out = 0.  16-byte accesses where acc and g are 16-byte aligned, scalar otherwise. ---- */
int coma_grad_accum(float* acc, const float* g, int64_t n, const int32_t* count_dev, double* partials,
                    int32_t* blocks_out, void* stream);
/* coma_adamw_ex: coma_adamw on the gradient g * s, s = c / count rounded once to fp32:
 *   count = *count_dev (device int32, micro-batches in the window; NULL: 1);
 *   norm  = sqrt(sum partials[0 .. n_partials) + *extra_sumsq) / count   (fp64; extra_sumsq: device fp64, may be NULL --
 *           the squared norm of gradients that live outside this buffer);
 *   c     = min(1, max_norm / (norm + 1e-6)), or 1 when partials == NULL (no clipping)
 *   -- torch.nn.utils.clip_grad_norm_(.., max_norm, norm_type=2) on the MEAN gradient of the window, a non-finite norm
 *   included (error_if_nonfinite=False: the coefficient becomes NaN).  Every block sums the partials in the same order, so
 *   all blocks use the bitwise-same s.  norm_out (device fp32, may be NULL): block 0 stores `norm`, the unclipped norm of
 *   the mean gradient.  Slots of `partials` at or beyond n_partials (<= 1024) are not read.  With count == 1 and c == 1
 *   the results are bitwise those of coma_adamw: the kernels of coma_adamw, coma_adamw_ex and coma_adamw_ema are
 *   instantiations of one update body (adamw_body in csrc/elementwise.hip), which differ in the factor s and in the
 *   average alone. ---- */
int coma_adamw_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int32_t step, const int32_t* step_dev,
                  const int32_t* count_dev, const double* partials, int32_t n_partials,
                  const double* extra_sumsq, float max_norm, float* norm_out, void* stream);

/* ---- exponential moving average of the weights inside the same sweep (FusedAdamW(ema_decay, ema_warmup)).
 * coma_adamw_ema: coma_adamw_ex with the same arguments (the same update body: p, m, v come out bitwise the same; with
 *   count_dev == NULL and partials == NULL bitwise coma_adamw's), then, per element, on the parameter p' just computed
 *       e' = fmaf(1 - d_t, p' - e, e)                      (torch's get_ema_multi_avg_fn: lerp(e, p', 1 - d))
 *   stored to ema (length n, fp32).  d_t is formed in fp32 on the device:
 *       ema_warmup == 0:  d_t = ema_decay
 *       otherwise:        d_t = min(ema_decay, (1 + t) / (10 + t)),  t = *step_dev when step_dev is non-NULL, else step
 *   (the update count, from 1: a replayed graph moves through the warm-up).  ema_decay must lie strictly inside (0, 1).
 *   The caller starts the average at the parameters' values (e_0 = p_0).  fp32 limit: an increment (1 - d)|p' - e| below
 *   half an ulp of e is lost.  16-byte accesses where all five buffers are 16-byte aligned, scalar otherwise.
 *   n == 0: no launch. ---- */
int coma_adamw_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int32_t step, const int32_t* step_dev,
                   const int32_t* count_dev, const double* partials, int32_t n_partials,
                   const double* extra_sumsq, float max_norm, float* norm_out, float* ema, float ema_decay,
                   int32_t ema_warmup, void* stream);
/* ---- learning-rate schedule and per-segment options inside the same sweep (FusedAdamW(lr_schedule, param_options)).
 * coma_adamw_sched: coma_adamw_ema with the same arguments (ema == NULL: coma_adamw_ex, ema_decay / ema_warmup unused),
 *   except that the learning rate of this update is formed on the device, once per block, in fp32:
 *       t = *sched_step_dev, else sched_step, else (both zero) the update count *step_dev / step;   s = t - 1
 *       warm  = warmup_start + (1 - warmup_start) * min(s, warmup_steps) / warmup_steps      (1 when warmup_steps == 0)
 *       u     = s - warmup_steps clamped to [0, total_steps]  (SCHED step: from below only)
 *       decay = 1                                                                 sched_kind 0, constant
 *               min_ratio + (1 - min_ratio) (1 + cos(pi u / total_steps)) / 2     sched_kind 1, cosine
 *               1 - (1 - min_ratio) u / total_steps                               sched_kind 2, linear
 *               gamma ^ floor(u / step_size)                                      sched_kind 3, step
 *       lr_t  = *lr_dev * warm * decay
 *   (torch's LinearLR(start_factor, total_iters) followed by CosineAnnealingLR / StepLR with scheduler.step() behind
 *   optimizer.step(); cosf and powf, no fast intrinsics).  A replayed graph walks through the schedule, and a new value in
 *   *lr_dev (a plateau scheduler) takes effect without a new capture.  sched_step / sched_step_dev are separate from step /
 *   step_dev so that a tensor with its own bias-correction count still follows the global schedule.  lr_out (device fp32,
 *   may be NULL): block 0 stores lr_t, before any scale.
 *   Element i has flat coordinate elem_base + i and belongs to the first segment k with seg_end[k] > coordinate (the last
 *   one beyond the table's end); it is updated with lr_t * seg_lr_scale[k] and the decay seg_wd[k].  seg_end (device int64)
 *   must be strictly ascending: the caller's contract, not checked on the device.  n_segs == 0: lr_t * lr_scale and
 *   weight_decay for every element.  n_segs <= 2048; the table is staged in LDS (16 bytes per segment and block).  Segments
 *   shorter than a 16-byte chunk and boundaries inside one are allowed.  With lr_scale == 1 and n_segs == 0 the results are
 *   bitwise those of coma_adamw / coma_adamw_ex / coma_adamw_ema called with lr = *lr_out, path by path: the 16-byte loop
 *   (all buffers 16-byte aligned, elements below 4 * (n / 4)) is bitwise their 16-byte loop, the scalar loop (its tail, and
 *   every element of a call with an unaligned buffer) bitwise their scalar loop.  As in those kernels the two loops do NOT
 *   give the same bits as each other: the 16-byte loop fuses each moment update into one fma, the scalar loop rounds its
 *   product and its sum separately.  So a slice passed with elem_base is bitwise the same elements of a whole launch only
 *   where every element stays on its loop -- the slice starts and, unless it reaches the end, ends at a multiple of four
 *   elements of 16-byte aligned buffers -- and differs in the last bits of m, v (and then p) otherwise.
 *   Checked before any launch: lr_dev non-NULL, sched_kind in [0, 4),
 *   total_steps >= 1 for cosine and linear, step_size >= 1, 0 < gamma <= 1, 0 <= min_ratio <= 1, 0 < warmup_start <= 1,
 *   warmup_steps >= 0, n_segs in [0, 2048].  n == 0: no launch, nothing written. ---- */
int coma_adamw_sched(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1,
                     float beta2, float eps, float weight_decay, int32_t step, const int32_t* step_dev,
                     const int32_t* count_dev, const double* partials, int32_t n_partials,
                     const double* extra_sumsq, float max_norm, float* norm_out, float* ema, float ema_decay,
                     int32_t ema_warmup, int32_t sched_kind, int32_t warmup_steps, float warmup_start,
                     int32_t total_steps, float min_ratio, int32_t step_size, float gamma, int32_t sched_step,
                     const int32_t* sched_step_dev, float lr_scale, const int64_t* seg_end,
                     const float* seg_lr_scale, const float* seg_wd, int32_t n_segs, int64_t elem_base,
                     float* lr_out, void* stream);
/* coma_swap_f32: exchange the CONTENTS of two disjoint device buffers of n floats (a[i] <-> b[i]); the addresses that
 *   parameter views and captured graphs hold stay valid.  a == b or overlapping ranges: error status, nothing launched.
 *   Same 16-byte / scalar paths as coma_adamw_ema.  n == 0: no launch. */
int coma_swap_f32(float* a, float* b, int64_t n, void* stream);

/* ---- 3-D SSIM (MONAI SSIMMetric(spatial_dims=3), attn_unet_data_parallel.py:1176,1234) ----
 * x, y: single-channel volumes; window: `win` (<= 11) separable weights (host pointer); c1 = (k1 R)^2, c2 = (k2 R)^2.
 * Writes one fp64 partial sum of the SSIM map per 8^3 output tile: partial[b * ntiles + t]; the per-sample SSIM is
 * sum_t partial / ((D-win+1)(H-win+1)(W-win+1)).                                                              */
size_t coma_ssim_ws_bytes(const coma_tensor* x, int32_t win);
int coma_ssim_partial(const coma_tensor* x, const coma_tensor* y, const float* window, int32_t win, float c1,
                      float c2, double* partial, size_t partial_bytes, int32_t* ntiles_out, void* stream);

/* ---- SSIM as a training loss (DESIGN.md section 4 "SSIM loss"): gradient of the per-sample mean SSIM w.r.t. x ----
 * coma_ssim_fwd_coef: coma_ssim_partial (same arguments, same partial sums) that also stores, per valid output voxel,
 *   the three fp32 coefficient maps a0 = dS/d mu_x, a2 = dS/d E[x^2], a4 = dS/d E[xy], planar [3][B][Do][Ho][Wo]
 *   (Do = D-win+1, ...), in `coef` (device, coma_ssim_coef_bytes(x, win) bytes; 0 = window does not fit).
 * coma_ssim_bwd: dx (=) gout[b] / (Do Ho Wo) * (W^T a0 + 2 x W^T a2 + y W^T a4), W^T the adjoint of the "valid"
 *   window ((W^T a)[v] = sum_k window[k] a[v - k] per axis).  gout: device fp32 [B], the upstream gradient of each
 *   sample's mean SSIM (read on the device).  dx: grid and dtype of x; y gets no gradient.  x, y, dx may be strided
 *   (ld, sb).  One block per 8^3 tile of dx, every voxel written by one thread: no atomics, bitwise repeatable.
 * Both return an error status with nothing launched unless: x, y (and dx) are single-channel volumes of equal grid and
 *   dtype, 1 <= win <= 11, the window fits the volume, and the partial / coef buffers are large enough.          */
size_t coma_ssim_coef_bytes(const coma_tensor* x, int32_t win);
int coma_ssim_fwd_coef(const coma_tensor* x, const coma_tensor* y, const float* window, int32_t win, float c1,
                       float c2, double* partial, size_t partial_bytes, int32_t* ntiles_out, float* coef,
                       size_t coef_bytes, void* stream);
int coma_ssim_bwd(const coma_tensor* x, const coma_tensor* y, const float* coef, const float* window, int32_t win,
                  const float* gout, const coma_tensor* dx, void* stream);

/* ---- input pipeline (replaces VolumeDataset_ADNI_A4_combined.py:95-133,:62) ----
 * Nearest-neighbour resample of a raw fp32 (z, y, x) volume with voxel spacing sp_* (mm) onto a Do x Ho x Wo grid with
 * spacing nsp_* (same origin and axes, identity transform, ITK rounding), optional nan_to_num, optional zeroing where
 * the dst-sized volume `zero_where` is 0 (the reference's `mri[roi == 0] = 0`).  Out-of-volume samples take
 * default_value (the reference passes the image's SimpleITK pixel-type id there).                              */
int coma_resample_nearest(const float* src, int32_t Dz, int32_t Hy, int32_t Wx, double sp_z, double sp_y,
                          double sp_x, float* dst, int32_t Do, int32_t Ho, int32_t Wo, double nsp_z,
                          double nsp_y, double nsp_x, float default_value, int32_t nan_to_num,
                          const float* zero_where, void* stream);

/* ---- on-device 3-D augmentation (build-side; DESIGN.md section 4 "Augmentation") ----
 * One launch warps the MRI, tau and ROI-label volumes ((B, D, H, W) fp32, contiguous) of a batch by the same per-sample
 * transform.  params[b] (device, COMA_AUG_NPARAM floats): a 3 x 4 row-major matrix A in (z, y, x) order mapping an
 * output voxel index to a source voxel index, then mri_scale, mri_shift, mri_gamma, noise_sigma.  disp: optional
 * (B, 3, gz, gy, gx) control grid of (z, y, x) displacements in voxels, 2..8 points per axis, interpolated trilinearly
 * with the align-corners convention (NULL: none; gz, gy, gx are then ignored).  For output voxel o of sample b:
 *   s = A_b (z, y, x, 1)^T + u_b(o);   roi_out = roi[floor(s + 0.5)] (0 outside);
 *   tau_out = trilinear(tau, s), corners outside the volume contributing 0;
 *   mri_out = mri_scale * g(trilinear(mri, s)) + mri_shift + noise_sigma * n, g(m) = m when mri_gamma == 1, else
 *   max(m, 0)^mri_gamma; then mri_out = 0 where roi_out == 0.
 * n = standard normal from Philox4x32-10 (key: low / high half of seed; counter: voxel index low, high, b, 0; index =
 * (z H + y) W + x), Box-Muller on the top 24 bits of output words 0 and 1: u1 = ((w0 >> 8) + 1) 2^-24,
 * u2 = (w1 >> 8) 2^-24, n = sqrt(-2 ln u1) cos(2 pi u2).  Not evaluated where noise_sigma == 0.
 * Outputs must not overlap the inputs or each other (error status, nothing launched).                          */
#define COMA_AUG_NPARAM 16
int coma_augment_warp(const float* mri, const float* tau, const float* roi, float* mri_out, float* tau_out,
                      float* roi_out, int32_t B, int32_t D, int32_t H, int32_t W, const float* params,
                      const float* disp, int32_t gz, int32_t gy, int32_t gx, uint64_t seed, void* stream);

/* ---- Gaussian smoothing of the tau target (DESIGN.md section 4 "Target smoothing"; the reference's `-smoothing`) ----
 * One launch filters a contiguous fp32 (B, D, H, W) batch of single-channel volumes into `out`, a distinct buffer, with a
 * separable filter.  taps_z / taps_y / taps_x: host pointers to nz / ny / nx fp32 weights (copied into the launch, so a
 * captured launch carries them); n must be odd, radius (n - 1) / 2 <= COMA_SMOOTH_MAX_RADIUS; a NULL pointer or n = 0
 * skips that axis (no halo, no pass).  With radius r the output along an axis is  sum_k taps[k] v[i - r + k]  (a
 * correlation), where v outside the volume is 0 (COMA_SMOOTH_ZEROS) or the nearest voxel inside (COMA_SMOOTH_NEAREST:
 * the index is clamped, also where the volume is shorter than the radius).
 * Arithmetic contract (tests compare bit for bit): the passes run in the order x, y, z over the axes that are not
 * skipped; each pass computes s = 0, then s = fmaf(taps[k], v[i - r + k], s) for k = 0 .. n - 1 in fp32, and its
 * result is rounded to fp32 before the next pass reads it.  With every axis skipped the output is a copy.
 * Fused source: with `in` NULL and `src` the raw (B, Dz, Hy, Wx) volumes, the filter's input is what
 * coma_resample_nearest(src, ..., default_value, nan_to_num, no zero_where) would write onto the (D, H, W) grid -- the
 * same index map, the same values, so the result is bit for bit the two-step one -- without that volume existing.
 * Exactly one of `in` and `src` is given; the other arguments of the unused form are ignored.
 * A block owns a tile of outputs; coma_gauss_smooth3d_tile reports its extents for a launch whose largest radius is
 * `radius` and whose z axis has a halo (z_filtered: nz > 1) or not.
 * Error status, nothing launched: radius > COMA_SMOOTH_MAX_RADIUS, even n, B / D / H / W < 1, unknown boundary mode,
 * `out` overlapping `in` or `src`, both or neither of `in` and `src`, non-positive spacings or source extents.        */
#define COMA_SMOOTH_ZEROS 0
#define COMA_SMOOTH_NEAREST 1
#define COMA_SMOOTH_MAX_RADIUS 8
#define COMA_SMOOTH_SMALL_RADIUS 4   /* up to here: the full tile and at least two blocks per CU */
#define COMA_SMOOTH_TILE_Z 8         /* halved when radius > COMA_SMOOTH_SMALL_RADIUS and the z axis has a halo */
#define COMA_SMOOTH_TILE_Y 8
#define COMA_SMOOTH_TILE_X 32
void coma_gauss_smooth3d_tile(int32_t radius, int32_t z_filtered, int32_t* tz, int32_t* ty, int32_t* tx);
int coma_gauss_smooth3d(const float* in, float* out, int32_t B, int32_t D, int32_t H, int32_t W, const float* taps_z,
                        int32_t nz, const float* taps_y, int32_t ny, const float* taps_x, int32_t nx,
                        int32_t boundary, const float* src, int32_t Dz, int32_t Hy, int32_t Wx, double sp_z,
                        double sp_y, double sp_x, double nsp_z, double nsp_y, double nsp_x, float default_value,
                        int32_t nan_to_num, void* stream);

/* ---- data-parallel gradient exchange over RCCL / xGMI (SURVEY.md section 8(b) last row, 8(e)): replaces the
 *      torch.nn.DataParallel the reference imports but never applies (attn_unet_data_parallel.py:32,1554).
 * One communicator per process (= per GPU).  Rank 0 creates the 128-byte id, the host distributes it by any means
 * (the Python host uses its torch.distributed group), every rank calls coma_comm_init on ITS device.  Collectives are
 * enqueued on the stream passed in -- a side HIP stream, so that a bucket's exchange overlaps the rest of backward -- and
 * never synchronise the host; they may be captured into a hipGraph.  All buffers are fp32 device pointers, reduction
 * is SUM (the reference sums the per-sample losses, criterions.py:560).  RCCL is bound at run time: an instance already
 * loaded in the process (PyTorch's) is shared.                                                                     */
#define COMA_COMM_ID_BYTES 128
int coma_comm_unique_id(void* id_out /* host, COMA_COMM_ID_BYTES */);
int coma_comm_init(const void* id /* host */, int32_t rank, int32_t nranks, void** comm_out);
int coma_comm_destroy(void* comm);
int coma_allreduce_sum_f32(void* comm, float* buf, int64_t n, void* stream);                       /* in place */
/* recv[n_per_rank] = this rank's slice of the sum of every rank's send[nranks * n_per_rank]; recv may alias that slice */
int coma_reduce_scatter_sum_f32(void* comm, const float* send, float* recv, int64_t n_per_rank, void* stream);
/* recv[nranks * n_per_rank] = concatenation of every rank's send[n_per_rank]; send may alias its own slice of recv */
int coma_allgather_f32(void* comm, const float* send, float* recv, int64_t n_per_rank, void* stream);
int coma_broadcast_f32(void* comm, float* buf, int64_t n, int32_t root, void* stream);            /* in place */

/* External events (the data-parallel exchange of a graph-replayed step WITHOUT a collective inside the graph;
 * coma_unet_amd/data_parallel.py GraphBucketWatch).  coma_event_record_external called on a stream that is being captured
 * adds an event-record node to the graph (hipGraphAddEventRecordNode behind the capture's current dependencies) instead of an internal
 * dependency; after every launch of the graph a stream OUTSIDE it can wait for that node with coma_stream_wait_external
 * (hipStreamWaitEvent) and run a bucket's all-reduce beside the rest of the replayed backward.
 * Outside a capture both behave as plain record / wait.  Events are created without timing.                          */
int coma_event_create(void** event_out);
int coma_event_destroy(void* event);
int coma_event_record_external(void* event, void* stream);
int coma_stream_wait_external(void* stream, void* event);

#ifdef __cplusplus
}
#endif
#endif /* COMA_UNET_H */
