"""Shapes of test_conv_ws_gpu.py and plain-Python mirrors of the launch arithmetic that decides whether a convolution uses
the scratch it was handed (csrc/conv_mfma.hip launch_gather, csrc/conv_duo.hip duo_takes, csrc/conv_mfma.h wgrad_replicas,
csrc/api.hip coma_conv_wgrad_ws_bytes).  test_conv_ws_cpu.py asserts that the constants below are still the ones in the
sources and that every case crosses the boundary it is listed for.

A problem is described the way the library sees it: the launch reads x (B, *dims, cin) and writes y with cout channels on
the grid `out_dims`; form 0 = convolution, form 1 = transposed convolution; dt "bf16" | "f32" for both tensors.  All
tensors of the table have pitches and bases that allow 16-byte accesses (the mirrors assume it)."""
from collections import namedtuple

WGRAD_NREP = 64
WGRAD_REP_MAX_ELEMS = 16384
NORM_WS_ROWS = 1024          # coma_norm_ws_bytes: 1024 partial rows of C {sum, sumsq} fp64 pairs + 256 bytes
FWD_WS_CAP = 64 << 20        # conv_mfma_fwd_ws_bytes names no split-K scratch beyond 64 MiB
STAT_REPLICAS = 8
TAIL = 64 << 10              # sentinel bytes behind the live extent of every scratch buffer

# gather_ksplit(): (no split at or above this many blocks, nor below this many K steps, aimed number of blocks)
KSPLIT_BF16 = (384, 16, 512)
KSPLIT_F32 = (192, 8, 256)
KSPLIT_MAX = 8


def vol(dims):
    return dims[0] * dims[1] * dims[2]


def out_dims(dims, k, stride, form):
    if form == 1:
        return tuple(n * stride for n in dims)
    p = (k - 1) // 2
    return tuple((n + 2 * p - k) // stride + 1 for n in dims)


# ---------------------------------------------------------------------------------------------------------------------
# forward / data gradient
# ---------------------------------------------------------------------------------------------------------------------
def gather_ksplit(blocks, nsteps, f32):
    lim, min_steps, aim = KSPLIT_F32 if f32 else KSPLIT_BF16
    if blocks >= lim or nsteps < min_steps:
        return 1
    ks = min(aim // blocks, KSPLIT_MAX, nsteps // 4)
    return 1 if ks < 2 else ks


def gather_grid(BN, mode, Mtot, N, B, taps, C, f32):
    """-> (gx, gy, ksplit): BN output channels and BM voxels of the Mtot-voxel M-grid per block; mode 1 (stride-2 transposed):
    one parity class of 8 taps per blockIdx.y slice, a K step per 32 (bf16) / 16 (fp32) channels."""
    BM = 128 if BN == 128 else 256
    lck = 4 if f32 else 5
    gx, gy = (Mtot + BM - 1) // BM, (N // BN) * (8 if mode == 1 else 1)
    return gx, gy, gather_ksplit(gx * gy * B, (1 if mode == 1 else taps) * (C >> lck), f32)


def halo_ok(c):
    """bf16: the halo-tiled stride-1 3x3x3 family (conv_thin16_k / conv_mfma_halo2_k / conv_mfma_duo_k / conv_mfma_halo_k)"""
    D, H, W = c.dims
    if W < 16 and c.cin % 32 == 0 and c.cout % 32 == 0:
        return False
    return c.k == 3 and c.stride == 1 and W >= 8 and H * W >= 32 and (c.cin >= 8 or c.cout >= 8 or c.cin * c.cout >= 8)


def f32_halo_ok(c):
    D, H, W = c.dims
    if W < 16 and c.cin % 32 == 0 and c.cout % 32 == 0:
        return False
    return c.k == 3 and c.stride == 1 and W >= 8 and H * W >= 32 and c.cin % 16 == 0 and c.cout >= 16


def thin16f_ok(c):
    return c.k == 3 and c.stride == 1 and c.dims[2] >= 32 and c.cin <= 16 and c.cout <= (16 if c.cin > 8 else 32)


def pw_ok(c):
    return c.k == 1 and c.stride == 1 and 8 <= c.cin <= 64 and c.cin % 8 == 0 and 4 <= c.cout <= 64 and vol(c.dims) >= 4096


def tconv_ok(c):
    if c.form != 1 or c.stride != 2 or c.k != 3:
        return False
    ck = 64 // (4 if c.dt == "f32" else 2)
    return c.dims[2] >= 32 and c.cin % ck == 0 and c.cout % 32 == 0


def duo_frag_bytes(c):
    """scratch conv_mfma_duo_k wants for a fragment-ordered copy of the weights (C >= 64 stride-1 3^3 bf16 layers), else 0"""
    if c.dt != "bf16" or c.k != 3 or c.stride != 1 or c.dims[2] < 16:
        return 0
    if c.cin < 64 or c.cin % 16 or c.cout % 32:
        return 0
    return (c.B if c.ps else 1) * 27 * c.cout * c.cin * 2


def duo_wide_ok(c):
    return duo_frag_bytes(c) > 0 and c.cin > 32 and c.cin % 32 == 0 and max(c.dims) <= 510


def gather_problem(c):
    """-> (BN, mode, Mtot) of the conv_mfma_gather_k launch, or None when another family takes the problem"""
    f32 = c.dt == "f32"
    if f32:
        if thin16f_ok(c) or f32_halo_ok(c) or c.cin % 16 or c.cout % 32:
            return None
    elif halo_ok(c) or pw_ok(c) or c.cin % 32 or c.cout % 32:
        return None
    if tconv_ok(c):
        return None
    BN = 128 if c.cout % 128 == 0 else 64 if c.cout % 64 == 0 else 32
    mode = 1 if c.form == 1 and c.stride == 2 else 0
    od = out_dims(c.dims, c.k, c.stride, c.form)
    Mtot = vol(tuple((n + 1) // 2 for n in od)) if mode else vol(od)
    return BN, mode, Mtot


def case_ksplit(c):
    g = gather_problem(c)
    if g is None:
        return 1
    return gather_grid(g[0], g[1], g[2], c.cout, c.B, c.k ** 3, c.cin, c.dt == "f32")[2]


def case_blocks(c):
    g = gather_problem(c)
    gx, gy, _ = gather_grid(g[0], g[1], g[2], c.cout, c.B, c.k ** 3, c.cin, c.dt == "f32")
    return gx * gy * c.B


def fwd_ws_bytes(c):
    """conv_mfma_fwd_ws_bytes"""
    if c.dt == "f32":
        if thin16f_ok(c) or f32_halo_ok(c):
            return 0
    elif halo_ok(c):
        return duo_frag_bytes(c)
    elif pw_ok(c):
        return 0
    if tconv_ok(c):
        return 0
    nbytes = 4 * c.B * vol(out_dims(c.dims, c.k, c.stride, c.form)) * c.cout
    if nbytes > FWD_WS_CAP:
        return 0
    return nbytes if case_ksplit(c) > 1 else 0


Fwd = namedtuple("Fwd", "name dt cin cout k stride form dims ps B kind ksplit")
# kind: "gather" (split-K partial tiles in ws), "duo" (fragment-ordered weights in ws), "none" (the query answers 0)
FWD_CASES = [
    Fwd("gather_s1-bf16", "bf16", 64, 32, 3, 1, 0, (4, 5, 8), False, 2, "gather", 8),
    Fwd("gather_s1-f32", "f32", 64, 32, 3, 1, 0, (4, 5, 8), False, 2, "gather", 8),
    Fwd("gather_s2", "bf16", 32, 64, 3, 2, 0, (8, 10, 12), False, 2, "gather", 6),
    Fwd("gather_tr", "bf16", 512, 32, 3, 2, 1, (2, 3, 4), False, 2, "gather", 4),
    Fwd("gather_k1", "bf16", 512, 32, 1, 1, 0, (4, 4, 4), False, 2, "gather", 4),
    Fwd("duo_wide", "bf16", 64, 32, 3, 1, 0, (3, 5, 32), False, 2, "duo", 1),
    Fwd("duo_ragged", "bf16", 96, 64, 3, 1, 0, (3, 5, 40), False, 2, "duo", 1),
    Fwd("control", "bf16", 32, 32, 3, 1, 0, (3, 5, 32), False, 2, "none", 1),
    Fwd("gather_s1-ps", "bf16", 64, 32, 3, 1, 0, (4, 5, 8), True, 2, "gather", 8),
    Fwd("duo_wide-ps", "bf16", 64, 32, 3, 1, 0, (3, 5, 32), True, 2, "duo", 1),
]
FWD = {c.name: c for c in FWD_CASES}


# ---------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_out_elems(c):
    return c.k ** 3 * c.cout * c.cin * (c.B if c.ps else 1)


def wgrad2_ok(c):
    return c.stride == 1 and c.k in (1, 3) and c.dt == "bf16" and c.dims[2] >= 32


def conv_mfma_wgrad_ws_bytes(c):
    wsz = wgrad_out_elems(c)
    return 4 * wsz * WGRAD_NREP if (wgrad2_ok(c) or c.dt == "f32") and wsz <= WGRAD_REP_MAX_ELEMS else 0


def norm_ws_bytes(C):
    return NORM_WS_ROWS * C * 16 + 256


def wgrad_ws_bytes(c):
    """coma_conv_wgrad_ws_bytes = max(norm ws of dy, replica ws)"""
    return max(norm_ws_bytes(c.cout), conv_mfma_wgrad_ws_bytes(c))


def wgrad_K(c):
    """accumulated terms behind one weight-gradient element: the voxels (of every sample when batch-summed) + the replica fold"""
    return vol(c.dims) * (1 if c.ps else c.B) + WGRAD_NREP


Wg = namedtuple("Wg", "name dt cin cout k dims ps B algo kernel rep stride form")
# kernel: prefix of coma_last_kernel(); rep: the launcher merges into replicas when it is handed the queried scratch
WGRAD_CASES = [
    Wg("thin16_w", "bf16", 16, 16, 3, (3, 4, 35), False, 2, 0, "conv_thin16_wgrad_k", True, 1, 0),
    Wg("thin16_w-ps", "bf16", 16, 16, 3, (3, 4, 35), True, 2, 0, "conv_thin16_wgrad_k", True, 1, 0),
    Wg("wgrad2", "bf16", 32, 16, 3, (3, 4, 35), False, 2, 0, "conv_mfma_wgrad2_k", True, 1, 0),
    Wg("wgrad2_k1", "bf16", 64, 32, 1, (3, 4, 35), False, 2, 0, "conv_mfma_wgrad2_k", True, 1, 0),
    Wg("thin16f_w", "f32", 8, 16, 3, (3, 4, 35), False, 2, 0, "conv_thin16f_wgrad_k", True, 1, 0),
    Wg("planned_f32", "f32", 16, 32, 3, (4, 5, 9), False, 2, 0, "conv_f32_wgrad_k", True, 1, 0),
    Wg("planned_f32_k1", "f32", 32, 16, 1, (4, 5, 6), False, 2, 0, "conv_f32_wgrad_k", True, 1, 0),
    Wg("split_thin", "f32", 8, 8, 3, (3, 5, 33), False, 2, 6, "conv_split_thin_wgrad_k", True, 1, 0),
    Wg("pw_f32", "f32", 8, 4, 1, (16, 17, 17), False, 2, 7, "conv_pw_f32_wgrad_k", True, 1, 0),
    Wg("over_ps3", "bf16", 16, 16, 3, (3, 4, 35), True, 3, 0, "conv_thin16_wgrad_k", False, 1, 0),
    Wg("over_32x32", "bf16", 32, 32, 3, (3, 4, 35), False, 2, 0, "conv_mfma_wgrad2_k", False, 1, 0),
]
WGRAD = {c.name: c for c in WGRAD_CASES}
WSZ = {"thin16_w": 6912, "wgrad2": 13824, "over_ps3": 20736, "over_32x32": 27648}      # the figures the cases are listed with

# the production-path (ops.ZeroArena) tests: (forward case or weight-gradient case) by name
ARENA_CASES = ["gather_s1-bf16", "duo_wide", "thin16_w", "planned_f32"]
