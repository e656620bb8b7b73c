"""Shared by test_roi_losses_cpu.py, test_roi_losses_kernels_gpu.py, test_roi_losses_step_gpu.py and
make_roi_loss_golden.py: the fp64 restatement of the three voxel-weighted ROI losses, a plain-Python mirror of the launch
arithmetic of csrc/roi_loss.hip, the cases, and the bounds counted from the kernel source.

The restatement is plain torch on whatever device its inputs live on and shares no code with the kernels.  It follows the
reference's literal two-pass form (criterions.py:28-122): the mask is built by the `roi == idx` loop over a volume of ones,
RoiRSE's m is mean(mask * gt) and its denominator sum (gt - m)^2.
"""
import torch

U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8          # bound of one bf16 rounding relative to the value (test_nonconv_sizes_gpu.py's u_out)
U_F64 = 2.0 ** -53

WMSE, RSE, RRMSE = 0, 1, 2
KINDS = {"wmse": WMSE, "rse": RSE, "rrmse": RRMSE}

# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic of csrc/roi_loss.hip (test_roi_losses_cpu.py searches the source for the constants)
# ---------------------------------------------------------------------------------------------------------------------
THREADS = 256
RWL_BLOCKS = 512            # roi_wloss_partial_k: one block per 256 * 8 voxels, capped -- loss_partial_k's arithmetic
RWL_PER_BLOCK = 256 * 8
RWL_REC = 4                 # doubles per block record
FINALIZE_LANES = 64
BWD_CAP = 8192


def cdiv(a, b):
    return -(-a // b)


def vol(dims):
    return dims[0] * dims[1] * dims[2]


def fwd_blocks(V):
    return max(1, min(cdiv(V, RWL_PER_BLOCK), RWL_BLOCKS))


def ws_bytes(B):
    return B * RWL_BLOCKS * RWL_REC * 8


def vec4_ok(ld, sb, elem_offset):
    """rwl_vec4 of one tensor: voxel pitch 1, sample stride a multiple of 4, base on a 4-element boundary (element offset
    from a 16-byte aligned allocation)."""
    return ld == 1 and sb % 4 == 0 and elem_offset % 4 == 0


def fwd_trips(V, vec):
    """Trips of the forward grid-stride loop the busiest thread makes (items: voxels, or 4-voxel groups)."""
    return cdiv(V // 4 if vec else V, fwd_blocks(V) * THREADS)


def bwd_blocks(V, vec):
    return max(1, min(cdiv(cdiv(V, 4) if vec else V, THREADS), BWD_CAP))


def finalize_trips(V):
    return cdiv(fwd_blocks(V), FINALIZE_LANES)


# ---------------------------------------------------------------------------------------------------------------------
# the cases: (name, dims, B, layout).  layout: "dense" contiguous samples; "padded" contiguous voxels with the sample stride
# rounded up to a multiple of 4; "pitched" pred / dpred at the 16-byte voxel pitch; (the path each one takes is asserted
# from the mirror above by test_roi_losses_cpu.py and stated again at the GPU test)
# ---------------------------------------------------------------------------------------------------------------------
CASES = [
    ("tail", (5, 6, 7), 3, "dense"),          # under one block; V = 210: sample stride no multiple of 4 -> scalar path
    ("vtail", (5, 6, 7), 3, "padded"),        # the same volume at sample stride 212 -> vector path with 2 scalar tail voxels
    ("mid", (32, 33, 35), 3, "dense"),        # vector path, 19 blocks
    ("cap", (64, 128, 129), 2, "dense"),      # V = 512 * 2064: past the 512-block cap, 3 vector trips, 8 finalise trips
    ("pitched", (32, 33, 35), 3, "pitched"),  # scalar path through the voxel pitch, 8 trips
]
GOLDEN_DIMS = (5, 6, 7)
GOLDEN_B = (1, 2, 3)
OTHER_LABELS = (0, 2, 4999)                  # not in the 36-id table; 4999 is past the kernels' 4096-entry label table


def case_layout(dims, B, layout, esize):
    """-> dict(pred=(ld, sb), gt=(ld, sb), roi=(ld, sb), vec=whether the kernels take the 4-voxel path) in elements."""
    V = vol(dims)
    if layout == "dense":
        pl = gl = (1, V)
    elif layout == "padded":
        pl = gl = (1, cdiv(V, 4) * 4)
    else:
        ld = 16 // esize
        pl, gl = (ld, V * ld), (1, V)
    return dict(pred=pl, gt=gl, roi=gl, vec=all(vec4_ok(ld, sb, 0) for ld, sb in (pl, gl, gl)))


def mixed_weights(n=36, dtype=torch.float64):
    """225 everywhere but 100 and 7.5 at two slots (the mix of tests/golden/criterions_ref.npz)."""
    w = torch.full((n,), 225.0, dtype=dtype)
    w[3], w[20] = 100.0, 7.5
    return w


TEMPLATE_IDS = list(range(1, 9))             # the template-space table: ids 1..8 with weight 1 (validation.py:68,128)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 restatement, two-pass
# ---------------------------------------------------------------------------------------------------------------------
def mask64(roi, ids, w, bg=1.0):
    mask = torch.full(roi.shape, float(bg), dtype=torch.float64, device=roi.device)
    for i, idx in enumerate(ids):
        mask[roi == idx] = float(w[i])
    return mask


def _flat(t):
    return t.double().reshape(t.shape[0], -1)


def terms64(kind, pred, gt, roi, ids, w, bg=1.0):
    """-> (N, D) per sample, (B,) each; volumes of any layout whose first dimension is the batch."""
    p, g = _flat(pred), _flat(gt)
    mask = _flat(mask64(roi, ids, w, bg))
    num = torch.sum(mask * torch.square(g - p), dim=1)
    if kind == WMSE:
        den = torch.sum(mask, dim=1)
    elif kind == RSE:
        m = torch.mean(mask * g, dim=1)                              # the reference's weighted "mean"
        den = torch.sum(torch.square(g - m.view(-1, 1)), dim=1)      # ... under an UNWEIGHTED sum
    else:
        den = torch.sum(mask * torch.square(g), dim=1)
    return num, den


def loss64(kind, pred, gt, roi, ids, w, bg=1.0):
    """per-sample loss (B,) in fp64, differentiable in `pred`."""
    num, den = terms64(kind, pred, gt, roi, ids, w, bg)
    return torch.sqrt(num / den) if kind == RRMSE else num / den


def loss_coef_grad64(kind, pred, gt, roi, ids, w, gout, bg=1.0):
    """-> loss (B,), coef (B,), d (sum_b gout_b loss_b) / d pred by autograd on the restatement, D (B,)."""
    p = pred.detach().double().clone().requires_grad_(True)
    l = loss64(kind, p, gt, roi, ids, w, bg)
    (l * gout.double().reshape(-1)).sum().backward()
    _, den = terms64(kind, pred, gt, roi, ids, w, bg)
    coef = 1.0 / (den * l.detach()) if kind == RRMSE else 2.0 / den
    return l.detach(), coef, p.grad, den


def one_pass_den64(kind, gt, roi, ids, w, bg=1.0):
    """The kernels' one-pass denominators, in fp64: D = sum g^2 - 2 m sum g + V m^2 for RSE."""
    g = _flat(gt)
    mask = _flat(mask64(roi, ids, w, bg))
    V = g.shape[1]
    if kind == WMSE:
        return mask.sum(1)
    if kind == RRMSE:
        return (mask * g * g).sum(1)
    m = (mask * g).sum(1) / V
    return ((g * g).sum(1) - 2.0 * m * g.sum(1)) + V * m * m


def den_mass64(kind, gt, roi, ids, w, bg=1.0):
    """L1 mass of the terms of the one-pass denominator: what its fp64 roundings are relative to."""
    g = _flat(gt)
    mask = _flat(mask64(roi, ids, w, bg))
    V = g.shape[1]
    if kind != RSE:
        return one_pass_den64(kind, gt, roi, ids, w, bg)
    m = (mask * g).sum(1) / V
    return (g * g).sum(1) + 2.0 * m.abs() * g.abs().sum(1) + V * m * m


# ---------------------------------------------------------------------------------------------------------------------
# bounds, counted from csrc/roi_loss.hip.  u = 2^-24 per fp32 rounding, taken twice as test_nonconv_sizes_gpu.py does
# (2 K u); fp64 sums of V terms: (V + 8) 2^-53 of their L1 mass (V adds, the product roundings, the block / finalise tree).
#   rwl_acc: d = p - g rounds once in fp32 and enters the square twice -> K = 2 on N; w, g, g^2 are exact in double.
#   finalise: N / D (and the sqrt, which halves a relative error) in double, one cast to fp32 (u_out).
#   coef: 2 / D carries D's fp64 error and the cast; 1 / (D loss) also carries loss's half of N's: K = 1.
#   backward: scale = gout * coef (the stored fp32 coef: 1 (+ 1 for RRMSE's N), the product: 1), d: 1, scale * w: 1,
#   (.) * d: 1 -> K = 5 (6 for RRMSE), and the store's rounding u_out.
# ---------------------------------------------------------------------------------------------------------------------
K_LOSS = {WMSE: 2, RSE: 2, RRMSE: 1}
K_COEF = {WMSE: 0, RSE: 0, RRMSE: 1}
K_GRAD = {WMSE: 5, RSE: 5, RRMSE: 6}
# ceilings that must hold besides the counted bounds
LOSS_REL = 1e-6
GRAD_REL_L2 = {torch.float32: 1e-6, torch.bfloat16: 2.0 ** -9 + 1e-6}


def rel_bound(K, V, amp=1.0):
    """relative bound of a per-sample scalar: one fp32 cast + 2 K u + the fp64 sums (amplified by mass(D) / D)."""
    return U_F32 + 2.0 * K * U_F32 + (V + 8) * U_F64 * (1.0 + amp)


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


# ---------------------------------------------------------------------------------------------------------------------
# the golden inputs (tests/golden/roi_losses_ref.npz): values exactly representable in bf16, one fixture for every dtype
# ---------------------------------------------------------------------------------------------------------------------
def golden_inputs(B, roi_ids, seed=2024):
    """pred, gt (multiples of 1/64 in [0, 4): 8 significant bits), roi labels drawn from the ROI ids and OTHER_LABELS;
    (B, 1, 5, 6, 7) fp64."""
    g = torch.Generator().manual_seed(seed + B)
    shape = (B, 1) + GOLDEN_DIMS
    pred = torch.randint(0, 256, shape, generator=g).double() / 64.0
    gt = torch.randint(0, 256, shape, generator=g).double() / 64.0
    lab = torch.tensor(list(roi_ids) + list(OTHER_LABELS), dtype=torch.float64)
    roi = lab[torch.randint(0, lab.numel(), shape, generator=g)]
    return pred, gt, roi
