"""Shared by test_grad_diff_cpu.py, test_grad_diff_kernels_gpu.py and test_grad_diff_step_gpu.py: the fp64 restatement of the
gradient-difference loss, the mirror of the tile arithmetic of csrc/grad_diff.hip, the cases, the input construction and the
bounds counted from the kernel's arithmetic.

The restatement is plain torch on whatever device its inputs live on and shares no code with the kernels: narrow-slice
forward differences per axis, torch.where on N_a > 0, autograd for the gradient (torch's abs has the subgradient 0 at 0).

Bounds.  The kernels convert the staged fp32 values to fp64 and do ALL arithmetic there; the restatement does the same
operations on the same values, so gp, gg and t -- and every sign decision -- are the same numbers on both sides.  What is left:
  loss   S_a: a sum of n_a <= V non-negative fp64 terms in another order (<= n_a u64 relative each side); the quotient, the
         product with s_a and the sum over the axes (3 roundings each side); ONE cast to fp32 (u32).
  coef   s_a / N_a in fp64 (N_a an exactly represented integer), ONE cast to fp32 (u32).
  dpred  gout coef_a in fp64 from the fp32 coef (u32 off the restatement's), psi differences and the sum over the axes in
         fp64 (a handful of u64 on the magnitude), ONE cast to the output dtype.  The six terms may cancel, so the coef
         error is measured against A[v] = |gout| sum_a coef_a (|psi_a(v - e_a)| + |psi_a(v)|), not against the result:
         |dpred - ref| <= (u32 + 16 u64) A + u_out (|ref| + (u32 + 16 u64) A),  u_out = u32 (fp32) | 2^-8 (bf16: 8 significant bits, nearest-even).
"""
import torch

from _roi_loss_plan import U_F32, U_BF16, U_F64, cdiv, rel_l2  # noqa: F401

ABS, SIGNED = 0, 1
MODES = {"abs": ABS, "signed": SIGNED}
CONFIGS = [("abs", 1), ("abs", 2), ("signed", 1), ("signed", 2)]
# the axis weights (z, y, x) each configuration runs with: the default, the default, uneven ones, one axis switched off
AXIS_W = {("abs", 1): (1.0, 1.0, 1.0), ("abs", 2): (1.0, 1.0, 1.0), ("signed", 1): (0.5, 2.0, 1.25), ("signed", 2): (1.0, 0.0, 3.0)}
GOUT = [1.0, -2.0]

# ---------------------------------------------------------------------------------------------------------------------
# tile arithmetic of csrc/grad_diff.hip (test_grad_diff_cpu.py searches the source for the constants)
# ---------------------------------------------------------------------------------------------------------------------
GD_TZ, GD_TY, GD_TX = 8, 8, 32
GD_REC = 6                   # doubles per tile record
FIN_LANES = 64               # the finalise: lane l adds records l, l + 64, ...


def tiles(dims):
    return cdiv(dims[0], GD_TZ) * cdiv(dims[1], GD_TY) * cdiv(dims[2], GD_TX)


def ws_bytes(B, dims):
    return B * tiles(dims) * GD_REC * 8


def vec_ok(ld, sb, W, elem_offset, esize):
    """gd_vec: rows of 16-byte chunks -- voxel pitch 1, W and the sample stride multiples of the chunk, an aligned base"""
    n = 16 // esize
    return ld == 1 and W % n == 0 and sb % n == 0 and elem_offset % n == 0


# (name, (D, H, W), B): the smallest shapes that reach every path
CASES = [
    ("tiny", (3, 4, 5), 1),         # smaller than one tile
    ("edges", (9, 10, 37), 2),      # one, two and five voxels past a tile along z, y, x: 8 tiles, 7 of them partial
    ("flat", (1, 8, 40), 2),        # no z pair: the z coefficient is 0, everything stays finite; W % 8 == 0: 16-byte rows
    ("multi", (40, 40, 72), 2),     # 75 tiles per sample: past the finalise's 64 lanes; 16-byte rows
]
LAYOUTS = ("contig", "slice", "off1")      # dense | channel 0 of a (..., 4) fp32 / (..., 8) bf16 buffer | one element off the base
MASKS = (None, "brain", "zero")            # "brain": the LAST sample's labels all zero when B > 1; "zero": every label zero


def case(name):
    return next(c for c in CASES if c[0] == name)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * ord(c) for i, c in enumerate("/".join(str(k) for k in key))) % (2 ** 31))
    return g


def make_labels(dims, B, mask, gen):
    """(B, D, H, W) fp32 labels: about a quarter zeros among atlas ids (17 .. 2035) and a fraction"""
    pool = torch.tensor([0.0, 17.0, 1002.0, 2035.0, 53.5, 0.0, 18.0, 4999.0])
    lab = pool[torch.randint(0, len(pool), (B, *dims), generator=gen)]
    if mask == "zero":
        lab.zero_()
    elif B > 1:
        lab[B - 1].zero_()
    return lab


def exact_inputs(name, mask=None):
    """pred, gt (B, D, H, W) fp32 multiples of 1/64 in [0, 4) -- representable in bf16, every difference, |.| difference and
    square exact in fp32 -- with planted ties: gp = 0 (x neighbours copied), pred = gt (t = 0 in both modes) and
    pred = 255/64 - gt (gp = -gg: t = 0 under "abs" only); labels."""
    _, dims, B = case(name)
    gen = _gen("grad_diff", "exact", name)
    k = torch.randint(0, 256, (2, B, *dims), generator=gen)
    kp, kg = k[0].clone(), k[1]
    W = dims[2]
    if W >= 2:
        kp[..., 1::5] = kp[..., 0::5][..., :kp[..., 1::5].shape[-1]]          # gp_x = 0
    kp[:, :, 0, :] = kg[:, :, 0, :]                                           # the y = 0 rows: pred = gt
    kp[:, 0, -1, :] = 255 - kg[:, 0, -1, :]                                   # one row: gp = -gg along x
    return kp.float() / 64.0, kg.float() / 64.0, make_labels(dims, B, mask, gen)


def random_inputs(name, mask=None):
    """pred, gt uniform in [0, 4), fp32; labels"""
    _, dims, B = case(name)
    gen = _gen("grad_diff", "random", name)
    x = 4.0 * torch.rand((2, B, *dims), generator=gen)
    x = x.clamp_(max=float(torch.nextafter(torch.tensor(4.0), torch.tensor(0.0))))
    return x[0].contiguous(), x[1].contiguous(), make_labels(dims, B, mask, gen)


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def _v4(t):
    """(B, D, H, W) or (B, D, H, W, 1) -> (B, D, H, W)"""
    return t[..., 0] if t.dim() == 5 else t


def _diff(x, d):
    n = x.shape[d]
    return x.narrow(d, 1, n - 1) - x.narrow(d, 0, n - 1)


def axis_maps(pred, gt, roi, mode, d):
    """axis d in (1, 2, 3) of (B, D, H, W) fp64 volumes -> gp, t, m over the pairs (shape: one shorter along d)"""
    gp, gg = _diff(pred, d), _diff(gt, d)
    t = gp.abs() - gg.abs() if mode == ABS else gp - gg
    if roi is None:
        m = torch.ones_like(t)
    else:
        nz = (roi != 0).to(t.dtype)
        n = nz.shape[d]
        m = nz.narrow(d, 1, n - 1) * nz.narrow(d, 0, n - 1)
    return gp, t, m


def sums64(pred, gt, roi, mode, alpha):
    """-> S (B, 3), N (B, 3) in the order z, y, x"""
    pred, gt, roi = _v4(pred).double(), _v4(gt).double(), None if roi is None else _v4(roi)
    S, N = [], []
    for d in (1, 2, 3):
        _, t, m = axis_maps(pred, gt, roi, mode, d)
        phi = t.abs() if alpha == 1 else t * t
        S.append((m * phi).sum(dim=(1, 2, 3)))
        N.append(m.sum(dim=(1, 2, 3)))
    return torch.stack(S, 1), torch.stack(N, 1)


def coef64(N, axis_w):
    w = torch.as_tensor(axis_w, dtype=torch.float64, device=N.device)
    return torch.where(N > 0, w / N.clamp_min(1.0), torch.zeros_like(N))


def loss64(pred, gt, roi, mode, alpha, axis_w=(1.0, 1.0, 1.0)):
    """-> (B,) fp64; differentiable in pred"""
    S, N = sums64(pred, gt, roi, mode, alpha)
    w = torch.as_tensor(axis_w, dtype=torch.float64, device=S.device)
    return (w * torch.where(N > 0, S / N.clamp_min(1.0), torch.zeros_like(S))).sum(1)


def loss_coef_grad64(pred, gt, roi, mode, alpha, axis_w, gout):
    """-> loss (B,), coef (B, 3), d(sum_b gout_b loss_b)/d pred (B, D, H, W) by autograd, all fp64"""
    p = pred.detach().double().clone().requires_grad_(True)
    loss = loss64(p, gt, roi, mode, alpha, axis_w)
    (loss * gout.double().to(loss.device)).sum().backward()
    _, N = sums64(pred, gt, roi, mode, alpha)
    return loss.detach(), coef64(N, axis_w), _v4(p.grad)


def _scatter(B, dims, d, val, sign_lo, device):
    """a pair map `val` (one shorter along d) onto the voxels: + val at the pair's upper voxel, sign_lo * val at its lower"""
    out = torch.zeros((B, *dims), dtype=torch.float64, device=device)
    n = out.shape[d]
    out.narrow(d, 1, n - 1).add_(val)
    out.narrow(d, 0, n - 1).add_(sign_lo * val)
    return out


def closed_grad_amp64(pred, gt, roi, mode, alpha, axis_w, gout, tie=1e-5):
    """The gather form the backward kernel evaluates, from the restatement's maps: -> grad (B, D, H, W), the amplification A
    the bound rests on, and `near`: voxels touching a pair with |t| <= tie or |gp| <= tie (where a last-bit rounding of
    lower-precision arithmetic may flip a sign)."""
    p4, g4, r4 = _v4(pred).double(), _v4(gt).double(), None if roi is None else _v4(roi)
    B, dims = p4.shape[0], tuple(p4.shape[1:])
    _, N = sums64(pred, gt, roi, mode, alpha)
    c = coef64(N, axis_w) * gout.double().to(p4.device)[:, None]
    grad = torch.zeros_like(p4)
    amp = torch.zeros_like(p4)
    near = torch.zeros_like(p4)
    for a, d in enumerate((1, 2, 3)):
        gp, t, m = axis_maps(p4, g4, r4, mode, d)
        psi = m * (torch.sign(t) if alpha == 1 else 2.0 * t) * (torch.sign(gp) if mode == ABS else 1.0)
        ca = c[:, a].reshape(B, 1, 1, 1)
        grad += _scatter(B, dims, d, ca * psi, -1.0, p4.device)
        amp += _scatter(B, dims, d, (ca * psi).abs(), 1.0, p4.device)
        near += _scatter(B, dims, d, ((t.abs() <= tie) | (gp.abs() <= tie)).double(), 1.0, p4.device)
    return grad, amp, near > 0


# ---------------------------------------------------------------------------------------------------------------------
# bounds (the module docstring counts them)
# ---------------------------------------------------------------------------------------------------------------------
def loss_bound(V):
    """relative: one fp32 cast + the fp64 terms of both sides (sums of <= V terms, 3 more roundings)"""
    return U_F32 + 2.0 * (V + 3) * U_F64


def coef_bound():
    return U_F32 + 4.0 * U_F64


def grad_bound(ref, amp, dtype):
    """elementwise absolute bound on dpred"""
    u_out = U_BF16 if dtype == torch.bfloat16 else U_F32
    e = (U_F32 + 16.0 * U_F64) * amp
    return e + u_out * (ref.abs() + e)
