"""Shared by the SSIM-loss tests (no GPU needed here): the fp64 autograd reference, a plain-torch restatement of the
gradient formulas the kernels implement (DESIGN.md section 4 "SSIM loss"), the input generators and the cases.

Reference: `ssim_and_grad` differentiates the SSIM of oracle.metrics_oracle.ssim3d (same formulas, conv3d with the outer
product of an ARBITRARY 1-D window, so that an asymmetric window can tell a flipped adjoint from a right one) by autograd,
in fp64.  Restatement: the closed form, in a chosen dtype -- in fp64 it pins the formulas, in fp32 its distance from the
reference is the yardstick for the kernel's rounding."""
import numpy as np
import torch
import torch.nn.functional as F

ASYM7 = [0.05, 0.1, 0.3, 0.25, 0.15, 0.1, 0.05]
K1, K2 = 0.01, 0.03
C1, C2 = K1 ** 2, K2 ** 2                # data_range 1

# (shape, window kind, width): the smallest shapes that reach every edge of the 8^3 tiling
CASES = [((1, 1, 11, 11, 11), "gaussian", 11),     # one output voxel; the input tiling wider than the output's
         ((2, 1, 19, 20, 21), "gaussian", 11),     # two output tiles, three input tiles per axis, ragged in each
         ((2, 1, 15, 16, 17), "uniform", 7),
         ((1, 1, 27, 12, 20), "gaussian", 11)]     # four input tiles on one axis, a partial second tile on another
KINDS = ("rand", "smooth", "masked")
ASYM_CASE = ((2, 1, 15, 16, 17), "asym", 7)


def case_id(c):
    return "x".join(map(str, c[0][2:])) + f"-b{c[0][0]}-{c[1]}{c[2]}"


def window(kind, win, sigma=1.5):
    """1-D window, fp64."""
    if kind == "gaussian":
        dist = torch.arange((1 - win) / 2, (1 + win) / 2, 1.0, dtype=torch.float64)
        g = torch.exp(-torch.pow(dist / sigma, 2) / 2)
        return g / g.sum()
    if kind == "uniform":
        return torch.full((win,), 1.0 / win, dtype=torch.float64)
    if kind == "asym":
        assert win == len(ASYM7)
        return torch.tensor(ASYM7, dtype=torch.float64)
    raise ValueError(kind)


def make_inputs(shape, kind, seed):
    """(pred, target) fp32 in [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g)
    if kind == "smooth":
        y = F.avg_pool3d(F.pad(y, (2,) * 6, mode="replicate"), 5, stride=1)
    x = (y + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    if kind == "masked":                               # ~70 % of the voxels zero in both, like a skull-stripped volume
        keep = (torch.rand(shape, generator=g) > 0.7).float()
        x, y = x * keep, y * keep
    return x.contiguous(), y.contiguous()


def make_gout(B):
    """A different upstream gradient per sample, one of them negative."""
    return torch.tensor([-0.7, 1.3, 0.4, -2.1][:B], dtype=torch.float64)


def _kernel3(w1):
    return (w1[:, None, None] * w1[None, :, None] * w1[None, None, :])[None, None]


def _ssim_map(x, y, k, c1, c2):
    mx, my = F.conv3d(x, k), F.conv3d(y, k)
    mxx, myy, mxy = F.conv3d(x * x, k), F.conv3d(y * y, k), F.conv3d(x * y, k)
    sx, sy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    return ((2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1)) * ((2 * sxy + c2) / (sx + sy + c2))


def ssim_and_grad(x, y, w1, c1, c2, gout):
    """fp64 reference: per-sample mean SSIM (B,) and d(sum_b gout[b] * ssim_b)/dx by autograd."""
    x = x.detach().double().requires_grad_(True)
    y = y.detach().double()
    k = _kernel3(w1.double())
    s = _ssim_map(x, y, k, c1, c2)
    ssim = s.reshape(s.shape[0], -1).mean(1)
    (ssim * gout.double()).sum().backward()
    return ssim.detach(), x.grad.detach()


def restated(x, y, w1, c1, c2, gout, dtype):
    """The closed form of the gradient (what the kernels compute) with stock torch ops in `dtype`."""
    x, y = x.detach().to(dtype), y.detach().to(dtype)
    k = _kernel3(w1.double()).to(dtype)
    m0, m1 = F.conv3d(x, k), F.conv3d(y, k)
    m2, m3, m4 = F.conv3d(x * x, k), F.conv3d(y * y, k), F.conv3d(x * y, k)
    A1, B1 = 2 * m0 * m1 + c1, m0 * m0 + m1 * m1 + c1
    A2, B2 = 2 * (m4 - m0 * m1) + c2, (m2 - m0 * m0) + (m3 - m1 * m1) + c2
    Lm, C = A1 / B1, A2 / B2
    a0 = 2 * C * (m1 - m0 * Lm) / B1 + 2 * Lm * (m0 * C - m1) / B2
    a2 = -Lm * C / B2
    a4 = 2 * Lm / B2
    S = Lm * C
    n = S[0].numel()
    adj = lambda a: F.conv_transpose3d(a, k)           # the adjoint of the "valid" correlation
    dx = (gout.to(dtype).view(-1, 1, 1, 1, 1) / n) * (adj(a0) + 2 * x * adj(a2) + y * adj(a4))
    return S.reshape(S.shape[0], -1).mean(1), dx


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float((a - b).norm())


def np_window(kind, win):
    return window(kind, win).numpy().astype(np.float32)
