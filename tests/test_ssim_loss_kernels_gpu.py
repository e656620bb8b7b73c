"""The SSIM-loss kernels (csrc/metrics.hip: ssim_partial_k<T, true>, ssim_bwd_k) against the fp64 autograd reference of
_ssim_loss_plan, at the smallest shapes that reach every edge of the 8^3 tiling.

Bounds.  Values: |(1 - ssim_b) - fp64| <= 1e-4 (the metric's bound, test_metrics.py) and equal to 1 - metrics.ssim3d to 1e-6
(the coefficient-writing variant must not change the sums).  fp32 gradient: rel-L2 vs fp64 at most 8 x the rel-L2 the fp32
torch restatement of the same formulas reaches on the same inputs (8: the kernel's three separable roundings and its other
summation order), and below 1e-3 in any case -- a wrong formula, shift or flipped adjoint lands at 0.19 or more.  bf16:
inputs rounded to bf16 first, fp64 reference on the rounded inputs, bound 2 x the error of the fp32 restatement with its
gradient rounded to bf16, cap 1e-2."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _ssim_loss_plan as sp

pytestmark = pytest.mark.gpu


def _internal(t):
    """(B, 1, D, H, W) -> the kernels' (B, D, H, W, 1)"""
    return t.permute(0, 2, 3, 4, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(case, kind, bf16):
    """Inputs (rounded to bf16 first when `bf16`), fp64 SSIM and gradient, and the yardstick error of the fp32 restatement
    (its gradient rounded to bf16 when `bf16`).  Computed once per case, shared, never modified."""
    shape, wkind, win = case
    x, y = sp.make_inputs(shape, kind, seed=11)
    if bf16:
        x, y = x.bfloat16().float(), y.bfloat16().float()
    w1, g = sp.window(wkind, win), sp.make_gout(shape[0])
    ssim, dx = sp.ssim_and_grad(x, y, w1, sp.C1, sp.C2, g)
    _, dx32 = sp.restated(x, y, w1, sp.C1, sp.C2, g, torch.float32)
    if bf16:
        dx32 = dx32.bfloat16()
    return x, y, g, ssim, dx, sp.rel_l2(dx32, dx)


def _abi_fwd(x, y, w, coef=None, coef_bytes=None):
    """coma_ssim_fwd_coef on (B, D, H, W, 1) device tensors -> rc, per-sample ssim (fp64) or None, coef."""
    from coma_unet_amd import _lib as L
    cx, win = L.ct(x), len(w)
    B, D, H, W, _ = x.shape
    nbytes = max(int(L.lib.coma_ssim_ws_bytes(cx, win)), 8)
    cbytes = int(L.lib.coma_ssim_coef_bytes(cx, win))
    part = torch.zeros(nbytes // 8, dtype=torch.float64, device=x.device)
    if coef is None:
        coef = torch.empty(max(cbytes // 4, 1), dtype=torch.float32, device=x.device)
    nt = ctypes.c_int32(0)
    rc = L.lib.coma_ssim_fwd_coef(cx, L.ct(y), w.ctypes.data_as(ctypes.c_void_p), win, sp.C1, sp.C2, L.ptr(part), nbytes,
                                  ctypes.addressof(nt), L.ptr(coef), cbytes if coef_bytes is None else coef_bytes, L.stream())
    if rc != 0:
        return rc, None, coef
    nvalid = (D - win + 1) * (H - win + 1) * (W - win + 1)
    return rc, part[:B * nt.value].view(B, nt.value).sum(1) / nvalid, coef


def _abi_bwd(x, y, coef, w, gout, dx):
    from coma_unet_amd import _lib as L
    return L.lib.coma_ssim_bwd(L.ct(x), L.ct(y), L.ptr(coef), w.ctypes.data_as(ctypes.c_void_p), len(w), L.ptr(gout), L.ct(dx),
                               L.stream())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("case", sp.CASES, ids=sp.case_id)
def test_loss_and_gradient_vs_fp64(case, kind, dtype):
    from coma_unet_amd import SSIMLoss, metrics as M
    shape, wkind, win = case
    bf16 = dtype == torch.bfloat16
    x, y, g, ssim64, dx64, e_ref = _reference(case, kind, bf16)
    xd = x.cuda().to(dtype).requires_grad_(True)
    yd = y.cuda().to(dtype)
    crit = SSIMLoss(kernel_type=wkind, win_size=win, reduction=None)
    loss = crit(xd, yd)
    assert loss.shape == (shape[0], 1) and loss.dtype == torch.float32
    (loss.view(-1) * (-g).float().cuda()).sum().backward()          # = d sum_b gout[b] ssim_b / dx
    assert xd.grad.dtype == dtype and xd.grad.shape == xd.shape
    metric = M.ssim3d(xd.detach(), yd, 1.0, wkind, win)
    e_val = float((loss.detach().view(-1).double().cpu() - (1 - ssim64)).abs().max())
    e_metric = float((loss.detach().view(-1).double() - (1 - metric)).abs().max())
    e = sp.rel_l2(xd.grad, dx64)
    print(f"{sp.case_id(case)} {kind} {'bf16' if bf16 else 'fp32'}: value err {e_val:.2e}, vs metric {e_metric:.2e}, "
          f"grad rel-L2 {e:.2e} (restatement {e_ref:.2e})")
    assert e_val <= 1e-4
    assert e_metric <= 1e-6
    if bf16:
        assert e <= 2 * e_ref and e <= 1e-2
    else:
        assert e_ref < 1e-4                                          # the yardstick itself is sane
        assert e <= 8 * e_ref
        assert e < 1e-3


def test_adjoint_orientation_with_an_asymmetric_window():
    """Through the C ABI: the classes only build symmetric windows, under which a flipped adjoint is invisible (0.19 here)."""
    case = sp.ASYM_CASE
    shape, wkind, win = case
    x, y, g, ssim64, dx64, e_ref = _reference(case, "rand", False)
    w = sp.np_window(wkind, win)
    xd, yd = _internal(x).cuda(), _internal(y).cuda()
    rc, ssim, coef = _abi_fwd(xd, yd, w)
    assert rc == 0
    dx = torch.full_like(xd, float("nan"))
    assert _abi_bwd(xd, yd, coef, w, g.float().cuda(), dx) == 0
    e = sp.rel_l2(dx.permute(0, 4, 1, 2, 3), dx64)
    print(f"asymmetric window: value err {float((ssim.cpu() - ssim64).abs().max()):.2e}, grad rel-L2 {e:.2e} (restatement {e_ref:.2e})")
    assert float((ssim.cpu() - ssim64).abs().max()) <= 1e-4
    assert e_ref < 1e-4 and e <= 8 * e_ref and e < 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_strided_pred_and_dx_equal_contiguous_bitwise(dtype):
    case = sp.CASES[1]
    shape, wkind, win = case
    x, y, g, *_ = _reference(case, "rand", dtype == torch.bfloat16)
    w = sp.np_window(wkind, win)
    B, _, D, H, W = shape
    xc, yd, gd = _internal(x).cuda().to(dtype), _internal(y).cuda().to(dtype), g.float().cuda()
    rc, ssim_c, coef_c = _abi_fwd(xc, yd, w)
    dx_c = torch.zeros_like(xc)
    assert rc == 0 and _abi_bwd(xc, yd, coef_c, w, gd, dx_c) == 0
    # pred: a slice of a larger buffer -- batch stride 2 * D*H*W * 3, voxel pitch 3
    big = torch.full((B, 2, D, H, W, 3), 7.0, dtype=dtype, device="cuda")
    xs = big[:, 1, :, :, :, 1:2]
    xs.copy_(xc)
    assert xs.stride(0) != D * H * W and xs.stride(3) == 3
    dbig = torch.full((B, 3, D, H, W, 2), -5.0, dtype=dtype, device="cuda")
    dx_s = dbig[:, 2, :, :, :, 0:1]
    rc, ssim_s, coef_s = _abi_fwd(xs, yd, w)
    assert rc == 0 and _abi_bwd(xs, yd, coef_s, w, gd, dx_s) == 0
    assert torch.equal(ssim_s, ssim_c) and torch.equal(coef_s, coef_c)
    assert torch.equal(dx_s, dx_c) and float(dx_c.float().abs().sum()) > 0
    assert bool((dbig[:, :2] == -5.0).all()) and bool((dbig[:, 2, ..., 1] == -5.0).all())      # nothing beside the destination


def test_two_runs_are_bitwise_equal():
    from coma_unet_amd import SSIMLoss
    case = sp.CASES[1]
    x, y, g, *_ = _reference(case, "smooth", False)
    crit = SSIMLoss(reduction=None)
    runs = []
    for _ in range(2):
        xd = x.cuda().requires_grad_(True)
        loss = crit(xd, y.cuda())
        (loss.view(-1) * g.float().cuda()).sum().backward()
        runs.append((loss.detach().clone(), xd.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].abs().sum()) > 0


@pytest.mark.parametrize("what", ["win12", "small", "dtypes", "dx_dtype", "short_coef"])
def test_abi_refusals_launch_nothing(what):
    from coma_unet_amd import _lib as L
    shape, win = (1, 1, 12, 12, 12), 11
    if what == "small":
        shape = (1, 1, 12, 10, 12)
    if what == "win12":
        win = 12
    g = torch.Generator().manual_seed(1)
    x = _internal(torch.rand(shape, generator=g)).cuda()
    y = _internal(torch.rand(shape, generator=g)).cuda()
    if what == "dtypes":
        y = y.bfloat16()
    w = np.full((win,), 1.0 / win, dtype=np.float32)
    dx = torch.full_like(x, 123.0)
    if what == "dx_dtype":
        dx = dx.bfloat16()
    coef = torch.full((3 * 12 * 12 * 12,), 77.0, dtype=torch.float32, device="cuda")
    gout = torch.ones(1, device="cuda")
    if what == "short_coef":
        need = int(L.lib.coma_ssim_coef_bytes(L.ct(x), win))
        assert need == 3 * 2 * 2 * 2 * 4
        rc, _, _ = _abi_fwd(x, y, w, coef=coef, coef_bytes=need - 4)
        assert rc != 0 and b"coefficient buffer too small" in L.lib.coma_last_error()
    else:
        if what != "dx_dtype":
            rc, _, _ = _abi_fwd(x, y, w, coef=coef, coef_bytes=coef.numel() * 4)
            assert rc != 0
        assert _abi_bwd(x, y, coef, w, gout, dx) != 0
        assert L.lib.coma_last_error()
    torch.cuda.synchronize()
    assert bool((dx == 123.0).all()) and bool((coef == 77.0).all())
    if what in ("win12", "small"):
        assert int(L.lib.coma_ssim_coef_bytes(L.ct(x), win)) == 0
