"""What the gradient-difference loss (criterions.GradientDifferenceLoss / WithGradDiff, csrc/grad_diff.hip) costs, in ONE
process on one GPU, alternating blocks, warm-up first (the method of roi_mean.py), at 128^3 x 2:

  (a) the kernels alone through the C ABI, fp32 and bf16: the forward (tile pass + finalise) and the backward, on dense
      volumes (16-byte staging and stores) and with pred / dpred at the 16-byte voxel pitch (element-wise staging of pred),
      with mask None and mask "brain", against coma_roi_wloss_fwd (kind WMSE) / coma_roi_wloss_bwd on the same tensors in the
      same brackets -- us per call and TB/s on algorithmic bytes per voxel: forward 2 es (+ 4 with the mask) against roi_wloss's
      2 es + 4; backward 3 es (+ 4) against 3 es + 4 (the halo a tile re-reads is not counted);
  (b) the slice-based fp32 torch composition of the same formulas under autograd, forward + backward, on the device;
  (c) the graph-replayed bf16 step (static prompts, learning rate 0) with and without grad_diff_weight.

  python profiles/grad_diff.py [--size 128] [--blocks 5] [--steps 8] > profiles/grad_diff.txt

Aim, recorded and not gated: the forward with the mask (the same algorithmic bytes as roi_wloss fwd)
at 0.8 of roi_wloss fwd's rate in the same run on the same layout.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ev():
    return torch.cuda.Event(enable_timing=True)


def bracket(fns, blocks, per):
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(per):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / per)
    return t


def kernels(a, size, dtype, name):
    from coma_unet_amd import _lib as L
    from coma_unet_amd.roi_tables import ROI_INDICES
    from coma_unet_amd.synthetic import make_batch
    lib, ct, ptr = L.lib, L.ct, L.ptr
    B, (D, H, W) = a.batch, size
    V = B * D * H * W
    es = 2 if dtype == torch.bfloat16 else 4
    gen = torch.Generator(device="cuda").manual_seed(0)
    shape = (B, D, H, W, 1)
    b = make_batch(B, size, seed=1000)
    gt = b["tau"].permute(0, 2, 3, 4, 1).contiguous().cuda()
    dense = (gt + 0.1 * torch.randn(shape, generator=gen, device="cuda")).to(dtype)
    gt = gt.to(dtype)
    roi = b["roi"].permute(0, 2, 3, 4, 1).contiguous().cuda()
    ld = 16 // es
    pitched = torch.zeros((B, D, H, W, ld), dtype=dtype, device="cuda")[..., :1]
    pitched.copy_(dense)
    ids = torch.tensor(ROI_INDICES, dtype=torch.int32, device="cuda")
    w = torch.full((len(ROI_INDICES),), 225.0, device="cuda")
    loss, aux, gout = (torch.ones(B, device="cuda") for _ in range(3))
    coef = torch.full((B, 3), 1e-6, device="cuda")      # the backward calls' input; the forward calls write coef_fwd
    coef_fwd = torch.empty((B, 3), device="cuda")
    ws = torch.empty(max(lib.coma_roi_wloss_ws_bytes(ct(dense)), lib.coma_grad_diff_ws_bytes(ct(dense))), dtype=torch.uint8, device="cuda")
    aw = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    s = L.stream()
    fns, nbytes, keep = {}, {}, []
    cg, cr = ct(gt), ct(roi)
    for lay, pred in (("dense", dense), ("pitched", pitched)):
        dp = torch.empty_like(dense) if lay == "dense" else torch.zeros((B, D, H, W, ld), dtype=dtype, device="cuda")[..., :1]
        keep.append(dp)                      # (the descriptors hold raw pointers)
        cp, cd = ct(pred), ct(dp)
        fns[f"{lay} roi_wloss fwd"] = lambda cp=cp: L.check(lib.coma_roi_wloss_fwd(
            cp, cg, cr, ptr(ids), ptr(w), ids.numel(), 1.0, 0, ptr(loss), ptr(aux), ptr(ws), ws.numel(), s), "roi_wloss_fwd")
        nbytes[f"{lay} roi_wloss fwd"] = 2 * es + 4
        fns[f"{lay} roi_wloss bwd"] = lambda cp=cp, cd=cd: L.check(lib.coma_roi_wloss_bwd(
            cp, cg, cr, ptr(ids), ptr(w), ids.numel(), 1.0, ptr(gout), ptr(aux), cd, s), "roi_wloss_bwd")
        nbytes[f"{lay} roi_wloss bwd"] = 3 * es + 4
        for mask, r in (("none", None), ("brain", cr)):
            fns[f"{lay} grad_diff fwd {mask}"] = lambda cp=cp, r=r: L.check(lib.coma_grad_diff_fwd(
                cp, cg, r, 0, 1, aw, ptr(loss), ptr(coef_fwd), ptr(ws), ws.numel(), s), "grad_diff_fwd")
            nbytes[f"{lay} grad_diff fwd {mask}"] = 2 * es + (4 if r is not None else 0)
            fns[f"{lay} grad_diff bwd {mask}"] = lambda cp=cp, cd=cd, r=r: L.check(lib.coma_grad_diff_bwd(
                cp, cg, r, 0, 1, ptr(gout), ptr(coef), cd, s), "grad_diff_bwd")
            nbytes[f"{lay} grad_diff bwd {mask}"] = 3 * es + (4 if r is not None else 0)
    per = 20
    t = bracket(fns, a.blocks, per)
    med = {k: statistics.median(v) for k, v in t.items()}
    rate = {k: nbytes[k] * V / (med[k] * 1e-6) / 1e12 for k in fns}
    print(f"\n(a) {name}: kernels alone, {B} x {D}x{H}x{W}; us per call ({per} calls per bracket, {a.blocks} alternating brackets; a forward "
          f"call is the pass and its finalise); TB/s on algorithmic bytes")
    for k in fns:
        print(f"  {k:32s} {nbytes[k]:3d} B/voxel  median {med[k]:8.2f} us [{min(t[k]):8.2f} .. {max(t[k]):8.2f}]  {rate[k]:6.3f} TB/s")
    for lay in ("dense", "pitched"):
        for mask in ("none", "brain"):
            r = rate[f"{lay} grad_diff fwd {mask}"] / rate[f"{lay} roi_wloss fwd"]
            tag = f"(aim 0.8: {'MET' if r >= 0.8 else 'NOT MET'})" if mask == "brain" else "(fewer bytes: no aim)"
            print(f"  {lay:8s} mask {mask:5s} fwd rate / roi_wloss fwd rate = {r:5.2f} {tag};  "
                  f"fwd time / roi_wloss fwd time = {med[f'{lay} grad_diff fwd {mask}'] / med[f'{lay} roi_wloss fwd']:5.2f};  "
                  f"bwd time / roi_wloss bwd time = {med[f'{lay} grad_diff bwd {mask}'] / med[f'{lay} roi_wloss bwd']:5.2f}")


def torch_composition(a, size):
    """the term as a user would write it: fp32, strided slices, autograd -- forward + backward, alpha 1 "abs", mask None / "brain" """
    from coma_unet_amd.synthetic import make_batch
    import coma_unet_amd as cu
    B = a.batch
    b = make_batch(B, size, seed=1000)
    gt, roi = b["tau"].cuda(), b["roi"].cuda()
    pred = (gt + 0.1 * torch.randn(gt.shape, device="cuda")).requires_grad_(True)

    def compose(mask):
        total = 0.0
        nz = (roi != 0).float() if mask else None
        for d in (2, 3, 4):
            n = pred.shape[d]
            gp = pred.narrow(d, 1, n - 1) - pred.narrow(d, 0, n - 1)
            gg = gt.narrow(d, 1, n - 1) - gt.narrow(d, 0, n - 1)
            t = (gp.abs() - gg.abs()).abs()
            if mask:
                m = nz.narrow(d, 1, n - 1) * nz.narrow(d, 0, n - 1)
                total = total + (m * t).sum(dim=(1, 2, 3, 4)) / m.sum(dim=(1, 2, 3, 4)).clamp_min(1.0)
            else:
                total = total + t.mean(dim=(1, 2, 3, 4))
        return total

    def run_torch(mask):
        pred.grad = None
        compose(mask).sum().backward()

    def run_fused(crit):
        pred.grad = None
        crit(pred, gt, roi).sum().backward()

    crits = {m: cu.GradientDifferenceLoss(mask=m, reduction=None) for m in (None, "brain")}
    for m in (None, "brain"):                # the two agree before they are timed
        run_torch(m)
        g0, v0 = pred.grad.clone(), compose(m).detach()
        run_fused(crits[m])
        e = float((pred.grad - g0).norm() / g0.norm())
        print(f"  mask {m}: fused vs torch composition: loss rel diff {float(((crits[m](pred, gt, roi).reshape(-1) - v0).abs() / v0).max()):.2e}, gradient rel-L2 {e:.2e}")
    fns = {}
    for m in (None, "brain"):
        fns[f"torch slices fwd+bwd mask {m}"] = lambda m=m: run_torch(m)
        fns[f"fused module fwd+bwd mask {m}"] = lambda m=m: run_fused(crits[m])
    per = 5
    t = bracket(fns, a.blocks, per)
    print(f"\n(b) fp32, {B} x {size[0]}^3: forward + backward under autograd, us per call ({per} calls per bracket, {a.blocks} alternating brackets)")
    for k in fns:
        print(f"  {k:36s} median {statistics.median(t[k]):9.1f} us [{min(t[k]):9.1f} .. {max(t[k]):9.1f}]")


def build(size, batch, dtype, grad_diff_weight):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=dtype, static_prompts=True).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = cu.build_reference_criterion(dev, grad_diff_weight=grad_diff_weight)
    opt = train.make_optimizer(model, 0.0)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    for _ in range(2):                       # the flat layout, the workspaces: plain steps
        train.train_step(model, crit, opt, gb)
    return train.GraphedTrainStep(model, crit, opt, gb, prewarmed=True)


def steps(a, size):
    arms = {"default": build(size, a.batch, torch.bfloat16, None), "grad_diff_weight=1": build(size, a.batch, torch.bfloat16, 1.0)}
    for step in arms.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, step in arms.items():
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(a.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.steps)
    md = {k: statistics.median(v) for k, v in ms.items()}
    print(f"\n(c) bf16: ms per graph replay, {a.blocks} alternating blocks of {a.steps} replays")
    for k in arms:
        print(f"  {k:18s} median {md[k]:8.3f}   min {min(ms[k]):8.3f}   max {max(ms[k]):8.3f}   "
              f"vs default {md[k] - md['default']:+.3f} ms ({(md[k] / md['default'] - 1) * 100:+.2f} %)")
    print(f"  largest min-max spread between repeated blocks of one variant: {max(max(v) - min(v) for v in ms.values()):.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    size = (a.size,) * 3
    print(f"# grad_diff: {a.size}^3 x {a.batch}, {torch.cuda.get_device_name(0)}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            kernels(a, size, dtype, name)
        torch_composition(a, size)
        steps(a, size)
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


if __name__ == "__main__":
    main()
