"""What the ROI-mean loss (criterions.RoiMeanLoss / WithRoiMean, csrc/roi_mean.hip) costs, in ONE process on one GPU,
alternating blocks, warm-up first (the method of roi_losses.py), at 128^3 x 2:

  (a) the kernels alone through the C ABI, fp32 and bf16: the forward (segmented reduction + finalise) and the backward, on
      dense volumes (the 4-voxels-per-lane path) and with pred / dpred at the 16-byte voxel pitch (the scalar path), on
      make_batch's block labels and on an independent random label per voxel (the peel loop's worst case), against
      coma_roi_wloss_fwd (kind WMSE) / coma_roi_wloss_bwd on the same tensors in the same brackets -- us per call and TB/s on
      algorithmic bytes per voxel: forward 12 fp32 / 8 bf16 (pred, gt, roi read once); backward roi_mean 8 / 6 (roi read,
      dpred written), roi_wloss 16 / 10;
  (b) the graph-replayed bf16 step (static prompts, learning rate 0) with and without roi_mean_weight.

  python profiles/roi_mean.py [--size 128] [--blocks 5] [--steps 8] > profiles/roi_mean.txt

Aims, recorded and not gated: the forward at 0.8 of roi_wloss fwd's rate in the same run on the same
layout; the backward not slower (in us) than roi_wloss bwd.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ev():
    return torch.cuda.Event(enable_timing=True)


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
    lab = torch.tensor([float(i) for i in ROI_INDICES] + [0.0, 2.0, 4999.0], device="cuda")
    rois = {"blocks": b["roi"].permute(0, 2, 3, 4, 1).contiguous().cuda(),
            "random": lab[torch.randint(0, lab.numel(), shape, generator=gen, device="cuda")]}
    ld = 16 // es
    pitched = torch.zeros((B, D, H, W, ld), dtype=dtype, device="cuda")[..., :1]
    pitched.copy_(dense)
    ids = torch.tensor(ROI_INDICES, dtype=torch.int32, device="cuda")
    w = torch.full((len(ROI_INDICES),), 225.0, device="cuda")
    loss, aux, gout = (torch.ones(B, device="cuda") for _ in range(3))
    coef = torch.ones((B, ids.numel()), device="cuda")
    ws = torch.empty(max(lib.coma_roi_wloss_ws_bytes(ct(dense)), lib.coma_roi_mean_ws_bytes(ct(dense))), dtype=torch.uint8, device="cuda")
    s = L.stream()
    fns, keep = {}, []
    for lay, pred in (("dense", dense), ("pitched", pitched)):
        for pat, roi in rois.items():
            dp = torch.empty_like(dense) if lay == "dense" else torch.zeros((B, D, H, W, ld), dtype=dtype, device="cuda")[..., :1]
            cp, cg, cr, cd = ct(pred), ct(gt), ct(roi), ct(dp)
            key = f"{lay} {pat}"
            fns[f"{key} roi_wloss fwd"] = (2 * es + 4, lambda cp=cp, cr=cr: L.check(lib.coma_roi_wloss_fwd(
                cp, cg, cr, ptr(ids), ptr(w), ids.numel(), 1.0, 0, ptr(loss), ptr(aux), ptr(ws), ws.numel(), s), "roi_wloss_fwd"))
            fns[f"{key} roi_mean  fwd"] = (2 * es + 4, lambda cp=cp, cr=cr: L.check(lib.coma_roi_mean_fwd(
                cp, cg, cr, ptr(ids), ptr(w), ids.numel(), 0, 1.0, ptr(loss), ptr(coef), ptr(ws), ws.numel(), s), "roi_mean_fwd"))
            fns[f"{key} roi_wloss bwd"] = (3 * es + 4, lambda cp=cp, cr=cr, cd=cd: L.check(lib.coma_roi_wloss_bwd(
                cp, cg, cr, ptr(ids), ptr(w), ids.numel(), 1.0, ptr(gout), ptr(aux), cd, s), "roi_wloss_bwd"))
            fns[f"{key} roi_mean  bwd"] = (es + 4, lambda cr=cr, cd=cd: L.check(lib.coma_roi_mean_bwd(
                cr, ptr(ids), ids.numel(), ptr(gout), ptr(coef), cd, s), "roi_mean_bwd"))
            keep.append(dp)                  # (the descriptors hold raw pointers)
    for _, fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    per = 20
    t = {k: [] for k in fns}
    for _ in range(a.blocks):
        for k, (_, fn) in fns.items():
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(per):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / per)
    med = {k: statistics.median(v) for k, v in t.items()}
    rate = {k: fns[k][0] * V / (med[k] * 1e-6) / 1e12 for k in fns}
    print(f"\n(a) {name}: kernels alone, {B} x {D}x{H}x{W}; us per call ({per} calls per bracket, {a.blocks} alternating brackets; a forward "
          f"call is the reduction and its finalise); TB/s on algorithmic bytes")
    for k in fns:
        print(f"  {k:30s} {fns[k][0]:3d} B/voxel  median {med[k]:8.2f} us [{min(t[k]):8.2f} .. {max(t[k]):8.2f}]  {rate[k]:6.3f} TB/s")
    for lay in ("dense", "pitched"):
        for pat in rois:
            key = f"{lay} {pat}"
            r = rate[f"{key} roi_mean  fwd"] / rate[f"{key} roi_wloss fwd"]
            print(f"  {key:16s} fwd rate / roi_wloss fwd rate = {r:5.2f}  (aim 0.8: {'MET' if r >= 0.8 else 'NOT MET'})")
            r = med[f"{key} roi_mean  bwd"] / med[f"{key} roi_wloss bwd"]
            print(f"  {key:16s} bwd time / roi_wloss bwd time = {r:5.2f}  (aim <= 1: {'MET' if r <= 1.0 else 'NOT MET'})")


def build(size, batch, dtype, roi_mean_weight):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=dtype, static_prompts=True).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = cu.build_reference_criterion(dev, roi_mean_weight=roi_mean_weight)
    opt = train.make_optimizer(model, 0.0)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    for _ in range(2):                       # the flat layout, the workspaces: plain steps
        train.train_step(model, crit, opt, gb)
    return train.GraphedTrainStep(model, crit, opt, gb, prewarmed=True)


def steps(a, size):
    arms = {"default": build(size, a.batch, torch.bfloat16, None), "roi_mean_weight=1": build(size, a.batch, torch.bfloat16, 1.0)}
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
    print(f"\n(b) bf16: ms per graph replay, {a.blocks} alternating blocks of {a.steps} replays")
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
    print(f"# roi_mean: {a.size}^3 x {a.batch}, {torch.cuda.get_device_name(0)}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            kernels(a, size, dtype, name)
        steps(a, size)
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


if __name__ == "__main__":
    main()
