"""What the ROI-weighted losses (criterions.RoiWeightedMSE / RoiRSE / RoiRRMSE, csrc/roi_loss.hip) cost, in ONE process on one
GPU, alternating blocks, warm-up first (the method of ema.py / ssim_loss.py), at 128^3 x 2:

  (a) the kernels alone through the C ABI, fp32 and bf16: the forward (reduction + finalise) of each kind and the backward,
      on dense volumes (the 4-voxels-per-lane path) and with pred / dpred at the 16-byte voxel pitch the model's prediction
      has (the scalar path), against coma_roi_mse_fwd / coma_roi_mse_bwd in the same brackets -- us per call and TB/s on
      algorithmic bytes per voxel: forward 12 fp32 / 8 bf16 (pred, gt, roi read once), backward 16 / 10 (+ dpred written;
      roi_mse's backward does not read roi: 12 / 6);
  (b) the graph-replayed bf16 step (static prompts, learning rate 0) with each new loss against the RoiMSE step.

  python profiles/roi_losses.py [--size 128] [--blocks 5] [--steps 8] > profiles/roi_losses.txt

Aim, recorded and not gated: 0.9 of the roi_mse kernels' rate in the same run on the same layout; the
vector path should exceed it.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = (("wmse", 0), ("rse", 1), ("rrmse", 2))


def ev():
    return torch.cuda.Event(enable_timing=True)


def kernels(a, size, dtype, name):
    from coma_unet_amd import _lib as L
    from coma_unet_amd.roi_tables import ROI_INDICES
    lib, ct, ptr = L.lib, L.ct, L.ptr
    B, (D, H, W) = a.batch, size
    V = B * D * H * W
    es = 2 if dtype == torch.bfloat16 else 4
    gen = torch.Generator(device="cuda").manual_seed(0)
    shape = (B, D, H, W, 1)
    gt = torch.rand(shape, generator=gen, device="cuda")
    dense = (gt + 0.1 * torch.randn(shape, generator=gen, device="cuda")).to(dtype)
    gt = gt.to(dtype)
    lab = torch.tensor([float(i) for i in ROI_INDICES] + [0.0] * 12, device="cuda")
    roi = lab[torch.randint(0, lab.numel(), shape, generator=gen, device="cuda")]
    ld = 16 // es
    pitched = torch.zeros((B, D, H, W, ld), dtype=dtype, device="cuda")[..., :1]
    pitched.copy_(dense)
    ids = torch.tensor(ROI_INDICES, dtype=torch.int32, device="cuda")
    w = torch.full((len(ROI_INDICES),), 225.0, device="cuda")
    loss, aux, gout = (torch.ones(B, device="cuda") for _ in range(3))
    ws = torch.empty(max(lib.coma_roi_wloss_ws_bytes(ct(dense)), lib.coma_loss_ws_bytes(ct(dense))), dtype=torch.uint8, device="cuda")
    s = L.stream()
    fns, keep = {}, []
    for lay, pred in (("dense", dense), ("pitched", pitched)):
        dp = torch.empty_like(dense) if lay == "dense" else torch.zeros((B, D, H, W, ld), dtype=dtype, device="cuda")[..., :1]
        cp, cg, cr, cd = ct(pred), ct(gt), ct(roi), ct(dp)
        fns[f"{lay} roi_mse fwd"] = (2 * es + 4, lambda cp=cp: L.check(lib.coma_roi_mse_fwd(
            cp, cg, cr, ptr(ids), ptr(w), ids.numel(), ptr(loss), ptr(aux), ptr(ws), ws.numel(), s), "roi_mse_fwd"))
        for kn, kind in KINDS:
            fns[f"{lay} roi_wloss fwd {kn}"] = (2 * es + 4, lambda cp=cp, kind=kind: L.check(lib.coma_roi_wloss_fwd(
                cp, cg, cr, ptr(ids), ptr(w), ids.numel(), 1.0, kind, ptr(loss), ptr(aux), ptr(ws), ws.numel(), s), "roi_wloss_fwd"))
        fns[f"{lay} roi_mse bwd"] = (3 * es, lambda cp=cp, cd=cd: L.check(lib.coma_roi_mse_bwd(
            cp, cg, ptr(gout), ptr(aux), cd, s), "roi_mse_bwd"))
        fns[f"{lay} roi_wloss bwd"] = (3 * es + 4, lambda cp=cp, cd=cd: L.check(lib.coma_roi_wloss_bwd(
            cp, cg, cr, ptr(ids), ptr(w), ids.numel(), 1.0, ptr(gout), ptr(aux), cd, s), "roi_wloss_bwd"))
        keep.append(dp)                      # (the descriptors hold raw pointers)
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
        print(f"  {k:28s} {fns[k][0]:3d} B/voxel  median {med[k]:8.2f} us [{min(t[k]):8.2f} .. {max(t[k]):8.2f}]  {rate[k]:6.3f} TB/s")
    for lay in ("dense", "pitched"):
        for kn, _ in KINDS:
            r = rate[f"{lay} roi_wloss fwd {kn}"] / rate[f"{lay} roi_mse fwd"]
            print(f"  {lay:8s} fwd {kn:5s} rate / roi_mse fwd rate = {r:5.2f}  (aim 0.9: {'MET' if r >= 0.9 else 'NOT MET'})")
        r = rate[f"{lay} roi_wloss bwd"] / rate[f"{lay} roi_mse bwd"]
        print(f"  {lay:8s} bwd       rate / roi_mse bwd rate = {r:5.2f}  (aim 0.9: {'MET' if r >= 0.9 else 'NOT MET'})")


def build(size, batch, dtype, gen_loss):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=dtype, static_prompts=True).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = cu.build_reference_criterion(dev, gen_loss=gen_loss)
    opt = train.make_optimizer(model, 0.0)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    for _ in range(2):                       # the flat layout, the workspaces: plain steps
        train.train_step(model, crit, opt, gb)
    return train.GraphedTrainStep(model, crit, opt, gb, prewarmed=True)


def steps(a, size):
    arms = {k: build(size, a.batch, torch.bfloat16, k) for k in ("roi_mse", "roi_wmse", "roi_rse", "roi_rrmse")}
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
        print(f"  gen_loss={k:10s} median {md[k]:8.3f}   min {min(ms[k]):8.3f}   max {max(ms[k]):8.3f}   "
              f"vs roi_mse {md[k] - md['roi_mse']:+.3f} ms ({(md[k] / md['roi_mse'] - 1) * 100:+.2f} %)")
    print(f"  largest min-max spread between repeated blocks of one variant: {max(max(v) - min(v) for v in ms.values()):.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    size = (a.size,) * 3
    print(f"# roi_losses: {a.size}^3 x {a.batch}, {torch.cuda.get_device_name(0)}")
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
