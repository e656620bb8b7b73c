"""What the SSIM training loss (criterions.WithSSIM, train_dp(ssim_weight=...)) costs, in ONE process on one GPU, alternating
blocks, warm-up first (the method of ema.py / grad_accum.py), at 128^3 x 2 in bf16 and in fp32:

  (a) the graph-replayed step (static prompts, learning rate 0) without and with ssim_weight -- ms per replay;
  (b) the kernels alone through the C ABI: ssim_partial_k (the metric kernel), its coefficient-writing variant
      ssim_partial_k<T, true> and ssim_bwd_k -- ms per launch, and GB/s on algorithmic bytes (x, y read once, 12 B of
      coefficients per valid voxel written / read once, dx written once).

  python profiles/ssim_loss.py [--size 128] [--blocks 5] [--steps 8] > profiles/ssim_loss.txt

Expectations, recorded and not gated (DESIGN.md section 4 "SSIM loss"): ssim_bwd_k convolves 3 quantities over the cube
extents the forward kernel convolves 5 over, so it should not take longer than the forward kernel of the same run; the
coefficient-writing forward should stay within the time its extra 12 B per valid voxel of stores cost.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WEIGHT = 20.0


def build(size, batch, dtype, ssim_weight):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    from coma_unet_amd.train_loop import with_ssim
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=dtype, static_prompts=True).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = with_ssim(cu.build_reference_criterion(), ssim_weight)
    opt = train.make_optimizer(model, 0.0)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    for _ in range(2):                       # the flat layout, the workspaces: plain steps
        train.train_step(model, crit, opt, gb)
    return train.GraphedTrainStep(model, crit, opt, gb, prewarmed=True)


def ev():
    return torch.cuda.Event(enable_timing=True)


def fmt(v):
    return f"median {statistics.median(v):8.3f}   min {min(v):8.3f}   max {max(v):8.3f}   blocks {' '.join(f'{t:.3f}' for t in v)}"


def steps(a, size, dtype, name):
    arms = {"off": build(size, a.batch, dtype, None), "on": build(size, a.batch, dtype, WEIGHT)}
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
    spread = max(max(v) - min(v) for v in ms.values())
    print(f"\n(a) {name}: ms per graph replay, {a.blocks} alternating blocks of {a.steps} replays")
    print(f"  ssim_weight=None (today)  {fmt(ms['off'])}")
    print(f"  ssim_weight={WEIGHT:<5g}         {fmt(ms['on'])}")
    print(f"  on - off: {md['on'] - md['off']:+.3f} ms ({(md['on'] / md['off'] - 1) * 100:+.2f} %); largest min-max spread between "
          f"repeated blocks of one variant: {spread:.3f} ms")
    del arms
    torch.cuda.empty_cache()
    return md["on"] - md["off"]


def kernels(a, size, dtype, name):
    from coma_unet_amd import _lib as L
    from coma_unet_amd.metrics import ssim_window
    lib, ct, ptr = L.lib, L.ct, L.ptr
    B, (D, H, W), win = a.batch, size, 11
    gen = torch.Generator(device="cuda").manual_seed(0)
    y = torch.rand((B, D, H, W, 1), generator=gen, device="cuda")
    x = (y + 0.1 * torch.randn((B, D, H, W, 1), generator=gen, device="cuda")).clamp(0, 1).to(dtype)
    y = y.to(dtype)
    dx = torch.empty_like(x)
    w = ssim_window("gaussian", win, 1.5)
    wp = w.ctypes.data_as(ctypes.c_void_p)
    cx, cy, cdx = ct(x), ct(y), ct(dx)
    nbytes, cbytes = lib.coma_ssim_ws_bytes(cx, win), lib.coma_ssim_coef_bytes(cx, win)
    part = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    coef = torch.empty(cbytes // 4, dtype=torch.float32, device="cuda")
    gout = torch.ones(B, device="cuda")
    nt = ctypes.c_int32(0)
    c1, c2 = 1e-4, 9e-4
    es, V = x.element_size(), B * D * H * W
    fns = {
        "ssim_partial_k (metric)": (2 * V * es, lambda: L.check(lib.coma_ssim_partial(
            cx, cy, wp, win, c1, c2, ptr(part), nbytes, ctypes.addressof(nt), L.stream()), "ssim_partial")),
        "ssim_partial_k<T, true>": (2 * V * es + cbytes, lambda: L.check(lib.coma_ssim_fwd_coef(
            cx, cy, wp, win, c1, c2, ptr(part), nbytes, ctypes.addressof(nt), ptr(coef), cbytes, L.stream()), "ssim_fwd_coef")),
        "ssim_bwd_k": (3 * V * es + cbytes, lambda: L.check(lib.coma_ssim_bwd(
            cx, cy, ptr(coef), wp, win, ptr(gout), cdx, L.stream()), "ssim_bwd")),
    }
    for k in ("ssim_partial_k<T, true>", "ssim_partial_k (metric)", "ssim_bwd_k"):      # (coef is written before it is read)
        fns[k][1]()
    torch.cuda.synchronize()
    per = 10
    t = {k: [] for k in fns}
    for _ in range(a.blocks):
        for k, (_, fn) in fns.items():
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(per):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) / per)
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"\n(b) {name}: kernels alone, {B} x {D}x{H}x{W}, window {win}, coefficient maps {cbytes / 1e6:.1f} MB; ms per launch "
          f"({per} launches per bracket, {a.blocks} alternating brackets); GB/s on algorithmic bytes")
    for k, (by, _) in fns.items():
        print(f"  {k:26s} {by / 1e6:7.1f} MB  median {med[k]:7.4f} ms [{min(t[k]):7.4f} .. {max(t[k]):7.4f}]  "
              f"{by / (med[k] * 1e-3) / 1e9:7.1f} GB/s")
    f, fc, bw = med["ssim_partial_k (metric)"], med["ssim_partial_k<T, true>"], med["ssim_bwd_k"]
    print(f"  expectation 1: ssim_bwd_k no longer than the forward kernel of this run: {bw:.4f} ms vs {f:.4f} ms (metric) / "
          f"{fc:.4f} ms (coefficient-writing) -> {'MET' if bw <= fc else 'NOT MET'}")
    print(f"  expectation 2: coefficient-writing forward - metric forward = {fc - f:+.4f} ms for {cbytes / 1e6:.1f} MB of stores "
          f"({cbytes / max(fc - f, 1e-9) / 1e6:.0f} GB/s if that were all store time)")
    return fc + bw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    size = (a.size,) * 3
    print(f"# ssim_loss: {a.size}^3 x {a.batch}, static prompts, lr 0, graph replay, ssim_weight {WEIGHT}, gaussian-11, "
          f"{torch.cuda.get_device_name(0)}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            d_step = steps(a, size, dtype, name)
            d_kern = kernels(a, size, dtype, name)
            print(f"  {name}: step on - off {d_step:+.3f} ms; the two SSIM-loss kernels alone {d_kern:.3f} ms (the metric-free step "
                  f"also gains the second gradient's add into d pred and the (B, tiles) reductions)")
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


if __name__ == "__main__":
    main()
