"""What Augment3D costs, in ONE process on one GPU, alternating blocks, warm-up first (the method of ema.py):

  (a) augment_warp_k alone at 128^3 x 2 in three variants -- affine only, affine + a 4^3 elastic grid, the same + noise -- in us
      per launch and TB/s on ALGORITHMIC bytes (24 per voxel: three fp32 volumes read once and written once), beside
      resample_nn_k in the same run at its 8 bytes per voxel (one 128^3 volume per launch, as the input pipeline calls it);
  (b) the graph-replayed bf16 step at 128^3 x 2 (static prompts, lr 0), loading the batch into the graph's static inputs
      every step, without and with the warp in front -- ms per step.

  python profiles/augment.py [--size 128] [--blocks 6] [--steps 12] > profiles/augment.txt

Aim (a guess about how well 17 gathers per voxel share cache lines, not a gate): the warp at >= 0.5 of resample_nn_k's
algorithmic bytes/s of the same run.  (b): on - off should be the kernel time plus nothing beyond the block-to-block spread.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from profiles.ema import build, ev, fmt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=12)
    a = ap.parse_args()
    from coma_unet_amd import input_pipeline as P, synthetic
    from coma_unet_amd.augment import Augment3D, warp
    size = (a.size,) * 3
    V = a.size ** 3
    print(f"# augment: {a.size}^3 x {a.batch}, {torch.cuda.get_device_name(0)}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = synthetic.make_batch(a.batch, size, seed=1000)
        mri, tau, roi = (b[k].cuda() for k in ("mri", "tau", "roi"))
        out = tuple(torch.empty_like(t) for t in (mri, tau, roi))
        aug = Augment3D(rotate_deg=10.0, scale=(0.9, 1.1), translate_vox=4.0, elastic_grid=(4, 4, 4), elastic_sigma_vox=2.0, seed=0)
        params, disp = aug.sample_params(a.batch, size)
        noisy = params.copy()
        noisy[:, 15] = 0.02
        dev = lambda x: torch.from_numpy(x).cuda()
        p_aff, p_noise, d_el = dev(params), dev(noisy), dev(disp)
        src, dst = mri[0, 0].contiguous(), torch.empty(size, device="cuda")

        def resample():
            P.check(P.lib.coma_resample_nearest(P.ptr(src), *size, 1.0, 1.0, 1.0, P.ptr(dst), *size, 1.0, 1.0, 1.0, 0.0, 1, None, P.L.stream()),
                    "coma_resample_nearest")

        fns = {
            "resample_nn_k (yardstick)": (8 * V, resample),
            "warp, affine": (24 * V * a.batch, lambda: warp(mri, tau, roi, p_aff, None, 1, out)),
            "warp, affine + 4^3 elastic": (24 * V * a.batch, lambda: warp(mri, tau, roi, p_aff, d_el, 1, out)),
            "warp, affine + elastic + noise": (24 * V * a.batch, lambda: warp(mri, tau, roi, p_noise, d_el, 1, out)),
        }
        for _, fn in fns.values():
            for _ in range(3):
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
                t[k].append(e0.elapsed_time(e1) / per * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        rate = {k: by / (med[k] * 1e-6) / 1e12 for k, (by, _) in fns.items()}
        base = rate["resample_nn_k (yardstick)"]
        print(f"\n(a) kernels alone, us per launch ({per} launches per bracket, {a.blocks} alternating brackets); TB/s on algorithmic bytes; "
              f"ratio to resample_nn_k's rate of this run")
        for k, (by, _) in fns.items():
            print(f"  {k:32s} {by / 1e6:7.1f} MB  median {med[k]:8.2f} us [{min(t[k]):8.2f} .. {max(t[k]):8.2f}]  {rate[k]:5.2f} TB/s  "
                  f"x{rate[k] / base:4.2f}")
        for k in list(fns)[1:]:
            r = rate[k] / base
            print(f"aim: {k} at >= 0.5 of resample_nn_k's bytes/s: x{r:.3f} -> {'MET' if r >= 0.5 else 'NOT MET'}")
        foreground = float((roi != 0).float().mean())
        print(f"(foreground share of the synthetic ROI volume: {foreground:.2f}; the MRI gathers, the intensity map and the noise are "
              f"skipped on background voxels)")

        # ---- (b) the graph-replayed step, batch loaded every step ----
        step, _opt = build(size, a.batch, None)
        plain = {"mri": mri, "tau": tau, "roi": roi}
        statics = (step.batch["mri"], step.batch["tau"], step.batch["roi"])

        def off():
            step(plain)

        def on():
            aug(mri, tau, roi, out=statics)          # draws on the host, one launch straight into the graph's inputs
            step()

        def on_fixed():
            warp(mri, tau, roi, p_aff, d_el, 1, statics)
            step()

        arms = {"augment=None (today)": off, "augment, fresh draw per step": on, "augment, fixed parameters": on_fixed}
        for fn in arms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(a.blocks):
            for k, fn in arms.items():
                e0, e1 = ev(), ev()
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.steps)
        print(f"\n(b) ms per graph-replayed step (bf16, static prompts, lr 0), {a.blocks} alternating blocks of {a.steps} steps; 'None' "
              f"copies the batch into the graph's inputs, the augmenting arms write it there with the warp:")
        for k in arms:
            print(f"  {k:32s} {fmt(ms[k])}")
        md = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        k0 = "augment=None (today)"
        for k in list(arms)[1:]:
            print(f"  {k} - None: {md[k] - md[k0]:+.3f} ms ({(md[k] / md[k0] - 1) * 100:+.2f} %)")
        print(f"  kernel alone (a): {med['warp, affine + 4^3 elastic'] * 1e-3:.3f} ms; largest min-max spread between repeated blocks of one "
              f"variant: {spread:.3f} ms")
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


if __name__ == "__main__":
    main()
