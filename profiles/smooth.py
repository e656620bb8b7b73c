"""What smoothing the tau target costs, in ONE process on one GPU, alternating blocks, warm-up first (the method of ema.py):

  (a) gauss_smooth_k alone at 128^3 x 2 and at 192 x 224 x 192 x 1 in three variants -- the reference preset (in-plane, radius 4),
      the full 3-D radius-4 filter, and the reference preset on the fused resample source (one volume per launch, as
      prepare_sample calls it) -- in us per launch and TB/s on ALGORITHMIC bytes (8 per voxel: read once, written once), beside
      resample_nn_k in the same run (one volume per launch, 8 bytes per voxel), and beside what a user would otherwise write on
      the device: the separable F.conv3d passes in fp32 (two passes for the preset, three for the 3-D filter);
  (b) the graph-replayed bf16 step at 128^3 x 2 (static prompts, lr 0), loading the batch into the graph's static inputs every
      step, without and with smooth_tau in front (train_dp's order: smooth, then the graph load) -- ms per step.

  python profiles/smooth.py [--blocks 6] [--steps 12] > profiles/smooth.txt

No threshold is fixed in advance: the aim is to beat the ATen passes; the ratio is recorded either way.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from profiles.ema import build, ev, fmt  # noqa: E402


def aten_passes(taps_zyx):
    """The separable filter as zero-padded F.conv3d passes in the kernel's order x, y, z."""
    ks = []
    for axis, w in zip((2, 1, 0), (taps_zyx[2], taps_zyx[1], taps_zyx[0])):
        if w is None:
            continue
        shape, pad = [1, 1, 1, 1, 1], [0, 0, 0]
        shape[2 + axis], pad[axis] = len(w), len(w) // 2
        ks.append((torch.tensor(w, dtype=torch.float32, device="cuda").view(shape), tuple(pad)))

    def run(v):
        for k, pad in ks:
            v = F.conv3d(v, k, padding=pad)
        return v
    return run


def kernels(shape, batch, blocks, per=20):
    from coma_unet_amd import input_pipeline as P
    from coma_unet_amd.smooth import GaussianSmooth3D
    D, H, W = shape
    V = D * H * W
    vol = torch.rand((batch, 1, D, H, W), device="cuda")
    out = torch.empty_like(vol)
    src, dst = vol[0, 0].contiguous(), torch.empty(shape, device="cuda")
    ref, full = GaussianSmooth3D.reference(), GaussianSmooth3D(sigma=1.0, axes=("z", "y", "x"))
    aten_ref, aten_full = aten_passes(ref.taps), aten_passes(full.taps)
    err = float((aten_full(vol) - full(vol)).abs().max())

    def resample():
        P.check(P.lib.coma_resample_nearest(P.ptr(src), D, H, W, 1.0, 1.0, 1.0, P.ptr(dst), D, H, W, 1.0, 1.0, 1.0, 0.0, 1, None, P.L.stream()),
                "coma_resample_nearest")

    fns = {
        "resample_nn_k (yardstick, 1 volume)": (8 * V, resample),
        "smooth, reference preset": (8 * V * batch, lambda: ref(vol, out=out)),
        "ATen, 2 conv3d passes": (8 * V * batch, lambda: aten_ref(vol)),
        "smooth, 3-D radius 4": (8 * V * batch, lambda: full(vol, out=out)),
        "ATen, 3 conv3d passes": (8 * V * batch, lambda: aten_full(vol)),
        "smooth, preset, fused source (1 volume)": (8 * V, lambda: ref.resampled(src, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), size_xyz=(W, H, D))),
    }
    for _, fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(blocks):
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
    base = rate["resample_nn_k (yardstick, 1 volume)"]
    print(f"\n(a) {D} x {H} x {W} x {batch}: us per launch ({per} launches per bracket, {blocks} alternating brackets); TB/s on algorithmic bytes; "
          f"ratio to resample_nn_k's rate of this run.  (The fused-source and ATen arms allocate their output per call.)")
    for k, (by, _) in fns.items():
        print(f"  {k:42s} {by / 1e6:7.1f} MB  median {med[k]:8.2f} us [{min(t[k]):8.2f} .. {max(t[k]):8.2f}]  {rate[k]:5.2f} TB/s  x{rate[k] / base:4.2f}")
    for ours, theirs in (("smooth, reference preset", "ATen, 2 conv3d passes"), ("smooth, 3-D radius 4", "ATen, 3 conv3d passes")):
        r = med[theirs] / med[ours]
        print(f"  {ours} vs {theirs}: x{r:.2f} -> {'FASTER' if r > 1 else 'SLOWER'} than the ATen passes")
    print(f"  (max abs difference between the 3-D kernel and the ATen passes on this volume: {err:.2e})")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    from coma_unet_amd import synthetic
    from coma_unet_amd.smooth import GaussianSmooth3D
    print(f"# smooth: {torch.cuda.get_device_name(0)}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        med = kernels((128, 128, 128), 2, a.blocks)
        kernels((192, 224, 192), 1, a.blocks)
        if not a.no_step:
            size, batch = (128, 128, 128), 2
            b = synthetic.make_batch(batch, size, seed=1000)
            mri, tau, roi = (b[k].cuda() for k in ("mri", "tau", "roi"))
            g = GaussianSmooth3D.reference()
            step, _opt = build(size, batch, None)

            def off():
                step({"mri": mri, "tau": tau, "roi": roi})

            def on():
                step({"mri": mri, "tau": g(tau), "roi": roi})

            arms = {"smooth_tau=None (today)": off, "smooth_tau=True": on}
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
            print(f"\n(b) ms per graph-replayed step (bf16, static prompts, lr 0, 128^3 x 2), {a.blocks} alternating blocks of {a.steps} steps; both "
                  f"arms copy the batch into the graph's inputs, 'True' smooths tau first:")
            for k in arms:
                print(f"  {k:28s} {fmt(ms[k])}")
            md = {k: statistics.median(v) for k, v in ms.items()}
            spread = max(max(v) - min(v) for v in ms.values())
            print(f"  True - None: {md['smooth_tau=True'] - md['smooth_tau=None (today)']:+.3f} ms "
                  f"({(md['smooth_tau=True'] / md['smooth_tau=None (today)'] - 1) * 100:+.2f} %); kernel alone (a): "
                  f"{med['smooth, reference preset'] * 1e-3:.3f} ms; largest min-max spread between repeated blocks of one arm: {spread:.3f} ms")
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


if __name__ == "__main__":
    main()
