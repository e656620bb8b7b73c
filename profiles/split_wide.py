"""A/B of the split mode against the wide split mode in ONE process: conv_algo=4 (the yardstick: its code is unchanged)
against conv_algo=5 (plus the stride-2 data gradients, the transposed up-convolutions and their weight gradients on the
split kernels) at 128^3 x 2, static prompts, learning rate 0, same initial state and batch.  The method is that of
split_vs_fp32.py, whose helpers it uses.

  python profiles/split_wide.py [--size 128] [--blocks 6] [--steps 20] [--eager 5] > profiles/split_wide.txt

Prints: forward rel-L2 of mode 5's output against mode 4's; median and min-max ms/step of both modes over ALTERNATING
blocks of graph-replayed steps; per launch in the new kernels' scope the per-launch HIP-event time (ops.KernelTimer, eager
steps; a forward's time includes its statistics pass when that is not fused) of the exact kernel under conv_algo=4 and the
new kernel under conv_algo=5, the difference against the larger min-max spread, and useful TFLOP/s (2 x MACs, not x 3).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from split_vs_fp32 import PEAK_BF16, build, eager_records, rel      # noqa: E402

NEW = ("conv_split_tconv_k", "conv_split_wgrad2_k")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--eager", type=int, default=5)
    a = ap.parse_args()
    from coma_unet_amd import train
    size = (a.size,) * 3
    arms = {algo: build(algo, size, a.batch) for algo in (4, 5)}
    print(f"# split_wide: {a.size}^3 x {a.batch}, fp32 storage, static prompts, lr 0, {torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        outs = {algo: train.forward_loss(m, c, gb)[1][0].float().clone() for algo, (m, c, _o, gb) in arms.items()}
    print(f"forward rel-L2, conv_algo=5 output against conv_algo=4 output: {rel(outs[5], outs[4]):.3e}")
    del outs

    recs = {algo: eager_records(*arms[algo], a.eager) for algo in (4, 5)}

    steps = {algo: train.GraphedTrainStep(m, c, o, gb, warmup=2) for algo, (m, c, o, gb) in arms.items()}
    for algo in (4, 5):
        for _ in range(3):
            steps[algo]()
    torch.cuda.synchronize()
    ms = {4: [], 5: []}
    for _ in range(a.blocks):
        for algo in (4, 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                steps[algo]()
            e1.record()
            torch.cuda.synchronize()
            ms[algo].append(e0.elapsed_time(e1) / a.steps)
    print(f"\nms/step, {a.blocks} alternating blocks of {a.steps} graph-replayed steps each:")
    for algo, name in ((4, "conv_algo=4 (split)"), (5, "conv_algo=5 (wide split)")):
        v = ms[algo]
        print(f"  {name:26s} median {statistics.median(v):7.3f}   min {min(v):7.3f}   max {max(v):7.3f}   blocks {' '.join(f'{t:.3f}' for t in v)}")
    m4, m5 = statistics.median(ms[4]), statistics.median(ms[5])
    spread = max(max(ms[4]) - min(ms[4]), max(ms[5]) - min(ms[5]))
    print(f"  step ratio (algo 4 / algo 5, medians): {m4 / m5:.3f}x; difference {m4 - m5:.3f} ms, larger block spread of the two arms {spread:.3f} ms"
          f" -> {'MET' if m4 - m5 > spread else 'NOT MET'}")

    print(f"\nper-launch HIP-event ms over {a.eager} eager steps (median [min .. max]); layer = (x shape, Cout, k, stride, form)")
    print(f"{'kind':11s} {'layer':42s} {'algo 4 kernel':28s} {'ms':>24s}   {'algo 5 kernel':24s} {'ms':>24s} {'ratio':>6s} {'diff':>7s} {'spread':>7s} {'':7s} {'TFLOP/s':>8s} {'of peak':>8s}")
    s4 = s5 = 0.0
    for key in sorted(recs[5], key=repr):
        n5, t5, fl = recs[5][key]
        if not n5.startswith(NEW) or key not in recs[4]:
            continue
        n4, t4, _ = recs[4][key]
        f = lambda t: f"{statistics.median(t):8.3f} [{min(t):6.3f} .. {max(t):6.3f}]"
        md4, md5 = statistics.median(t4), statistics.median(t5)
        sp = max(max(t4) - min(t4), max(t5) - min(t5))
        tf = fl / (md5 * 1e-3) / 1e12
        per_step = len(t5) / a.eager
        s4 += md4 * per_step; s5 += md5 * per_step
        print(f"{key[0]:11s} {str(key[1]):42s} {n4:28s} {f(t4)}   {n5:24s} {f(t5)} {md4 / md5:6.2f} {md4 - md5:7.3f} {sp:7.3f} "
              f"{'MET' if md4 - md5 > sp else 'NOT MET':7s} {tf:8.1f} {100 * tf * 1e12 / PEAK_BF16:7.1f}%")
    print(f"\nsummed over the launches above (medians): {s4:.3f} ms (algo 4) -> {s5:.3f} ms (algo 5) per step")
    other = sum(statistics.median(t) * len(t) / a.eager for k, (n, t, _) in recs[5].items() if not n.startswith("conv_split"))
    print(f"convolution launches outside every split kernel's scope under conv_algo=5: {other:.3f} ms per step")


if __name__ == "__main__":
    main()
