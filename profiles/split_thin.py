"""A/B of the wide split mode against the thin split mode in ONE process: conv_algo=5 (the yardstick: its code is unchanged)
against conv_algo=6 (plus the few-channel full-resolution layers -- C <= 16: the modulator tails, the 1 -> 32 head
convolution, their data and weight gradients -- on conv_split_thin_k / conv_split_thin_wgrad_k) at 128^3 x 2, static prompts,
learning rate 0, same initial state and batch.  The method is that of split_vs_fp32.py, whose helpers it uses.

  python profiles/split_thin.py [--size 128] [--blocks 6] [--steps 20] [--eager 5] > profiles/split_thin.txt

Prints: forward rel-L2 of mode 6's output against mode 0's (exact fp32) and against mode 5's; median and min-max ms/step of
modes 5 and 6 over ALTERNATING blocks of graph-replayed steps; per thin launch of the step the per-launch HIP-event time
(ops.KernelTimer, eager steps; a forward's time includes its statistics pass when that is not fused, a weight gradient's its
memset and replica sum) of the exact kernel under conv_algo=5 and the new kernel under conv_algo=6, the difference against the
larger min-max spread (MET: the difference of the medians exceeds it), and useful TFLOP/s (2 x MACs, not x 3).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from split_vs_fp32 import PEAK_BF16, build, eager_records, rel      # noqa: E402

OLD = ("conv_thin16f_k", "conv_thin16f_wgrad_k")
NEW = ("conv_split_thin_k", "conv_split_thin_wgrad_k")


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
    print(f"# split_thin: {a.size}^3 x {a.batch}, fp32 storage, static prompts, lr 0, {torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        m0, c0, _o, gb0 = build(0, size, a.batch)
        out0 = train.forward_loss(m0, c0, gb0)[1][0].float().clone()
        del m0, c0, _o, gb0
    arms = {algo: build(algo, size, a.batch) for algo in (5, 6)}
    with torch.no_grad():
        outs = {algo: train.forward_loss(m, c, gb)[1][0].float().clone() for algo, (m, c, _o, gb) in arms.items()}
    print(f"forward rel-L2, conv_algo=6 output against conv_algo=0 output: {rel(outs[6], out0):.3e}")
    print(f"forward rel-L2, conv_algo=5 output against conv_algo=0 output: {rel(outs[5], out0):.3e}")
    print(f"forward rel-L2, conv_algo=6 output against conv_algo=5 output: {rel(outs[6], outs[5]):.3e}")
    del outs, out0

    recs = {algo: eager_records(*arms[algo], a.eager) for algo in (5, 6)}

    steps = {algo: train.GraphedTrainStep(m, c, o, gb, warmup=2) for algo, (m, c, o, gb) in arms.items()}
    for algo in (5, 6):
        for _ in range(3):
            steps[algo]()
    torch.cuda.synchronize()
    ms = {5: [], 6: []}
    for _ in range(a.blocks):
        for algo in (5, 6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                steps[algo]()
            e1.record()
            torch.cuda.synchronize()
            ms[algo].append(e0.elapsed_time(e1) / a.steps)
    print(f"\nms/step, {a.blocks} alternating blocks of {a.steps} graph-replayed steps each:")
    for algo, name in ((5, "conv_algo=5 (wide split)"), (6, "conv_algo=6 (thin split)")):
        v = ms[algo]
        print(f"  {name:26s} median {statistics.median(v):7.3f}   min {min(v):7.3f}   max {max(v):7.3f}   blocks {' '.join(f'{t:.3f}' for t in v)}")
    m5, m6 = statistics.median(ms[5]), statistics.median(ms[6])
    spread = max(max(ms[5]) - min(ms[5]), max(ms[6]) - min(ms[6]))
    print(f"  step ratio (algo 5 / algo 6, medians): {m5 / m6:.3f}x; difference {m5 - m6:.3f} ms, larger block spread of the two arms {spread:.3f} ms"
          f" -> {'MET' if m5 - m6 > spread else 'NOT MET'}")

    print(f"\nper-launch HIP-event ms over {a.eager} eager steps (median [min .. max]); layer = (x shape, Cout, k, stride, form)")
    print(f"{'kind':11s} {'layer':40s} {'algo 5 kernel':30s} {'ms':>24s}   {'algo 6 kernel':34s} {'ms':>24s} {'ratio':>6s} {'diff':>7s} {'spread':>7s} {'':7s} {'TFLOP/s':>8s} {'of peak':>8s}")
    s5 = s6 = 0.0
    for key in sorted(recs[5], key=repr):
        n5, t5, fl = recs[5][key]
        if not n5.startswith(OLD) or key not in recs[6]:
            continue
        n6, t6, _ = recs[6][key]
        f = lambda t: f"{statistics.median(t):8.3f} [{min(t):6.3f} .. {max(t):6.3f}]"
        md5, md6 = statistics.median(t5), statistics.median(t6)
        sp = max(max(t5) - min(t5), max(t6) - min(t6))
        tf = fl / (md6 * 1e-3) / 1e12
        per_step = len(t6) / a.eager
        s5 += md5 * per_step; s6 += md6 * per_step
        verdict = ("MET" if md5 - md6 > sp else "NOT MET") if n6.startswith(NEW) else "(exact)"
        print(f"{key[0]:11s} {str(key[1]):40s} {n5:30s} {f(t5)}   {n6:34s} {f(t6)} {md5 / md6:6.2f} {md5 - md6:7.3f} {sp:7.3f} "
              f"{verdict:7s} {tf:8.1f} {100 * tf * 1e12 / PEAK_BF16:7.1f}%")
    print(f"\nsummed over the launches above (medians): {s5:.3f} ms (algo 5) -> {s6:.3f} ms (algo 6) per step")
    other = sum(statistics.median(t) * len(t) / a.eager for k, (n, t, _) in recs[6].items() if not n.startswith("conv_split"))
    print(f"convolution launches outside every split kernel's scope under conv_algo=6: {other:.3f} ms per step")


if __name__ == "__main__":
    main()
