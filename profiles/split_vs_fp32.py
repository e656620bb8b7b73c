"""A/B of the two fp32-storage modes in ONE process: conv_algo=0 (exact fp32, v_mfma_f32_32x32x2_f32) against conv_algo=4
(split-bf16, csrc/conv_split.hip) at 128^3 x 2, static prompts, learning rate 0, same initial state and batch.

  python profiles/split_vs_fp32.py [--size 128] [--blocks 6] [--steps 20] [--eager 5] > profiles/split_vs_fp32.txt

Prints: forward rel-L2 of mode 4's output against mode 0's; median and min-max ms/step of both modes over ALTERNATING
blocks of graph-replayed steps (HIP events around each block); per layer of the split kernels' scope the per-launch
HIP-event time (ops.KernelTimer, eager steps) of the old and the new kernel; TFLOP/s of the new kernels counted as
USEFUL FLOPs (2 x MACs of the convolution, not x 3) and their share of the 2.5 PFLOP/s dense bf16 peak.
bench.py knows the bf16 and exact-fp32 modes only; the conv_algo=0 arm here is its fp32 step.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PEAK_BF16 = 2.5e15


def build(algo, size, batch):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=torch.float32, static_prompts=True, conv_algo=algo).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = cu.build_reference_criterion()
    opt = train.make_optimizer(model, 0.0)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    return model, crit, opt, gb


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def eager_records(model, crit, opt, gb, n):
    """{(kind, tag): (kernel name, [ms per launch over n eager steps], flops)}"""
    from coma_unet_amd import ops, train
    KT = ops.KernelTimer
    out = {}
    for _ in range(n):
        KT.enabled, KT.records = True, []
        try:
            train.train_step(model, crit, opt, gb)
            torch.cuda.synchronize()
            for kind, _algo, fb, e0, e1, tag, name in KT.records:
                if not kind.startswith("conv_"):
                    continue
                fl = fb[0] if isinstance(fb, tuple) else fb
                out.setdefault((kind, tag), (name, [], fl))[1].append(e0.elapsed_time(e1))
        finally:
            KT.enabled, KT.records = False, []
            ops.SidePrep.join()
    return out


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
    arms = {algo: build(algo, size, a.batch) for algo in (0, 4)}
    print(f"# split_vs_fp32: {a.size}^3 x {a.batch}, fp32 storage, static prompts, lr 0, {torch.cuda.get_device_name(0)}")

    with torch.no_grad():
        outs = {algo: train.forward_loss(m, c, gb)[1][0].float().clone() for algo, (m, c, _o, gb) in arms.items()}
    print(f"forward rel-L2, conv_algo=4 output against conv_algo=0 output: {rel(outs[4], outs[0]):.3e}")
    del outs

    # ---- per-launch kernel times, eager steps under ops.KernelTimer (also the warm-up of the capture below) ----
    recs = {algo: eager_records(*arms[algo], a.eager) for algo in (0, 4)}

    # ---- alternating blocks of graph-replayed steps ----
    steps = {algo: train.GraphedTrainStep(m, c, o, gb, warmup=2) for algo, (m, c, o, gb) in arms.items()}
    for algo in (0, 4):
        for _ in range(3):
            steps[algo]()
    torch.cuda.synchronize()
    ms = {0: [], 4: []}
    for _ in range(a.blocks):
        for algo in (0, 4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                steps[algo]()
            e1.record()
            torch.cuda.synchronize()
            ms[algo].append(e0.elapsed_time(e1) / a.steps)
    print(f"\nms/step, {a.blocks} alternating blocks of {a.steps} graph-replayed steps each:")
    for algo, name in ((0, "conv_algo=0 (exact fp32)"), (4, "conv_algo=4 (split bf16)")):
        v = ms[algo]
        print(f"  {name:26s} median {statistics.median(v):7.3f}   min {min(v):7.3f}   max {max(v):7.3f}   blocks {' '.join(f'{t:.3f}' for t in v)}")
    m0, m4 = statistics.median(ms[0]), statistics.median(ms[4])
    spread = max(max(ms[0]) - min(ms[0]), max(ms[4]) - min(ms[4]))
    print(f"  step ratio (algo 0 / algo 4, medians): {m0 / m4:.3f}x; difference {m0 - m4:.3f} ms, larger min-max spread of the two arms {spread:.3f} ms")

    # ---- per-layer table: the kernel a layer ran under algo 0 against the one it ran under algo 4 ----
    print(f"\nper-launch HIP-event ms over {a.eager} eager steps (median [min .. max]); layer = (x shape, Cout, k, stride, form)")
    print(f"{'kind':11s} {'layer':42s} {'algo 0 kernel':40s} {'ms':>24s}   {'algo 4 kernel':20s} {'ms':>24s} {'ratio':>6s} {'TFLOP/s':>8s} {'of peak':>8s}")
    tot = {}
    for key in sorted(recs[4], key=repr):
        n4, t4, fl = recs[4][key]
        if not n4.startswith("conv_split") or key not in recs[0]:
            continue
        n0, t0, _ = recs[0][key]
        f = lambda t: f"{statistics.median(t):8.3f} [{min(t):6.3f} .. {max(t):6.3f}]"
        md0, md4 = statistics.median(t0), statistics.median(t4)
        tf = fl / (md4 * 1e-3) / 1e12
        print(f"{key[0]:11s} {str(key[1]):42s} {n0:40s} {f(t0)}   {n4:20s} {f(t4)} {md0 / md4:6.2f} {tf:8.1f} {100 * tf * 1e12 / PEAK_BF16:7.1f}%")
        s = tot.setdefault((n0, n4), [0, 0.0, 0.0, 0.0])
        per_step = len(t4) / a.eager                      # a layer shape may occur several times in a step
        s[0] += per_step; s[1] += md0 * per_step; s[2] += md4 * per_step; s[3] += fl * per_step
    print("\nsummed over the layers above (medians):")
    for (n0, n4), (n, s0, s4, fl) in tot.items():
        tf = fl / (s4 * 1e-3) / 1e12
        print(f"  {n:4.0f} launches/step  {n0:40s} {s0:8.3f} ms  ->  {n4:20s} {s4:8.3f} ms   {s0 / s4:5.2f}x   "
              f"{tf:7.1f} useful TFLOP/s = {100 * tf * 1e12 / PEAK_BF16:.1f}% of the 2.5 PFLOP/s dense bf16 peak")
    other0 = sum(statistics.median(t) * len(t) / a.eager for k, (n, t, _) in recs[0].items() if not (k in recs[4] and recs[4][k][0].startswith("conv_split")))
    other4 = sum(statistics.median(t) * len(t) / a.eager for k, (n, t, _) in recs[4].items() if not n.startswith("conv_split"))
    print(f"  convolution launches outside the split kernels' scope: {other0:.3f} ms (algo 0), {other4:.3f} ms (algo 4) per step")


if __name__ == "__main__":
    main()
