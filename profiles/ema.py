"""What the weight average of FusedAdamW(ema_decay) costs, in ONE process on one GPU, alternating blocks, warm-up first (the
method of grad_accum.py):

  (a) the kernels alone on buffers of the 128^3 model's real flat size: adamw_k (28 algorithmic bytes per element), adamw_ema_k
      (36), and adamw_k followed by a separate fp32 lerp pass over (e, p) (28 + 12 = 40: what a host-driven
      torch.optim.swa_utils.AveragedModel update adds behind the step) -- ms per launch and TB/s on algorithmic bytes;
  (b) the graph-replayed step at 128^3 x 2, bf16, static prompts, learning rate 0 (AdamW still sweeps), without and with
      ema_decay -- ms per replay;
  (c) one swap_ema() (coma_swap_f32 over the flat buffer: 16 bytes per element).

  python profiles/ema.py [--size 128] [--blocks 6] [--steps 12] > profiles/ema.txt

Aim (the project's usual one for a streaming kernel): adamw_ema_k at >= 0.9 of adamw_k's bytes/s of the same run, and no
slower than the unfused pair.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DECAY = 0.999


def build(size, batch, ema_decay):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=torch.bfloat16, static_prompts=True).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = cu.build_reference_criterion()
    opt = train.make_optimizer(model, 0.0, ema_decay=ema_decay)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    for _ in range(2):                       # the flat layout, the workspaces: plain steps
        train.train_step(model, crit, opt, gb)
    return train.GraphedTrainStep(model, crit, opt, gb, prewarmed=True), opt


def ev():
    return torch.cuda.Event(enable_timing=True)


def fmt(v):
    return f"median {statistics.median(v):7.3f}   min {min(v):7.3f}   max {max(v):7.3f}   blocks {' '.join(f'{t:.3f}' for t in v)}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=12)
    a = ap.parse_args()
    from coma_unet_amd import ops
    size = (a.size,) * 3
    print(f"# ema: {a.size}^3 x {a.batch}, bf16, static prompts, lr 0, graph replay, {torch.cuda.get_device_name(0)}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        arms = {"off": build(size, a.batch, None), "on": build(size, a.batch, DECAY)}
        for step, _ in arms.values():
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        assert arms["off"][1].flat_ema is None and arms["on"][1].flat_ema is not None
        n = arms["off"][1].flat_p.numel()
        print(f"flat buffer: {n} fp32 elements ({n * 4 / 1e6:.1f} MB per buffer)")

        # ---- (b) the graph-replayed step ----
        ms = {k: [] for k in arms}
        for _ in range(a.blocks):
            for name, (step, _opt) in arms.items():
                e0, e1 = ev(), ev()
                e0.record()
                for _ in range(a.steps):
                    step()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.steps)
        print(f"\n(b) ms per graph replay, {a.blocks} alternating blocks of {a.steps} replays:")
        print(f"  ema_decay=None (today)   {fmt(ms['off'])}")
        print(f"  ema_decay={DECAY:<6g}         {fmt(ms['on'])}")
        md = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        print(f"  on - off: {md['on'] - md['off']:+.3f} ms ({(md['on'] / md['off'] - 1) * 100:+.2f} %); largest min-max spread between "
              f"repeated blocks of one variant: {spread:.3f} ms")

        # ---- (c) one swap_ema() ----
        opt = arms["on"][1]
        for _ in range(2):
            opt.swap_ema()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.blocks):
            e0, e1 = ev(), ev()
            e0.record()
            opt.swap_ema()
            opt.swap_ema()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 2)
        sw = statistics.median(ts)
        print(f"\n(c) one swap_ema() (coma_swap_f32, {n} elements, 16 B/elem): median {sw:.4f} ms [{min(ts):.4f} .. {max(ts):.4f}]  "
              f"{16 * n / (sw * 1e-3) / 1e12:.2f} TB/s")

        # ---- (a) the kernels alone, on buffers of the real flat size ----
        del arms, opt
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(0)
        p, g, m, v, e = (torch.randn(n, generator=gen, device="cuda") for _ in range(5))
        m.mul_(0.01)
        v.abs_().mul_(1e-4)
        stepd = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        hp = (0.0, 0.9, 0.999, 1e-8, 1e-2)

        def pair():
            ops.adamw_(p, g, m, v, *hp, 5, stepd)
            e.lerp_(p, 1.0 - DECAY)

        fns = {
            "adamw_k (yardstick)": (28, lambda: ops.adamw_(p, g, m, v, *hp, 5, stepd)),
            "adamw_ema_k": (36, lambda: ops.adamw_ema_(p, g, m, v, e, DECAY, False, *hp, 5, stepd)),
            "adamw_ema_k, warm-up": (36, lambda: ops.adamw_ema_(p, g, m, v, e, DECAY, True, *hp, 5, stepd)),
            "adamw_k + fp32 lerp pass": (40, pair),
            "fp32 lerp pass alone": (12, lambda: e.lerp_(p, 1.0 - DECAY)),
        }
        for _, fn in fns.values():
            fn()
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
        med = {k: statistics.median(tv) for k, tv in t.items()}
        rate = {k: by * n / (med[k] * 1e-3) / 1e12 for k, (by, _) in fns.items()}
        base = rate["adamw_k (yardstick)"]
        print(f"\n(a) kernels alone, {n} elements, ms per launch ({per} launches per bracket, {a.blocks} alternating brackets); TB/s on "
              f"algorithmic bytes; ratio to adamw_k's rate of this run")
        for k, (by, _) in fns.items():
            tv = t[k]
            lo, hi = by * n / (max(tv) * 1e-3) / 1e12, by * n / (min(tv) * 1e-3) / 1e12
            print(f"  {k:28s} {by:2d} B/elem  median {med[k]:7.4f} ms [{min(tv):7.4f} .. {max(tv):7.4f}]  {rate[k]:5.2f} TB/s "
                  f"[{lo:5.2f} .. {hi:5.2f}]  x{rate[k] / base:4.2f}")
        r = rate["adamw_ema_k"] / base
        print(f"\naim 1: adamw_ema_k at >= 0.9 of adamw_k's bytes/s: x{r:.3f} -> {'MET' if r >= 0.9 else 'NOT MET'}")
        print(f"aim 2: no slower than the unfused pair: {med['adamw_ema_k']:.4f} ms vs {med['adamw_k + fp32 lerp pass']:.4f} ms -> "
              f"{'MET' if med['adamw_ema_k'] <= med['adamw_k + fp32 lerp pass'] else 'NOT MET'}")
        print(f"expected (b) on - off from the kernels alone: {med['adamw_ema_k'] - med['adamw_k (yardstick)']:+.3f} ms; measured "
              f"{md['on'] - md['off']:+.3f} ms; block spread {spread:.3f} ms")
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


if __name__ == "__main__":
    main()
