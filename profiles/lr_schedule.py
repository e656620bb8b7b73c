"""What the device-side learning-rate schedule and the parameter options of FusedAdamW(lr_schedule, param_options) cost, in ONE
process on one GPU, alternating blocks, warm-up first (the method of grad_accum.py / ema.py):

  (a) the kernels alone on buffers of the 128^3 model's real flat size, 28 algorithmic bytes per element each: adamw_k (the
      yardstick), adamw_sched_k uniform (no table), adamw_sched_k with the model's real "no_decay_1d" segment table, and with
      a synthetic table at the cap (MAX_SEGS segments: 32 KB of LDS per block) -- us per launch and TB/s.  The base rate is 0
      here too: every load, operation and store of the sweep takes place, p is written back unchanged, and the buffers stay
      what they were from bracket to bracket;
  (b) the graph-replayed step at 128^3 x 2, bf16, static prompts, base rate 0 (AdamW still sweeps): plain, with a
      warm-up-plus-cosine schedule, and with the schedule and "no_decay_1d" -- ms per replay;
  (c) for the record, one GraphedTrainStep._capture() of that step: what a per-step schedule would pay per step through the
      host-side learning rate (a device synchronise and a capture of the whole step).

  python profiles/lr_schedule.py [--size 128] [--blocks 6] [--steps 12] > profiles/lr_schedule.txt

Aim (the project's usual one for a streaming kernel): adamw_sched_k at >= 0.9 of adamw_k's bytes/s of the same run, uniform and
with the real table.  The ratio is reported whatever it is.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCHED = dict(warmup_steps=500, decay="cosine", total_steps=100000, min_ratio=0.01)


def build(size, batch, **opts):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=torch.bfloat16, static_prompts=True).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = cu.build_reference_criterion()
    opt = train.make_optimizer(model, 0.0, **opts)
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
    from coma_unet_amd.optim import LRSchedule
    size = (a.size,) * 3
    print(f"# lr_schedule: {a.size}^3 x {a.batch}, bf16, static prompts, base rate 0, graph replay, {torch.cuda.get_device_name(0)}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        arms = {"plain": build(size, a.batch), "sched": build(size, a.batch, lr_schedule=SCHED),
                "sched+no_decay_1d": build(size, a.batch, lr_schedule=SCHED, param_options="no_decay_1d")}
        for step, _ in arms.values():
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        assert arms["plain"][1]._lr_dev is None and arms["sched"][1]._seg_tab is None
        tab = tuple(t.clone() for t in arms["sched+no_decay_1d"][1]._seg_tab)
        n = arms["plain"][1].flat_p.numel()
        print(f"flat buffer: {n} fp32 elements ({n * 4 / 1e6:.1f} MB per buffer); \"no_decay_1d\" table: {tab[0].numel()} segments "
              f"for {len(arms['plain'][1]._flat_params)} tensors")

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
        for k in arms:
            print(f"  {k:20s} {fmt(ms[k])}")
        md = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        for k in ("sched", "sched+no_decay_1d"):
            print(f"  {k} - plain: {md[k] - md['plain']:+.3f} ms ({(md[k] / md['plain'] - 1) * 100:+.2f} %)")
        print(f"  largest min-max spread between repeated blocks of one variant: {spread:.3f} ms")

        # ---- (c) one capture ----
        step, opt = arms["plain"]
        cap = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step._capture()
            torch.cuda.synchronize()
            cap.append((time.perf_counter() - t0) * 1e3)
        print(f"\n(c) one GraphedTrainStep._capture() of the plain step (host clock, synchronised): {' '.join(f'{c:.0f}' for c in cap)} ms "
              f"-- against {md['plain']:.2f} ms per replay")

        # ---- (a) the kernels alone, on buffers of the real flat size ----
        del arms, opt, step
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(0)
        p, g, m, v = (torch.randn(n, generator=gen, device="cuda") for _ in range(4))
        m.mul_(0.01)
        v.abs_().mul_(1e-4)
        stepd = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        lr_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
        lr_out = torch.zeros(1, dtype=torch.float32, device="cuda")
        hp = (0.9, 0.999, 1e-8, 1e-2)
        sched = LRSchedule(**SCHED).kernel_args()
        M = ops.MAX_SEGS
        ends = [n * (k + 1) // M for k in range(M)]
        cap_tab = (torch.tensor(ends, dtype=torch.int64, device="cuda"),
                   torch.tensor([1.0 if k % 2 else 0.5 for k in range(M)], dtype=torch.float32, device="cuda"),
                   torch.tensor([0.0 if k % 2 else 1e-2 for k in range(M)], dtype=torch.float32, device="cuda"))

        def sched_fn(segs):
            return lambda: ops.adamw_sched_(p, g, m, v, lr_dev, sched, *hp, 5, stepd, segs=segs, lr_out=lr_out)
        fns = {
            "adamw_k (yardstick)": lambda: ops.adamw_(p, g, m, v, 0.0, *hp, 5, stepd),
            "adamw_sched_k, uniform": sched_fn(None),
            f"adamw_sched_k, no_decay_1d ({tab[0].numel()})": sched_fn(tab),
            f"adamw_sched_k, {M} segments": sched_fn(cap_tab),
        }
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        per = 10
        t = {k: [] for k in fns}
        for _ in range(a.blocks):
            for k, fn in fns.items():
                e0, e1 = ev(), ev()
                e0.record()
                for _ in range(per):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) / per)
        by = 28
        med = {k: statistics.median(tv) for k, tv in t.items()}
        rate = {k: by * n / (med[k] * 1e-3) / 1e12 for k in fns}
        base = rate["adamw_k (yardstick)"]
        print(f"\n(a) kernels alone, {n} elements, {by} B/elem, base rate 0 (the whole sweep runs, p is stored unchanged), us per "
              f"launch ({per} launches per bracket, {a.blocks} alternating brackets); TB/s on algorithmic bytes; ratio to adamw_k's "
              f"rate of this run")
        for k in fns:
            tv = t[k]
            lo, hi = by * n / (max(tv) * 1e-3) / 1e12, by * n / (min(tv) * 1e-3) / 1e12
            print(f"  {k:38s} median {med[k] * 1e3:7.1f} us [{min(tv) * 1e3:7.1f} .. {max(tv) * 1e3:7.1f}]  {rate[k]:5.2f} TB/s "
                  f"[{lo:5.2f} .. {hi:5.2f}]  x{rate[k] / base:5.3f}")
        for k in list(fns)[1:3]:
            r = rate[k] / base
            print(f"aim: {k} at >= 0.9 of adamw_k's bytes/s: x{r:.3f} -> {'MET' if r >= 0.9 else 'NOT MET'}")
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


if __name__ == "__main__":
    main()
