"""What gradient accumulation and global-norm clipping (FusedAdamW(grad_acc_batch, max_grad_norm)) cost, in ONE process at
128^3 x 2, bf16, static prompts, learning rate 0 (AdamW still sweeps), graph-replayed:

  (a) today's step (grad_acc_batch=1, no clip)           (c) grad_acc_batch=1 with clip
  (b) grad_acc_batch=4 without clip                      (d) grad_acc_batch=4 with clip

  python profiles/grad_accum.py [--size 128] [--blocks 6] [--steps 12] > profiles/grad_accum.txt

Alternating blocks of replays of each variant (the method of pointwise_f32.py).  (a) and (c): ms per replay.  (b) and (d): a
block is --steps / 4 whole windows; HIP events bracket the three micro-batch replays and the applying replay of every window:
mean ms per micro-batch replay and ms of the applying replay.  Then each new kernel alone on buffers of the real flat size,
together with adamw_k in the same process (10 launches per HIP-event bracket, alternating brackets): TB/s on algorithmic
bytes -- accumulate 12 bytes per element (8 on a window's first micro-batch), norm-only 4, coma_adamw_ex 28 as adamw_k -- and
the ratio to adamw_k's rate of this run (the yardstick; target >= 0.9).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 4
MAX_NORM = 1.0


def build(size, batch, grad_acc_batch, max_grad_norm):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=torch.bfloat16, static_prompts=True).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = cu.build_reference_criterion()
    opt = train.make_optimizer(model, 0.0)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    for _ in range(2):                       # the flat layout, the workspaces: plain steps
        train.train_step(model, crit, opt, gb)
    opt.param_groups[0]["grad_acc_batch"] = grad_acc_batch
    opt.param_groups[0]["max_grad_norm"] = max_grad_norm
    step = train.GraphedTrainStep(model, crit, opt, gb, prewarmed=True)
    return step, opt


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
    print(f"# grad_accum: {a.size}^3 x {a.batch}, bf16, static prompts, lr 0, graph replay, {torch.cuda.get_device_name(0)}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        arms = {"a": build(size, a.batch, 1, None), "b": build(size, a.batch, K, None),
                "c": build(size, a.batch, 1, MAX_NORM), "d": build(size, a.batch, K, MAX_NORM)}
        for step, _ in arms.values():
            for _ in range(K):
                step()
        torch.cuda.synchronize()
        assert all(o.pending == 0 for _, o in arms.values())
        n = arms["a"][1].flat_p.numel()
        print(f"flat buffer: {n} fp32 elements ({n * 4 / 1e6:.1f} MB per buffer)")
        ms = {"a": [], "c": [], "b_micro": [], "b_apply": [], "d_micro": [], "d_apply": []}
        for _ in range(a.blocks):
            for name, (step, opt) in arms.items():
                if name in ("a", "c"):
                    e0, e1 = ev(), ev()
                    e0.record()
                    for _ in range(a.steps):
                        step()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / a.steps)
                else:
                    marks = []
                    for _ in range(max(1, a.steps // K)):
                        e = [ev() for _ in range(3)]
                        e[0].record()
                        for _ in range(K - 1):
                            step()
                        e[1].record()
                        step()
                        e[2].record()
                        marks.append(e)
                    torch.cuda.synchronize()
                    assert opt.pending == 0
                    ms[name + "_micro"].append(statistics.mean(e[0].elapsed_time(e[1]) / (K - 1) for e in marks))
                    ms[name + "_apply"].append(statistics.mean(e[1].elapsed_time(e[2]) for e in marks))
        print(f"\nms per graph replay, {a.blocks} alternating blocks ({a.steps} replays of (a) / (c), {max(1, a.steps // K)} windows of {K} of (b) / (d) per block):")
        rows = (("a", "(a) K=1, no clip (today)"), ("c", f"(c) K=1, clip {MAX_NORM:g}"), ("b_micro", f"(b) K={K}, micro-batch replay"),
                ("b_apply", f"(b) K={K}, applying replay"), ("d_micro", f"(d) K={K} + clip, micro-batch replay"),
                ("d_apply", f"(d) K={K} + clip, applying replay"))
        for k, label in rows:
            print(f"  {label:38s} {fmt(ms[k])}")
        md = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        print(f"  largest min-max spread between repeated blocks of one variant: {spread:.3f} ms")
        print(f"  (a) - (b) micro-batch replay: {md['a'] - md['b_micro']:+.3f} ms (the micro-batch replay runs the accumulate kernel instead of adamw_k)")
        print(f"  (b) applying replay - (a): {md['b_apply'] - md['a']:+.3f} ms;  (c) - (a): {md['c'] - md['a']:+.3f} ms;  (d) applying replay - (a): {md['d_apply'] - md['a']:+.3f} ms")
        print(f"  mean ms per micro-batch over a window: (b) {((K - 1) * md['b_micro'] + md['b_apply']) / K:.3f}, (d) {((K - 1) * md['d_micro'] + md['d_apply']) / K:.3f}, (a) {md['a']:.3f}")

        # ---- the kernels alone, on buffers of the real flat size ----
        del arms
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(0)
        p, g, m, v, acc = (torch.randn(n, generator=gen, device="cuda") for _ in range(5))
        m.mul_(0.01)
        v.abs_().mul_(1e-4)
        parts = torch.zeros(ops.ACC_PARTIALS, dtype=torch.float64, device="cuda")
        norm = torch.zeros(1, dtype=torch.float32, device="cuda")
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        two = torch.full((1,), 2, dtype=torch.int32, device="cuda")
        four = torch.full((1,), K, dtype=torch.int32, device="cuda")
        stepd = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        hp = (0.0, 0.9, 0.999, 1e-8, 1e-2)
        nb = ops.grad_accum_(None, acc, None, parts)
        fns = {
            "adamw_k (yardstick)": (28, lambda: ops.adamw_(p, g, m, v, *hp, 5, stepd)),
            "adamw_ex_k, count": (28, lambda: ops.adamw_ex_(p, acc, m, v, *hp, 5, stepd, four)),
            "adamw_ex_k, count + clip": (28, lambda: ops.adamw_ex_(p, acc, m, v, *hp, 5, stepd, four, parts, nb, None, MAX_NORM, norm)),
            "grad_accum_k, acc += g": (12, lambda: ops.grad_accum_(acc, g, two, None)),
            "grad_accum_k, acc += g, partials": (12, lambda: ops.grad_accum_(acc, g, two, parts)),
            "grad_accum_k, acc = g (first)": (8, lambda: ops.grad_accum_(acc, g, zero, None)),
            "grad_accum_k, norm only": (4, lambda: ops.grad_accum_(None, acc, None, parts)),
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
        rate = {k: by * n / (statistics.median(t[k]) * 1e-3) / 1e12 for k, (by, _) in fns.items()}
        base = rate["adamw_k (yardstick)"]
        print(f"\nkernels alone, {n} elements, ms per launch ({per} launches per bracket, {a.blocks} alternating brackets); TB/s on algorithmic bytes; "
              f"ratio to adamw_k's rate of this run (target >= 0.9 for the accumulate kernel and coma_adamw_ex)")
        for k, (by, _) in fns.items():
            tv = t[k]
            lo, hi = by * n / (max(tv) * 1e-3) / 1e12, by * n / (min(tv) * 1e-3) / 1e12
            verdict = "" if k.startswith("adamw_k") or by == 4 else ("MET" if rate[k] >= 0.9 * base else "NOT MET")
            print(f"  {k:34s} {by:2d} B/elem  median {statistics.median(tv):7.4f} ms [{min(tv):7.4f} .. {max(tv):7.4f}]  {rate[k]:5.2f} TB/s "
                  f"[{lo:5.2f} .. {hi:5.2f}]  x{rate[k] / base:4.2f} {verdict}")
        acc_ms = statistics.median(t["grad_accum_k, acc += g"])
        adam_ms = statistics.median(t["adamw_k (yardstick)"])
        print(f"\nexpected (b) micro-batch replay - (a) from the kernels alone: accumulate {acc_ms:.3f} ms - adamw_k {adam_ms:.3f} ms = {acc_ms - adam_ms:+.3f} ms; "
              f"measured {md['b_micro'] - md['a']:+.3f} ms; block spread {spread:.3f} ms")
        print(f"expected (b) applying replay - (a): accumulate {acc_ms:.3f} ms + (adamw_ex_k - adamw_k) "
              f"{statistics.median(t['adamw_ex_k, count']) - adam_ms:+.3f} ms; measured {md['b_apply'] - md['a']:+.3f} ms")
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


if __name__ == "__main__":
    main()
