"""What frozen-BatchNorm training (model.freeze_batchnorm(), or BatchNorm3d holders in eval mode inside a train-mode model)
costs and saves, in ONE process on one GPU:

  1. the step at 128^3 x 2, static prompts, learning rate 0, graph-replayed: frozen against plain training of the same model,
     alternating blocks of replays (the method of grad_accum.py), for bf16 and for compute_dtype=float32, conv_algo=7;
  2. norm_act_bwd_frozen_k alone on a 128^3 x 32 volume (B = 2), bf16 and fp32, with the parameter sums and as the pure
     streaming pass, against norm_act_fwd_k in the same run: TB/s on algorithmic bytes (forward 2 T, backward 3 T) and the
     ratio of the two rates (the aim: 0.9);
  3. the frozen gate (ops.GateFrozen: 1 launch forward, 2 backward) against ops.GateFused (2 + 3) at C = 32, F = 16, 128^3 x 2;
  4. --resources: registers / scratch / occupancy of the new kernels as hipcc reports them (no GPU needed).

  python profiles/frozen_bn.py [--size 128] [--blocks 6] [--steps 12] [--resources] [--no-gpu] > profiles/frozen_bn.txt
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ev():
    return torch.cuda.Event(enable_timing=True)


def fmt(v):
    return f"median {statistics.median(v):7.3f}   min {min(v):7.3f}   max {max(v):7.3f}   blocks {' '.join(f'{t:.3f}' for t in v)}"


def build(size, batch, frozen, **kw):
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, static_prompts=True, **kw).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = cu.build_reference_criterion()
    opt = train.make_optimizer(model, 0.0)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    train.train_step(model, crit, opt, gb)          # (moves the running statistics off (0, 1) in both arms)
    if frozen:
        model.freeze_batchnorm()
    for _ in range(2):
        train.train_step(model, crit, opt, gb)
    return train.GraphedTrainStep(model, crit, opt, gb, prewarmed=True)


def step_times(a):
    size = (a.size,) * 3
    for label, kw in (("bf16", dict(compute_dtype=torch.bfloat16)), ("fp32, conv_algo=7", dict(compute_dtype=torch.float32, conv_algo=7))):
        arms = {"plain": build(size, a.batch, False, **kw), "frozen": build(size, a.batch, True, **kw)}
        for step in arms.values():
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(a.blocks):
            for name, step in arms.items():
                e0, e1 = ev(), ev()
                e0.record()
                for _ in range(a.steps):
                    step()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.steps)
        print(f"\n[1] step, {a.size}^3 x {a.batch}, {label}: ms per graph replay, {a.blocks} alternating blocks of {a.steps} replays")
        for k in arms:
            print(f"  {k:8s} {fmt(ms[k])}")
        spread = max(max(v) - min(v) for v in ms.values())
        d = statistics.median(ms["frozen"]) - statistics.median(ms["plain"])
        print(f"  frozen - plain: {d:+.3f} ms ({d / statistics.median(ms['plain']):+.1%}); largest min-max spread between blocks of one arm: {spread:.3f} ms; "
              f"{'not slower beyond the spread' if d <= spread else 'SLOWER than the plain step beyond the spread'}")
        del arms
        torch.cuda.empty_cache()


def norm_alone(a):
    from coma_unet_amd import ops, _lib as L
    lib, ct, ptr = L.lib, L.ct, L.ptr
    B, C = a.batch, 32
    shape = (B, a.size, a.size, a.size, C)
    print(f"\n[2] norm kernels alone, {a.size}^3 x {C} (B = {B}), BatchNorm + ReLU, ms per launch (10 launches per bracket, {a.blocks} alternating "
          f"brackets); TB/s on algorithmic bytes; ratio to norm_act_fwd_k's rate of the same run (aim 0.9)")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for dt in (torch.bfloat16, torch.float32):
        x = torch.randn(shape, generator=gen, device="cuda").to(dt)
        dy = torch.randn(shape, generator=gen, device="cuda").to(dt)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, var = torch.randn(1, C, device="cuda") * 0.3, torch.rand(1, C, device="cuda") + 0.5
        rstd = torch.rsqrt(var + 1e-5)
        gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.3
        dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        rec = torch.zeros(ops.STAT_REPLICAS * ((C * 3 + 7) & ~7), dtype=torch.float64, device="cuda")
        bsum = ops.stat_record(1, C, 3, x.device)
        sums = ops.stat_record(1, C, 2, x.device)
        L.check(lib.coma_norm_stats(ct(x), L.NORM_BATCH, ptr(sums), L.stream()), "stats")
        s = L.stream()
        T = x.numel() * x.element_size()
        fns = {
            "norm_act_fwd_k (tables)": (2, lambda: L.check(lib.coma_norm_act_fwd(ct(x), L.NORM_BATCH, None, 1e-5, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                                                                  L.ACT_RELU, None, None, None, 0.1, ct(y), s), "fwd")),
            "norm_act_bwd_frozen_k + sums": (3, lambda: L.check(lib.coma_norm_act_bwd_frozen(ct(x), ct(dy), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), L.ACT_RELU,
                                                                                            None, ct(dx), ptr(dg), ptr(db), None, ptr(rec), s), "bwd_frozen")),
            "norm_act_bwd_frozen_k streaming": (3, lambda: L.check(lib.coma_norm_act_bwd_frozen(ct(x), ct(dy), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), L.ACT_RELU,
                                                                                               None, ct(dx), None, None, None, None, s), "bwd_frozen")),
            "training backward (2 launches)": (5, lambda: L.check(lib.coma_norm_act_bwd(ct(x), ct(dy), L.NORM_BATCH, ptr(sums), 1e-5, ptr(gamma), ptr(beta), L.ACT_RELU,
                                                                                      None, ct(dx), ptr(dg), ptr(db), None, ptr(bsum), s), "bwd")),
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
        rate = {k: by * T / (statistics.median(t[k]) * 1e-3) / 1e12 for k, (by, _) in fns.items()}
        base = rate["norm_act_fwd_k (tables)"]
        print(f"  {'bf16' if dt == torch.bfloat16 else 'fp32'}: T = {T / 1e6:.0f} MB")
        for k, (by, _) in fns.items():
            tv = t[k]
            verdict = "" if not k.startswith("norm_act_bwd_frozen") else ("MET" if rate[k] >= 0.9 * base else "NOT MET")
            print(f"    {k:34s} {by} T  median {statistics.median(tv):7.4f} ms [{min(tv):7.4f} .. {max(tv):7.4f}]  {rate[k]:5.2f} TB/s  x{rate[k] / base:4.2f} {verdict}")
        del x, dy, y, dx
        torch.cuda.empty_cache()


def gate_alone(a):
    from coma_unet_amd import ops, _lib as L
    B, C, F_ = a.batch, 32, 16
    xs, fs = (B, a.size, a.size, a.size, C), (B, a.size, a.size, a.size, F_)
    print(f"\n[3] the gate behind its W_g / W_x convolutions, C = {C}, F = {F_}, {a.size}^3 x {B}: ms per call ({a.blocks} alternating brackets of 5 calls); "
          f"launches: GateFused 2 forward + 3 backward, GateFrozen 1 forward + 2 backward (the pass and a one-block finalise)")
    gen = torch.Generator(device="cuda").manual_seed(1)
    for dt in (torch.bfloat16, torch.float32):
        rn = lambda shape, sc=1.0: (torch.randn(shape, generator=gen, device="cuda") * sc).to(dt)
        x, g1, x1, datt = rn(xs), rn(fs, 1.3), rn(fs, 0.8), rn(xs)
        un = lambda n, lo, hi: (torch.rand(n, generator=gen, device="cuda") * (hi - lo) + lo).requires_grad_(True)
        P = dict(gam_g=un(F_, 0.5, 1.5), bet_g=un(F_, -0.3, 0.3), gam_x=un(F_, 0.5, 1.5), bet_x=un(F_, -0.3, 0.3),
                 w=(torch.randn(F_, generator=gen, device="cuda") * 0.5).requires_grad_(True), b=un(1, -0.2, 0.2), gam_p=un(1, 0.5, 1.5), bet_p=un(1, -0.3, 0.3))
        run = [torch.zeros(F_, device="cuda"), torch.ones(F_, device="cuda"), torch.zeros(F_, device="cuda"), torch.ones(F_, device="cuda"),
               torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")]
        stats = tuple((torch.randn(1, n, device="cuda") * 0.3, torch.rsqrt(torch.rand(1, n, device="cuda") + 0.5)) for n in (F_, F_, 1))
        xg, g1g, x1g = (t.requires_grad_(True) for t in (x, g1, x1))
        att_buf = torch.empty(xs, dtype=dt, device="cuda")

        def fused():
            sums = []
            for t_ in (g1, x1):       # (in the model these records come out of the convolutions' epilogues: not timed)
                rec = ops.stat_record(1, F_, 2, t_.device)
                L.check(L.lib.coma_norm_stats(L.ct(t_.detach()), L.NORM_BATCH, L.ptr(rec), L.stream()), "norm_stats")
                sums.append(rec)
            e = [ev() for _ in range(3)]
            e[0].record()
            att, _psi = ops.GateFused.apply(xg, g1g, x1g, sums[0], sums[1], P["gam_g"], P["bet_g"], P["gam_x"], P["bet_x"], P["w"], P["b"],
                                            P["gam_p"], P["bet_p"], tuple(run), 0.1, (1e-5, 1e-5, 1e-5), ops.Out(att_buf))
            e[1].record()
            att.backward(datt)
            e[2].record()
            return e

        def frozen():
            e = [ev() for _ in range(3)]
            e[0].record()
            att, _psi = ops.GateFrozen.apply(xg, g1g, x1g, P["gam_g"], P["bet_g"], P["gam_x"], P["bet_x"], P["w"], P["b"], P["gam_p"], P["bet_p"],
                                             stats, ops.Out(att_buf))
            e[1].record()
            att.backward(datt)
            e[2].record()
            return e

        leaves = [xg, g1g, x1g, *P.values()]

        def clean(fn):
            for t_ in leaves:          # (no accumulate launches behind the backward)
                t_.grad = None
            return fn()

        arms = {"GateFused (training)": lambda: clean(fused), "GateFrozen": lambda: clean(frozen)}
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        t = {k: ([], []) for k in arms}
        for _ in range(a.blocks):
            for k, fn in arms.items():
                marks = [fn() for _ in range(5)]
                torch.cuda.synchronize()
                t[k][0].append(statistics.mean(e[0].elapsed_time(e[1]) for e in marks))
                t[k][1].append(statistics.mean(e[1].elapsed_time(e[2]) for e in marks))
        print(f"  {'bf16' if dt == torch.bfloat16 else 'fp32'} (host-timed brackets around eager launches: launch gaps included in both arms)")
        for k in arms:
            f_, b_ = statistics.median(t[k][0]), statistics.median(t[k][1])
            print(f"    {k:22s} forward {f_:7.3f} ms [{min(t[k][0]):.3f} .. {max(t[k][0]):.3f}]   backward {b_:7.3f} ms [{min(t[k][1]):.3f} .. {max(t[k][1]):.3f}]   "
                  f"sum {f_ + b_:7.3f} ms")
        del x, g1, x1, datt, xg, g1g, x1g, att_buf
        torch.cuda.empty_cache()


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    print("\n[4] hipcc -Rpass-analysis=kernel-resource-usage, gfx950, -O3: the new kernels")
    print(f"  {'kernel':58s} VGPRs  scratch B/lane  VGPR spills  waves/SIMD  LDS B/block")
    with tempfile.TemporaryDirectory() as tmp:
        for src in ("norm.hip", "gate.hip"):
            r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-c", os.path.join(ROOT, "coma_unet_amd", "csrc", src),
                                "-o", os.path.join(tmp, src + ".o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
            for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
                name = blk.split()[0]
                if "frozen" not in name:
                    continue
                m = re.match(r"_Z\d+([a-z_0-9]+?)(?:I(f|DF16b)Li(\d)E(?:Lb([01])E)?E)?v", name)       # (c++filt does not know DF16b)
                dem = name if not m else m.group(1) + ("" if not m.group(2) else "<%s, %s%s>" % (
                    "float" if m.group(2) == "f" else "__bf16", m.group(3), "" if m.group(4) is None else (", sums" if m.group(4) == "1" else ", streaming")))
                g = lambda k: re.search(re.escape(k) + r": (\d+)", blk).group(1)
                vals = [g(k) for k in ("VGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")]
                print("  %-58s %5s  %14s  %11s  %10s  %11s" % (dem, *vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    if not a.no_gpu:
        print(f"# frozen_bn: {a.size}^3 x {a.batch}, static prompts, lr 0, {torch.cuda.get_device_name(0)}")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step_times(a)
            norm_alone(a)
            gate_alone(a)
            side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
    if a.resources:
        resources()


if __name__ == "__main__":
    main()
