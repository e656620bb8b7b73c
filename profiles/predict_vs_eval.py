"""Inference A/B at 128^3 x 2, bf16 and fp32 (method of profiles/split_vs_fp32.py: arms alternate inside ONE process).

  python profiles/predict_vs_eval.py [--size 128] [--blocks 6] [--steps 10] [--reps 30]     # writes profiles/predict_vs_eval.txt

Per dtype, one child process each (own time limit; the driver stops at the first failure and starts nothing after it):
  blocks  alternating blocks of forwards, HIP events around each block:
          (a) the plain model.eval() forward under no_grad (list of prior dicts, as contrastive_test calls it),
          (b) Predictor(graph=False), (c) Predictor(graph=True)
  gates   per-launch HIP-event times of the four gate levels: the new launch against the SUM of the launches it replaces
          (MFMA form: W_g, W_x, two BatchNorm applies, add-ReLU, psi convolution, sigmoid-BN apply, multiply;
          element-wise form: the last six).  A bracket around an eval BatchNorm apply includes the two small ATen
          launches that derive rstd from running_var: they are part of what the piecewise path runs per forward.
A condition holds when the difference of the medians exceeds the larger min-max spread of the two sides.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
LIMITS = {"blocks": 420, "gates": 300}          # seconds per child step


def fmt(v):
    return f"median {statistics.median(v):8.3f}   min {min(v):8.3f}   max {max(v):8.3f}"


def step_blocks(a, dtype):
    import torch
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic
    dev = torch.device("cuda:0")
    size = (a.size,) * 3
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=dtype).to(dev)
    model.set_save_attn(None)
    b = synthetic.make_batch(a.batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    with torch.no_grad():                 # one training-mode forward: running statistics that are not the initial ones
        model.train(True)
        model(gb["mri"], gb["covars"], roi_pred_dicts=gb["roi_pred_dicts"], sample_roi_mask=gb["roi"])
    model.eval()
    model.set_training(False)

    def plain():
        with torch.no_grad():
            return model(gb["mri"], gb["covars"], roi_pred_dicts=gb["roi_pred_dicts"], sample_roi_mask=gb["roi"])
    eager, graphed = cu.Predictor(model, gb, graph=False), cu.Predictor(model, gb, graph=True)
    arms = (("a", "plain eval forward", plain), ("b", "Predictor(graph=False)", eager), ("c", "Predictor(graph=True)", graphed))
    ref = plain().float().clone()
    rel = lambda y: float((y.float().double() - ref.double()).norm() / ref.double().norm())
    print(f"\n## {dtype}: {a.size}^3 x {a.batch}, {torch.cuda.get_device_name(0)}")
    print(f"output rel-L2 against the plain eval forward: eager predictor {rel(eager()):.3e}, graphed predictor {rel(graphed()):.3e}")
    for _k, _n, fn in arms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _n, _f in arms}
    for _ in range(a.blocks):
        for k, _n, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.steps)
    print(f"ms per forward, {a.blocks} alternating blocks of {a.steps} forwards each:")
    for k, n, _f in arms:
        print(f"  ({k}) {n:24s} {fmt(ms[k])}   blocks {' '.join(f'{t:.3f}' for t in ms[k])}")
    for k in ("b", "c"):
        d = statistics.median(ms["a"]) - statistics.median(ms[k])
        spread = max(max(ms["a"]) - min(ms["a"]), max(ms[k]) - min(ms[k]))
        print(f"  (a) - ({k}): {d:.3f} ms, larger min-max spread {spread:.3f} ms, ratio {statistics.median(ms['a']) / statistics.median(ms[k]):.3f}x"
              f" -> condition {'holds' if d > spread else 'MISSED'}")


def step_gates(a, dtype):
    import torch
    from coma_unet_amd import _lib as L
    from coma_unet_amd import fold_gate, ops
    from coma_unet_amd.attn_unet_data_parallel import ObservableAttentionBlock
    from coma_unet_amd.layers import Config, conv_plain, norm_act
    dev = torch.device("cuda:0")
    print(f"\n## {dtype}: per-launch HIP-event ms of the gate levels, batch {a.batch}, {a.reps} repetitions")

    def timed(fn):
        for _ in range(3):
            fn()
        t = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return t

    for C, n in ((32, a.size), (64, a.size // 2), (128, a.size // 4), (256, a.size // 8)):
        torch.manual_seed(C)
        cfg = Config(compute_dtype=dtype)
        blk = ObservableAttentionBlock(cfg, f_int=C // 2, f_g=C, f_l=C).to(dev).eval()
        with torch.no_grad():
            for bn in (blk.W_g[1], blk.W_x[1], blk.psi[1]):
                bn.running_mean.uniform_(-0.5, 0.5)
                bn.running_var.uniform_(0.5, 2.0)
        cat = torch.randn(a.batch, n, n, n, 2 * C, device=dev).to(dtype)
        x = torch.randn(a.batch, n, n, n, C, device=dev).to(dtype)
        g, out = cat[..., C:], cat[..., :C]
        fold = fold_gate(blk)
        with torch.no_grad():
            g1r, x1r = blk.W_g[0](g), blk.W_x[0](x)
            bn_ = lambda t, bn, act: norm_act(cfg, t, bn, L.NORM_BATCH, act, None, False)
            g1, x1 = bn_(g1r, blk.W_g[1], L.ACT_NONE), bn_(x1r, blk.W_x[1], L.ACT_NONE)
            s = ops.AddRelu.apply(g1, x1)
            pr = blk.psi[0](s)
            psi = bn_(pr, blk.psi[1], L.ACT_SIGMOID)
            pieces = [("W_g conv", lambda: blk.W_g[0](g)), ("W_x conv", lambda: blk.W_x[0](x)),
                      ("BN_g apply", lambda: bn_(g1r, blk.W_g[1], L.ACT_NONE)), ("BN_x apply", lambda: bn_(x1r, blk.W_x[1], L.ACT_NONE)),
                      ("add-ReLU", lambda: ops.AddRelu.apply(g1, x1)), ("psi conv", lambda: blk.psi[0](s)),
                      ("sigmoid-BN apply", lambda: bn_(pr, blk.psi[1], L.ACT_SIGMOID)),
                      ("multiply", lambda: ops.GateMul.apply(x, psi, ops.Out(out)))]
            old = [(nm, timed(fn)) for nm, fn in pieces]
            g1n = conv_plain(cfg, g, blk.W_g[0].conv, 1, 1, False, with_bias=False)
            x1n = conv_plain(cfg, x, blk.W_x[0].conv, 1, 1, False, with_bias=False)
            new = [("gate_eval_fwd_k", 2, timed(lambda: ops.gate_eval_fwd(x, g1n, x1n, fold, out, True)))]
            if "wg" in fold and ops.gate_eval_mfma_ok(g, x, C // 2):
                new.append(("gate_eval_mfma_k", 0, timed(lambda: ops.gate_eval_mfma(g, x, fold, out, True))))
        print(f"level C={C} {n}^3:")
        for nm, t in old:
            print(f"    {nm:18s} {fmt(t)}")
        for nm, first, t in new:
            rep = old[first:]
            so, sp = sum(statistics.median(v) for _n, v in rep), sum(max(v) - min(v) for _n, v in rep)
            d, spread = so - statistics.median(t), max(sp, max(t) - min(t))
            print(f"  {nm:18s}   {fmt(t)}   replaces {len(rep)} launches, summed medians {so:8.3f} (summed spreads {sp:.3f}): "
                  f"{so / statistics.median(t):5.2f}x, difference {d:.3f} vs spread {spread:.3f} -> condition {'holds' if d > spread else 'MISSED'}")
        del cat, x, g1r, x1r, g1, x1, s, pr, psi, g1n, x1n
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", choices=("blocks", "gates"))
    ap.add_argument("--dtype", choices=("bf16", "fp32"))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "predict_vs_eval.txt"))
    a = ap.parse_args()
    if a.step:                                    # child: one GPU step
        import torch
        dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
        (step_blocks if a.step == "blocks" else step_gates)(a, dt)
        return 0
    text = [f"# predict_vs_eval: {a.size}^3 x {a.batch}; (a) plain eval forward, (b) Predictor(graph=False), (c) Predictor(graph=True)"]
    rc = 0
    for step in ("blocks", "gates"):
        for dt in ("bf16", "fp32"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--dtype", dt, "--size", str(a.size), "--batch", str(a.batch),
                   "--blocks", str(a.blocks), "--steps", str(a.steps), "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LIMITS[step])
                rc, outp = r.returncode, r.stdout
            except subprocess.TimeoutExpired as e:
                rc, outp = 124, (e.stdout or "") + f"\n{step} {dt}: time limit of {LIMITS[step]} s"
            if isinstance(outp, bytes):
                outp = outp.decode(errors="replace")
            print(outp, flush=True)
            if rc != 0:                           # stop at the first failure: nothing more is started on the GPU
                print(f"{step} {dt} failed (rc={rc}); {a.out} not written", flush=True)
                return rc
            text.append(outp.rstrip())
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
