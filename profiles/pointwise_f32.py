"""A/B of the thin split mode against the pointwise mode in ONE process: conv_algo=6 (the yardstick: its code is unchanged)
against conv_algo=7 (plus the attention gates' 1x1x1 convolutions W_g / W_x -- forward, data gradient, weight gradient -- on
conv_pw_f32_k / conv_pw_f32_wgrad_k, exact fp32 MFMA) at 128^3 x 2, static prompts, learning rate 0, same initial state and
batch.  The method is that of split_vs_fp32.py / split_thin.py, whose helpers it uses.

  python profiles/pointwise_f32.py [--size 128] [--blocks 6] [--steps 20] [--eager 5] > profiles/pointwise_f32.txt

Prints: forward rel-L2 of mode 7's output against mode 0's (exact fp32) and against mode 6's; median and min-max ms/step of
modes 6 and 7 over ALTERNATING blocks of graph-replayed steps; per pointwise launch of the step the per-launch HIP-event time
(ops.KernelTimer, eager steps; a forward's time includes its statistics, a weight gradient's its memset and replica sum) of the
old kernel under conv_algo=6 and the new kernel under conv_algo=7, the difference against the larger min-max spread (MET: the
difference of the medians exceeds it), and the new kernel's TB/s on algorithmic bytes: 4 (C + N) per voxel, plus 4 N for a
launch that accumulates into its output (a layer key with two launches per step, of which one accumulates, counts 2 N).
Then the fp32 Predictor's eval forward under both modes, in alternating blocks, the same way; and, through ops._conv_fwd /
ops._conv_bwd on stand-alone tensors, every kernel instance the step does not contain (forward C = 8 .. 64 against N = 16 and
64, the weight-gradient tile shapes) at 64^3 x 2 and 128^3 x 2: 10 launches per HIP-event bracket, alternating brackets of the
two modes, the same rule ("(same)": the problem is outside the new kernels' predicate and runs the old kernel under both
modes).  The predicates of csrc/conv_pw_f32.hip hold the classes that met it.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from split_vs_fp32 import build, rel      # noqa: E402

NEW = ("conv_pw_f32_k", "conv_pw_f32_wgrad_k")


class _LibShim:
    """ops.lib with the COMA_ACCUMULATE bit of the last forward / data-gradient call kept (the bytes of a launch depend on it)."""

    def __init__(self, lib, accumulate):
        self._lib, self._acc, self.last = lib, accumulate, 0

    def __getattr__(self, k):
        return getattr(self._lib, k)

    def coma_conv_fwd_ws(self, *a):
        self.last = 1 if int(a[8]) & self._acc else 0
        return self._lib.coma_conv_fwd_ws(*a)


def eager_records(model, crit, opt, gb, n):
    """{(kind, tag): (kernel name, [ms per launch over n eager steps], [accumulate flag per launch])}"""
    from coma_unet_amd import _lib as L
    from coma_unet_amd import ops, train
    KT = ops.KernelTimer
    shim, accs = _LibShim(ops.lib, L.ACCUMULATE), []
    orig_lib, orig_run = ops.lib, KT.run.__func__

    def run(cls, kind, algo, flops, fn, tag=None, name=None):
        shim.last = 0
        r = orig_run(cls, kind, algo, flops, fn, tag, name)
        if cls.enabled:
            accs.append(shim.last)
        return r
    out = {}
    ops.lib, KT.run = shim, classmethod(run)
    try:
        for _ in range(n):
            KT.enabled, KT.records = True, []
            del accs[:]
            try:
                train.train_step(model, crit, opt, gb)
                torch.cuda.synchronize()
                for (kind, _algo, _fb, e0, e1, tag, name), acc in zip(KT.records, accs):
                    if kind.startswith("conv_"):
                        rec = out.setdefault((kind, tag), (name, [], []))
                        rec[1].append(e0.elapsed_time(e1)); rec[2].append(acc)
            finally:
                KT.enabled, KT.records = False, []
                ops.SidePrep.join()
    finally:
        ops.lib, KT.run = orig_lib, classmethod(orig_run)
    return out


def blocks(fns, nblocks, nsteps):
    ms = {k: [] for k in fns}
    for _ in range(nblocks):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(nsteps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / nsteps)
    return ms


def report(ms, names, unit):
    for k, name in names:
        v = ms[k]
        print(f"  {name:26s} median {statistics.median(v):7.3f}   min {min(v):7.3f}   max {max(v):7.3f}   blocks {' '.join(f'{t:.3f}' for t in v)}")
    m6, m7 = statistics.median(ms[6]), statistics.median(ms[7])
    spread = max(max(ms[6]) - min(ms[6]), max(ms[7]) - min(ms[7]))
    print(f"  {unit} ratio (algo 6 / algo 7, medians): {m6 / m7:.3f}x; difference {m6 - m7:.3f} ms, larger block spread of the two arms {spread:.3f} ms"
          f" -> {'MET' if m6 - m7 > spread else 'NOT MET'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--eager", type=int, default=5)
    a = ap.parse_args()
    import coma_unet_amd as cu
    from coma_unet_amd import train
    size = (a.size,) * 3
    print(f"# pointwise_f32: {a.size}^3 x {a.batch}, fp32 storage, static prompts, lr 0, {torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        m0, c0, _o, gb0 = build(0, size, a.batch)
        out0 = train.forward_loss(m0, c0, gb0)[1][0].float().clone()
        del m0, c0, _o, gb0
    arms = {algo: build(algo, size, a.batch) for algo in (6, 7)}
    with torch.no_grad():
        outs = {algo: train.forward_loss(m, c, gb)[1][0].float().clone() for algo, (m, c, _o, gb) in arms.items()}
    print(f"forward rel-L2, conv_algo=7 output against conv_algo=0 output: {rel(outs[7], out0):.3e}")
    print(f"forward rel-L2, conv_algo=6 output against conv_algo=0 output: {rel(outs[6], out0):.3e}")
    print(f"forward rel-L2, conv_algo=7 output against conv_algo=6 output: {rel(outs[7], outs[6]):.3e}")
    del outs, out0

    recs = {algo: eager_records(*arms[algo], a.eager) for algo in (6, 7)}

    steps = {algo: train.GraphedTrainStep(m, c, o, gb, warmup=2) for algo, (m, c, o, gb) in arms.items()}
    for algo in (6, 7):
        for _ in range(3):
            steps[algo]()
    torch.cuda.synchronize()
    ms = blocks(steps, a.blocks, a.steps)
    print(f"\nms/step, {a.blocks} alternating blocks of {a.steps} graph-replayed steps each:")
    report(ms, ((6, "conv_algo=6 (thin split)"), (7, "conv_algo=7 (pointwise)")), "step")

    print(f"\nper-launch HIP-event ms over {a.eager} eager steps (median [min .. max]); layer = (x shape, Cout, k, stride, form); "
          f"n = launches per step, acc = of them accumulating")
    print(f"{'kind':11s} {'layer':38s} {'n':>2s} {'acc':>3s} {'algo 6 kernel':34s} {'ms':>24s}   {'algo 7 kernel':34s} {'ms':>24s} {'ratio':>6s} {'diff':>7s} {'spread':>7s} {'':7s} {'MB':>7s} {'TB/s':>6s}")
    s6 = s7 = 0.0
    for key in sorted(recs[7], key=repr):
        n7, t7, acc7 = recs[7][key]
        if not n7.startswith(NEW) or key not in recs[6]:
            continue
        n6, t6, _ = recs[6][key]
        kind, (xs, cout, _k, _s, _f) = key
        f = lambda t: f"{statistics.median(t):8.3f} [{min(t):6.3f} .. {max(t):6.3f}]"
        md6, md7 = statistics.median(t6), statistics.median(t7)
        sp = max(max(t6) - min(t6), max(t7) - min(t7))
        per_step = len(t7) / a.eager
        vox = xs[0] * xs[1] * xs[2] * xs[3]
        c_in, c_out = (cout, xs[4]) if kind == "conv_dgrad" else (xs[4], cout)      # (a data gradient reads Cout channels, writes C)
        by = 4.0 * vox * (c_in + c_out + c_out * sum(acc7) / len(acc7))
        s6 += md6 * per_step; s7 += md7 * per_step
        print(f"{kind:11s} {str(key[1]):38s} {per_step:2.0f} {sum(acc7) / a.eager:3.0f} {n6:34s} {f(t6)}   {n7:34s} {f(t7)} {md6 / md7:6.2f} {md6 - md7:7.3f} {sp:7.3f} "
              f"{'MET' if md6 - md7 > sp else 'NOT MET':7s} {by / 1e6:7.1f} {by / (md7 * 1e-3) / 1e12:6.2f}")
    print(f"\nsummed over the launches above (medians): {s6:.3f} ms (algo 6) -> {s7:.3f} ms (algo 7) per step")
    other = sum(statistics.median(t) * len(t) / a.eager for k, (n, t, _) in recs[7].items() if not n.startswith(("conv_split",) + NEW))
    print(f"convolution launches outside every split and pointwise kernel's scope under conv_algo=7: {other:.3f} ms per step")

    # ---- the fp32 Predictor's eval forward under both modes ----
    del steps, recs
    preds = {}
    for algo in (6, 7):
        m, _c, _o, gb = arms[algo]
        m.eval()
        m.set_training(False)
        preds[algo] = cu.Predictor(m, gb, graph=True)
    del arms
    torch.cuda.empty_cache()
    y = {algo: p().float().clone() for algo, p in preds.items()}
    print(f"\nPredictor(graph=True) eval forward, fp32: output rel-L2 conv_algo=7 against conv_algo=6 {rel(y[7], y[6]):.3e}")
    del y
    for algo in (6, 7):
        for _ in range(3):
            preds[algo]()
    torch.cuda.synchronize()
    ms = blocks(preds, a.blocks, a.steps)
    print(f"ms per forward, {a.blocks} alternating blocks of {a.steps} forwards each:")
    report(ms, ((6, "conv_algo=6 (thin split)"), (7, "conv_algo=7 (pointwise)")), "forward")

    del preds
    torch.cuda.empty_cache()
    instances(a)


def instances(a):
    """Every kernel instance on stand-alone tensors, old kernel (conv_algo=6) against new (conv_algo=7)."""
    from coma_unet_amd import _lib as L
    from coma_unet_amd import ops
    dev = torch.device("cuda:0")
    print(f"\nkernel instances on stand-alone tensors, batch {a.batch}: ms per launch (10 launches per bracket, {a.blocks} alternating brackets), plain forward "
          f"(no statistics, no accumulate) / weight gradient (with its memset and replica sum)")
    print(f"{'kind':6s} {'C':>3s} {'N':>3s} {'grid':>5s} {'algo 6 kernel':34s} {'ms':>24s}   {'algo 7 kernel':34s} {'ms':>24s} {'ratio':>6s} {'diff':>7s} {'spread':>7s} {'':7s} {'TB/s':>6s}")
    probs = [("fwd", c, n) for n in (16, 64) for c in (8, 16, 24, 32, 40, 48, 56, 64)] + \
            [("fwd", 48, 32), ("fwd", 64, 32), ("wgrad", 8, 4), ("wgrad", 32, 16), ("wgrad", 16, 32), ("wgrad", 64, 32), ("wgrad", 32, 64), ("wgrad", 64, 64)]
    for side in (a.size // 2, a.size):
        for kind, c, n in probs:
            if side == a.size and c + n > 64:          # (the step's full-resolution level has 32 channels at most)
                continue
            torch.manual_seed(c * 100 + n)
            g = (a.batch, side, side, side)
            x = torch.randn(g + (c,), device=dev)
            y = torch.randn(g + (n,), device=dev)
            wk = torch.randn((1, 1, n, c), device=dev) / c ** 0.5
            names, fns = {}, {}
            for algo in (6, 7):
                if kind == "fwd":
                    fns[algo] = lambda algo=algo: ops._conv_fwd(x, wk, None, 1, 1, 0, False, algo, ops.Out(y), None)
                else:
                    fns[algo] = lambda algo=algo: ops._conv_bwd(x, None, y, 1, 1, 0, False, algo, (1, 1, n, c), False, True, 0, None)
                with torch.no_grad():
                    for _ in range(3):
                        fns[algo]()
                names[algo] = L.lib.coma_last_kernel().decode()
            torch.cuda.synchronize()
            with torch.no_grad():
                ms = blocks(fns, a.blocks, 10)
            f = lambda t: f"{statistics.median(t):8.3f} [{min(t):6.3f} .. {max(t):6.3f}]"
            md6, md7 = statistics.median(ms[6]), statistics.median(ms[7])
            sp = max(max(ms[6]) - min(ms[6]), max(ms[7]) - min(ms[7]))
            by = 4.0 * a.batch * side ** 3 * (c + n)
            verdict = ("MET" if md6 - md7 > sp else "NOT MET") if names[7].startswith(NEW) else "(same)"
            print(f"{kind:6s} {c:3d} {n:3d} {side:4d}^3 {names[6]:34s} {f(ms[6])}   {names[7]:34s} {f(ms[7])} {md6 / md7:6.2f} {md6 - md7:7.3f} {sp:7.3f} "
                  f"{verdict:7s} {by / (md7 * 1e-3) / 1e12:6.2f}")
            del x, y, wk, fns
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
