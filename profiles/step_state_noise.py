"""Measures what tests/test_step_state_gpu.py's bounds are derived from and writes profiles/step_state_noise.txt:

  1. the repeat spread of the stateless reference: five evaluations of the same (weights, batch) per measured step, every pair
     compared per tensor as |a - b| / (|a| + FLOOR * gmax * sqrt(numel)) -- the form of the test's bound --, worst tensor per
     conv mode and tensor class over the four steps;
  2. the bounds derived from it: 4 x the worst spread seen in this run or recorded from an earlier one (RECORDED), rounded up
     to two digits, never below the starting bound of the mode; the loss bound never below 8 ulp of the fp32 loss value;
  3. the power condition under those bounds: how far the reference gradients of consecutive steps lie apart;
  4. the distance of the stateful default-switch trajectory from the reference, in units of its bound (what the tests assert).

    python profiles/step_state_noise.py [OUT.txt]
"""
import itertools
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _step_state as ss      # noqa: E402

REPEATS = 5
MARGIN = 4.0
# bounds a mode starts from: the direct kernels' 1e-3 per tensor and 1e-5 on the loss (test_model_gpu.py); the other modes
# start from nothing but their own spread
START = {"fp32-direct": {"conv": 1e-3, "scalar": 1e-3, "prompt": 1e-3, "loss": 1e-5}}
# the loss is one fp32 number merged by atomics: repeats land on neighbouring fp32 values (spread 1.1e-7 = 1 ulp at a loss of
# ~64), and five repeats do not see the tail of that -- no loss bound below 8 ulp
LOSS_FLOOR = 8 * 2.0 ** -23
# Worst spreads of earlier runs of this script (profiles/step_state_noise.txt keeps their records).  The merge-order noise is
# heavy-tailed: between two runs the worst tensor of a class moved by up to 5x (fp32-auto conv 2.6e-2 / 5.3e-3, bf16-auto
# scalar 8.0 / 20.7), so the bounds come from everything measured so far, not from the last five repeats alone.
RECORDED = {
    "fp32-direct": {"conv": 4.492e-07, "scalar": 1.969e-06, "prompt": 0.0, "loss": 0.0},
    "fp32-auto": {"conv": 2.574e-02, "scalar": 2.092e-01, "prompt": 2.585e-03, "loss": 1.109e-07},
    "bf16-auto": {"conv": 8.039e-01, "scalar": 2.074e+01, "prompt": 1.477e-01, "loss": 2.433e-04},
    "split": {"conv": 9.570e-03, "scalar": 1.053e-01, "prompt": 8.085e-03, "loss": 2.191e-07},
    "split-wide": {"conv": 6.987e-03, "scalar": 4.321e-02, "prompt": 4.693e-03, "loss": 1.260e-07},
}


def round_up(x):
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return float(f"{math.ceil(x / 10 ** e - 1e-9) * 10 ** e:.1e}")


def main(out_path):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tests/_step_state.py: A = {ss.A}, seed {ss.SEED}, warm-up {ss.WARMUP}, measured steps {ss.MEASURED}, FLOOR = {ss.FLOOR}")
    say(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    derived = {}
    for mode in ss.MODES:
        t0 = time.time()
        say(f"\n== {mode}: {ss.MODES[mode][0]} at {ss.MODES[mode][1]}")
        worst = {"conv": (0.0, ""), "scalar": (0.0, ""), "prompt": (0.0, ""), "loss": (0.0, "")}
        plain = {"conv": (0.0, ""), "scalar": (0.0, ""), "prompt": (0.0, "")}      # |a - b| / |a| without the floor, for the record
        for k in ss.MEASURED:
            m = ss.fresh_model(mode)
            for j in range(1, k + 1):
                ss.perturb(m, j)
            reps = [ss.stateless(m, ss.batch(mode, k)) for _ in range(REPEATS)]
            del m
            for (ga, la), (gb, lb) in itertools.combinations(reps, 2):
                dist, gmax = ss.distances(gb, ga)
                for n, numel, d, r in dist:
                    c = ss.tensor_class(n)
                    s = d / (r + ss.FLOOR * gmax * numel ** 0.5) if d > 0 else 0.0
                    if s > worst[c][0]:
                        worst[c] = (s, f"{n} step {k}")
                    if r > 0 and d / r > plain[c][0]:
                        plain[c] = (d / r, f"{n} step {k}")
                s = abs(la - lb) / abs(la)
                if s > worst["loss"][0]:
                    worst["loss"] = (s, f"step {k}")
            del reps
        say("repeat spread of the stateless reference (worst tensor of the class, 4 steps x 10 pairs of 5 repeats):")
        for c, (s, n) in worst.items():
            say(f"  {c:7s} {s:.3e}   {n}" + (f"      [without the floor: {plain[c][0]:.3e} {plain[c][1]}]" if c in plain else ""))
        start = START.get(mode, {})
        rec = RECORDED.get(mode, {})
        derived[mode] = {c: max(start.get(c, 0.0), round_up(MARGIN * max(s, rec.get(c, 0.0)))) for c, (s, _) in worst.items()}
        derived[mode]["loss"] = max(derived[mode]["loss"], round_up(LOSS_FLOOR))
        say(f"worst spreads recorded before this run: {rec}")
        say(f"derived bounds ({MARGIN:g} x the worst spread of this run and the recorded ones, rounded up, not below the mode's "
            f"starting bounds): {derived[mode]}")
        ss.TOL[mode] = derived[mode]
        say("power: consecutive reference steps, tensors closer than 4 bounds")
        for k in ss.MEASURED:
            ref, prev = ss.reference(mode, k)[0], ss.reference(mode, k - 1)[0]
            weak, st, se, zero = ss.power(mode, ref, prev)
            dist, gmax = ss.distances(prev, ref)
            ratios = sorted(d / r for _, _, d, r in dist if r > 0)
            say(f"  step {k} vs {k - 1}: |ref_k - ref_k-1| / |ref_k| min {ratios[0]:.3e} median {ratios[len(ratios) // 2]:.3e}; "
                f"weak {len(weak)} of {len(dist)} tensors ({st:.2%}), {se:.5%} of the elements; "
                f"{len(zero)} more are exactly zero in both steps; weak: {weak}")
        say("stateful default-switch trajectory against the reference, worst |got - ref| / bound per class:")
        run = ss.Run(mode)
        for k in ss.MEASURED:
            ref_g, ref_l = ss.reference(mode, k)
            try:
                got_g, got_l = run.take(k)
            except AssertionError as e:
                say(f"  step {k}: {e!r}")
                break
            say(f"  step {k}: PrepAhead served {run.prep_ahead_used} layers so far, WgradSide.launched {ss.ops_counts()}")
            dist, gmax = ss.distances(got_g, ref_g)
            w = {}
            for n, numel, d, r in dist:
                c = ss.tensor_class(n)
                q = d / ss.bound(derived[mode][c], numel, r, gmax)
                if q >= w.get(c, (-1.0, ""))[0]:
                    w[c] = (q, n)
            say(f"  step {k}: " + "; ".join(f"{c} {q:.3f} ({n})" for c, (q, n) in w.items())
                + f"; loss {abs(got_l - ref_l) / abs(ref_l) / derived[mode]['loss']:.3f}")
        del run
        torch.cuda.synchronize()
        say(f"({time.time() - t0:.1f} s)")
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    say("\nTOL = {")
    for mode, d in derived.items():
        say(f'    "{mode}": {d},')
    say("}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "step_state_noise.txt"))
