"""Shared by test_lr_schedule_cpu.py, test_lr_schedule_kernels_gpu.py and test_lr_schedule_step_gpu.py: the fp64 learning rate of
FusedAdamW(lr_schedule, param_options) -- through optim.LRSchedule.factor, the one place the formula lives -- with the absolute
error bound of the kernel's fp32 value carried alongside, and the sizes and segment layouts the kernels are run at.

The bound counts roundings from the kernel source (csrc/elementwise.hip: adamw_body<WINDOW, EMA, SCHED>, the block in front of
the segment staging), u = 2^-24; every operation is counted as rounded on its own (where the compiler fuses a multiply into an
add there is one rounding fewer, never one more):
  inputs ........................ base, warmup_start f0, min_ratio r and gamma reach the kernel as floats: u |x| each
  (float)min(s, Wm), (float)Wm,
  (float)u, (float)T, (float)(u / S)  exact below 2^24, else u |x|
  q = min / Wm .................. one rounding
  warm = f0 + (1 - f0) * q ...... three roundings (1 - f0; the product; the sum)
  x = PI_F * (u / T) ............ two roundings, and |PI_F - pi| = 8.75e-8 (PI_F = 3.14159265358979f rounds to 0x40490fdb)
  cosf(x) ....................... |cos'| <= 1 carries the error of x; the function itself: COS_ULPS ulp of a value <= 1,
                                  2 u each (x stays inside [0, pi]: no argument reduction)
  0.5f * (1 + cos) .............. one rounding (the sum; halving is exact)
  decay = r + (1 - r) * that .... three roundings;   linear: 1 - (1 - r) * (u / T): four
  powf(gamma, k) ................ gamma's own rounding k times over, and POW_ULPS ulp of the result
  lr_t = (base * warm) * decay .. two roundings
COS_ULPS = POW_ULPS = 4 is a budget above the accuracy the ROCm device library states for either function; the whole bound
must stay <= 1e-5 * base for every case tested (test_lr_schedule_cpu.py checks that), so the budget cannot hide a wrong count:
a kernel one update off lies 1e-2 * base or more away.
"""
import math

import numpy as np

import _ema_plan as EP
import _nonconv_plan as NP

U = NP.U_F32
THREADS, EW_CAP = NP.THREADS, NP.EW_CAP
CASES = EP.CASES                      # (name, n, element offset): tiny / vec4 / scalar / few
PI_F = float(np.float32(3.14159265358979))
COS_ULPS = POW_ULPS = 4
REL_CAP = 1e-5                        # the bound of every tested case stays below REL_CAP * base
MAX_SEGS = 2048                       # the kernel's cap (ops.MAX_SEGS; test_lr_schedule_cpu.py checks they agree)

BASE = NP.ADAMW_HP[0]
WM, T = 3, 8
STEPS = (1, 2, WM, WM + 1, WM + (T + 1) // 2, WM + T, WM + T + 5)
# name -> LRSchedule arguments
KINDS = {
    "constant": dict(warmup_steps=WM, warmup_start=1.0 / 3.0, decay="constant"),
    "cosine": dict(warmup_steps=WM, warmup_start=1.0 / 3.0, decay="cosine", total_steps=T, min_ratio=0.1),
    "linear": dict(warmup_steps=WM, warmup_start=1.0 / 3.0, decay="linear", total_steps=T, min_ratio=0.1),
    "step": dict(warmup_steps=WM, warmup_start=1.0 / 3.0, decay="step", step_size=3, gamma=0.5),
}
LONG = (dict(warmup_steps=0, decay="cosine", total_steps=100000, min_ratio=0.0), 60001)      # (arguments, t)
STEP_SCHED = dict(warmup_steps=2, decay="cosine", total_steps=4, min_ratio=0.1)             # test_lr_schedule_step_gpu.py
STEP_SCHED_LOOP = dict(warmup_steps=3, decay="cosine", total_steps=20, min_ratio=0.1)       # its train_dp run


def schedule(args):
    from coma_unet_amd.optim import LRSchedule
    return args if isinstance(args, LRSchedule) else LRSchedule(**args)


def lr_ref(args, base, t):
    """fp64: base * factor(t - 1) for the update that brings the count to t."""
    return float(base) * schedule(args).factor(t - 1)


# ---- (value, absolute error of the fp32 computation) pairs -------------------------------------------------------------
def _inp(x):
    return (float(x), U * abs(float(x)))


def _int(i):
    return (float(i), 0.0 if abs(i) <= 2 ** 24 else U * abs(i))


def _rnd(v, e):
    return (v, e + U * (abs(v) + e))


def _add(a, b, sign=1.0):
    return _rnd(a[0] + sign * b[0], a[1] + b[1])


def _mul(a, b):
    return _rnd(a[0] * b[0], abs(a[0]) * b[1] + abs(b[0]) * a[1] + a[1] * b[1])


def _div(a, b):
    lo = abs(b[0]) - b[1]
    assert lo > 0
    v = a[0] / b[0]
    return _rnd(v, a[1] / lo + abs(v) * b[1] / lo)


ONE = (1.0, 0.0)


def lr_bound(args, base, t):
    """-> (fp64 lr_t, absolute bound of the kernel's fp32 lr_t)."""
    sc = schedule(args)
    s = max(t - 1, 0)
    Wm, Tt = sc.warmup_steps, sc.total_steps
    warm = ONE
    if Wm > 0:
        f0 = _inp(sc.warmup_start)
        warm = _add(f0, _mul(_add(ONE, f0, -1.0), _div(_int(min(s, Wm)), _int(Wm))))
    u = max(s - Wm, 0)
    if sc.decay != "step" and Tt is not None:
        u = min(u, Tt)
    dec = ONE
    if sc.decay == "cosine":
        r = _inp(sc.min_ratio)
        x = _mul((math.pi, abs(PI_F - math.pi)), _div(_int(u), _int(Tt)))
        c = (math.cos(x[0]), x[1] + COS_ULPS * 2 * U)
        half = _add(ONE, c)
        half = (0.5 * half[0], 0.5 * half[1])
        dec = _add(r, _mul(_add(ONE, r, -1.0), half))
    elif sc.decay == "linear":
        r = _inp(sc.min_ratio)
        dec = _add(ONE, _mul(_add(ONE, r, -1.0), _div(_int(u), _int(Tt))), -1.0)
    elif sc.decay == "step":
        k = u // sc.step_size
        v = sc.gamma ** k
        dec = (v, v * ((1 + U) ** k - 1) + _int(k)[1] * abs(v * math.log(sc.gamma)) + POW_ULPS * 2 * U * v)
    lr = _mul(_mul(_inp(base), warm), dec)
    ref = lr_ref(sc, base, t)
    assert abs(lr[0] - ref) <= 1e-12 * abs(ref) + 1e-300, (lr[0], ref)      # the same formula, restated
    return ref, lr[1]


def lr_f32(args, base, t):
    """The kernel's expressions in numpy float32 on the host (numpy's cos / power in place of cosf / powf): a CPU stand-in
    that lets test_lr_schedule_cpu.py try the bound without a GPU."""
    f = np.float32
    sc = schedule(args)
    kind, Wm, f0, Tt, r, S, gamma = sc.kernel_args()
    f0, r, gamma = f(f0), f(r), f(gamma)
    s = max(t - 1, 0)
    warm = f(1)
    if Wm > 0:
        warm = f(f0 + f(f(f(1) - f0) * f(f(min(s, Wm)) / f(Wm))))
    u = max(s - Wm, 0)
    if sc.decay != "step":
        u = min(u, Tt)
    dec = f(1)
    if sc.decay == "cosine":
        dec = f(r + f(f(f(1) - r) * f(f(0.5) * f(f(1) + np.cos(f(f(PI_F) * f(f(u) / f(Tt))), dtype=f)))))
    elif sc.decay == "linear":
        dec = f(f(1) - f(f(f(1) - r) * f(f(u) / f(Tt))))
    elif sc.decay == "step":
        dec = np.power(gamma, f(u // S), dtype=f)
    return float(f(f(f(base) * warm) * dec))


# ---- segment layouts -----------------------------------------------------------------------------------------------------
def segment_ends(n):
    """Boundaries inside and at the edge of the first 16-byte chunk (1, 3, 4), at the edge between two blocks' chunks (1023,
    1024, 1025), a run of segments of lengths 1, 1, 2 inside one chunk (2048 .. 2052), one just past the first grid pass
    (4 * THREADS * EW_CAP + 2) and one inside the scalar tail (n - 2); the last segment ends at n."""
    grid = 4 * THREADS * EW_CAP
    assert n > grid + 8 and n % 4 == 3
    return [1, 3, 4, 1023, 1024, 1025, 2048, 2049, 2050, 2052, grid + 2, n - 2, n]


def segment_options(k):
    """Distinct (lr_scale, weight_decay) per segment, among them a scale of 0 and a decay of 0."""
    scales = [1.0, 0.0, 0.5, 2.0, 0.1, 1.5, 0.25, 3.0, 0.75, 1.25, 0.05, 0.6, 1.75]
    wds = [1e-2, 0.1, 0.0, 0.3, 5e-2, 0.2, 1e-3, 0.0, 0.15, 2e-2, 0.25, 0.07, 0.12]
    assert k <= len(scales)
    return scales[:k], wds[:k]
