"""Shared by test_ema_cpu.py, test_ema_kernels_gpu.py and test_ema_step_gpu.py: the fp64 restatement of the weight average of
FusedAdamW(ema_decay, ema_warmup) -- the decay d_t and e' = e + (1 - d_t)(p' - e) -- with the error bound of the kernel's
fp32 arithmetic carried alongside, and the sizes at which the kernels are run.

The bound counts roundings from the kernel source (csrc/elementwise.hip: adamw_body<WINDOW, EMA>, the body of adamw_ema_k),
u = 2^-24:
  d_t ........................... ema_decay as passed (a float), or fminf(ema_decay, (1.f + t) / (10.f + t)): both sums are
                                  exact (small integers), the division rounds once: u d absolute; fminf is exact
  w = 1.f - d_t ................. one rounding: u w;  together |w^ - w| <= u (d + w)(1 + u) = u (1 + u)
  diff = p' - e ................. one rounding: u |diff|
  e' = fmaf(w, diff, e) ......... ONE rounding of the result: u |e'|
and the error b the stored average already carries: it reaches e' with the weight (1 - w) and widens |diff| by b:
  b' = ((1 - w) b + (u (1 + u) + u w)(|p' - e| + b) + u |e'|)(1 + 4u)
(the last factor: the roundings are relative to computed values that lie within the bound of the exact ones).  p' is the
kernel's own fp32 parameter: the recurrence takes it as exact input.
"""
import torch

import _nonconv_plan as NP

U = NP.U_F32
THREADS = NP.THREADS
EW_CAP = NP.EW_CAP             # ew_grid's cap: adamw_ema_k and swap_f32_k launch at most this many blocks of 256 threads
WARM_A, WARM_B = 1.0, 10.0     # d_t = min(d, (WARM_A + t) / (WARM_B + t))

# adamw_ema_k / swap_f32_k: (name, n, element offset of the slices into 16-byte aligned buffers)
CASES = [("tiny", 5, 0),                                           # one partly filled block
         ("vec4", 4 * (THREADS * EW_CAP + 256) + 3, 0),            # 16-byte path past one grid pass, 3-element scalar tail
         ("scalar", THREADS * EW_CAP + 259, 1),                    # scalar path (one element off 16-byte alignment), past one pass
         ("few", 4 * THREADS * 37 + 2, 0)]                         # fewer blocks than the cap


def blocks(n, aligned):
    """Blocks coma_adamw_ema / coma_swap_f32 launch."""
    if n == 0:
        return 0
    return NP.ew_grid(NP.cdiv(n, 4) if aligned else n)


def decay_at(decay, warmup, t):
    """-> (d_t in fp64 from the float the kernel receives, absolute bound of the kernel's fp32 w = 1 - d_t)."""
    d = NP.f32(decay)
    if warmup:
        d = min(d, (WARM_A + t) / (WARM_B + t))
    return d, U * (1 + U)


def ema_init(e0):
    return dict(e=e0.double().clone(), b=torch.zeros_like(e0, dtype=torch.float64))


def ema_update(st, p_new, decay, warmup, t):
    """One update of the state `st` (ema_init) with the fp32 parameters `p_new` of update number t, in place.  -> d_t."""
    d, e_w = decay_at(decay, warmup, t)
    w = 1.0 - d
    e, b = st["e"], st["b"]
    diff = p_new.double() - e
    new = e + w * diff
    st["b"] = ((1 - w) * b + (e_w + U * w) * (diff.abs() + b) + U * new.abs()) * (1 + 4 * U)
    st["e"] = new
    return d
