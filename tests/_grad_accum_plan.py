"""Shared by test_grad_accum_cpu.py, test_grad_accum_kernels_gpu.py and test_grad_accum_step_gpu.py: the fp64 restatement
of one accumulation window of FusedAdamW(grad_acc_batch, max_grad_norm) -- accumulate, mean, global norm, clip coefficient,
then _nonconv_plan.adamw_step -- with the error bounds of the kernels' arithmetic carried alongside the values.

The bounds count roundings from the kernel sources (csrc/elementwise.hip: grad_accum_k; adamw_body<WINDOW>, the body of
adamw_ex_k), u = 2^-24:
  acc = g ......................... exact
  acc += g ........................ one rounding of the new value: u |acc|
  sum of squares .................. squares and sums in fp64: (n + 2) 2^-53 relative, on top of what acc's error moves it
  norm = sqrt(sum) / count ........ fp64: 2 more roundings of 2^-53; half the relative error of the sum
  c = min(1, max / (norm + 1e-6)) . fp64; min is 1-Lipschitz: the relative error of the norm, 2 roundings of 2^-53
  s = (float)(c / count) .......... one fp64 rounding, ONE fp32 rounding
  g^ = acc * s .................... one more fp32 rounding
and the error of g^ enters adamw_k's recurrence (m = b1 m + (1 - b1) g^, v = b2 v + (1 - b2) g^ g^) with the weights
(1 - b1) into m and (1 - b2) (2 |g^| + e) e into v, and reaches p through them (_nonconv_plan.adamw_step derives the bound
of the update from the bounds of m and v).
"""
import torch

import _nonconv_plan as NP

U = NP.U_F32
U64 = NP.U_F64
THREADS = 256
ACC_CAP = 1024                 # ACC_BLOCKS of elementwise.hip: grid cap of grad_accum_k, longest table of partials
ACC_UNROLL = 2                 # trips of grad_accum_k's float4 loop taken together
CLIP_EPS = 1e-6                # torch.nn.utils.clip_grad_norm_'s

# grad_accum_k / adamw_ex_k: (name, n, element offset of the slices into 16-byte aligned buffers)
CASES = [("tiny", 5, 0),                                               # one partly filled block
         ("vec4", 4 * THREADS * ACC_CAP + 1027, 0),                    # float4 path past one grid pass, 3-element scalar tail
         ("scalar", THREADS * ACC_CAP + 259, 1),                       # scalar path (not 16-byte aligned) past one grid pass
         ("few", 4 * THREADS * 37 + 2, 0),                             # fewer blocks than the cap
         # grad_accum_k takes two trips of its grid-stride loop at a time: every thread once through that unrolled loop,
         # the first 700 once more through the single trip behind it
         ("unroll", 4 * (ACC_UNROLL * THREADS * ACC_CAP + 700) + 3, 0)]


def accum_blocks(n, aligned):
    """Blocks coma_grad_accum launches = live partials."""
    if n == 0:
        return 0
    items = NP.cdiv(n, 4) if aligned else n
    return max(1, min(NP.cdiv(items, THREADS), ACC_CAP))


def accumulate(gs):
    """Prefix sums of the micro-batch gradients in fp64 and the bound of the fp32 accumulator after each:
    -> [(A_j, b_j)], A_0 = g_0 exactly, b_j = (b_{j-1} + u |A_j|)(1 + 2u) (the rounding is relative to the COMPUTED value,
    which is within b_j of A_j)."""
    out = []
    A = gs[0].double().clone()
    b = torch.zeros_like(A)
    out.append((A.clone(), b.clone()))
    for g in gs[1:]:
        A = A + g.double()
        b = (b + U * A.abs()) * (1 + 2 * U)
        out.append((A.clone(), b.clone()))
    return out


def sumsq(A, b):
    """fp64 sum of squares of an accumulator and the relative bound of the kernel's (fp64 sums over the fp32 values)."""
    s = float((A * A).sum())
    moved = float((2 * A.abs() * b + b * b).sum())
    return s, (moved / s if s > 0 else 0.0) + (A.numel() + 2) * U64


def scale(total, rel_total, count, max_norm):
    """norm, clip coefficient and s = c / count of the kernel from the window's total sum of squares.
    -> dict(norm, b_norm (of the fp32 norm_out), c, s, e_s (relative bound of the fp32 s))."""
    norm = total ** 0.5 / count
    e_norm = 0.5 * rel_total * (1 + rel_total) + 2 * U64
    if max_norm is None:
        c, e_c = 1.0, 0.0
    else:
        mx = NP.f32(max_norm)                       # the kernel takes max_norm as a float
        c = min(1.0, mx / (norm + CLIP_EPS))
        e_c = e_norm + 2 * U64
    s = c / count
    return dict(norm=norm, b_norm=norm * (e_norm + U * (1 + e_norm)), c=c, s=s, e_s=(e_c + U64) * (1 + U) + U)


def apply(st, A, b, sc, t, hp=NP.ADAMW_HP):
    """One update of the state `st` (_nonconv_plan.adamw_init) with g^ = A * s, in place.  The input error
    e = (b s + |A| s (e_s + u))(1 + 4u) is injected into the running bounds of m and v before the step: adamw_step scales
    the old bounds by b1 / b2, so the injected terms are divided by them -- after the step they stand with the weights named in
    the module docstring, and adamw_step carries them into the bound of p.  -> (g^, e, adamw_step's report)."""
    b1, b2 = NP.f32(hp[1]), NP.f32(hp[2])
    ghat = A * sc["s"]
    e = (b * abs(sc["s"]) + ghat.abs() * (sc["e_s"] + U)) * (1 + 4 * U)
    st["bm"] = st["bm"] + (1 - b1) * e / b1
    st["bv"] = st["bv"] + (1 - b2) * (2 * ghat.abs() + e) * e / b2
    info = NP.adamw_step(st, ghat, t, hp)
    return ghat, e, info


def window(st, gs, t, max_norm=None, extra_total=0.0, extra_rel=0.0, hp=NP.ADAMW_HP):
    """A whole window on one flat tensor: micro-batch gradients `gs` (fp32 values), update number t.  extra_total /
    extra_rel: the sum of squares of the accumulated gradients outside this tensor and its relative bound.
    -> dict(acc [(A_j, b_j)], total, norm, b_norm, c, s, e_s, ghat, b_ghat)."""
    acc = accumulate(gs)
    A, b = acc[-1]
    tot, rel = sumsq(A, b)
    total = tot + extra_total
    rel_total = (tot * rel + extra_total * extra_rel) / total if total > 0 else 0.0
    sc = scale(total, rel_total, len(gs), max_norm)
    ghat, e, info = apply(st, A, b, sc, t, hp)
    return dict(acc=acc, total=total, ghat=ghat, b_ghat=e, info=info, **sc)
