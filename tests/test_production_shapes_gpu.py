"""Every kernel of the benched step (128^3, batch 2, bf16, per-sample CondConv weights) at its real shape against the
full-size fp64 reference of oracle/fp64_ref.py.

The per-kernel tests of test_ops_gpu.py run tiny grids: a persistent kernel's tile-to-tile loop, the 1024 / G row-chunk
cap of the norm statistics and the 2M-voxel weight-gradient reductions only run at production size.  Here every
convolution call of one eager training step is a row of PRODUCTION_ROWS (harvested: test_harvest_matches_table), and
each row is checked at its full shape with two checks that together catch one wrong tile:
  * the worst-case per-element bound |got - ref| <= 2^-8 |ref| + 2 K 2^-24 A (+ 2^-8 |base| when accumulating),
    A = |x| (*) |w| + |b| -- it holds for any summation order, so it cannot fail on a correct kernel;
  * the maximum over slabs of rel-L2: a slab is one (sample, z-plane), or one (sample, tap) of a weight gradient.
"""
import gc
import os
import zlib

import pytest
import torch

from oracle import fp64_ref as R

pytestmark = pytest.mark.gpu

SIZE, BATCH, E = (128, 128, 128), 2, 8
SLAB_TOL = 5e-3          # bf16 outputs: max over (sample, z-plane) slabs of rel-L2
WGRAD_SLAB_TOL = 1e-4    # fp32 weight gradients: max over (sample, tap) slabs of rel-L2

_NORMS = {None: "-", 0: "batch", 1: "instance"}          # (L.NORM_BATCH, L.NORM_INSTANCE)
_ACTS = ["none", "relu", "prelu", "leaky", "sigmoid", "prelu_relu"]      # (L.ACT_* codes)


def _ops():
    from coma_unet_amd import ops, _lib
    return ops, _lib


def _dt(t):
    return "bf16" if t.dtype == torch.bfloat16 else ("f32" if t.dtype == torch.float32 else str(t.dtype))


# ---------------------------------------------------------------------------------------------------------------------
# harvest: what one eager step runs
# ---------------------------------------------------------------------------------------------------------------------
def harvest(size=SIZE, batch=BATCH):
    """One eager train_step of the benched model with ops._conv_fwd / ops._conv_bwd / NormAct / GateFused wrapped;
    -> sorted list of row tuples (see PRODUCTION_ROWS).  ops.KernelTimer is on for the step (it names the kernel of
    every launch); it also keeps the weight gradients off the side stream -- the kernels are the same, only the
    stream they are queued on differs."""
    ops, L = _ops()
    import coma_unet_amd as cu
    from coma_unet_amd import synthetic, train
    from coma_unet_amd.criterions import build_reference_criterion
    KT = ops.KernelTimer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=size, compute_dtype=torch.bfloat16, static_prompts=True).to(dev)
    model.set_save_attn(None)
    model.train(True)
    crit = build_reference_criterion(dev)
    opt = train.make_optimizer(model, 1e-3)
    b = synthetic.make_batch(batch, size, seed=1000)
    gb = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
    gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], batch, dev)
    rows = set()
    o_fwd, o_bwd = ops._conv_fwd, ops._conv_bwd
    o_norm, o_gate = ops.NormAct.apply, ops.GateFused.apply

    def names(n0, kind):
        return [r[6] for r in KT.records[n0:] if r[0] == kind]

    def fwd(x, wk_f, bias, ksize, stride, form, per_sample, algo, out, norm):
        n0 = len(KT.records)
        y, sums = o_fwd(x, wk_f, bias, ksize, stride, form, per_sample, algo, out, norm)
        mode = norm[0] if isinstance(norm, (tuple, list)) else norm
        rows.add(("fwd", tuple(x.shape), _dt(x), wk_f.shape[2], ksize, stride, form, bool(per_sample), algo, _dt(wk_f),
                  _NORMS[mode], bias is not None, x.stride(3), y.stride(3), names(n0, "conv_fwd")[-1]))
        return y, sums

    def bwd(x, wk_d, dy, ksize, stride, form, per_sample, algo, wshape, need_dx, need_dw, bias_mode, p_bias, fork=None,
            side=False):
        n0 = len(KT.records)
        pre = None if fork is None else fork.buf is not None
        dx, dwk, dbias = o_bwd(x, wk_d, dy, ksize, stride, form, per_sample, algo, wshape, need_dx, need_dw, bias_mode, p_bias,
                               fork, side)
        key = (tuple(x.shape), _dt(x), dy.shape[4], ksize, stride, form, bool(per_sample), algo)
        if need_dx:
            tgt = "plain" if fork is None else ("fork+=" if (pre and dx is None) else ("fork=" if not pre else "fork+add"))
            rows.add(("dgrad",) + key + (_dt(wk_d), tgt, dy.stride(3), x.stride(3), names(n0, "conv_dgrad")[-1]))
        if need_dw:
            rows.add(("wgrad",) + key + (bias_mode, x.stride(3), dy.stride(3), names(n0, "conv_wgrad")[-1]))
        return dx, dwk, dbias

    def norm(x, gamma, beta, slope, rmean, rvar, mode, act, momentum, eps, training, out, pre=None):
        rows.add(("norm", tuple(x.shape), _dt(x), _NORMS[mode], _ACTS[act], gamma is not None, slope is not None, pre is not None,
                  x.stride(3), out.t.stride(3) if out is not None else x.shape[4]))
        return o_norm(x, gamma, beta, slope, rmean, rvar, mode, act, momentum, eps, training, out, pre)

    def gate(x, g1raw, *rest):
        rows.add(("gate", tuple(x.shape), _dt(x), g1raw.shape[4], x.stride(3), rest[-1].t.stride(3) if rest[-1] is not None else x.shape[4]))
        return o_gate(x, g1raw, *rest)

    ops._conv_fwd, ops._conv_bwd = fwd, bwd
    ops.NormAct.apply, ops.GateFused.apply = staticmethod(norm), staticmethod(gate)      # (shadow Function.apply)
    KT.enabled, KT.records = True, []
    try:
        train.train_step(model, crit, opt, gb)
        torch.cuda.synchronize()
    finally:
        ops._conv_fwd, ops._conv_bwd = o_fwd, o_bwd
        del ops.NormAct.apply, ops.GateFused.apply
        KT.enabled, KT.records = False, []
        ops.SidePrep.join()
    del model, opt, gb
    gc.collect()
    torch.cuda.empty_cache()
    return sorted(rows, key=repr)


# The harvested table.  conv rows: (what, x shape (B, D, H, W, C), dtype, Cout, k, stride, form (1 = transposed),
# per-sample, algo, weight dtype, <fwd: norm mode, bias | dgrad: target | wgrad: bias mode>, pitches, kernel).
PRODUCTION_ROWS = [
    ('dgrad', (2, 128, 128, 128, 16), 'bf16', 1, 3, 1, 0, False, 0, 'bf16', 'plain', 8, 16, 'conv_thin16_k<8, 1>'),
    ('dgrad', (2, 128, 128, 128, 16), 'bf16', 16, 3, 1, 0, False, 0, 'bf16', 'plain', 16, 16, 'conv_thin16_k<16, 1>'),
    ('dgrad', (2, 128, 128, 128, 2), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'plain', 8, 8, 'p1_scale_k<__bf16>'),
    ('dgrad', (2, 128, 128, 128, 2), 'bf16', 8, 3, 1, 0, False, 0, 'bf16', 'plain', 8, 8, 'conv_thin16_k<8, 1>'),
    ('dgrad', (2, 128, 128, 128, 3), 'bf16', 16, 3, 1, 0, False, 0, 'bf16', 'plain', 16, 8, 'conv_thin16_k<16, 1>'),
    ('dgrad', (2, 128, 128, 128, 32), 'bf16', 1, 1, 1, 0, True, 0, 'f32', 'plain', 1, 32, 'p1_scale_k<__bf16>'),
    ('dgrad', (2, 128, 128, 128, 32), 'bf16', 16, 1, 1, 0, False, 0, 'bf16', 'fork+=', 16, 32, 'conv_mfma_pw_k<1, 1>'),
    ('dgrad', (2, 128, 128, 128, 32), 'bf16', 16, 1, 1, 0, False, 0, 'bf16', 'fork+=', 16, 64, 'conv_mfma_pw_k<1, 1>'),
    ('dgrad', (2, 128, 128, 128, 32), 'bf16', 32, 3, 1, 0, True, 0, 'bf16', 'plain', 32, 32, 'conv_mfma_duo_k<0, 5>'),
    ('dgrad', (2, 128, 128, 128, 32), 'bf16', 64, 3, 2, 0, True, 0, 'bf16', 'fork+=', 64, 32, 'conv_mfma_tconv_k<__bf16, 0>'),
    ('dgrad', (2, 128, 128, 128, 64), 'bf16', 32, 3, 1, 0, False, 0, 'bf16', 'plain', 32, 64, 'conv_mfma_duo_k<0, 5>'),
    ('dgrad', (2, 128, 128, 128, 8), 'bf16', 1, 3, 1, 0, False, 0, 'bf16', 'plain', 8, 8, 'conv_thin16_k<8, 1>'),
    ('dgrad', (2, 128, 128, 128, 8), 'bf16', 8, 3, 1, 0, False, 0, 'bf16', 'plain', 8, 8, 'conv_thin16_k<8, 1>'),
    ('dgrad', (2, 16, 16, 16, 256), 'bf16', 128, 1, 1, 0, False, 0, 'bf16', 'fork+=', 128, 256, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('dgrad', (2, 16, 16, 16, 256), 'bf16', 128, 1, 1, 0, False, 0, 'bf16', 'fork+=', 128, 512, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('dgrad', (2, 16, 16, 16, 256), 'bf16', 128, 3, 2, 1, True, 0, 'bf16', 'plain', 128, 256, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('dgrad', (2, 16, 16, 16, 256), 'bf16', 256, 3, 1, 0, True, 0, 'bf16', 'plain', 256, 256, 'conv_mfma_duo_k<0, 4>'),
    ('dgrad', (2, 16, 16, 16, 256), 'bf16', 512, 3, 2, 0, True, 0, 'bf16', 'fork+=', 512, 256, 'conv_mfma_gather_k<128, 1, __bf16>'),
    ('dgrad', (2, 16, 16, 16, 512), 'bf16', 256, 3, 1, 0, False, 0, 'bf16', 'plain', 256, 512, 'conv_mfma_duo_k<0, 4>'),
    ('dgrad', (2, 32, 32, 32, 128), 'bf16', 128, 3, 1, 0, True, 0, 'bf16', 'plain', 128, 128, 'conv_mfma_duo_k<0, 5>'),
    ('dgrad', (2, 32, 32, 32, 128), 'bf16', 256, 3, 2, 0, True, 0, 'bf16', 'fork+=', 256, 128, 'conv_mfma_gather_k<128, 1, __bf16>'),
    ('dgrad', (2, 32, 32, 32, 128), 'bf16', 64, 1, 1, 0, False, 0, 'bf16', 'fork+=', 64, 128, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('dgrad', (2, 32, 32, 32, 128), 'bf16', 64, 1, 1, 0, False, 0, 'bf16', 'fork+=', 64, 256, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('dgrad', (2, 32, 32, 32, 128), 'bf16', 64, 3, 2, 1, True, 0, 'bf16', 'plain', 64, 128, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('dgrad', (2, 32, 32, 32, 256), 'bf16', 128, 3, 1, 0, False, 0, 'bf16', 'plain', 128, 256, 'conv_mfma_duo_k<0, 5>'),
    ('dgrad', (2, 64, 64, 64, 128), 'bf16', 64, 3, 1, 0, False, 0, 'bf16', 'plain', 64, 128, 'conv_mfma_duo_k<0, 5>'),
    ('dgrad', (2, 64, 64, 64, 64), 'bf16', 128, 3, 2, 0, True, 0, 'bf16', 'fork+=', 128, 64, 'conv_mfma_tconv_k<__bf16, 0>'),
    ('dgrad', (2, 64, 64, 64, 64), 'bf16', 32, 1, 1, 0, False, 0, 'bf16', 'fork+=', 32, 128, 'conv_mfma_pw_k<2, 2>'),
    ('dgrad', (2, 64, 64, 64, 64), 'bf16', 32, 1, 1, 0, False, 0, 'bf16', 'fork+=', 32, 64, 'conv_mfma_pw_k<2, 2>'),
    ('dgrad', (2, 64, 64, 64, 64), 'bf16', 32, 3, 2, 1, True, 0, 'bf16', 'plain', 32, 64, 'conv_mfma_gather_k<64, 0, __bf16>'),
    ('dgrad', (2, 64, 64, 64, 64), 'bf16', 64, 3, 1, 0, True, 0, 'bf16', 'plain', 64, 64, 'conv_mfma_duo_k<0, 5>'),
    ('dgrad', (2, 8, 8, 8, 1), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'plain', 8, 8, 'p1_dot_k<__bf16>'),
    ('dgrad', (2, 8, 8, 8, 512), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'plain', 8, 512, 'p1_scale_k<__bf16>'),
    ('dgrad', (2, 8, 8, 8, 512), 'bf16', 256, 3, 2, 1, True, 0, 'bf16', 'plain', 256, 512, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('dgrad', (2, 8, 8, 8, 512), 'bf16', 512, 3, 1, 0, True, 0, 'bf16', 'plain', 512, 512, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('fwd', (2, 128, 128, 128, 1), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 8, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 128, 128, 128, 1), 'bf16', 32, 3, 1, 0, True, 0, 'bf16', 'batch', True, 8, 32, 'conv_thin16_k<8, 2>'),
    ('fwd', (2, 128, 128, 128, 16), 'bf16', 1, 3, 1, 0, False, 0, 'bf16', 'instance', True, 16, 8, 'conv_thin16_k<16, 1>'),
    ('fwd', (2, 128, 128, 128, 16), 'bf16', 16, 3, 1, 0, False, 0, 'bf16', 'instance', True, 16, 16, 'conv_thin16_k<16, 1>'),
    ('fwd', (2, 128, 128, 128, 2), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'instance', True, 8, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 128, 128, 128, 2), 'bf16', 8, 3, 1, 0, False, 0, 'bf16', 'instance', True, 8, 8, 'conv_thin16_k<8, 1>'),
    ('fwd', (2, 128, 128, 128, 3), 'bf16', 16, 3, 1, 0, False, 0, 'bf16', 'instance', True, 8, 16, 'conv_thin16_k<8, 1>'),
    ('fwd', (2, 128, 128, 128, 32), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 32, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 128, 128, 128, 32), 'bf16', 1, 1, 1, 0, True, 0, 'f32', '-', True, 32, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 128, 128, 128, 32), 'bf16', 16, 1, 1, 0, False, 0, 'bf16', 'batch', True, 32, 16, 'conv_mfma_pw_k<2, 1>'),
    ('fwd', (2, 128, 128, 128, 32), 'bf16', 16, 1, 1, 0, False, 0, 'bf16', 'batch', True, 64, 16, 'conv_mfma_pw_k<2, 1>'),
    ('fwd', (2, 128, 128, 128, 32), 'bf16', 32, 3, 1, 0, True, 0, 'bf16', 'batch', True, 32, 32, 'conv_mfma_duo_k<1, 5>'),
    ('fwd', (2, 128, 128, 128, 32), 'bf16', 64, 3, 2, 0, True, 0, 'bf16', 'batch', True, 32, 64, 'conv_mfma_gather_k<64, 0, __bf16>'),
    ('fwd', (2, 128, 128, 128, 64), 'bf16', 32, 3, 1, 0, False, 0, 'bf16', 'instance', True, 64, 32, 'conv_mfma_duo_k<1, 5>'),
    ('fwd', (2, 128, 128, 128, 8), 'bf16', 1, 3, 1, 0, False, 0, 'bf16', 'instance', True, 8, 8, 'conv_thin16_k<8, 1>'),
    ('fwd', (2, 128, 128, 128, 8), 'bf16', 8, 3, 1, 0, False, 0, 'bf16', 'instance', True, 8, 8, 'conv_thin16_k<8, 1>'),
    ('fwd', (2, 16, 16, 16, 1), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 8, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 16, 16, 16, 256), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 256, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 16, 16, 16, 256), 'bf16', 128, 1, 1, 0, False, 0, 'bf16', 'batch', True, 256, 128, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('fwd', (2, 16, 16, 16, 256), 'bf16', 128, 1, 1, 0, False, 0, 'bf16', 'batch', True, 512, 128, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('fwd', (2, 16, 16, 16, 256), 'bf16', 128, 3, 2, 1, True, 0, 'bf16', 'instance', True, 256, 128, 'conv_mfma_gather_k<128, 1, __bf16>'),
    ('fwd', (2, 16, 16, 16, 256), 'bf16', 256, 3, 1, 0, True, 0, 'bf16', 'batch', True, 256, 256, 'conv_mfma_duo_k<1, 4>'),
    ('fwd', (2, 16, 16, 16, 256), 'bf16', 512, 3, 2, 0, True, 0, 'bf16', 'batch', True, 256, 512, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('fwd', (2, 16, 16, 16, 512), 'bf16', 256, 3, 1, 0, False, 0, 'bf16', 'instance', True, 512, 256, 'conv_mfma_duo_k<1, 4>'),
    ('fwd', (2, 32, 32, 32, 1), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 8, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 32, 32, 32, 128), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 128, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 32, 32, 32, 128), 'bf16', 128, 3, 1, 0, True, 0, 'bf16', 'batch', True, 128, 128, 'conv_mfma_duo_k<1, 5>'),
    ('fwd', (2, 32, 32, 32, 128), 'bf16', 256, 3, 2, 0, True, 0, 'bf16', 'batch', True, 128, 256, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('fwd', (2, 32, 32, 32, 128), 'bf16', 64, 1, 1, 0, False, 0, 'bf16', 'batch', True, 128, 64, 'conv_mfma_gather_k<64, 0, __bf16>'),
    ('fwd', (2, 32, 32, 32, 128), 'bf16', 64, 1, 1, 0, False, 0, 'bf16', 'batch', True, 256, 64, 'conv_mfma_gather_k<64, 0, __bf16>'),
    ('fwd', (2, 32, 32, 32, 128), 'bf16', 64, 3, 2, 1, True, 0, 'bf16', 'instance', True, 128, 64, 'conv_mfma_tconv_k<__bf16, 1>'),
    ('fwd', (2, 32, 32, 32, 256), 'bf16', 128, 3, 1, 0, False, 0, 'bf16', 'instance', True, 256, 128, 'conv_mfma_duo_k<1, 5>'),
    ('fwd', (2, 64, 64, 64, 1), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 8, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 64, 64, 64, 128), 'bf16', 64, 3, 1, 0, False, 0, 'bf16', 'instance', True, 128, 64, 'conv_mfma_duo_k<1, 5>'),
    ('fwd', (2, 64, 64, 64, 64), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 64, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 64, 64, 64, 64), 'bf16', 128, 3, 2, 0, True, 0, 'bf16', 'batch', True, 64, 128, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('fwd', (2, 64, 64, 64, 64), 'bf16', 32, 1, 1, 0, False, 0, 'bf16', 'batch', True, 128, 32, 'conv_mfma_pw_k<4, 1>'),
    ('fwd', (2, 64, 64, 64, 64), 'bf16', 32, 1, 1, 0, False, 0, 'bf16', 'batch', True, 64, 32, 'conv_mfma_pw_k<4, 1>'),
    ('fwd', (2, 64, 64, 64, 64), 'bf16', 32, 3, 2, 1, True, 0, 'bf16', 'instance', True, 64, 32, 'conv_mfma_tconv_k<__bf16, 1>'),
    ('fwd', (2, 64, 64, 64, 64), 'bf16', 64, 3, 1, 0, True, 0, 'bf16', 'batch', True, 64, 64, 'conv_mfma_duo_k<1, 5>'),
    ('fwd', (2, 8, 8, 8, 1), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 8, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 8, 8, 8, 512), 'bf16', 1, 1, 1, 0, False, 0, 'f32', 'batch', True, 512, 8, 'p1_dot_k<__bf16>'),
    ('fwd', (2, 8, 8, 8, 512), 'bf16', 256, 3, 2, 1, True, 0, 'bf16', 'instance', True, 512, 256, 'conv_mfma_gather_k<128, 1, __bf16>'),
    ('fwd', (2, 8, 8, 8, 512), 'bf16', 512, 3, 1, 0, True, 0, 'bf16', 'batch', True, 512, 512, 'conv_mfma_gather_k<128, 0, __bf16>'),
    ('gate', (2, 128, 128, 128, 32), 'bf16', 16, 32, 64),
    ('gate', (2, 16, 16, 16, 256), 'bf16', 128, 256, 512),
    ('gate', (2, 32, 32, 32, 128), 'bf16', 64, 128, 256),
    ('gate', (2, 64, 64, 64, 64), 'bf16', 32, 64, 128),
    ('norm', (2, 128, 128, 128, 1), 'bf16', 'batch', 'relu', True, False, True, 8, 1),
    ('norm', (2, 128, 128, 128, 1), 'bf16', 'instance', 'leaky', False, False, True, 8, 1),
    ('norm', (2, 128, 128, 128, 1), 'bf16', 'instance', 'leaky', False, False, True, 8, 8),
    ('norm', (2, 128, 128, 128, 1), 'bf16', 'instance', 'prelu_relu', False, True, True, 8, 1),
    ('norm', (2, 128, 128, 128, 16), 'bf16', 'instance', 'leaky', False, False, True, 16, 16),
    ('norm', (2, 128, 128, 128, 32), 'bf16', 'batch', 'relu', True, False, True, 32, 32),
    ('norm', (2, 128, 128, 128, 32), 'bf16', 'instance', 'prelu', False, True, True, 32, 32),
    ('norm', (2, 128, 128, 128, 32), 'bf16', 'instance', 'prelu', False, True, True, 32, 64),
    ('norm', (2, 128, 128, 128, 8), 'bf16', 'instance', 'leaky', False, False, True, 8, 8),
    ('norm', (2, 16, 16, 16, 1), 'bf16', 'batch', 'relu', True, False, True, 8, 1),
    ('norm', (2, 16, 16, 16, 256), 'bf16', 'batch', 'relu', True, False, True, 256, 256),
    ('norm', (2, 16, 16, 16, 256), 'bf16', 'instance', 'prelu', False, True, True, 256, 256),
    ('norm', (2, 16, 16, 16, 256), 'bf16', 'instance', 'prelu', False, True, True, 256, 512),
    ('norm', (2, 32, 32, 32, 1), 'bf16', 'batch', 'relu', True, False, True, 8, 1),
    ('norm', (2, 32, 32, 32, 128), 'bf16', 'batch', 'relu', True, False, True, 128, 128),
    ('norm', (2, 32, 32, 32, 128), 'bf16', 'instance', 'prelu', False, True, True, 128, 128),
    ('norm', (2, 32, 32, 32, 128), 'bf16', 'instance', 'prelu', False, True, True, 128, 256),
    ('norm', (2, 64, 64, 64, 1), 'bf16', 'batch', 'relu', True, False, True, 8, 1),
    ('norm', (2, 64, 64, 64, 64), 'bf16', 'batch', 'relu', True, False, True, 64, 64),
    ('norm', (2, 64, 64, 64, 64), 'bf16', 'instance', 'prelu', False, True, True, 64, 128),
    ('norm', (2, 64, 64, 64, 64), 'bf16', 'instance', 'prelu', False, True, True, 64, 64),
    ('norm', (2, 8, 8, 8, 1), 'bf16', 'batch', 'relu', True, False, True, 8, 1),
    ('norm', (2, 8, 8, 8, 512), 'bf16', 'batch', 'relu', True, False, True, 512, 512),
    ('wgrad', (2, 128, 128, 128, 1), 'bf16', 32, 3, 1, 0, True, 0, 1, 8, 32, 'conv_thin16_wgrad_k<8, 2>'),
    ('wgrad', (2, 128, 128, 128, 16), 'bf16', 1, 3, 1, 0, False, 0, 2, 16, 8, 'conv_thin16_wgrad_k<16, 1>'),
    ('wgrad', (2, 128, 128, 128, 16), 'bf16', 16, 3, 1, 0, False, 0, 2, 16, 16, 'conv_thin16_wgrad_k<16, 1>'),
    ('wgrad', (2, 128, 128, 128, 2), 'bf16', 1, 1, 1, 0, False, 0, 2, 8, 8, 'p1_wsum_k<__bf16>'),
    ('wgrad', (2, 128, 128, 128, 2), 'bf16', 8, 3, 1, 0, False, 0, 2, 8, 8, 'conv_thin16_wgrad_k<8, 1>'),
    ('wgrad', (2, 128, 128, 128, 3), 'bf16', 16, 3, 1, 0, False, 0, 2, 8, 16, 'conv_thin16_wgrad_k<8, 1>'),
    ('wgrad', (2, 128, 128, 128, 32), 'bf16', 1, 1, 1, 0, True, 0, 1, 32, 1, 'p1_wsum_k<__bf16>'),
    ('wgrad', (2, 128, 128, 128, 32), 'bf16', 16, 1, 1, 0, False, 0, 2, 32, 16, 'conv_mfma_wgrad2_k<1, 2, 1, 1>'),
    ('wgrad', (2, 128, 128, 128, 32), 'bf16', 16, 1, 1, 0, False, 0, 2, 64, 16, 'conv_mfma_wgrad2_k<1, 2, 1, 1>'),
    ('wgrad', (2, 128, 128, 128, 32), 'bf16', 32, 3, 1, 0, True, 0, 1, 32, 32, 'conv_mfma_wgrad2_k<1, 2, 3, 1>'),
    ('wgrad', (2, 128, 128, 128, 32), 'bf16', 64, 3, 2, 0, True, 0, 1, 32, 64, 'conv_bf16_wgrad16_k<2, 0>'),
    ('wgrad', (2, 128, 128, 128, 64), 'bf16', 32, 3, 1, 0, False, 0, 2, 64, 32, 'conv_mfma_wgrad2_k<1, 2, 3, 1>'),
    ('wgrad', (2, 128, 128, 128, 8), 'bf16', 1, 3, 1, 0, False, 0, 2, 8, 8, 'conv_thin16_wgrad_k<8, 1>'),
    ('wgrad', (2, 128, 128, 128, 8), 'bf16', 8, 3, 1, 0, False, 0, 2, 8, 8, 'conv_thin16_wgrad_k<8, 1>'),
    ('wgrad', (2, 16, 16, 16, 256), 'bf16', 128, 1, 1, 0, False, 0, 2, 256, 128, 'conv_mfma_wgrad_k<1, 2, 0, 1>'),
    ('wgrad', (2, 16, 16, 16, 256), 'bf16', 128, 1, 1, 0, False, 0, 2, 512, 128, 'conv_mfma_wgrad_k<1, 2, 0, 1>'),
    ('wgrad', (2, 16, 16, 16, 256), 'bf16', 128, 3, 2, 1, True, 0, 2, 256, 128, 'conv_mfma_wgrad_k<1, 2, 1, 1>'),
    ('wgrad', (2, 16, 16, 16, 256), 'bf16', 256, 3, 1, 0, True, 0, 1, 256, 256, 'conv_mfma_wgrad_k<2, 1, 0, 1>'),
    ('wgrad', (2, 16, 16, 16, 256), 'bf16', 512, 3, 2, 0, True, 0, 1, 256, 512, 'conv_mfma_wgrad_k<2, 1, 0, 1>'),
    ('wgrad', (2, 16, 16, 16, 512), 'bf16', 256, 3, 1, 0, False, 0, 2, 512, 256, 'conv_mfma_wgrad_k<1, 2, 0, 1>'),
    ('wgrad', (2, 32, 32, 32, 128), 'bf16', 128, 3, 1, 0, True, 0, 1, 128, 128, 'conv_mfma_wgrad2_k<1, 2, 3, 1>'),
    ('wgrad', (2, 32, 32, 32, 128), 'bf16', 256, 3, 2, 0, True, 0, 1, 128, 256, 'conv_mfma_wgrad_k<2, 1, 0, 1>'),
    ('wgrad', (2, 32, 32, 32, 128), 'bf16', 64, 1, 1, 0, False, 0, 2, 128, 64, 'conv_mfma_wgrad2_k<1, 2, 1, 1>'),
    ('wgrad', (2, 32, 32, 32, 128), 'bf16', 64, 1, 1, 0, False, 0, 2, 256, 64, 'conv_mfma_wgrad2_k<1, 2, 1, 1>'),
    ('wgrad', (2, 32, 32, 32, 128), 'bf16', 64, 3, 2, 1, True, 0, 2, 128, 64, 'conv_bf16_wgrad16_k<2, 1>'),
    ('wgrad', (2, 32, 32, 32, 256), 'bf16', 128, 3, 1, 0, False, 0, 2, 256, 128, 'conv_mfma_wgrad2_k<1, 2, 3, 1>'),
    ('wgrad', (2, 64, 64, 64, 128), 'bf16', 64, 3, 1, 0, False, 0, 2, 128, 64, 'conv_mfma_wgrad2_k<1, 2, 3, 1>'),
    ('wgrad', (2, 64, 64, 64, 64), 'bf16', 128, 3, 2, 0, True, 0, 1, 64, 128, 'conv_bf16_wgrad16_k<2, 0>'),
    ('wgrad', (2, 64, 64, 64, 64), 'bf16', 32, 1, 1, 0, False, 0, 2, 128, 32, 'conv_mfma_wgrad2_k<1, 2, 1, 1>'),
    ('wgrad', (2, 64, 64, 64, 64), 'bf16', 32, 1, 1, 0, False, 0, 2, 64, 32, 'conv_mfma_wgrad2_k<1, 2, 1, 1>'),
    ('wgrad', (2, 64, 64, 64, 64), 'bf16', 32, 3, 2, 1, True, 0, 2, 64, 32, 'conv_bf16_wgrad16_k<2, 1>'),
    ('wgrad', (2, 64, 64, 64, 64), 'bf16', 64, 3, 1, 0, True, 0, 1, 64, 64, 'conv_mfma_wgrad2_k<1, 2, 3, 1>'),
    ('wgrad', (2, 8, 8, 8, 1), 'bf16', 1, 1, 1, 0, False, 0, 2, 8, 8, 'p1_wsum_k<__bf16>'),
    ('wgrad', (2, 8, 8, 8, 512), 'bf16', 1, 1, 1, 0, False, 0, 2, 512, 8, 'p1_wsum_k<__bf16>'),
    ('wgrad', (2, 8, 8, 8, 512), 'bf16', 256, 3, 2, 1, True, 0, 2, 512, 256, 'conv_mfma_wgrad_k<1, 2, 1, 1>'),
    ('wgrad', (2, 8, 8, 8, 512), 'bf16', 512, 3, 1, 0, True, 0, 1, 512, 512, 'conv_mfma_wgrad_k<2, 1, 0, 1>'),
]

CONV_ROWS = [r for r in PRODUCTION_ROWS if r[0] in ("fwd", "dgrad", "wgrad")]
NORM_ROWS = [r for r in PRODUCTION_ROWS if r[0] == "norm"]
GATE_ROWS = [r for r in PRODUCTION_ROWS if r[0] == "gate"]
REPORT = {}            # row id -> measured (worst ratio to the per-element bound, max slab rel-L2): printed at the end


def _row_id(r):
    return "-".join(str(v).replace(" ", "") for v in r)


def test_harvest_matches_table():
    """The set of (layer shape, dispatch, kernel) calls of one eager 128^3 batch-2 bf16 step is exactly PRODUCTION_ROWS:
    a change of layers or dispatch must update the table (and with it the parity rows below)."""
    got = harvest()
    want = sorted(PRODUCTION_ROWS, key=repr)
    missing = [r for r in want if r not in got]
    extra = [r for r in got if r not in want]
    assert not missing and not extra, f"missing {missing}\nextra {extra}"


def _buf(shape, ld, dtype, fill):
    """A (B, D, H, W, C) view with voxel pitch ld >= C whose foreign lanes hold `fill`."""
    C = shape[-1]
    b = torch.full(tuple(shape[:-1]) + (max(ld, C),), fill, dtype=dtype, device="cuda")
    return b[..., :C]


def _rand(shape, ld, gen, scale=1.0, dtype=torch.bfloat16):
    v = _buf(shape, ld, dtype, 3.0e4)        # (finite garbage in the foreign lanes: a kernel that reads them is far off)
    v.copy_(torch.randn(tuple(shape), generator=gen, device="cuda") * scale)
    return v


def _prep(cin, cout, k, tr, ps, wdt_f, wdt_d, gen):
    """Per-sample (E = 8 experts mixed by a routing in (0, 1), what the CondConv layers run) or shared weights, scaled so
    the outputs are O(1); -> (wk_f, wk_d) from ops.PrepWeights."""
    ops, _ = _ops()
    wshape = (cin, cout, k, k, k) if tr else (cout, cin, k, k, k)
    sc = 1.0 / (E * cin * k ** 3) ** 0.5 * 2.0
    dt = {"bf16": torch.bfloat16, "f32": torch.float32, None: None}
    if ps:
        master = torch.randn((E, *wshape), generator=gen, device="cuda") * sc
        r = torch.rand((BATCH, E), generator=gen, device="cuda")
        return ops.PrepWeights.apply(master, r, tr, dt[wdt_f], dt[wdt_d])
    master = torch.randn(wshape, generator=gen, device="cuda") * sc * E ** 0.5
    return ops.PrepWeights.apply(master, None, tr, dt[wdt_f], dt[wdt_d])


def _free():
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("row", CONV_ROWS, ids=_row_id)
def test_conv_row_matches_fp64(row):
    ops, L = _ops()
    what, xs, dt, cout, k, s, form, ps = row[:8]
    algo = row[8]
    B, cin = xs[0], xs[4]
    tr = form == 1
    og = R.out_grid(xs[1:4], k, s, tr)
    ys = (B, *og, cout)
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(row).encode()))
    stats = {}
    try:
        with torch.no_grad():
            if what == "fwd":
                wdt, norm, has_bias, xld, yld, kern = row[9:]
                x = _rand(xs, xld, gen)
                wk_f, _ = _prep(cin, cout, k, tr, ps, wdt, None, gen)
                bias = torch.randn(((B, cout) if ps else (cout,)), generator=gen, device="cuda") * 0.5 if has_bias else None
                ybuf = _buf(ys, yld, torch.bfloat16, -7.0)
                mode = {"batch": L.NORM_BATCH, "instance": L.NORM_INSTANCE, "-": None}[norm]
                y, sums = ops._conv_fwd(x, wk_f, bias, k, s, form, ps, algo, ops.Out(ybuf), mode)
                tag = L.lib.coma_last_kernel().decode()
                assert tag == kern, tag
                if yld > cout:
                    assert bool((ybuf.as_strided((B, *og, yld - cout), ybuf.stride(), ybuf.storage_offset() + cout) == -7.0).all()), \
                        "foreign lanes of the output written"
                ref, A = R.conv_fwd(x.double(), wk_f.double(), None if bias is None else bias.double(), k, s, tr)
                stats["ratio"] = R.check_elementwise(y, ref, R.elem_bound(ref, A, k ** 3 * cin + 1), "y")
                stats["slab"] = R.slab_rel_l2(y, ref, 2)
                assert stats["slab"] < SLAB_TOL, stats
                if mode is not None:        # fused statistics: must describe the STORED output
                    G = B if mode == L.NORM_INSTANCE else 1
                    n = og[0] * og[1] * og[2] * (1 if G == B else B)
                    mean, rstd = ops.stats_from_sums(sums, G, cout, n, 1e-5)
                    yf = y.double()
                    red = (1, 2, 3) if G == B else (0, 1, 2, 3)
                    m_ref = yf.mean(red).reshape(mean.shape)
                    v_ref = yf.var(red, unbiased=False).reshape(mean.shape)
                    assert float((mean.double() - m_ref).abs().max()) < 1e-5 * (1.0 + float(m_ref.abs().max()))
                    assert float(((rstd.double() - (v_ref + 1e-5).rsqrt()).abs() / (v_ref + 1e-5).rsqrt()).max()) < 1e-5
            elif what == "dgrad":
                wdt, tgt, dyld, xld, kern = row[9:]
                dy = _rand(ys, dyld, gen)
                _, wk_d = _prep(cin, cout, k, tr, ps, wdt, wdt, gen)
                x = _buf(xs, xld, torch.bfloat16, 0.0)
                fork, base = None, None
                if tgt == "fork+=":
                    fork = ops.GradFork()
                    base = ops._new(xs, torch.bfloat16, x.device)
                    base.copy_(torch.randn(xs, generator=gen, device="cuda"))
                    fork.buf = base
                    base = base.double()
                wsh = (B if ps else 1, k ** 3, cout, cin)
                dx, _, _ = ops._conv_bwd(x, wk_d, dy, k, s, form, ps, algo, wsh, True, False, 0, None, fork)
                tag = L.lib.coma_last_kernel().decode()
                assert tag == kern, tag
                if fork is not None:
                    assert dx is None, "expected the data gradient accumulated in the kernel's epilogue"
                    dx = fork.buf
                ref, A = R.conv_dgrad(dy.double(), wk_d.double().transpose(2, 3), xs[1:4], k, s, tr)
                if base is not None:
                    ref = ref + base
                stats["ratio"] = R.check_elementwise(dx, ref, R.elem_bound(ref, A, k ** 3 * cout, base=base), "dx")
                stats["slab"] = R.slab_rel_l2(dx, ref, 2)
                assert stats["slab"] < SLAB_TOL, stats
            else:
                bias_mode, xld, dyld, kern = row[9:]
                x = _rand(xs, xld, gen)
                dy = _rand(ys, dyld, gen)
                wsh = (B if ps else 1, k ** 3, cout, cin)
                _, dwk, dbias = ops._conv_bwd(x, None, dy, k, s, form, ps, algo, wsh, False, True, bias_mode, None)
                tag = L.lib.coma_last_kernel().decode()
                assert tag == kern, tag
                ref, A = R.conv_wgrad(x.double(), dy.double(), k, s, tr, ps)
                nvox = (xs[1] * xs[2] * xs[3]) if tr else (og[0] * og[1] * og[2])
                K = nvox * (1 if ps else B)
                stats["ratio"] = R.check_elementwise(dwk, ref, R.elem_bound(ref, A, K, u_out=R.U_F32), "dw")
                stats["slab"] = R.slab_rel_l2(dwk, ref, 2)
                assert stats["slab"] < WGRAD_SLAB_TOL, stats
                if bias_mode == 1:
                    bref = dy.double().sum((1, 2, 3))
                    bref = bref if ps else bref.sum(0)
                    babs = dy.double().abs().sum((1, 2, 3))
                    babs = babs if ps else babs.sum(0)
                    R.check_elementwise(dbias, bref, R.elem_bound(bref, babs, K, u_out=R.U_F32), "dbias")
                elif bias_mode == 2:
                    assert dbias is None or float(dbias.abs().max()) == 0.0
        torch.cuda.synchronize()
        REPORT[_row_id(row)] = stats
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# normalisation + activation
# ---------------------------------------------------------------------------------------------------------------------
def _rows_plan(R_, C, G, vec):
    """(nchunks, rows per chunk) of make_rows (csrc/norm_common.h) for R_ rows of a group."""
    cv = C // vec
    cvp = 1
    while cvp < cv:
        cvp <<= 1
    cvp = min(cvp, 256)
    ry = 256 // cvp
    nch = max(1, min(-(-R_ // (ry * 16)), max(1, 1024 // G)))
    return nch, -(-R_ // nch), ry


def _synthetic_norm_rows():
    """Row counts that force the ragged paths of the row walk: R = nchunks * ch - j below the chunk cap, and over the
    1024 / G cap with a ragged last chunk."""
    out = []
    acts = ["prelu", "relu", "leaky", "sigmoid", "prelu_relu", "none", "prelu"]
    for i, C in enumerate((1, 3, 8, 16, 32, 64, 96)):
        vec = 8 if C % 8 == 0 else (4 if C % 4 == 0 else 1)
        for mode, G in (("batch", 1), ("instance", BATCH)):
            _, _, ry = _rows_plan(1, C, G, vec)
            per = ry * 16
            cap = max(1, 1024 // G)
            below = 5 * per - 3                            # 5 chunks, the last one 3 rows short
            over = cap * (per + 4) - 3                     # past the cap: longer chunks, the last one 3 rows short
            for Rg in (below, over):
                V = Rg if G == BATCH else -(-Rg // BATCH)
                out.append(("norm", (BATCH, 1, 1, V, C), "bf16", mode, acts[(i + len(out)) % len(acts)], mode == "batch",
                            "prelu" in acts[(i + len(out)) % len(acts)], False, (C + 7) // 8 * 8 if C % 8 else C, C))
    return out


@pytest.mark.parametrize("row", NORM_ROWS + _synthetic_norm_rows(), ids=_row_id)
def test_norm_act_row_matches_fp64(row):
    """NormAct forward + backward (statistics pass, apply, partial sums over the row chunks, apply backward) at every
    (C, grid, mode, act) of the step and at synthetic ragged row counts: y and dx per element against the fp64
    reference, dgamma / dbeta / dslope per channel, the running statistics."""
    ops, L = _ops()
    _, xs, dt, mode, act, affine, has_slope, _pre, xld, yld = row
    C = xs[4]
    if has_slope and act not in ("prelu", "prelu_relu"):
        has_slope = False
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(row).encode()))
    try:
        x = _rand(xs, xld, gen, 1.5)
        x.add_(0.7)
        dy = _rand(xs, C, gen)
        gamma = (torch.rand(C, generator=gen, device="cuda") + 0.5) if affine else None
        beta = (torch.randn(C, generator=gen, device="cuda") * 0.3) if affine else None
        slope = torch.tensor([-0.3 if act == "prelu_relu" else 0.2], device="cuda") if has_slope else None
        ref = R.norm_act_ref(x.double(), dy.double(), mode, act, gamma, beta, slope)
        xg = x.requires_grad_(True)
        gg, bg, sg = (None if t is None else t.clone().requires_grad_(True) for t in (gamma, beta, slope))
        rm = torch.zeros(C, device="cuda") if affine else None
        rv = torch.ones(C, device="cuda") if affine else None
        ybuf = _buf(xs, yld, torch.bfloat16, -7.0)
        code = {"batch": L.NORM_BATCH, "instance": L.NORM_INSTANCE}[mode]
        y = ops.NormAct.apply(xg, gg, bg, sg, rm, rv, code, _ACTS.index(act), 0.1, 1e-5, True, ops.Out(ybuf))
        y.backward(dy)
        torch.cuda.synchronize()
        K = 16                              # (fp32 terms behind one element of the elementwise stages)
        st = {"ratio_y": R.check_elementwise(y, ref["y"], R.elem_bound(ref["y"], ref["mag_y"], K), "y"),
              "ratio_dx": R.check_elementwise(xg.grad, ref["dx"], R.elem_bound(ref["dx"], ref["mag_dx"], K), "dx"),
              "slab_y": R.slab_rel_l2(y, ref["y"], 1), "slab_dx": R.slab_rel_l2(xg.grad, ref["dx"], 1)}
        assert st["slab_y"] < SLAB_TOL and st["slab_dx"] < SLAB_TOL, st
        nrow = x.numel() // C
        for name, got, mag in (("dgamma", gg, None), ("dbeta", bg, None), ("dslope", sg, None)):
            if got is None:
                continue
            want = ref[name]
            # a sum over all rows: fp64 partial records, rounded to fp32 -- bound it by the L1 mass of its terms
            dz = ref["dz_mass"][name]
            st[name] = R.check_elementwise(got.grad, want, R.elem_bound(want, dz, 64, u_out=R.U_F32), name)
        if affine:
            assert float((rm.double() - ref["running_mean"]).abs().max()) < 1e-5 * (1 + float(ref["running_mean"].abs().max()))
            assert float((rv.double() - ref["running_var"]).abs().max()) < 1e-5 * (1 + float(ref["running_var"].abs().max()))
        REPORT[_row_id(row)] = st
        del nrow
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# attention gate, expert mix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", GATE_ROWS, ids=_row_id)
def test_gate_block_row_matches_fp64(row):
    """ObservableAttentionBlock (W_g / W_x pointwise convolutions + GateFused) at each production level against the
    shared fp64 gate reference (oracle.fp64_ref.gate_ref) on the GPU; the gate output is written into the concat slice
    of the step's pitch.  The intermediate g1 / x1 are stored in bf16 by the kernels and not by the reference, so the
    bound is the bf16 one of test_fused_gate_block_matches_torch, taken per (sample, z-plane) slab."""
    ops, L = _ops()
    from coma_unet_amd.attn_unet_data_parallel import ObservableAttentionBlock
    from coma_unet_amd.layers import Config
    _, xs, dt, Fi, xld, yld = row
    C = xs[4]
    torch.manual_seed(C)
    try:
        blk = ObservableAttentionBlock(Config(compute_dtype=torch.bfloat16), f_int=Fi, f_g=C, f_l=C).cuda()
        blk.train()
        with torch.no_grad():
            for bn in (blk.W_g[1], blk.W_x[1], blk.psi[1]):
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.uniform_(-0.3, 0.3)
        gen = torch.Generator(device="cuda").manual_seed(C + 1)
        gi = _rand(xs, C, gen).requires_grad_(True)
        xi = _rand(xs, xld, gen).requires_grad_(True)
        gy = _rand(xs, C, gen)
        P = {k: v.detach().double().clone().requires_grad_(True) for k, v in blk.named_parameters()}
        rm = {n: [torch.zeros(c, dtype=torch.float64, device="cuda"), torch.ones(c, dtype=torch.float64, device="cuda")]
              for n, c in (("W_g", Fi), ("W_x", Fi), ("psi", 1))}
        cf = lambda t: t.detach().double().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        gr, xr = cf(gi), cf(xi)
        att_r, psi_r = R.gate_ref(P, gr, xr, rm)
        (att_r * gy.double().permute(0, 4, 1, 2, 3)).sum().backward()
        cl = lambda t: t.detach().permute(0, 2, 3, 4, 1)
        ybuf = _buf(xs, yld, torch.bfloat16, -7.0)
        blk.save_attn = True
        att, psi = blk(gi, xi, out=ybuf)
        att.backward(gy)
        torch.cuda.synchronize()
        tol = 2e-2
        st = {"slab_att": R.slab_rel_l2(att, cl(att_r), 2), "slab_psi": R.slab_rel_l2(psi, cl(psi_r), 2),
              "slab_dg": R.slab_rel_l2(gi.grad, cl(gr.grad), 2), "slab_dx": R.slab_rel_l2(xi.grad, cl(xr.grad), 2)}
        assert st["slab_att"] < tol and st["slab_psi"] < tol, st
        assert st["slab_dg"] < 4 * tol and st["slab_dx"] < 4 * tol, st
        if yld > C:
            assert bool((ybuf.as_strided((*xs[:4], yld - C), ybuf.stride(), ybuf.storage_offset() + C) == -7.0).all())
        for k, v in blk.named_parameters():
            if k.endswith("0.conv.bias"):
                assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
                continue
            e = float((v.grad.double() - P[k].grad).norm() / P[k].grad.norm())
            st[k] = e
            assert e < 4 * tol, (k, e)
        for name in ("W_g", "W_x", "psi"):
            bn = getattr(blk, name)[1]
            assert float((bn.running_mean.double() - rm[name][0]).norm() / rm[name][0].norm().clamp_min(1e-30)) < 10 * tol
            assert float((bn.running_var.double() - rm[name][1]).norm() / rm[name][1].norm()) < 10 * tol
        REPORT[_row_id(row)] = st
    finally:
        _free()


def test_prep_weights_e8_largest_layer_matches_fp64():
    """PrepWeights forward (expert mix + both kernel layouts, bf16) and backward (dmaster, droute) at E = 8 for the
    largest per-sample layer of the step, against fp64 einsum."""
    ops, L = _ops()
    conv = [r for r in CONV_ROWS if r[0] == "fwd" and r[7]]
    _, xs, _, cout, k, s, form, _ps = max(conv, key=lambda r: r[1][4] * r[3] * r[4] ** 3)[:8]
    cin, tr = xs[4], form == 1
    gen = torch.Generator(device="cuda").manual_seed(8)
    wshape = (cin, cout, k, k, k) if tr else (cout, cin, k, k, k)
    try:
        master = (torch.randn((E, *wshape), generator=gen, device="cuda") * 0.05).requires_grad_(True)
        r = torch.rand((BATCH, E), generator=gen, device="cuda").requires_grad_(True)
        wk_f, wk_d = ops.PrepWeights.apply(master, r, tr, torch.bfloat16, torch.bfloat16)
        m = master.detach().double()
        mix = torch.einsum("be,e...->b...", r.detach().double(), m)
        amix = torch.einsum("be,e...->b...", r.detach().double().abs(), m.abs())
        lay = lambda t: (t.transpose(1, 2) if tr else t).reshape(BATCH, cout, cin, k ** 3).permute(0, 3, 1, 2)
        ref, A = lay(mix), lay(amix)
        st = {"ratio_wk_f": R.check_elementwise(wk_f, ref, R.elem_bound(ref, A, E), "wk_f"),
              "ratio_wk_d": R.check_elementwise(wk_d, ref.transpose(2, 3), R.elem_bound(ref, A, E).transpose(2, 3), "wk_d")}
        dwk = torch.randn(wk_f.shape, generator=gen, device="cuda")
        wk_f.backward(dwk)
        torch.cuda.synchronize()
        d = dwk.bfloat16().double()          # (autograd hands the node the gradient in wk_f's dtype)
        unlay = lambda t: t.permute(0, 2, 3, 1).reshape(BATCH, cout, cin, k, k, k)
        dmix = unlay(d)
        if tr:
            dmix = dmix.transpose(1, 2)
        dm_ref = torch.einsum("be,b...->e...", r.detach().double(), dmix)
        dm_abs = torch.einsum("be,b...->e...", r.detach().double().abs(), dmix.abs())
        st["ratio_dmaster"] = R.check_elementwise(master.grad, dm_ref, R.elem_bound(dm_ref, dm_abs, BATCH, u_out=R.U_F32), "dmaster")
        dr_ref = torch.einsum("b...,e...->be", dmix, m)
        dr_abs = torch.einsum("b...,e...->be", dmix.abs(), m.abs())
        st["ratio_dr"] = R.check_elementwise(r.grad, dr_ref, R.elem_bound(dr_ref, dr_abs, m[0].numel(), u_out=R.U_F32), "dr")
        REPORT["prep_weights_e8"] = st
    finally:
        _free()


def test_zz_report():
    """Prints the measured error of every row that ran (worst ratio to the per-element bound, max slab rel-L2)."""
    for k, v in REPORT.items():
        print("ROW", k, {a: (round(b, 6) if isinstance(b, float) else b) for a, b in v.items()})
    out = os.environ.get("PRODUCTION_ROWS_REPORT")
    if out:
        import json
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1)
