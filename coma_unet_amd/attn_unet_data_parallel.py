"""MI355X drop-in for the reference module ``attn_unet_data_parallel`` (model part).

Same class names, constructor signature, ``forward(x, covariate, roi_pred_dicts,
sample_roi_mask)`` contract, attribute surface (``set_save_attn``, ``set_training``,
``get_depth``, ``decoder_ds``, ``embeddings_out``, ``roi_indices``, ``roi_ind_names_dict``)
and state_dict keys as /root/reference/attn_unet_data_parallel.py:120-693, with every
tensor op executed by libcoma_unet.so (hand-written HIP for gfx950).

Stated deviations from the reference text:
 * ``volume_shape`` kwarg -- the reference hard-codes 128^3 prompts (:544-555,610);
 * the duplicated U-Net pass of :664/:666 is executed once; its only observable effect
   (two BatchNorm running-stat updates per step) is reproduced by folding both updates
   into one (``bn_updates_per_forward=2``);
 * ``compute_dtype`` kwarg (torch.float32 | torch.bfloat16): storage type of activations;
   accumulation, statistics and parameters stay fp32;
 * ROI priors may also be passed as a (B, 36, 2) tensor instead of a list of dicts.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import ops
from ._lib import lib, ct, check
from .layers import (Config, Convolution, MonaiConvBlock, CondConvolution, CondConvBlock, norm_act, conv_plain,
                     conv_then_bn, reset_cov_cache, cov_rows, _norm_params, bn_frozen, frozen_stats)
from .ops import Out
from .roi_tables import ROI_INDICES, ROI_NAMES, ROI_INDEX_TO_NAME
from .metrics import RoiCorrMetric, calc_roi_metrics          # noqa: F401  (:36-96, :1361-1397 of the reference module)


def to_internal(x: torch.Tensor) -> torch.Tensor:
    """(B, C, D, H, W) -> channels-last (B, D, H, W, C) view/copy."""
    return x.permute(0, 2, 3, 4, 1)


def to_external(x: torch.Tensor) -> torch.Tensor:
    """channels-last (B, D, H, W, C) -> logical (B, C, D, H, W) (zero-copy view)."""
    return x.permute(0, 4, 1, 2, 3)


def _padded_input(x, dtype):
    """(B, C, D, H, W) external volume -> internal (B, D, H, W, C) in the compute dtype, pitch-padded (ops._new)."""
    v = to_internal(x)
    xi = ops._new(tuple(v.shape), dtype, x.device)
    if v.dtype in (torch.float32, torch.bfloat16) and (v.shape[4] == 1 or v.stride(4) == 1) and not v.requires_grad:
        try:
            cv = ct(v)                 # (B, 1, D, H, W) contiguous IS channels-last with one channel
        except AssertionError:
            cv = None
        if cv is not None:
            check(lib.coma_cast_copy(cv, ct(xi), L.stream()), "coma_cast_copy")
            return xi
    xi.copy_(v)
    return xi


def _refresh_after_load(module, _incompatible_keys):
    module.refresh_frozen_batchnorm()


class UpBlock(nn.Module):
    """attn_unet_data_parallel.py:120-131 (conditional branch)."""

    def __init__(self, cfg, in_channels, out_channels, strides=2, kernel_size=3, num_covars=6):
        super().__init__()
        self.up = CondConvolution(cfg, in_channels, out_channels, strides=strides, kernel_size=kernel_size,
                                  is_transposed=True, num_covars=num_covars)

    def forward(self, x, covariate=None, out=None):
        return self.up(x, covariate, out)


class ObservableAttentionBlock(nn.Module):
    """MONAI AttentionBlock + attn_unet_data_parallel.py:134-150: the attention gate
    psi = sigmoid(BN(W_psi relu(BN(W_g g) + BN(W_x x)))),  out = x * psi."""

    def __init__(self, cfg, f_int, f_g, f_l):
        super().__init__()
        self.cfg = cfg
        self.W_g = nn.Sequential(Convolution(cfg, f_g, f_int, kernel_size=1, conv_only=True), nn.BatchNorm3d(f_int))
        self.W_x = nn.Sequential(Convolution(cfg, f_l, f_int, kernel_size=1, conv_only=True), nn.BatchNorm3d(f_int))
        self.psi = nn.Sequential(Convolution(cfg, f_int, 1, kernel_size=1, conv_only=True), nn.BatchNorm3d(1), nn.Sigmoid())
        self.relu = nn.ReLU()
        self.save_attn = None

    def forward(self, g, x, out=None):
        cfg = self.cfg
        # a gate with a frozen BatchNorm (layers.bn_frozen) takes the piecewise path below, which decides per BatchNorm
        frozen = self.training and any(bn_frozen(cfg, m) for m in (self.W_g[1], self.W_x[1], self.psi[1]))
        if self.training and cfg.fused_gate and not frozen:
            # W_g / W_x: MFMA 1x1x1 convolutions with their BatchNorm statistics out of the epilogue; everything behind them
            # (two BatchNorm applies, add, ReLU, psi dot product, its BatchNorm statistics, sigmoid, multiply) is two launches
            # forward and three backward (ops.GateFused, csrc/gate.hip)
            g1raw, sums_g = conv_plain(cfg, g, self.W_g[0].conv, 1, 1, False, None, L.NORM_BATCH)
            x1raw, sums_x = conv_plain(cfg, x, self.W_x[0].conv, 1, 1, False, None, L.NORM_BATCH)
            gg, bg, rmg, rvg, mom, eg = _norm_params(cfg, self.W_g[1], True)
            gx, bx, rmx, rvx, _m, ex = _norm_params(cfg, self.W_x[1], True)
            gp, bp, rmp, rvp, _m, ep = _norm_params(cfg, self.psi[1], True)
            pc = self.psi[0].conv
            att, psi = ops.GateFused.apply(x, g1raw, x1raw, sums_g, sums_x, gg, bg, gx, bx, pc.weight, pc.bias, gp, bp,
                                           (rmg, rvg, rmx, rvx, rmp, rvp), mom, (eg, ex, ep), Out(out) if out is not None else None)
            if self.save_attn:
                return att, psi
            return att
        if not self.training and cfg.eval_fused and getattr(self, "_eval_fold", None) is not None:
            # inference: every BatchNorm is a known affine map, folded once (inference.fold_gate) -- the whole gate is one
            # launch (bf16, C <= 64: W_g / W_x included), or one launch behind the two convolutions
            from .inference import gate_eval
            att, psi = gate_eval(self, g, x, out=out, want_psi=bool(self.save_attn))
            if self.save_attn:
                return att, psi
            return att
        g1 = x1 = None
        if frozen and cfg.fused_gate and all(bn_frozen(cfg, m) for m in (self.W_g[1], self.W_x[1], self.psi[1])):
            # all three BatchNorms frozen: plain W_g / W_x convolutions (biases, no statistics epilogue), then one launch
            # forward and one pass + finalise backward (ops.GateFrozen); outside the kernels' envelope the pieces below
            # take the two raw products
            g1raw = conv_plain(cfg, g, self.W_g[0].conv, 1, 1, False)
            x1raw = conv_plain(cfg, x, self.W_x[0].conv, 1, 1, False)
            if ops.gate_frozen_ok(x, g1raw, x1raw, out if out is not None else x):
                gg, bg = self.W_g[1].weight, self.W_g[1].bias
                gx, bx = self.W_x[1].weight, self.W_x[1].bias
                gp, bp = self.psi[1].weight, self.psi[1].bias
                pc = self.psi[0].conv
                stats = (frozen_stats(self.W_g[1]), frozen_stats(self.W_x[1]), frozen_stats(self.psi[1]))
                att, psi = ops.GateFrozen.apply(x, g1raw, x1raw, gg, bg, gx, bx, pc.weight, pc.bias, gp, bp, stats,
                                                Out(out) if out is not None else None)
                if self.save_attn:
                    return att, psi
                return att
            g1 = norm_act(cfg, g1raw, self.W_g[1], L.NORM_BATCH, L.ACT_NONE, None, True)
            x1 = norm_act(cfg, x1raw, self.W_x[1], L.NORM_BATCH, L.ACT_NONE, None, True)
        if g1 is None:
            g1 = conv_then_bn(cfg, g, self.W_g[0], self.W_g[1], L.ACT_NONE, self.training)
            x1 = conv_then_bn(cfg, x, self.W_x[0], self.W_x[1], L.ACT_NONE, self.training)
        s = ops.AddRelu.apply(g1, x1)
        psi = conv_then_bn(cfg, s, self.psi[0], self.psi[1], L.ACT_SIGMOID, self.training)
        att = ops.GateMul.apply(x, psi, Out(out) if out is not None else None)
        if self.save_attn:
            return att, psi
        return att


class AttentionLayer(nn.Module):
    """attn_unet_data_parallel.py:152-241."""

    def __init__(self, cfg, in_channels, out_channels, submodule, up_kernel_size=3, strides=2, num_covars=6):
        super().__init__()
        self.cfg = cfg
        self.attention = ObservableAttentionBlock(cfg, f_g=in_channels, f_l=in_channels, f_int=in_channels // 2)
        self.upconv = UpBlock(cfg, out_channels, in_channels, strides=strides, kernel_size=up_kernel_size,
                              num_covars=num_covars)
        self.merge = Convolution(cfg, 2 * in_channels, in_channels)
        self.submodule = submodule
        self.save_attn = None

    def set_save_attn(self, status):
        self.save_attn = status
        self.attention.save_attn = status

    def forward(self, x, covariate=None):
        # x feeds the next encoder block, the gate's W_x convolution and its final multiply; the up-convolution's output
        # feeds W_g and the merge convolution: their data gradients meet in ONE buffer each (ops.GradFork) instead of being
        # added pairwise by autograd
        if self.cfg.grad_forks:
            x = ops.fork(x)
        if isinstance(self.submodule, nn.Sequential):
            x_sub = x
            for sub in self.submodule:
                if isinstance(sub, AttentionLayer):
                    x_sub = sub(x_sub, covariate=covariate)
                else:
                    x_sub = sub(x_sub, covariate=covariate[:, :, :5])
        else:
            x_sub = self.submodule(x, covariate=covariate[:, :, :5])
        if isinstance(x_sub, tuple):
            x_sub, rest = x_sub
        else:
            rest = x_sub
        B, D, H, W, C = x.shape
        # torch.cat((att, fromlower), dim=1) of :229 -- both producers write their channel slice directly
        cat = torch.empty((B, D, H, W, 2 * C), dtype=x.dtype, device=x.device)
        fromlower = self.upconv(x_sub, covariate, out=cat[..., C:])
        if self.cfg.grad_forks:
            fromlower = ops.fork(fromlower)
        att = self.attention(g=fromlower, x=x, out=cat[..., :C])
        if self.save_attn is not None:
            att, _coeff = att   # the reference dumps coeff to disk here (data_util.save_attention_coeffs)
        att_m = self.merge(ops.JoinSlices.apply(Out(cat), att, fromlower))
        return att_m, (x, (x_sub, rest))


class ObservableAttentionUnet(nn.Module):
    """attn_unet_data_parallel.py:243-434 (conditional=True, the only constructible form)."""

    def __init__(self, spatial_dims, in_channels, out_channels, channels: Sequence[int], strides: Sequence[int],
                 kernel_size=3, up_kernel_size=3, dropout=0.0, conditional=False, cfg: Config = None):
        super().__init__()
        if not conditional:
            raise ValueError("conditional=False is not constructible in the reference either: covariate kwargs are "
                             "passed unconditionally into blocks that reject them (attn_unet_data_parallel.py:209-223)")
        assert spatial_dims == 3 and kernel_size == 3 and up_kernel_size == 3
        assert not dropout, "dropout>0 is never used by the reference drivers"
        self.cfg = cfg or Config()
        cfg = self.cfg
        self.dimensions, self.in_channels, self.out_channels = spatial_dims, in_channels, out_channels
        self.channels, self.strides = list(channels), list(strides)
        self.kernel_size, self.dropout, self.conditional = kernel_size, dropout, conditional
        self.with_regression = True
        self.up_kernel_size = up_kernel_size
        self.save_attn = None
        head = CondConvBlock(cfg, in_channels, channels[0], num_covars=5)
        reduce_channels = CondConvolution(cfg, channels[0], out_channels, kernel_size=1, strides=1, conv_only=True,
                                          num_experts=8, num_covars=5 + int(self.with_regression))

        def _create_block(ch, st):
            if len(ch) > 2:
                sub = _create_block(ch[1:], st[1:])
                return AttentionLayer(cfg, ch[0], ch[1],
                                      submodule=nn.Sequential(CondConvBlock(cfg, ch[0], ch[1], strides=st[0], num_covars=5), sub),
                                      up_kernel_size=up_kernel_size, strides=st[0], num_covars=6)
            return AttentionLayer(cfg, ch[0], ch[1],
                                  submodule=CondConvBlock(cfg, ch[0], ch[1], strides=st[0], num_covars=5),
                                  up_kernel_size=up_kernel_size, strides=st[0], num_covars=6)

        self.model = nn.ModuleList([head, _create_block(self.channels, self.strides), reduce_channels])

    def batchnorms(self):
        """Every nn.BatchNorm3d holder of the model (cached: the module tree is fixed after construction)."""
        bns = self.__dict__.get("_bn_list")
        if bns is None:
            bns = self.__dict__["_bn_list"] = [m for m in self.modules() if isinstance(m, nn.BatchNorm3d)]
        return bns

    def freeze_batchnorm(self, on=True):
        """Frozen-BatchNorm training: while the model is in train mode every BatchNorm3d normalises with its running
        statistics and writes neither them nor its step counter (fine-tuning a resumed checkpoint at a batch size whose
        own statistics are noise).  Sticky: survives ``train()`` / ``eval()``; the per-module torch idiom (BatchNorm3d
        holders in eval mode inside a train-mode model) is honoured as well.  Calling it again re-reads the running
        statistics into the per-BatchNorm (mean, rstd) tables in place.  InstanceNorm layers are untouched."""
        for c in (self.cfg, getattr(self, "cfg_heads", None)):
            if c is not None:
                c.frozen_bn = bool(on)
        if on:
            self.refresh_frozen_batchnorm(every=True)
        return self

    def refresh_frozen_batchnorm(self, every=False):
        """Re-derive the (mean, rstd) tables of the frozen BatchNorms from the running buffers, in place (a captured step
        keeps reading the same addresses).  every=False: only the tables that exist."""
        for m in self.batchnorms():
            if (every or "_coma_frozen" in m.__dict__) and m.running_mean is not None and m.running_mean.is_cuda:
                frozen_stats(m, refresh=True)

    def set_save_attn(self, v):
        self.save_attn = v
        encdec = self.model[1]
        while isinstance(encdec, AttentionLayer):
            encdec.set_save_attn(v)
            seq = encdec.submodule
            if isinstance(seq, nn.Sequential):
                encdec = seq[-1]
            else:
                break

    def _unet(self, xi, covariate, out=None):
        """xi: internal (B, D, H, W, Cin).  Returns internal tensors."""
        enc, dec = [], []
        h = self.model[0](xi, covariate=covariate[:, :, :5])
        h, x_submod = self.model[1](h, covariate)
        dec.append(h)
        while isinstance(x_submod, tuple):
            e_i, d_next_rest = x_submod
            enc.append(e_i)
            d_next, rest = d_next_rest
            (dec if isinstance(rest, tuple) else enc).append(d_next)
            x_submod = rest
        y = self.model[2](h, covariate=covariate, out=out)
        return y, enc, dec

    def forward(self, x, covariate=None):
        xi = _padded_input(x, self.cfg.compute_dtype)
        reset_cov_cache()
        y, enc, dec = self._unet(xi, covariate)
        return to_external(y), [to_external(e) for e in enc], [to_external(d) for d in dec]


class ProjectionHead(nn.Module):
    """attn_unet_data_parallel.py:436-454."""

    def __init__(self, cfg, in_channels, out_channels=None, latent_space_dim=None, kernel_size=3):
        super().__init__()
        self.conv = MonaiConvBlock(cfg, in_channels, 1, kernel_size=1)
        self.act_fn = nn.ReLU()

    def forward(self, xi):
        # ConvBlock ends in ReLU, so the trailing act_fn (:452) is the identity on its output
        return self.conv(xi).flatten(1)


class StackedFusionConvLayers(nn.Module):
    """attn_unet_data_parallel.py:480-501."""

    def __init__(self, cfg, cin, cmid, cout, num_convs):
        super().__init__()
        self.blocks = nn.Sequential(
            *([Convolution(cfg, cin, cmid, act="leakyrelu")] +
              [Convolution(cfg, cmid, cmid, act="leakyrelu") for _ in range(num_convs - 2)] +
              [Convolution(cfg, cmid, cout, act="leakyrelu")]))

    def forward(self, x, out=None):
        n = len(self.blocks)
        for i, blk in enumerate(self.blocks):
            x = blk(x, out if i == n - 1 else None)
        return x


class ContrastiveAttentionUNET_DP(ObservableAttentionUnet):
    """attn_unet_data_parallel.py:503-693."""

    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, channels: Sequence[int],
                 strides: Sequence[int], latent_spaces: Sequence[int], kernel_size=3, up_kernel_size=3,
                 dropout: float = 0, training: bool = True, embeddings_out: bool = False, conditional: bool = False,
                 decoder_ds: bool = False, **kwargs):
        cfg = Config(compute_dtype=kwargs.get("compute_dtype", torch.float32),
                     conv_algo=kwargs.get("conv_algo", 0),
                     bn_updates_per_forward=kwargs.get("bn_updates_per_forward", 2))
        super().__init__(spatial_dims, in_channels, out_channels, channels, strides, kernel_size, up_kernel_size,
                         dropout, conditional, cfg=cfg)
        self.training = training
        self.embeddings_out, self.decoder_ds = embeddings_out, decoder_ds
        self.depth = len(channels)
        vs = tuple(kwargs.get("volume_shape", (128, 128, 128)))
        self.volume_shape = vs
        # the duplicated pass of :664/:666 covers the U-Net only; the heads run once per forward
        cfg1 = Config(cfg.compute_dtype, cfg.conv_algo, 1)
        self.cfg_heads = cfg1
        self.projection_heads = nn.ModuleList(
            [ProjectionHead(cfg1, channels[i], int((128 / (2 ** i)) ** 3), latent_spaces[i]) for i in range(len(channels))])
        self.final_projection_head = nn.Sequential(nn.AdaptiveAvgPool3d(1), nn.Linear(out_channels, latent_spaces[-1]), nn.ReLU())
        self.pos_dynamic_prompt = nn.Parameter(torch.randn(1, 1, *vs))
        self.neg_dynamic_prompt = nn.Parameter(torch.randn(1, 1, *vs))
        self.fusion_layer = StackedFusionConvLayers(cfg, 2, 8, 1, 3)
        self.modulator = Convolution(cfg, 2, 1, act="relu")        # never used in forward (parameters only)
        self.modulator_3c = Convolution(cfg, 3, 1, act="relu")     # never used in forward
        self.reweigh = nn.Parameter(torch.ones(vs))
        self.final_act = nn.ReLU()
        self.pos_reweigh = nn.Parameter(torch.ones((1, *vs)))
        self.neg_reweigh = nn.Parameter(torch.ones((1, *vs)))
        self.deep_modulator_3c = StackedFusionConvLayers(cfg, 3, 16, 1, 3)
        self.final_pred_head = Convolution(cfg, 2, 1, kernel_size=1, act="prelu_relu")
        self.roi_indices = list(ROI_INDICES)
        self.roi_names = list(ROI_NAMES)
        self.roi_ind_names_dict = dict(ROI_INDEX_TO_NAME)
        self.roi_ind_vol_names_dict = {k: "vol_" + "_".join(v.split("-")) for k, v in ROI_INDEX_TO_NAME.items()}
        self.general_dynamic_prompt = nn.Parameter(torch.randn(1, 1, *vs))
        self.roi_wise_reweigh = nn.ParameterList([nn.Parameter(torch.ones(1)) for _ in self.roi_indices])
        self.all_stages, self.only_stage_two = True, False
        self.with_uq = kwargs.get("with_uq", False)
        self.static_prompts = kwargs.get("static_prompts", False)
        self.register_buffer("_roi_ids", torch.tensor(self.roi_indices, dtype=torch.int32), persistent=False)
        # the frozen BatchNorms' (mean, rstd) tables follow a later load_state_dict
        self.register_load_state_dict_post_hook(_refresh_after_load)

    def set_training(self, mode):
        self.training = mode

    def get_depth(self):
        return self.depth

    # -- ROI prior dicts -> (B, 36, 2) device tensor (host shim; the painting itself is a HIP kernel)
    def _priors(self, roi_pred_dicts, B, device):
        if torch.is_tensor(roi_pred_dicts):
            return roi_pred_dicts.to(device=device, dtype=torch.float32).contiguous()
        tab = np.empty((B, len(self.roi_indices), 2), dtype=np.float32)
        for b in range(B):
            for i, idx in enumerate(self.roi_indices):
                d = roi_pred_dicts[b][self.roi_ind_names_dict[idx]]
                tab[b, i, 0] = np.nan_to_num(d["loc"])
                tab[b, i, 1] = np.nan_to_num(d["std"])
        return torch.from_numpy(tab).to(device)

    def _modulator_with_uq(self, xi, covariate, roi_pred_dicts, sample_roi_mask, unet_out_dst, prompt_use=(True, True),
                           after_unet=None):
        """attn_unet_data_parallel.py:630-658 on internal tensors.  ``unet_out_dst(cat_a)`` runs the U-Net and
        makes its reduce conv write straight into channel 1 of the (modulated_prompt, out) buffer."""
        cfg = self.cfg
        B, D, H, W, _ = xi.shape
        dt, dev = xi.dtype, xi.device
        assert (D, H, W) == self.volume_shape, f"model built for {self.volume_shape}, got {(D, H, W)}"
        cat_a = ops._new((B, D, H, W, 2), dt, dev)   # cat((modulated_prompt, out)) :654
        cat_b = ops._new((B, D, H, W, 2), dt, dev)   # cat((out, fusion(...)))     :654
        out_a, enc, dec = unet_out_dst(cat_a[..., 1:2])
        if after_unet is not None:
            after_unet(enc)          # (the projection heads: queued here, beside the tail below)
        out_b = ops.Copy.apply(out_a, Out(cat_b[..., 0:1]))
        prior = self._priors(roi_pred_dicts, B, dev)
        abeta = covariate.reshape(B, -1)[:, 0].to(device=dev, dtype=torch.float32).contiguous()
        roi = to_internal(sample_roi_mask.reshape(B, 1, D, H, W)).to(device=dev, dtype=torch.float32)
        p3 = ops.RoiPaint.apply(self.pos_dynamic_prompt, self.neg_dynamic_prompt, roi, xi, prior, self._roi_ids, abeta, dt,
                                prompt_use[0], prompt_use[1])
        dm = self.deep_modulator_3c(p3)
        general = to_internal(self.general_dynamic_prompt).to(dt)
        modulated = ops.AddBcast.apply(general, dm, Out(cat_a[..., 0:1]))
        fus = self.fusion_layer(ops.JoinSlices.apply(Out(cat_a), modulated, out_a), out=cat_b[..., 1:2])
        final = self.final_pred_head(ops.JoinSlices.apply(Out(cat_b), out_b, fus))   # IN + PReLU + final ReLU
        return final, enc, dec

    def forward(self, x, covariate=None, roi_pred_dicts=None, sample_roi_mask=None):
        if covariate is not None:     # one cast for every conditional layer (each routing reads fp32 covariates)
            covariate = covariate.to(device=x.device, dtype=torch.float32).contiguous()
        xi = _padded_input(x, self.cfg.compute_dtype)
        reset_cov_cache()
        if covariate is not None and covariate.dim() == 3 and covariate.shape[2] > 5:
            cov_rows(covariate[:, :, :5], x.shape[0], x.device)      # the 5-covariate layers' rows: one copy, made before the fork
        ops.SidePrep.begin(x.device)      # (opt-in) weight preparation runs beside the convolutions from here on
        cfgs = (self.cfg, self.cfg_heads) if self.training else ()
        for c in cfgs:
            c.begin_forward()
        # every layer's routing + expert mix up front, on a few streams beside each other (ops.PrepAhead; the first forward of
        # a configuration records which layers prepare what)
        if covariate is not None and covariate.dim() == 3 and x.is_cuda:
            ops.PrepAhead.begin(self, (tuple(x.shape), x.dtype, self.cfg.compute_dtype, self.training, torch.is_grad_enabled(),
                                       bool(x.requires_grad), self.static_prompts, bool(self.cfg.eval_fused),
                                       # frozen gates run piecewise (one more prepared layer each): their own plans
                                       self.training and (self.cfg.frozen_bn or sum(not m.training for m in self.batchnorms()))),
                                 x.device, covariate, x.shape[0])
        ok = False
        try:
            res = self._forward(x, xi, covariate, roi_pred_dicts, sample_roi_mask)
            ok = True
            return res
        finally:
            ops.PrepAhead.end(ok)
            for c in cfgs:
                c.end_forward()

    def _forward(self, x, xi, covariate, roi_pred_dicts, sample_roi_mask):
        # which learned prompts this batch selects (:638-639).  The reference does one .item() per sample
        # mid-forward; here it is one host read BEFORE any kernel is queued, and `static_prompts` skips it
        # (both prompts then always receive a gradient, zeros when unselected).
        if self.static_prompts:
            use = (True, True)
        else:
            ab = covariate.reshape(x.shape[0], -1)[:, 0].tolist()
            use = (any(a == 1 for a in ab), any(a != 1 for a in ab))
        # The five projection heads (two 1x1x1 convolutions to ONE channel with their norms each: ~30 launches of 5-30 us) need
        # the encoder features only.  They are queued right behind the U-Net on an idle side stream (one of ops.PrepAhead's),
        # so that they run beside the full-resolution tail instead of behind it; the main stream waits for them at the end.
        want_proj = self.training or self.embeddings_out
        side = {"projected": None, "stream": None}

        def heads(enc_):
            dev = enc_[0].device
            if (ops.PrepAhead.enabled and not ops.SidePrep._on and dev.type == "cuda" and not ops.KernelTimer.enabled
                    and os.environ.get("COMA_HEADS_SIDE", "1") != "0"):
                st = ops.PrepAhead.streams(dev)[0]
                st.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(st):
                    side["projected"] = [self.projection_heads[i](enc_[i]) for i in range(self.depth)]
                side["stream"] = st
                if st not in ops.PrepAhead.branch_streams:
                    ops.PrepAhead.branch_streams.append(st)
        out, enc, _dec = self._modulator_with_uq(xi, covariate, roi_pred_dicts, sample_roi_mask,
                                                 lambda dst: self._unet(xi, covariate, out=dst), use,
                                                 heads if want_proj else None)
        out_ext = to_external(out)
        if not want_proj:
            return out_ext
        if side["projected"] is not None:
            projected = side["projected"]
            cur = torch.cuda.current_stream(out.device)
            cur.wait_stream(side["stream"])
            for t in projected:
                t.record_stream(cur)
        else:
            projected = [self.projection_heads[i](enc[i]) for i in range(self.depth)]
        m = ops.SpatialMean.apply(out)                                   # AdaptiveAvgPool3d(1)
        lin = self.final_projection_head[1]
        # Linear(1 -> 2048) as a broadcast multiply-add: (B,1,1,1,2048), 2048 numbers of glue.  (F.linear sent the backward
        # through a rocBLAS GEMM of shape (2, 2048) x (2048, 1) that takes 49 us per step.)
        if lin.in_features == 1:
            final_proj = F.relu(m.view(-1, 1, 1, 1, 1) * lin.weight.view(-1) + lin.bias)
        else:
            final_proj = F.relu(F.linear(m.view(-1, 1, 1, 1, 1), lin.weight, lin.bias))
        if self.embeddings_out:
            return out_ext, projected, final_proj, [to_external(e) for e in enc]
        if self.decoder_ds:
            return out_ext, projected, final_proj, []
        return out_ext, projected, final_proj


# the host loops of the reference module (train_dp :696, contrastive_test :1129, print_metrics :1109): same names here,
# so `attn_unet_data_parallel.train_dp(...)` of validation.py:158 resolves after the import swap
from .train_loop import train_dp, contrastive_test, print_metrics, record_results, extract_id   # noqa: E402,F401
