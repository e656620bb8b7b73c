"""Inference path: eval-mode attention gates as one fused launch, the forward captured in a hipGraph and replayed.

In eval mode every BatchNorm of the gate (MONAI AttentionBlock, attn_unet_data_parallel.py:134-150) is a known affine map:

    att = x * psi,   psi = sigmoid(a_p * (w_psi . relu(scale_g * (W_g g) + scale_x * (W_x x) + shift)) + b_p)

``fold_gate`` folds the running statistics, the BatchNorm affines and the three convolution biases into five small tables
once; ``gate_eval`` runs the gate from them (csrc/gate.hip: ``gate_eval_mfma_k`` with both 1x1x1 convolutions inside for
bf16 tensors of up to 64 channels, ``gate_eval_fwd_k`` behind the two convolutions otherwise); ``Predictor`` owns the folds,
static input buffers and the captured graph.  Everything here is opt-in: a model nobody wraps in a ``Predictor`` launches
exactly what it launched before (``Config.eval_fused`` is False outside a Predictor's own forwards).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops

MFMA_ROWS = 32        # gate_eval_mfma_k's row tile: folded weights and its tables are zero-padded to this many rows

# which form served the gates so far (diagnostic / tests)
counts = {"mfma": 0, "elementwise": 0}


def _rstd(bn):
    return torch.rsqrt(bn.running_var + bn.eps)


def fold_gate(block):
    """The folded tensors of one ObservableAttentionBlock in eval mode, in the dtype of its parameters (fp32 in a model):

      scale_g, scale_x [F]   gamma * rstd of BN_g / BN_x
      shift [F]              both betas, both means and both convolution biases: what is added to
                             scale_g * (W_g g) + scale_x * (W_x x), the products WITHOUT their biases
      w_psi [F], psi_ab [2]  psi = sigmoid(psi_ab[0] * (w_psi . s) + psi_ab[1])
      wg, wx                 bf16 [32][C]: diag(scale_g) W_g, diag(scale_x) W_x, zero rows beyond F   } only where the MFMA
      shift32, w_psi32       shift / w_psi zero-padded to 32 entries                                   } form can apply

    Plain torch on the parameters' device, no host read."""
    cg, bng = block.W_g[0].conv, block.W_g[1]
    cx, bnx = block.W_x[0].conv, block.W_x[1]
    cp, bnp = block.psi[0].conv, block.psi[1]
    with torch.no_grad():
        f_int = cg.weight.shape[0]
        sg, sx = bng.weight * _rstd(bng), bnx.weight * _rstd(bnx)
        bias_g = cg.bias if cg.bias is not None else torch.zeros_like(sg)
        bias_x = cx.bias if cx.bias is not None else torch.zeros_like(sx)
        shift = (bng.bias + (bias_g - bng.running_mean) * sg) + (bnx.bias + (bias_x - bnx.running_mean) * sx)
        a_p = (bnp.weight * _rstd(bnp)).reshape(1)
        b_psi = cp.bias.reshape(1) if cp.bias is not None else torch.zeros_like(a_p)
        b_p = a_p * b_psi + bnp.bias.reshape(1) - a_p * bnp.running_mean.reshape(1)
        fold = {"scale_g": sg.contiguous(), "scale_x": sx.contiguous(), "shift": shift.contiguous(),
                "w_psi": cp.weight.reshape(-1).clone(), "psi_ab": torch.cat([a_p, b_p]).contiguous()}
        c_g, c_x = cg.weight.shape[1], cx.weight.shape[1]
        if c_g == c_x and c_g % 16 == 0 and 16 <= c_g <= 64 and f_int <= MFMA_ROWS:
            def padded(t, rows=MFMA_ROWS):
                z = torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
                z[:t.shape[0]] = t
                return z
            fold["wg"] = padded(sg[:, None] * cg.weight.reshape(f_int, c_g)).to(torch.bfloat16)
            fold["wx"] = padded(sx[:, None] * cx.weight.reshape(f_int, c_x)).to(torch.bfloat16)
            fold["shift32"], fold["w_psi32"] = padded(shift), padded(fold["w_psi"])
    return fold


def gate_eval(block, g, x, out=None, want_psi=False, fold=None, form=None):
    """The eval-mode gate of `block` on internal (B, D, H, W, C) tensors: (att, psi or None).  `out`: destination view
    (a channel slice of the concat buffer).  fold: fold_gate(block) (default: the fold a Predictor attached).
    form: None picks (the MFMA form wherever coma_gate_eval_mfma_ok answers 1 and the level is not excluded), or
    "elementwise" to force the kernel behind the W_g / W_x convolutions."""
    from .layers import conv_plain
    cfg = block.cfg
    fold = fold if fold is not None else block._eval_fold
    f_int = fold["scale_g"].numel()
    if form is None:
        form = "mfma" if ("wg" in fold and ops.gate_eval_mfma_ok(g, x, f_int) and
                          (out is None or ops.gate_eval_mfma_ok(out, x, f_int))) else "elementwise"
    counts[form] += 1
    if form == "mfma":
        return ops.gate_eval_mfma(g, x, fold, out, want_psi)
    with torch.no_grad():
        g1raw = conv_plain(cfg, g, block.W_g[0].conv, 1, 1, False, with_bias=False)
        x1raw = conv_plain(cfg, x, block.W_x[0].conv, 1, 1, False, with_bias=False)
    return ops.gate_eval_fwd(x, g1raw, x1raw, fold, out, want_psi)


def _gates(model):
    from .attn_unet_data_parallel import ObservableAttentionBlock
    return [m for m in model.modules() if isinstance(m, ObservableAttentionBlock)]


class Predictor:
    """The eval forward of a ContrastiveAttentionUNET_DP at one fixed batch shape, folded and (graph=True) replayed.

        pred = Predictor(model, batch)            # folds, warms up, captures
        y = pred(next_batch)                      # copies into the static inputs, replays: (B, 1, D, H, W)
        pred.refresh()                            # after the model's parameters / running statistics changed

    `batch`: {"mri", "covars", "roi", "roi_pred_dicts"} with device tensors (the priors as a (B, 36, 2) tensor or the
    reference's list of dicts).  The returned tensor is the predictor's own output buffer: the next call rewrites it.
    The model is left as it was found: its mode flags are restored after every forward, and parameters, running
    statistics and num_batches_tracked are never written (eval mode, no_grad).  graph=False runs the same fast path
    eagerly.

    Predicting from the weight average of ``FusedAdamW(ema_decay=...)``: either load it into a model of its own
    (``model.load_state_dict(ckpt["ema_state_dict"])``, then build the Predictor on that model), or build or ``refresh()``
    the Predictor inside ``with optimizer.ema_weights():`` -- the swap is by content, so the captured graph's addresses
    stay valid; the folds are copies of the parameters' values, so ``refresh()`` once more after the block to predict
    from the iterate again."""

    def __init__(self, model, batch, graph=True, warmup=2):
        if getattr(model, "embeddings_out", False):
            raise ValueError("Predictor: build the model with embeddings_out=False (the embeddings are not part of the inference path)")
        if getattr(model, "save_attn", None):
            raise ValueError("Predictor: save_attn must be unset (model.set_save_attn(None))")
        mri = batch["mri"]
        p0 = next(model.parameters())
        if not (torch.is_tensor(mri) and mri.is_cuda and p0.is_cuda):
            raise ValueError("Predictor: the model and the batch must live on the GPU (there is no CPU path)")
        self.model, self.graphed = model, bool(graph)
        dev = mri.device
        B = mri.shape[0]
        self.batch = {k: batch[k].to(dev).clone() for k in ("mri", "covars", "roi")}
        self.batch["roi_pred_dicts"] = model._priors(batch["roi_pred_dicts"], B, dev).clone()
        self._folds = {}          # gate block -> fold (tensors updated IN PLACE by refresh: a captured graph holds their addresses)
        self._stats = {}          # eval BatchNorm3d -> (mean, rstd) fp32 (1, C)
        self.refresh()
        self.graph = None
        self.out = None
        if self.graphed:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(max(int(warmup), 2)):      # first: ops.PrepAhead records its plan; second: sizes its buffers
                    self._forward()
            torch.cuda.current_stream(dev).wait_stream(side)
            from ._lib import pin_workspace
            self._ws = pin_workspace(dev)                 # the graph bakes this buffer's address in
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self.out = self._forward()

    # ---- folding ----
    def refresh(self):
        """(Re)fold every gate and every eval BatchNorm's (mean, rstd) from the model's current state, into the tensors
        the forward (and a captured graph) already reads."""
        with torch.no_grad():
            for blk in _gates(self.model):
                new = fold_gate(blk)
                old = self._folds.get(blk)
                if old is None:
                    self._folds[blk] = new
                else:
                    for k, v in new.items():
                        old[k].copy_(v)
            for m in self.model.modules():
                if isinstance(m, nn.BatchNorm3d):
                    C = m.num_features
                    mean = m.running_mean.reshape(1, C).float()
                    rstd = torch.rsqrt(m.running_var.reshape(1, C).float() + m.eps)
                    old = self._stats.get(m)
                    if old is None:
                        self._stats[m] = (mean.clone(), rstd.contiguous())
                    else:
                        old[0].copy_(mean)
                        old[1].copy_(rstd)

    # ---- inputs ----
    def fits(self, mri):
        return tuple(mri.shape) == tuple(self.batch["mri"].shape)

    def load(self, batch):
        """Copy a batch into the static input buffers (a list of prior dicts goes through model._priors)."""
        for k in ("mri", "covars", "roi"):
            if k in batch:
                self.batch[k].copy_(batch[k].reshape(self.batch[k].shape), non_blocking=True)
        if batch.get("roi_pred_dicts") is not None:
            pr = self.batch["roi_pred_dicts"]
            pr.copy_(self.model._priors(batch["roi_pred_dicts"], pr.shape[0], pr.device), non_blocking=True)

    # ---- execution ----
    def _forward(self):
        model, cfg = self.model, self.model.cfg
        modes = [(m, m.training) for m in model.modules()]
        saved = (cfg.eval_fused, cfg.eval_stats, model.static_prompts)
        gates = list(self._folds.items())
        try:
            for m, _t in modes:
                m.training = False
            # (static_prompts only skips the host read that decides which prompt gets a gradient: no effect on the output)
            cfg.eval_fused, cfg.eval_stats, model.static_prompts = True, self._stats, True
            for blk, fold in gates:
                blk._eval_fold = fold
            b = self.batch
            with torch.no_grad():
                return model(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        finally:
            for blk, _f in gates:
                blk._eval_fold = None
            cfg.eval_fused, cfg.eval_stats, model.static_prompts = saved
            for m, t in modes:
                m.training = t

    def __call__(self, batch=None):
        if batch is not None:
            self.load(batch)
        if self.graph is not None:
            self.graph.replay()
            return self.out
        self.out = self._forward()
        return self.out
