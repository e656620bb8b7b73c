"""MI355X drop-in for the live loss path of the reference ``criterions`` module.

Same class names / call signatures as /root/reference/criterions.py:
``RoiMSE`` (:124-211), ``GenerativeContrastiveLoss`` (:485-575),
``LabelDifference`` / ``FeatureSimilarity`` / ``RnCLoss`` (:579-644), and the two voxel-weighted alternatives the
drivers keep at hand, ``RoiRRMSE`` / ``RoiRSE`` (:28-122), with ``RoiWeightedMSE`` beside them, and ``RoiMeanLoss`` /
``WithRoiMean``, a loss on the regional means the validation loop reports, and ``GradientDifferenceLoss`` / ``WithGradDiff``,
an edge term on the image gradient (neither has a counterpart upstream).  The voxel losses are
fused HIP kernels (one pass: label->weight LUT, squared/absolute difference, per-sample
reduction; gradient in one more pass).  RnC works on a (B, 512) feature matrix and a (B, 6)
label matrix -- a few thousand numbers -- and stays as torch glue.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .roi_tables import ROI_INDICES


def _vol_internal(t: torch.Tensor, dtype=None):
    """(B, 1, D, H, W) -> (B, D, H, W, 1)"""
    assert t.dim() == 5 and t.shape[1] == 1, t.shape
    v = t.permute(0, 2, 3, 4, 1)
    return v if dtype is None else v.to(dtype)


class _RoiTables:
    """Device-side ROI id / weight tables shared by the ROI losses."""

    def _tables(self, dev):
        """ROI id / weight tables on the device, rebuilt only when the weights object changes
        (no host->device copy inside the step: keeps it hipGraph-capturable)."""
        key = (dev, id(self.roi_weights), getattr(self.roi_weights, "_version", 0), tuple(self.roi_indices))
        if getattr(self, "_tab_key", None) != key:
            self._tab = (torch.as_tensor(list(self.roi_indices), dtype=torch.int32, device=dev),
                         torch.as_tensor(self.roi_weights, dtype=torch.float32).to(dev).contiguous())
            self._tab_key = key
        return self._tab


class RoiMSE(_RoiTables, nn.Module):
    """loss_b = mean_vox(mask_b) * mean_vox((pred_b - gt_b)^2), mask = ROI weight of each voxel's label."""

    def __init__(self, roi_weights, roi_indices, reduction="mean", scale_factor=360, voxel_wise=False, template=None):
        super().__init__()
        self.roi_weights = roi_weights
        self.roi_indices = roi_indices
        self.batch_reduction = reduction
        self.scale_factor = scale_factor
        self.voxel_wise = voxel_wise
        self.voxel_weights = None
        if voxel_wise:
            # criterions.py:135-145.  The reference reads its label template from a private file
            # (data_util.load_template(), absent upstream); here it is the `template` argument (a (D, H, W) label volume).
            if template is None:
                try:
                    import data_util
                    template = data_util.load_template()
                except Exception as e:
                    raise NotImplementedError("RoiMSE(voxel_wise=True) needs the label template: pass template=<(D,H,W) label "
                                              "volume> (the reference loads it with data_util.load_template(), criterions.py:138)") from e
            roi_mask = torch.as_tensor(template)
            w = torch.as_tensor(roi_weights, dtype=torch.float32)
            voxel_weights = torch.ones(tuple(roi_mask.shape), dtype=torch.float32, device=w.device)
            roi_mask = roi_mask.to(w.device)
            for i, idx in enumerate(self.roi_indices):
                voxel_weights[roi_mask == idx] = w[i]
            norm_voxel_weights = voxel_weights / torch.norm(voxel_weights)
            nscaling_factor = 5. / torch.mean(norm_voxel_weights)
            self.voxel_weights = nscaling_factor * norm_voxel_weights

    def calculate_new_voxel_weights(self, errors, voxel_weights, with_update=False):   # criterions.py:161-168
        new_weights = voxel_weights * (1 + errors.to(device=self.voxel_weights.device))
        new_weights = new_weights / torch.norm(new_weights)
        scaling_factor = torch.mean(voxel_weights) / torch.mean(new_weights)
        new_weights *= scaling_factor
        if with_update:
            self.update_weights(new_weights)
        return new_weights

    def __str__(self):
        return (f"RoiMSE(\n  (roi_indices, roi_weights)={list(zip(self.roi_indices, self.roi_weights))}\n"
                f"  batch_reduciton={self.batch_reduction}\n)")

    def calculate_new_weights(self, errors, with_update=False):   # criterions.py:154-159
        new_weights = self.roi_weights * (1 / 2) * errors.to(device=self.roi_weights.device)
        new_weights = self.scale_factor * (new_weights / torch.norm(new_weights))
        if with_update:
            self.update_weights(new_weights)
        return new_weights

    def update_weights(self, weights):   # criterions.py:170-172 (a no-op upstream)
        return

    def forward(self, pred, gt, roi):
        dev = pred.device
        p = _vol_internal(pred)
        if self.voxel_weights is not None:
            # criterions.py:189-198: the mask is the (constant) voxel-weight volume, and the per-sample loss is
            # mean(mask * mean_vox((pred - gt)^2)) = mean(voxel_weights) * MSE_b: the same fused kernel with one label
            # (every voxel "0") whose weight is that mean (5 by construction, :143-145)
            key = (dev, tuple(p.shape[:4]))
            if getattr(self, "_vw_key", None) != key:
                self._vw = (torch.zeros(1, dtype=torch.int32, device=dev),
                            self.voxel_weights.float().mean().reshape(1).to(dev).contiguous(),
                            torch.zeros(tuple(p.shape[:4]) + (1,), dtype=torch.float32, device=dev))
                self._vw_key = key
            ids0, w0, zeros = self._vw
            loss = ops.RoiMSELoss.apply(p, _vol_internal(gt, p.dtype).contiguous(), zeros, ids0, w0)
            return torch.mean(loss) if self.batch_reduction == "mean" else loss
        ids, w = self._tables(dev)
        loss = ops.RoiMSELoss.apply(p, _vol_internal(gt, p.dtype).contiguous(),
                                    _vol_internal(roi, torch.float32).contiguous(), ids, w)   # (B, 1)
        if self.batch_reduction == "mean":
            return torch.mean(loss)
        return loss


class _RoiVoxelWeighted(_RoiTables, nn.Module):
    """The voxel-weighted ROI losses (one fused reduction + one streaming backward, csrc/roi_loss.hip): every voxel's
    squared error is weighted by w_v = roi_weights[slot of its label], or `background_weight` where the label is not in
    `roi_indices` (the reference starts its mask from torch.ones: 1).  Per sample, N = sum w (pred - gt)^2 and
        RoiWeightedMSE  N / sum w
        RoiRSE          N / sum (gt - m)^2,  m = mean(w gt)     (criterions.py:101-121)
        RoiRRMSE        sqrt(N / sum w gt^2)                    (criterions.py:40-67)
    RoiRSE's denominator is the reference's: UNWEIGHTED, about the weighted "mean" m (:109-112).  No clamps: a zero
    denominator, or a zero numerator under RoiRRMSE, gives inf / nan values or gradients exactly as the reference's
    autograd does.  The target gets no gradient.

    `reduction` ("mean": batch mean; "sum", as the reference for anything but "mean": batch sum; None: the per-sample
    (B, 1) vector, what train_dp sets) is also readable and writable as `batch_reduction`, the attribute the training
    loop, GenerativeContrastiveLoss and WithSSIM use."""

    KIND = None
    voxel_wise = False
    voxel_weights = None

    def __init__(self, roi_weights, roi_indices, reduction="mean", background_weight=1.0, scale_factor=360):
        super().__init__()
        name = type(self).__name__
        if reduction not in ("mean", "sum", None):
            raise ValueError(f"{name}: reduction must be 'mean', 'sum' or None, got {reduction!r}")
        n = len(roi_indices)
        if not 1 <= n <= 64:
            raise ValueError(f"{name}: 1..64 ROI indices expected, got {n}")
        if len(roi_weights) != n:
            raise ValueError(f"{name}: {len(roi_weights)} weights for {n} ROI indices")
        bg = float(background_weight)
        if bg != bg or bg in (float("inf"), float("-inf")):
            raise ValueError(f"{name}: background_weight must be finite, got {background_weight}")
        self.roi_weights = roi_weights
        self.roi_indices = roi_indices
        self.batch_reduction = reduction
        self.background_weight = bg
        self.scale_factor = scale_factor

    @property
    def reduction(self):
        return self.batch_reduction

    @reduction.setter
    def reduction(self, value):
        self.batch_reduction = value

    def __str__(self):
        return (f"{type(self).__name__}(\n  roi_weights={self.roi_weights}\n  roi_indices={self.roi_indices}\n"
                f"  reduction={self.batch_reduction}\n)")

    calculate_new_weights = RoiMSE.calculate_new_weights      # criterions.py:154-159: what the training loop calls
    update_weights = RoiMSE.update_weights                    # (a no-op upstream)

    def forward(self, pred, gt, roi):
        name = type(self).__name__
        if roi is None:
            raise ValueError(f"{name}: needs the ROI label volume")
        if pred.dim() != 5 or pred.shape[1] != 1 or pred.shape != gt.shape or pred.shape != roi.shape:
            raise ValueError(f"{name}: (B, 1, D, H, W) volumes of equal shape expected, got {tuple(pred.shape)}, "
                             f"{tuple(gt.shape)}, {tuple(roi.shape)}")
        ids, w = self._tables(pred.device)
        p = _vol_internal(pred)
        loss = ops.RoiWeightedLoss.apply(p, _vol_internal(gt.detach(), p.dtype).contiguous(),
                                         _vol_internal(roi, torch.float32).contiguous(), ids, w,
                                         self.background_weight, self.KIND)   # (B, 1)
        if self.batch_reduction is None:
            return loss
        return torch.mean(loss) if self.batch_reduction == "mean" else torch.sum(loss)


class RoiWeightedMSE(_RoiVoxelWeighted):
    """sum_v w_v (pred - gt)^2 / sum_v w_v per sample."""

    KIND = ops.RoiWeightedLoss.WMSE

    def __init__(self, roi_weights, roi_indices, reduction="mean", background_weight=1.0):
        super().__init__(roi_weights, roi_indices, reduction, background_weight)


class RoiRSE(_RoiVoxelWeighted):
    """Relative squared error weighted by ROI: the reference's class (criterions.py:82-121), constructor and forward."""

    KIND = ops.RoiWeightedLoss.RSE

    def __init__(self, roi_weights, roi_indices, reduction="mean"):
        super().__init__(roi_weights, roi_indices, reduction)


class RoiRRMSE(_RoiVoxelWeighted):
    """Relative root mean squared error weighted by ROI: the reference's class (criterions.py:28-67)."""

    KIND = ops.RoiWeightedLoss.RRMSE

    def __init__(self, roi_weights, roi_indices, reduction="mean"):
        super().__init__(roi_weights, roi_indices, reduction)


class VoxelL1(nn.Module):
    """Per-sample voxel MAE (BASELINE config C2 names an L1 loss; the reference only has MAE as a metric,
    attn_unet_data_parallel.py:1215 -- provided as an optional generative loss)."""

    def __init__(self, reduction="mean"):
        super().__init__()
        self.batch_reduction = reduction

    def forward(self, pred, gt, roi=None):
        p = _vol_internal(pred)
        loss = ops.L1Loss.apply(p, _vol_internal(gt, p.dtype).contiguous())
        return torch.mean(loss) if self.batch_reduction == "mean" else loss


class SSIMLoss(nn.Module):
    """1 - SSIM per sample, differentiable in `pred` (the value is 1 - metrics.ssim3d; the constructor is
    monai.losses.SSIMLoss's without spatial_dims).  The target is a label and gets no gradient."""

    MAX_WIN = 11        # SSIM_MAXW of csrc/metrics.hip

    def __init__(self, data_range=1.0, kernel_type="gaussian", win_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03, reduction="mean"):
        super().__init__()
        from .metrics import ssim_window
        if int(win_size) != win_size or not 1 <= win_size <= self.MAX_WIN:
            raise ValueError(f"SSIMLoss: win_size must be an integer in 1..{self.MAX_WIN}, got {win_size}")
        if kernel_type not in ("gaussian", "uniform"):
            raise ValueError(f"SSIMLoss: kernel_type must be 'gaussian' or 'uniform', got {kernel_type!r}")
        if reduction not in ("mean", None):
            raise ValueError(f"SSIMLoss: reduction must be 'mean' or None, got {reduction!r}")
        if not float(data_range) > 0 or (kernel_type == "gaussian" and not float(kernel_sigma) > 0):
            raise ValueError("SSIMLoss: data_range and kernel_sigma must be positive")
        self.win_size = int(win_size)
        self.window = ssim_window(kernel_type, self.win_size, kernel_sigma)
        self.c1, self.c2 = (k1 * float(data_range)) ** 2, (k2 * float(data_range)) ** 2
        self.batch_reduction = reduction

    def forward(self, pred, gt, roi=None):
        if pred.dim() != 5 or pred.shape[1] != 1 or pred.shape != gt.shape:
            raise ValueError(f"SSIMLoss: (B, 1, D, H, W) volumes of equal shape expected, got {tuple(pred.shape)}, {tuple(gt.shape)}")
        if min(pred.shape[2:]) < self.win_size:
            raise ValueError(f"SSIMLoss: volume {tuple(pred.shape[2:])} is smaller than the {self.win_size}-wide window")
        p = _vol_internal(pred)
        loss = ops.SSIMLoss.apply(p, _vol_internal(gt.detach(), p.dtype).contiguous(), self.window, self.c1, self.c2)   # (B, 1)
        return torch.mean(loss) if self.batch_reduction == "mean" else loss


class WithSSIM(nn.Module):
    """A generative loss plus an SSIM term: base(pred, gt, roi) + ssim_weight * (1 - ssim_b) -- per sample while
    `batch_reduction` is None, else the batch mean of both.  `batch_reduction` IS the base loss's (one shared attribute),
    and everything the training loop reads from `criterion.gen_loss` (ROI tables, weight updates) is the base loss's."""

    _BASE_ATTRS = ("batch_reduction", "roi_indices", "roi_weights", "voxel_wise", "voxel_weights", "scale_factor")
    _BASE_METHODS = ("calculate_new_weights", "calculate_new_voxel_weights", "update_weights")

    def __init__(self, base, ssim_weight, **ssim_kwargs):
        super().__init__()
        if not hasattr(base, "batch_reduction"):
            raise ValueError("WithSSIM: base must be a generative loss with a batch_reduction attribute")
        w = float(ssim_weight)
        if not (w >= 0.0 and w != float("inf")):
            raise ValueError(f"WithSSIM: ssim_weight must be a finite number >= 0, got {ssim_weight}")
        self.base = base
        self.ssim_weight = w
        self.ssim = SSIMLoss(**dict(ssim_kwargs, reduction=None))

    def __getattr__(self, name):
        if name in WithSSIM._BASE_ATTRS or name in WithSSIM._BASE_METHODS:
            return getattr(super().__getattr__("base"), name)
        return super().__getattr__(name)

    def __setattr__(self, name, value):
        if name in WithSSIM._BASE_ATTRS:
            setattr(self.base, name, value)
        else:
            super().__setattr__(name, value)

    def forward(self, pred, gt, roi=None):
        loss = self.base(pred, gt, roi)
        s = self.ssim(pred, gt)                                    # (B, 1)
        return loss + self.ssim_weight * (s if self.batch_reduction is None else torch.mean(s))


class RoiMeanLoss(_RoiTables, nn.Module):
    """A loss on the regional means (the per-ROI SUVR means the validation loop reports): per sample, with
    d_r = mean_r(pred) - mean_r(gt) over the voxels labelled roi_indices[r],
        loss_b = sum_r w_r phi(d_r) / sum_r w_r     over the regions PRESENT in the sample's label volume
    phi = d^2 (kind "mse"), |d| ("l1") or huber_loss's pointwise form with `delta` ("huber").  A region without voxels is
    skipped; a sample with no present region (or zero total weight) has loss 0 and gradient 0 -- never NaN.  Labels follow
    the kernels' table rules: exact integer values, the first occurrence of a duplicated id wins.  One fused label-segmented
    reduction without atomics (csrc/roi_mean.hip, bitwise repeatable) and one streaming backward; the target gets no gradient.

    `reduction` ("mean", "sum" or None: the per-sample (B, 1) vector) is also readable and writable as `batch_reduction`."""

    KINDS = ops.RoiMeanLoss.KINDS

    def __init__(self, roi_weights, roi_indices, kind="mse", delta=1.0, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum", None):
            raise ValueError(f"RoiMeanLoss: reduction must be 'mean', 'sum' or None, got {reduction!r}")
        if kind not in self.KINDS:
            raise ValueError(f"RoiMeanLoss: kind must be one of {sorted(self.KINDS)}, got {kind!r}")
        n = len(roi_indices)
        if not 1 <= n <= 64:
            raise ValueError(f"RoiMeanLoss: 1..64 ROI indices expected, got {n}")
        if len(roi_weights) != n:
            raise ValueError(f"RoiMeanLoss: {len(roi_weights)} weights for {n} ROI indices")
        d = float(delta)
        if kind == "huber" and not (d > 0.0 and d != float("inf")):
            raise ValueError(f"RoiMeanLoss: huber delta must be positive and finite, got {delta}")
        self.roi_weights = roi_weights
        self.roi_indices = roi_indices
        self.kind = kind
        self.delta = d
        self.batch_reduction = reduction

    @property
    def reduction(self):
        return self.batch_reduction

    @reduction.setter
    def reduction(self, value):
        self.batch_reduction = value

    def __str__(self):
        return (f"RoiMeanLoss(\n  roi_weights={self.roi_weights}\n  roi_indices={self.roi_indices}\n  kind={self.kind}\n"
                f"  reduction={self.batch_reduction}\n)")

    def forward(self, pred, gt, roi):
        if roi is None:
            raise ValueError("RoiMeanLoss: needs the ROI label volume")
        if pred.dim() != 5 or pred.shape[1] != 1 or pred.shape != gt.shape or pred.shape != roi.shape:
            raise ValueError(f"RoiMeanLoss: (B, 1, D, H, W) volumes of equal shape expected, got {tuple(pred.shape)}, "
                             f"{tuple(gt.shape)}, {tuple(roi.shape)}")
        ids, w = self._tables(pred.device)
        p = _vol_internal(pred)
        loss = ops.RoiMeanLoss.apply(p, _vol_internal(gt.detach(), p.dtype).contiguous(),
                                     _vol_internal(roi, torch.float32).contiguous(), ids, w,
                                     self.KINDS[self.kind], self.delta)   # (B, 1)
        if self.batch_reduction is None:
            return loss
        return torch.mean(loss) if self.batch_reduction == "mean" else torch.sum(loss)


class WithRoiMean(nn.Module):
    """A generative loss plus a regional-mean term: base(pred, gt, roi) + roi_mean_weight * roi_mean_b (RoiMeanLoss) -- per
    sample while `batch_reduction` is None, else reduced over the batch as the base is.  `batch_reduction` IS the base
    loss's, and so is everything else WithSSIM forwards; the two wrappers nest in either order.  The term's tables are
    `roi_weights` / `roi_indices` when given, else the base's LIVE ones: a weight update of the base reaches the term."""

    _BASE_ATTRS = WithSSIM._BASE_ATTRS
    _BASE_METHODS = WithSSIM._BASE_METHODS

    def __init__(self, base, roi_mean_weight, kind="mse", delta=1.0, roi_weights=None, roi_indices=None):
        super().__init__()
        if not hasattr(base, "batch_reduction"):
            raise ValueError("WithRoiMean: base must be a generative loss with a batch_reduction attribute")
        w = float(roi_mean_weight)
        if not (w >= 0.0 and w != float("inf")):
            raise ValueError(f"WithRoiMean: roi_mean_weight must be a finite number >= 0, got {roi_mean_weight}")
        if (roi_weights is None) != (roi_indices is None):
            raise ValueError("WithRoiMean: give both roi_weights and roi_indices, or neither (the base's tables)")
        live = roi_weights is None
        if live and not (hasattr(base, "roi_weights") and hasattr(base, "roi_indices")):
            raise ValueError("WithRoiMean: base has no ROI tables: pass roi_weights and roi_indices")
        self.base = base
        self.roi_mean_weight = w
        self.live_tables = live
        self.roi_mean = RoiMeanLoss(base.roi_weights if live else roi_weights, base.roi_indices if live else roi_indices,
                                    kind=kind, delta=delta, reduction=None)

    def __getattr__(self, name):
        if name in WithRoiMean._BASE_ATTRS or name in WithRoiMean._BASE_METHODS:
            return getattr(super().__getattr__("base"), name)
        return super().__getattr__(name)

    def __setattr__(self, name, value):
        if name in WithRoiMean._BASE_ATTRS:
            setattr(self.base, name, value)
        else:
            super().__setattr__(name, value)

    def forward(self, pred, gt, roi=None):
        loss = self.base(pred, gt, roi)
        if self.live_tables:
            self.roi_mean.roi_weights, self.roi_mean.roi_indices = self.base.roi_weights, self.base.roi_indices
        m = self.roi_mean(pred, gt, roi)                           # (B, 1)
        red = self.batch_reduction
        return loss + self.roi_mean_weight * (m if red is None else torch.mean(m) if red == "mean" else torch.sum(m))


class GradientDifferenceLoss(nn.Module):
    """Gradient-difference loss (Mathieu et al. 2016; Nie et al. 2018): the edge term that counters the blur of a squared-error
    loss.  Per sample, with gp / gg the forward differences of pred / gt along axis a in (z, y, x),
        loss_b = sum_a axis_weights[a] * mean over the counted pairs of | |gp| - |gg| |^alpha    (mode "abs", the classic form)
                                                                     or |  gp  -  gg  |^alpha    (mode "signed")
    alpha 1 or 2.  mask None counts every pair; mask "brain" only those whose two voxels both have a non-zero label in `roi`
    (the MRI is zeroed outside the label volume: the brain boundary is no edge to learn).  An axis of length 1 or without a
    counted pair contributes 0 -- never NaN; sign(0) = 0 in the gradient, torch's subgradient of abs.  One fused tile pass
    forward and one backward (csrc/grad_diff.hip), no atomics, bitwise repeatable; the target gets no gradient.  For physical
    gradients on anisotropic voxels pass axis_weights = (1 / spacing_a) ** alpha.

    `reduction` ("mean", "sum" or None: the per-sample (B, 1) vector) is also readable and writable as `batch_reduction`."""

    MODES = ops.GradDiffLoss.MODES

    def __init__(self, alpha=1, mode="abs", axis_weights=(1.0, 1.0, 1.0), mask=None, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum", None):
            raise ValueError(f"GradientDifferenceLoss: reduction must be 'mean', 'sum' or None, got {reduction!r}")
        if isinstance(alpha, bool) or alpha not in (1, 2):
            raise ValueError(f"GradientDifferenceLoss: alpha must be 1 or 2, got {alpha!r}")
        if mode not in self.MODES:
            raise ValueError(f"GradientDifferenceLoss: mode must be one of {sorted(self.MODES)}, got {mode!r}")
        if mask not in (None, "brain"):
            raise ValueError(f"GradientDifferenceLoss: mask must be None or 'brain', got {mask!r}")
        try:
            aw = tuple(float(a) for a in axis_weights)
        except TypeError:
            aw = ()
        if len(aw) != 3 or not all(a >= 0.0 and a != float("inf") for a in aw):
            raise ValueError(f"GradientDifferenceLoss: axis_weights must be three finite numbers >= 0 (z, y, x), got {axis_weights!r}")
        self.alpha = int(alpha)
        self.mode = mode
        self.axis_weights = aw
        self.mask = mask
        self.batch_reduction = reduction

    @property
    def reduction(self):
        return self.batch_reduction

    @reduction.setter
    def reduction(self, value):
        self.batch_reduction = value

    def __str__(self):
        return (f"GradientDifferenceLoss(\n  alpha={self.alpha}\n  mode={self.mode}\n  axis_weights={self.axis_weights}\n"
                f"  mask={self.mask}\n  reduction={self.batch_reduction}\n)")

    def per_sample(self, pred, gt, roi=None, differentiable=True):
        """The (B, 1) per-sample values; `differentiable=False`: the forward kernel alone, nothing saved."""
        if pred.dim() != 5 or pred.shape[1] != 1 or pred.shape != gt.shape or (roi is not None and roi.shape != pred.shape):
            raise ValueError(f"GradientDifferenceLoss: (B, 1, D, H, W) volumes of equal shape expected, got {tuple(pred.shape)}, "
                             f"{tuple(gt.shape)}" + ("" if roi is None else f", {tuple(roi.shape)}"))
        if self.mask == "brain" and roi is None:
            raise ValueError("GradientDifferenceLoss: mask='brain' needs the ROI label volume")
        p = _vol_internal(pred)
        g = _vol_internal(gt.detach(), p.dtype).contiguous()
        r = _vol_internal(roi, torch.float32).contiguous() if self.mask == "brain" else None
        if differentiable:
            return ops.GradDiffLoss.apply(p, g, r, self.MODES[self.mode], self.alpha, self.axis_weights)
        return ops.grad_diff_values(p.detach(), g, r, self.MODES[self.mode], self.alpha, self.axis_weights).view(-1, 1)

    def forward(self, pred, gt, roi=None):
        loss = self.per_sample(pred, gt, roi)                      # (B, 1)
        if self.batch_reduction is None:
            return loss
        return torch.mean(loss) if self.batch_reduction == "mean" else torch.sum(loss)


class WithGradDiff(nn.Module):
    """A generative loss plus a gradient-difference term: base(pred, gt, roi) + grad_diff_weight * gdl_b
    (GradientDifferenceLoss(**kwargs)) -- per sample while `batch_reduction` is None, else reduced over the batch as the base
    is.  `batch_reduction` IS the base loss's, and so is everything else WithSSIM forwards; nests with WithSSIM and
    WithRoiMean in any order."""

    _BASE_ATTRS = WithSSIM._BASE_ATTRS
    _BASE_METHODS = WithSSIM._BASE_METHODS

    def __init__(self, base, grad_diff_weight, **kwargs):
        super().__init__()
        if not hasattr(base, "batch_reduction"):
            raise ValueError("WithGradDiff: base must be a generative loss with a batch_reduction attribute")
        w = float(grad_diff_weight)
        if not (w >= 0.0 and w != float("inf")):
            raise ValueError(f"WithGradDiff: grad_diff_weight must be a finite number >= 0, got {grad_diff_weight}")
        self.base = base
        self.grad_diff_weight = w
        self.grad_diff = GradientDifferenceLoss(**dict(kwargs, reduction=None))

    def __getattr__(self, name):
        if name in WithGradDiff._BASE_ATTRS or name in WithGradDiff._BASE_METHODS:
            return getattr(super().__getattr__("base"), name)
        return super().__getattr__(name)

    def __setattr__(self, name, value):
        if name in WithGradDiff._BASE_ATTRS:
            setattr(self.base, name, value)
        else:
            super().__setattr__(name, value)

    def forward(self, pred, gt, roi=None):
        loss = self.base(pred, gt, roi)
        g = self.grad_diff(pred, gt, roi)                          # (B, 1)
        red = self.batch_reduction
        return loss + self.grad_diff_weight * (g if red is None else torch.mean(g) if red == "mean" else torch.sum(g))


class LabelDifference(nn.Module):
    def __init__(self, distance_type="l1"):
        super().__init__()
        self.distance_type = distance_type

    def forward(self, labels):
        if self.distance_type != "l1":
            raise ValueError(self.distance_type)
        return torch.abs(labels[:, None, :] - labels[None, :, :]).sum(dim=-1)


class FeatureSimilarity(nn.Module):
    def __init__(self, similarity_type="l2"):
        super().__init__()
        self.similarity_type = similarity_type

    def forward(self, features):
        if self.similarity_type != "l2":
            raise ValueError(self.similarity_type)
        return -(features[:, None, :] - features[None, :, :]).norm(2, dim=-1)


class RnCLoss(nn.Module):
    """Rank-N-Contrast, criterions.py:607-644."""

    def __init__(self, temperature=2, label_diff="l1", feature_sim="l2"):
        super().__init__()
        self.t = temperature
        self.label_diff_fn = LabelDifference(label_diff)
        self.feature_sim_fn = FeatureSimilarity(feature_sim)

    def forward(self, features, labels):
        features = features.float()
        labels = labels.float()
        if len(features.shape) == 2 * len(labels.shape):
            features = torch.cat([features[:, 0], features[:, 1]], dim=0)
            labels = labels.repeat(2, 1)
        if features.shape[0] == 2:
            # n = 2 (the reference's batch size, run.sh:13): each row has ONE off-diagonal logit, which is its own only
            # "negative", so every log-probability is log(e^l / e^l) = 0 and the loss and its gradient are identically zero
            # (tests/golden/criterions_ref.npz rnc0 holds the reference's 0.0 and zero gradient for n = 2; n = 1 takes
            # the general path below, whose empty loop returns the python float 0.0 with NO gradient, as upstream).
            # Same value, same zero gradient into `features` (so the last projection head keeps receiving zeros and AdamW
            # keeps decaying it, as upstream) -- without the ~30 tiny launches of the general form.
            return (features * 0.0).sum()
        label_diffs = self.label_diff_fn(labels)
        logits = self.feature_sim_fn(features).div(self.t)
        logits_max, _ = torch.max(logits, dim=1, keepdim=True)
        logits = logits - logits_max.detach()
        exp_logits = logits.exp()
        n = logits.shape[0]
        # remove the diagonal with a static gather (masked_select would need a host sync)
        key = (n, logits.device)
        if getattr(self, "_offdiag_key", None) != key:
            cols = [[j for j in range(n) if j != i] for i in range(n)]
            self._offdiag = torch.tensor(cols, dtype=torch.long).reshape(n, max(n - 1, 0)).to(logits.device)
            self._offdiag_key = key
        idx = self._offdiag
        logits = torch.gather(logits, 1, idx)
        exp_logits = torch.gather(exp_logits, 1, idx)
        label_diffs = torch.gather(label_diffs, 1, idx)
        loss = 0.0
        for k in range(n - 1):
            pos_logits = logits[:, k]
            pos_label_diffs = label_diffs[:, k]
            neg_mask = (label_diffs >= pos_label_diffs.view(-1, 1)).float()
            pos_log_probs = pos_logits - torch.log((neg_mask * exp_logits).sum(dim=-1))
            loss = loss + -(pos_log_probs / (n * (n - 1))).sum()
        return loss


class _ZeroWeighted(torch.autograd.Function):
    """A loss term whose weight is exactly 0.0 (criterions.py:562 `regulatory_weight * triplet`, validation.py:154): value 0,
    gradient zeros -- what `0.0 * term` gives for any finite term -- without evaluating the term (TripletMarginLoss on
    (B,1,1,1,2048): ~35 tiny ATen launches forward + backward)."""

    @staticmethod
    def forward(ctx, x):
        ctx.meta = (x.shape, x.dtype, x.device)
        return torch.zeros((), dtype=torch.float32, device=x.device)

    @staticmethod
    def backward(ctx, g):
        shape, dtype, device = ctx.meta
        return torch.zeros(shape, dtype=dtype, device=device)


class GenerativeContrastiveLoss(nn.Module):
    """L = gen_weight * sum_b gen_b + reg_weight * pred_space + ds_reg_weight * ds  (criterions.py:544-575)."""

    def __init__(self, ds_contra_loss, gen_loss, pred_space_contra_loss, regulatory_weight, ds_regulatory_weight):
        super().__init__()
        self.ds_contra_loss = ds_contra_loss
        self.gen_loss = gen_loss
        self.pred_space_contra_loss = pred_space_contra_loss
        self.reg_weight = regulatory_weight
        self.ds_reg_weight = ds_regulatory_weight
        self.gen_weight = 1.0
        self.skip_zero_weighted = True      # False: always evaluate the 0.0-weighted term, as the reference does

    def get_pred_space_contra_loss(self, representations):
        return self.pred_space_contra_loss(*representations)

    def get_ds_contra_loss(self, intermediate_extractions):
        return self.ds_contra_loss(*intermediate_extractions)

    def forward(self, prediction, target, roi, final_representations, intermediate_extractions):
        gen_loss = self.gen_loss(prediction, target, roi)
        reduced_gen_loss = torch.sum(gen_loss) if self.gen_loss.batch_reduction is None else gen_loss
        if self.reg_weight == 0.0 and self.skip_zero_weighted:
            total_pred_space = _ZeroWeighted.apply(final_representations[0])      # == 0.0 * triplet(...) for any finite triplet
        else:
            pred_space = self.get_pred_space_contra_loss(tuple(r.float() for r in final_representations))
            total_pred_space = self.reg_weight * pred_space
        ds = self.get_ds_contra_loss(intermediate_extractions)
        total_ds = self.ds_reg_weight * ds
        total = self.gen_weight * reduced_gen_loss + total_pred_space + total_ds
        return total, gen_loss, total_pred_space, total_ds


GEN_LOSSES = {"roi_mse": lambda w: RoiMSE(w, ROI_INDICES, voxel_wise=False), "roi_rse": lambda w: RoiRSE(w, ROI_INDICES),
              "roi_rrmse": lambda w: RoiRRMSE(w, ROI_INDICES), "roi_wmse": lambda w: RoiWeightedMSE(w, ROI_INDICES)}


def build_reference_criterion(device="cuda", gen_loss="roi_mse", roi_mean_weight=None, grad_diff_weight=None):
    """validation.py:130-154 with ``-rnc`` + attn_unet_data_parallel.py:717.  `gen_loss`: "roi_mse" (the live driver line,
    validation.py:146) or one of the alternatives the reference keeps beside it (:132-133), "roi_rse" / "roi_rrmse", or
    "roi_wmse".  `roi_mean_weight` (None: as the reference): the generative loss wrapped in WithRoiMean with that weight;
    `grad_diff_weight` (None: as the reference): wrapped in WithGradDiff with that weight (the classic term: alpha 1, "abs")."""
    if gen_loss not in GEN_LOSSES:
        raise ValueError(f"build_reference_criterion: gen_loss must be one of {sorted(GEN_LOSSES)}, got {gen_loss!r}")
    w = torch.full((len(ROI_INDICES),), 225.0, device=device)
    crit = GenerativeContrastiveLoss(RnCLoss(), GEN_LOSSES[gen_loss](w),
                                     nn.TripletMarginLoss(1), regulatory_weight=0.0, ds_regulatory_weight=1.0)
    crit.gen_loss.batch_reduction = None
    if roi_mean_weight is not None:
        crit.gen_loss = WithRoiMean(crit.gen_loss, roi_mean_weight)
    if grad_diff_weight is not None:
        crit.gen_loss = WithGradDiff(crit.gen_loss, grad_diff_weight)
    return crit
