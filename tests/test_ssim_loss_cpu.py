"""SSIM loss without a GPU: the gradient formulas the kernels implement (restated in fp64 against autograd), the WithSSIM
wrapper's delegation, argument validation and train_dp's opt-in wrapping."""
import pytest
import torch
import torch.nn as nn

import _ssim_loss_plan as sp


@pytest.mark.parametrize("kind", sp.KINDS)
@pytest.mark.parametrize("case", sp.CASES + [sp.ASYM_CASE], ids=sp.case_id)
def test_restated_gradient_equals_fp64_autograd(case, kind):
    """Pins the formulas of DESIGN.md section 4 "SSIM loss": measured 1e-14, bound 1e-10."""
    shape, wkind, win = case
    x, y = sp.make_inputs(shape, kind, seed=3)
    w1, g = sp.window(wkind, win), sp.make_gout(shape[0])
    ssim, dx = sp.ssim_and_grad(x, y, w1, sp.C1, sp.C2, g)
    ssim_r, dx_r = sp.restated(x, y, w1, sp.C1, sp.C2, g, torch.float64)
    e = sp.rel_l2(dx_r, dx)
    print(f"{sp.case_id(case)} {kind}: restated-vs-autograd rel-L2 {e:.2e}")
    assert float(dx.norm()) > 0
    assert e <= 1e-10
    assert float((ssim_r - ssim).abs().max()) <= 1e-12


def test_reference_matches_the_metric_oracle():
    """ssim_and_grad differentiates the same SSIM the metric tests check against."""
    from oracle.metrics_oracle import ssim3d
    for (shape, wkind, win) in sp.CASES:
        x, y = sp.make_inputs(shape, "rand", seed=5)
        ssim, _ = sp.ssim_and_grad(x, y, sp.window(wkind, win), sp.C1, sp.C2, sp.make_gout(shape[0]))
        ref = ssim3d(x, y, kernel_type=wkind, win_size=win)
        assert float((ssim - ref).abs().max()) <= 1e-12


class _Base(nn.Module):
    """Stand-in generative loss with everything train_dp / record_results read from criterion.gen_loss."""

    def __init__(self):
        super().__init__()
        self.batch_reduction = "mean"
        self.roi_indices = [17, 18]
        self.roi_weights = torch.tensor([225.0, 225.0])
        self.voxel_wise = False
        self.voxel_weights = None
        self.scale_factor = 360
        self.calls = []

    def calculate_new_weights(self, errors, with_update=False):
        self.calls.append(("calculate_new_weights", with_update))
        return self.roi_weights * errors

    def calculate_new_voxel_weights(self, errors, voxel_weights, with_update=False):
        self.calls.append(("calculate_new_voxel_weights", with_update))
        return voxel_weights

    def update_weights(self, weights):
        self.calls.append(("update_weights",))


def test_with_ssim_delegates_to_the_base_loss():
    from coma_unet_amd import WithSSIM
    base = _Base()
    w = WithSSIM(base, 0.5, win_size=7, kernel_type="uniform")
    assert w.base is base and w.ssim_weight == 0.5 and w.ssim.win_size == 7 and w.ssim.batch_reduction is None
    for name in ("roi_indices", "roi_weights", "voxel_wise", "voxel_weights", "scale_factor"):
        assert getattr(w, name) is getattr(base, name), name
    new = torch.tensor([1.0, 2.0])
    w.roi_weights = new                                  # a write goes through to the base loss
    assert base.roi_weights is new and "roi_weights" not in w.__dict__
    out = w.calculate_new_weights(torch.tensor([2.0, 3.0]), with_update=True)
    assert torch.equal(out, torch.tensor([2.0, 6.0]))
    w.calculate_new_voxel_weights(None, new, with_update=False)
    w.update_weights(new)
    assert base.calls == [("calculate_new_weights", True), ("calculate_new_voxel_weights", False), ("update_weights",)]


def test_with_ssim_shares_batch_reduction_with_the_base():
    from coma_unet_amd import WithSSIM
    base = _Base()
    w = WithSSIM(base, 1.0)
    assert w.batch_reduction == "mean"
    w.batch_reduction = None                             # what train_dp does to criterion.gen_loss
    assert base.batch_reduction is None and w.batch_reduction is None
    base.batch_reduction = "mean"
    assert w.batch_reduction == "mean"
    assert "batch_reduction" not in w.__dict__


def test_ssim_loss_argument_validation():
    from coma_unet_amd import SSIMLoss
    with pytest.raises(ValueError):
        SSIMLoss(win_size=12)
    with pytest.raises(ValueError):
        SSIMLoss(win_size=0)
    with pytest.raises(ValueError):
        SSIMLoss(kernel_type="box")
    with pytest.raises(ValueError):
        SSIMLoss(reduction="sum")
    with pytest.raises(ValueError):
        SSIMLoss(data_range=0.0)
    loss = SSIMLoss(win_size=11)
    assert loss.batch_reduction == "mean" and loss.window.shape == (11,)
    small = torch.zeros(1, 1, 11, 10, 11)
    with pytest.raises(ValueError):                      # refused before anything touches the device
        loss(small, small)
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 2, 12, 12, 12), torch.zeros(1, 2, 12, 12, 12))
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 1, 12, 12, 12), torch.zeros(1, 1, 12, 12, 13))


def test_with_ssim_argument_validation():
    from coma_unet_amd import WithSSIM
    with pytest.raises(ValueError):
        WithSSIM(_Base(), -1.0)
    with pytest.raises(ValueError):
        WithSSIM(_Base(), float("nan"))
    with pytest.raises(ValueError):
        WithSSIM(_Base(), float("inf"))
    with pytest.raises(ValueError):
        WithSSIM(nn.MSELoss(), 1.0)                      # no batch_reduction: not a generative loss of this package
    with pytest.raises(ValueError):
        WithSSIM(_Base(), 1.0, win_size=13)
    w = WithSSIM(_Base(), 1.0, reduction="mean")         # the SSIM term's own reduction is the wrapper's business
    assert w.ssim.batch_reduction is None


def test_train_dp_wrapping_is_opt_in_and_happens_once():
    from coma_unet_amd import GenerativeContrastiveLoss, RnCLoss, WithSSIM
    from coma_unet_amd.train_loop import with_ssim
    base = _Base()
    crit = GenerativeContrastiveLoss(RnCLoss(), base, nn.TripletMarginLoss(1), 0.0, 1.0)
    assert with_ssim(crit, None, dict(win_size=7)) is crit and crit.gen_loss is base     # None: nothing touched
    with_ssim(crit, 0.25, dict(win_size=7))
    wrapped = crit.gen_loss
    assert isinstance(wrapped, WithSSIM) and wrapped.base is base and wrapped.ssim_weight == 0.25 and wrapped.ssim.win_size == 7
    with_ssim(crit, 0.5)                                 # a second call does not wrap the wrapper
    assert crit.gen_loss is wrapped and wrapped.base is base and wrapped.ssim_weight == 0.5
    crit.gen_loss.batch_reduction = None                 # train_dp's next line
    assert base.batch_reduction is None
