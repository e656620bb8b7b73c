"""What the gradient-difference loss tests rest on, checked without a GPU: the fp64 restatement of tests/_grad_diff_plan.py
against a hand-computed 2 x 2 x 3 example and against central finite differences, its autograd gradient against the gather
form the backward kernel evaluates, the tile mirror against the source, the C ABI's declarations and bindings, and the
constructor / wrapper behaviour of the Python classes (no kernel is called)."""
import os
import re

import pytest
import torch

import _grad_diff_plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (z, y, x); worked out by hand below
PRED = [[[0, 1, 3], [5, 2, 2]], [[1, 4, 4], [0, 3, 7]]]
GT = [[[0, 2, 3], [1, 2, 2]], [[2, 2, 2], [0, 1, 5]]]
# x pairs (gp | gg per row):  z0y0 (1, 2 | 2, 1)   z0y1 (-3, 0 | 1, 0)   z1y0 (3, 0 | 0, 0)   z1y1 (3, 4 | 1, 4)
#   abs    t: -1, 1,  2, 0, 3, 0, 2, 0   sum |t| =  9  sum t^2 = 19      signed t: -1, 1, -4, 0, 3, 0, 2, 0   sum |t| = 11  sum t^2 = 31
# y pairs (gp | gg per z):    z0 (5, 1, -1 | 1, 0, -1)   z1 (-1, -1, 3 | -2, -1, 3)
#   abs    t:  4, 1, 0, -1, 0, 0         sum |t| =  6  sum t^2 = 18      signed t:  4, 1, 0, 1, 0, 0          sum |t| =  6  sum t^2 = 18
# z pairs (gp | gg per y):    y0 (1, 3, 1 | 2, 0, -1)    y1 (-5, 1, 5 | -1, -1, 3)
#   abs    t: -1, 3, 0, 4, 0, 2          sum |t| = 10  sum t^2 = 30      signed t: -1, 3, 2, -4, 2, 2         sum |t| = 14  sum t^2 = 38
# N = (6, 6, 8) for (z, y, x)
HAND_S = {("abs", 1): (10, 6, 9), ("abs", 2): (30, 18, 19), ("signed", 1): (14, 6, 11), ("signed", 2): (38, 18, 31)}
HAND_LOSS = {("abs", 1): 91 / 24, ("abs", 2): 10.375, ("signed", 1): 113 / 24, ("signed", 2): 317 / 24}


def _hand():
    return torch.tensor([PRED], dtype=torch.float64), torch.tensor([GT], dtype=torch.float64)


@pytest.mark.parametrize("mode,alpha", P.CONFIGS)
def test_restatement_equals_the_hand_computed_example(mode, alpha):
    pred, gt = _hand()
    S, N = P.sums64(pred, gt, None, P.MODES[mode], alpha)
    assert S.tolist() == [[float(s) for s in HAND_S[(mode, alpha)]]] and N.tolist() == [[6.0, 6.0, 8.0]]
    assert abs(float(P.loss64(pred, gt, None, P.MODES[mode], alpha)) - HAND_LOSS[(mode, alpha)]) <= 1e-15 * 16
    # axis weights (2, 0, 4): 2 S_z / 6 + 4 S_x / 8
    sz, _, sx = HAND_S[(mode, alpha)]
    assert abs(float(P.loss64(pred, gt, None, P.MODES[mode], alpha, (2.0, 0.0, 4.0))) - (sz / 3 + sx / 2)) <= 1e-15 * 16
    # the (5 | 1) voxel at (z0, y1, x0) masked out: its x pair (t 2 | -4), y pair (t 4) and z pair (t 4 | -4) leave
    roi = torch.ones(1, 2, 2, 3)
    roi[0, 0, 1, 0] = 0.0
    S, N = P.sums64(pred, gt, roi, P.MODES[mode], alpha)
    tx = {"abs": 2, "signed": 4}[mode]
    want = [sz - 4 ** alpha, HAND_S[(mode, alpha)][1] - 4 ** alpha, sx - tx ** alpha]
    assert S.tolist() == [[float(s) for s in want]] and N.tolist() == [[5.0, 5.0, 7.0]]
    if (mode, alpha) == ("abs", 1):
        assert abs(float(P.loss64(pred, gt, roi, P.ABS, 1)) - 2.6) <= 1e-15
    # an axis of length 1, or without a counted pair: 0, not NaN
    flat = P.loss64(pred[:, :1], gt[:, :1], None, P.MODES[mode], alpha)
    assert bool(torch.isfinite(flat).all()) and float(P.sums64(pred[:, :1], gt[:, :1], None, P.MODES[mode], alpha)[1][0, 0]) == 0.0
    assert float(P.loss64(pred, gt, torch.zeros(1, 2, 2, 3), P.MODES[mode], alpha)) == 0.0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode,alpha", P.CONFIGS)
def test_restatement_gradient_equals_finite_differences_and_the_gather_form(mode, alpha, masked):
    g = torch.Generator().manual_seed(5)
    B, dims = 2, (3, 4, 5)
    pred, gt = 4.0 * torch.rand((B, *dims), generator=g, dtype=torch.float64), 4.0 * torch.rand((B, *dims), generator=g, dtype=torch.float64)
    roi = (torch.rand((B, *dims), generator=g) > 0.25).float() * 17.0 if masked else None
    m, aw = P.MODES[mode], (0.5, 2.0, 1.25)
    gout = torch.tensor([1.0, -2.0], dtype=torch.float64)
    for d in (1, 2, 3):                                                    # away from ties: no kink within the step
        gp, t, _ = P.axis_maps(pred, gt, None, m, d)
        assert float(t.abs().min()) > 1e-4 and float(gp.abs().min()) > 1e-4
    loss, coef, grad = P.loss_coef_grad64(pred, gt, roi, m, alpha, aw, gout)
    closed, amp, near = P.closed_grad_amp64(pred, gt, roi, m, alpha, aw, gout)
    assert float((closed - grad).abs().max()) <= 1e-14 * float(amp.max()) and not bool(near.any())
    assert bool((amp >= grad.abs() - 1e-15).all())
    eps, f = 1e-6, lambda x: float((P.loss64(x, gt, roi, m, alpha, aw) * gout).sum())
    flat = pred.reshape(-1)
    for i in range(0, flat.numel(), 7):
        hi, lo = flat.clone(), flat.clone()
        hi[i] += eps
        lo[i] -= eps
        fd = (f(hi.reshape(pred.shape)) - f(lo.reshape(pred.shape))) / (2 * eps)
        assert abs(fd - float(grad.reshape(-1)[i])) <= 1e-8 * max(1.0, float(amp.reshape(-1)[i])), (i, fd, float(grad.reshape(-1)[i]))
    if masked:                                                             # a voxel outside the mask gets no gradient
        assert float(grad[roi == 0].abs().max()) == 0.0 and float(grad.abs().max()) > 0


def test_ties_have_zero_subgradient():
    """sign(0) = 0: pred = gt gives gradient 0 under every configuration; gp = 0 contributes nothing under "abs", alpha 1."""
    pred, gt, _ = P.exact_inputs("tiny")
    gout = torch.ones(1, dtype=torch.float64)
    for mode, alpha in P.CONFIGS:
        _, _, grad = P.loss_coef_grad64(gt, gt, None, P.MODES[mode], alpha, (1.0, 1.0, 1.0), gout)
        assert float(grad.abs().max()) == 0.0
        closed, _, near = P.closed_grad_amp64(pred, gt, None, P.MODES[mode], alpha, (1.0, 1.0, 1.0), gout)
        _, _, grad = P.loss_coef_grad64(pred, gt, None, P.MODES[mode], alpha, (1.0, 1.0, 1.0), gout)
        assert float((closed - grad).abs().max()) <= 1e-15 and bool(near.any())            # the planted ties are there


def _decl_args(hdr, name):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
    assert m, name
    return [a for a in m.group(1).split(",") if a.strip()]


def test_symbols_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "coma_unet.h")).read()
    from coma_unet_amd import _lib
    for name, nargs in (("coma_grad_diff_ws_bytes", 1), ("coma_grad_diff_fwd", 11), ("coma_grad_diff_bwd", 9)):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
        assert len(_decl_args(hdr, name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.lib.coma_abi_version() == 3
    with open(os.path.join(ROOT, "coma_unet_amd", "build.py")) as f:
        assert '"grad_diff.hip"' in f.read()


def test_mirror_constants_are_the_sources():
    with open(os.path.join(ROOT, "coma_unet_amd", "csrc", "grad_diff.hip")) as f:
        src = f.read()
    for needle in (f"GD_TZ = {P.GD_TZ}", "GD_TY = COMA_SMOOTH_TILE_Y", "GD_TX = COMA_SMOOTH_TILE_X", f"GD_REC = {P.GD_REC}",
                   "GD_TX == 32 && GD_TY == 8", "i += 64", "t->ld == 1 && t->W % n == 0 && t->sb % n == 0",
                   "(size_t)gd_ntiles(pred, nullptr, nullptr) * GD_REC * sizeof(double)"):
        assert needle in src, needle
    for banned in ("atomicAdd", "atomic_", "atomicMin", "atomicMax", "atomicCAS"):
        assert banned not in src, banned
    assert P.tiles(P.case("multi")[1]) == 75 > P.FIN_LANES and P.tiles(P.case("tiny")[1]) == 1 and P.tiles(P.case("edges")[1]) == 8
    assert P.ws_bytes(2, (40, 40, 72)) == 2 * 75 * 48
    assert P.vec_ok(1, 40 * 40 * 72, 72, 0, 4) and P.vec_ok(1, 40 * 40 * 72, 72, 0, 2) and not P.vec_ok(1, 40 * 40 * 72, 72, 1, 4)
    assert not P.vec_ok(1, 9 * 10 * 37, 37, 0, 4) and not P.vec_ok(4, 4 * 320, 40, 0, 4) and P.vec_ok(1, 320, 40, 0, 2)
    assert P.loss_bound(2 * 40 * 40 * 72) <= 1.001 * P.U_F32                 # "a few fp32 ulp": one cast


def test_exact_inputs_are_exact():
    for name, _, _ in P.CASES:
        pred, gt, lab = P.exact_inputs(name, "brain")
        for t in (pred, gt):
            assert bool((t * 64 == (t * 64).round()).all()) and float(t.min()) >= 0 and float(t.max()) < 4
            assert torch.equal(t.bfloat16().float(), t)
        assert bool((lab == 0).any()) and bool((lab != 0).any())
    pred, gt, lab = P.random_inputs("multi", "brain")
    assert float(pred.max()) < 4.0 and float(lab[1].abs().max()) == 0.0 and float(lab[0].abs().max()) > 0


def test_module_argument_guards():
    import coma_unet_amd as cu
    G = cu.GradientDifferenceLoss
    for kw in (dict(alpha=3), dict(alpha=0), dict(alpha=1.5), dict(alpha=True), dict(mode="l2"), dict(mask="roi"), dict(reduction="max"),
               dict(axis_weights=(1, 1)), dict(axis_weights=(1, -1, 1)), dict(axis_weights=(1, float("inf"), 1)),
               dict(axis_weights=(1, float("nan"), 1)), dict(axis_weights=2.0)):
        with pytest.raises(ValueError, match="GradientDifferenceLoss"):
            G(**kw)
    m = G(alpha=2, mode="signed", axis_weights=(1, 2, 3), mask="brain", reduction=None)
    assert (m.alpha, m.mode, m.axis_weights, m.mask, m.batch_reduction) == (2, "signed", (1.0, 2.0, 3.0), "brain", None)
    m.batch_reduction = "sum"
    assert m.reduction == "sum"
    m.reduction = "mean"
    assert m.batch_reduction == "mean" and "GradientDifferenceLoss" in str(m)
    x = torch.zeros(2, 1, 4, 4, 4)
    with pytest.raises(ValueError, match="brain"):
        m(x, x)                                                             # mask="brain" without roi
    for bad in ((torch.zeros(2, 2, 4, 4, 4),) * 2, (torch.zeros(2, 4, 4, 4),) * 2, (x, torch.zeros(2, 1, 4, 4, 5)),
                (x, x, torch.zeros(2, 1, 4, 4, 5))):
        with pytest.raises(ValueError, match="B, 1, D, H, W"):
            m(*bad)
    with pytest.raises(ValueError, match="B, 1, D, H, W"):
        G()(x, torch.zeros(2, 1, 4, 5, 4))
    from coma_unet_amd import metrics
    with pytest.raises(ValueError, match="GradientDifferenceLoss"):
        metrics.gradient_difference(x, x, alpha=5)
    with pytest.raises(ValueError, match="brain"):
        metrics.gradient_difference(x, x, mask="brain")


class _Stub(torch.nn.Module):
    """a base loss as the training loop sees one"""

    def __init__(self):
        super().__init__()
        self.batch_reduction = None
        self.roi_indices, self.roi_weights = [17, 18], torch.tensor([1.0, 2.0])
        self.voxel_wise, self.voxel_weights, self.scale_factor = False, None, 360
        self.calls = []

    def calculate_new_weights(self, errors, with_update=False):
        self.calls.append(("w", with_update))
        return errors

    def calculate_new_voxel_weights(self, errors, voxel_weights, with_update=False):
        self.calls.append(("v", with_update))
        return voxel_weights

    def update_weights(self, weights):
        self.calls.append(("u", None))


def test_wrapper_guards_and_attribute_forwarding():
    import coma_unet_amd as cu
    base = _Stub()
    for w in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="WithGradDiff"):
            cu.WithGradDiff(base, w)
    with pytest.raises(ValueError, match="WithGradDiff"):
        cu.WithGradDiff(torch.nn.MSELoss(), 1.0)
    with pytest.raises(ValueError, match="GradientDifferenceLoss"):
        cu.WithGradDiff(base, 1.0, alpha=7)
    top = cu.WithGradDiff(base, 0.25, alpha=2, mode="signed", mask="brain", axis_weights=(1, 2, 3), reduction="mean")
    assert top.grad_diff_weight == 0.25 and top.grad_diff.batch_reduction is None          # the term is always per sample inside
    assert (top.grad_diff.alpha, top.grad_diff.mode, top.grad_diff.mask) == (2, "signed", "brain")
    assert cu.WithGradDiff._BASE_ATTRS == cu.WithSSIM._BASE_ATTRS and cu.WithGradDiff._BASE_METHODS == cu.WithSSIM._BASE_METHODS
    for name in cu.WithSSIM._BASE_ATTRS:
        assert getattr(top, name) is getattr(base, name), name
    top.batch_reduction = "mean"
    assert base.batch_reduction == "mean" and "batch_reduction" not in top.__dict__
    w2 = torch.tensor([3.0, 4.0])
    top.roi_weights = w2
    assert base.roi_weights is w2
    top.calculate_new_weights(w2, with_update=True)
    top.calculate_new_voxel_weights(w2, w2)
    top.update_weights(w2)
    assert base.calls == [("w", True), ("v", False), ("u", None)]
    with pytest.raises(AttributeError):
        top.no_such_attribute


@pytest.mark.parametrize("order", ["gs", "sg", "gm", "mg", "gsm", "smg", "msg"])
def test_wrappers_nest_in_any_order(order):
    """g: WithGradDiff, s: WithSSIM, m: WithRoiMean, listed from the outside in, around one stub base"""
    import coma_unet_amd as cu
    base = _Stub()
    top = base
    for c in reversed(order):
        top = (cu.WithGradDiff(top, 0.5) if c == "g" else cu.WithSSIM(top, 0.3, win_size=5) if c == "s"
               else cu.WithRoiMean(top, 0.7, kind="l1"))
    assert top.batch_reduction is None and top.roi_indices is base.roi_indices and top.roi_weights is base.roi_weights
    top.batch_reduction = "mean"
    assert base.batch_reduction == "mean"
    g = top
    while g is not base:
        assert g.batch_reduction == "mean" and g.scale_factor == 360
        g = g.base
    top.calculate_new_weights(torch.ones(2), with_update=True)
    assert base.calls == [("w", True)]


def test_train_dp_helper_wraps_once_and_leaves_none_alone():
    import coma_unet_amd as cu
    from coma_unet_amd.train_loop import with_grad_diff, with_roi_mean, with_ssim

    class Crit:
        pass

    c = Crit()
    c.gen_loss = base = _Stub()
    assert with_grad_diff(c) is c and with_grad_diff(c, None, dict(alpha=2)) is c and c.gen_loss is base       # None: untouched
    with_grad_diff(c, 0.5, dict(alpha=2, mask="brain"))
    g = c.gen_loss
    assert type(g) is cu.WithGradDiff and g.base is base and g.grad_diff_weight == 0.5 and g.grad_diff.alpha == 2
    with_grad_diff(c, 0.75)                                                 # a second call only takes the new weight
    assert c.gen_loss is g and g.grad_diff_weight == 0.75 and g.grad_diff.alpha == 2
    # train_dp's order: grad diff, roi mean, ssim; then again, and once more with only the grad-diff weight changed
    c.gen_loss = base
    for w in (0.5, 0.6):
        with_grad_diff(c, w)
        with_roi_mean(c, 0.7)
        with_ssim(c, 0.3, dict(win_size=5))
        top = c.gen_loss
        assert type(top) is cu.WithSSIM and type(top.base) is cu.WithRoiMean and type(top.base.base) is cu.WithGradDiff
        assert top.base.base.base is base and top.base.base.grad_diff_weight == w
    # the term added LATER than the others goes below them
    c.gen_loss = base
    with_roi_mean(c, 0.7)
    with_ssim(c, 0.3, dict(win_size=5))
    with_grad_diff(c, 0.2)
    top = c.gen_loss
    assert type(top) is cu.WithSSIM and type(top.base) is cu.WithRoiMean and type(top.base.base) is cu.WithGradDiff
    assert top.base.base.base is base
    import inspect
    from coma_unet_amd import train_loop
    assert "grad_diff_weight" in train_loop.train_dp.__doc__ and "grad_diff_weight" in inspect.getsource(train_loop.train_dp)


def test_build_reference_criterion_takes_the_option():
    import coma_unet_amd as cu
    c0 = cu.build_reference_criterion("cpu")
    assert type(c0.gen_loss) is cu.RoiMSE
    assert type(cu.build_reference_criterion("cpu", grad_diff_weight=None).gen_loss) is cu.RoiMSE
    c1 = cu.build_reference_criterion("cpu", grad_diff_weight=0.1)
    assert type(c1.gen_loss) is cu.WithGradDiff and type(c1.gen_loss.base) is cu.RoiMSE and c1.gen_loss.grad_diff_weight == 0.1
    assert c1.gen_loss.batch_reduction is None and (c1.gen_loss.grad_diff.alpha, c1.gen_loss.grad_diff.mode) == (1, "abs")
    c2 = cu.build_reference_criterion("cpu", roi_mean_weight=2.0, grad_diff_weight=0.1)
    assert type(c2.gen_loss) is cu.WithGradDiff and type(c2.gen_loss.base) is cu.WithRoiMean
