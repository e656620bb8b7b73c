"""The gradient-difference term on the GPU at module level and inside the 32^3 x 2 training step: the module under autograd
against the plan's restatement, WithGradDiff against its two terms, nested with WithSSIM / WithRoiMean, through
GenerativeContrastiveLoss at the model's own prediction, graph replay against eager steps, and the default step's kernel list
with the option off."""
import json
import os

import numpy as np
import pytest
import torch

import _grad_diff_plan as P
from _roi_loss_plan import rel_l2
from oracle import fp64_ref as R

pytestmark = pytest.mark.gpu

S = (32, 32, 32)
V = 32 ** 3
LAMBDA = 50.0        # the term of an untrained model is O(0.1 .. 1) and the RoiMSE term O(100): keeps the term visible
GOLD = os.path.join(os.path.dirname(__file__), "golden", "default_step_kernels_32.json")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _gpu_batch(b):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}


def _volumes(B=2, seed=53):
    """(B, 1, D, H, W) pred / gt / roi on the GPU: make_batch's tau and labels, pred = tau + noise"""
    from coma_unet_amd.synthetic import make_batch
    b = make_batch(B, S, seed=seed)
    g = torch.Generator().manual_seed(seed)
    pred = b["tau"] + 0.2 * torch.randn(b["tau"].shape, generator=g)
    return pred.cuda(), b["tau"].cuda(), b["roi"].cuda()


def _table():
    from coma_unet_amd.roi_tables import ROI_INDICES
    return list(ROI_INDICES), torch.full((len(ROI_INDICES),), 225.0, device="cuda")


to5 = lambda t: t.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("mode,alpha", P.CONFIGS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_module_matches_the_restatement(dt, mode, alpha):
    """every reduction, with and without the mask; the restatement sees the values the kernel sees (rounded to dt)"""
    import coma_unet_amd as cu
    pred32, gt32, roi = _volumes()
    pred0, gt0 = pred32.to(DT[dt]), gt32.to(DT[dt])
    aw = P.AXIS_W[(mode, alpha)]
    gouts = {"mean": torch.full((2,), 0.5), "sum": torch.ones(2), None: torch.ones(2)}
    assert bool((roi == 0).any()) and bool((roi != 0).any())
    for mask in (None, "brain"):
        r64 = to5(roi) if mask else None
        for red in ("mean", "sum", None):
            crit = cu.GradientDifferenceLoss(alpha=alpha, mode=mode, axis_weights=aw, mask=mask, reduction=red)
            pred = pred0.clone().requires_grad_(True)
            loss = crit(pred, gt0, roi)
            gout = gouts[red].double().cuda()
            lref, _, gref = P.loss_coef_grad64(to5(pred0), to5(gt0), r64, P.MODES[mode], alpha, aw, gout)
            _, amp, _ = P.closed_grad_amp64(to5(pred0), to5(gt0), r64, P.MODES[mode], alpha, aw, gout)
            want = lref.reshape(2, 1) if red is None else (lref.mean() if red == "mean" else lref.sum())
            assert loss.shape == want.shape and loss.dtype == torch.float32
            err = float(((loss.detach().double() - want).abs() / want.abs()).max())
            assert err <= P.loss_bound(V) + 3 * P.U_F32, (mask, red, err)       # (+ the fp32 reduction over two samples)
            loss.sum().backward()
            assert pred.grad.shape == pred.shape and pred.grad.dtype == DT[dt]
            got = to5(pred.grad)[..., 0]
            worst = R.check_elementwise(got, gref, P.grad_bound(gref, amp, DT[dt]), f"{dt} {mode}{alpha} {mask} {red}")
            assert float(gref.abs().max()) > 0
            if mask:
                assert float(got[to5(roi)[..., 0] == 0].abs().max()) == 0.0      # outside the brain: no gradient
            print(f"{dt} {mode}{alpha} mask {mask} {red}: loss rel err {err:.2e}, dpred rel-L2 {rel_l2(got, gref):.2e}, worst / bound {worst:.3f}")
    from coma_unet_amd import metrics
    vals = metrics.gradient_difference(pred0, gt0, roi, alpha=alpha, mode=mode, axis_weights=aw, mask="brain")
    crit = cu.GradientDifferenceLoss(alpha=alpha, mode=mode, axis_weights=aw, mask="brain", reduction=None)
    assert vals.shape == (2,) and not vals.requires_grad and torch.equal(vals, crit(pred0, gt0, roi).reshape(-1))


@pytest.mark.parametrize("red", [None, "mean"])
def test_with_grad_diff_equals_the_two_terms(red):
    import coma_unet_amd as cu
    ids, w = _table()
    pred0, gt, roi = _volumes()
    lam, kw = 0.75, dict(alpha=2, mode="signed", mask="brain")
    both = cu.WithGradDiff(cu.RoiMSE(w, ids, reduction=red), lam, **kw)
    assert both.batch_reduction == red
    vals, grads = [], []
    for term in (both, cu.RoiMSE(w, ids, reduction=red), cu.GradientDifferenceLoss(reduction=red, **kw)):
        p = pred0.clone().requires_grad_(True)
        v = term(p, gt, roi)
        v.sum().backward()
        vals.append(v.detach().double())
        grads.append(p.grad.double())
    assert vals[0].shape == ((2, 1) if red is None else ())
    want_v, want_g = vals[1] + lam * vals[2], grads[1] + lam * grads[2]
    assert float(((vals[0] - want_v).abs() / want_v.abs()).max()) <= 1e-6
    assert rel_l2(grads[0], want_g) <= 1e-6
    assert float(grads[2].abs().max()) > 0 and rel_l2(grads[0], grads[1]) > 1e-3          # the term really contributes


@pytest.mark.parametrize("order", ["gsm", "sgm", "msg"])
def test_nests_with_ssim_and_roi_mean(order):
    """g: WithGradDiff, s: WithSSIM, m: WithRoiMean, listed from the outside in around RoiMSE"""
    import coma_unet_amd as cu
    ids, w = _table()
    pred0, gt, roi = _volumes()
    lg, ls, lm = 30.0, 0.4, 0.6
    skw, gkw = dict(win_size=5, data_range=2.0), dict(alpha=1, mode="abs")
    base = cu.RoiMSE(w, ids, reduction=None)
    top = base
    for c in reversed(order):
        top = (cu.WithGradDiff(top, lg, **gkw) if c == "g" else cu.WithSSIM(top, ls, **skw) if c == "s" else cu.WithRoiMean(top, lm, kind="l1"))
    assert top.batch_reduction is None
    vals, grads = [], []
    for term in (top, cu.RoiMSE(w, ids, reduction=None), cu.GradientDifferenceLoss(reduction=None, **gkw), cu.SSIMLoss(reduction=None, **skw),
                 cu.RoiMeanLoss(w, ids, kind="l1", reduction=None)):
        p = pred0.clone().requires_grad_(True)
        v = term(p, gt, roi)
        v.sum().backward()
        vals.append(v.detach().double())
        grads.append(p.grad.double())
    want_v = vals[1] + lg * vals[2] + ls * vals[3] + lm * vals[4]
    want_g = grads[1] + lg * grads[2] + ls * grads[3] + lm * grads[4]
    assert vals[0].shape == (2, 1) and float(((vals[0] - want_v).abs() / want_v.abs()).max()) <= 1e-6
    assert rel_l2(grads[0], want_g) <= 1e-6 and float((lg * grads[2]).norm() / want_g.norm()) > 1e-2
    top.batch_reduction = "mean"
    assert base.batch_reduction == "mean"
    v = top(pred0, gt, roi)
    assert v.dim() == 0 and abs(float(v) - float(want_v.mean())) <= 1e-6 * abs(float(want_v.mean()))


def _static_model(dtype, seed=4):
    import coma_unet_amd as cu
    torch.manual_seed(seed)
    gm = cu.build_model(volume_shape=S, static_prompts=True, compute_dtype=dtype).cuda()
    gm.set_save_attn(None)
    gm.train(True)
    return gm


def test_through_the_criterion_at_the_models_prediction():
    """fp32 32^3 x 2 model with build_reference_criterion(grad_diff_weight=LAMBDA): through GenerativeContrastiveLoss the
    generative loss is RoiMSE + LAMBDA * the restatement, and what the loss hands back to the model at its own prediction (a
    channel slice of a pitched buffer) is the sum of the two gradients."""
    import coma_unet_amd as cu
    from coma_unet_amd.roi_tables import ROI_INDICES
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import forward_loss
    gm = _static_model(torch.float32, seed=9)
    b = make_batch(2, S, seed=43)
    gb = _gpu_batch(b)
    gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
    crit = cu.build_reference_criterion("cuda", grad_diff_weight=LAMBDA)
    assert type(crit) is cu.GenerativeContrastiveLoss and type(crit.gen_loss) is cu.WithGradDiff and crit.gen_loss.batch_reduction is None
    losses, outs = forward_loss(gm, crit, gb)
    seen = []
    outs[0].register_hook(lambda gr: seen.append(gr.detach().clone()))
    losses[0].backward()
    assert len(seen) == 1 and losses[1].shape == (2, 1)
    pred = outs[0].detach()
    p = pred.clone().requires_grad_(True)
    base = cu.RoiMSE(crit.gen_loss.roi_weights, ROI_INDICES, reduction=None)(p, gb["tau"], gb["roi"])
    base.sum().backward()
    one = torch.ones(2, dtype=torch.float64, device="cuda")
    lref, _, gref = P.loss_coef_grad64(to5(pred), to5(gb["tau"]), None, P.ABS, 1, (1.0, 1.0, 1.0), one)
    want = base.detach().double().reshape(-1) + LAMBDA * lref
    assert float(((losses[1].detach().double().reshape(-1) - want).abs() / want).max()) <= 2e-6
    gwant = p.grad.double() + LAMBDA * gref.unsqueeze(1)
    e = rel_l2(seen[0], gwant.reshape(seen[0].shape))
    share = float((LAMBDA * gref).norm() / gwant.norm())
    print(f"gen loss {losses[1].reshape(-1).tolist()} (term {(LAMBDA * lref).tolist()}); gradient rel-L2 {e:.3e}, term's share {share:.3f}")
    assert e <= 2e-6 and share > 0.05


def test_graph_replay_matches_eager_steps_with_grad_diff():
    """test_roi_mean_step_gpu.test_graph_replay_matches_eager_steps_with_roi_mean's pattern and bounds (2e-2 on the losses, the
    parameters' total movement within 10 %, lr 1e-5, bf16 model) over three changing batches, the term on."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer, GraphedTrainStep
    raw = [make_batch(2, S, seed=s) for s in (29, 30, 31)]
    traj, moved, sample = [], [], []
    for graphed in (False, True):
        gm = _static_model(torch.bfloat16)
        p0 = {n: p.detach().clone() for n, p in gm.named_parameters()}
        gbs = []
        for b in raw:
            gb = _gpu_batch(b)
            gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
            gbs.append(gb)
        opt = make_optimizer(gm, 1e-5)
        crit = cu.build_reference_criterion("cuda", grad_diff_weight=LAMBDA)
        crit.gen_loss.grad_diff.mask = "brain"
        if graphed:
            step = GraphedTrainStep(gm, crit, opt, gbs[0], warmup=2)           # 2 eager warm-up steps on the first batch inside
            run = lambda gb: step(gb)
        else:
            for _ in range(2):
                train_step(gm, crit, opt, gbs[0])
            run = lambda gb: train_step(gm, crit, opt, gb)
        ls = []
        for gb in gbs:
            losses, _ = run(gb)
            ls.append((float(losses[0]), losses[1].detach().float().reshape(-1).cpu().clone()))
        traj.append(ls)
        torch.cuda.synchronize()
        moved.append(sum(float((p.detach() - p0[n]).abs().sum()) for n, p in gm.named_parameters()))
        sample.append({n: p.detach().float().cpu().clone() for n, p in list(gm.named_parameters())[::17]})
    print("eager", [t for t, _ in traj[0]], "graph", [t for t, _ in traj[1]], "moved", moved)
    for (tg, gg), (te, ge) in zip(traj[1], traj[0]):
        assert np.isfinite(tg) and abs(tg - te) <= 2e-2 * abs(te)
        assert float((gg - ge).abs().max()) <= 2e-2 * float(ge.abs().max())
    assert len({round(float(g_[0]), 4) for _, g_ in traj[1]}) == 3              # the replays really saw three different batches
    assert moved[1] > 0 and abs(moved[1] - moved[0]) <= 0.1 * moved[0]
    for n, pe in sample[0].items():
        assert float((sample[1][n] - pe).abs().max()) <= 2 * 5 * 1e-5 * (3.17 + 1e-2 * float(pe.abs().max())) + 1e-7, n


def test_default_step_kernel_list_is_unchanged_with_the_option_off(monkeypatch):
    """grad_diff_weight=None: the criterion is not wrapped, no grad-diff kernel is called, and the bracketed launches of one
    default 32^3 step are tests/golden/default_step_kernels_32.json (recorded as test_frozen_bn_model_gpu.py does)."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import forward_loss
    from coma_unet_amd.train_loop import with_grad_diff
    calls = []
    orig = ops._grad_diff_fwd
    monkeypatch.setattr(ops, "_grad_diff_fwd", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    with open(GOLD) as f:
        want = json.load(f)
    torch.manual_seed(321)
    gm = cu.build_model(volume_shape=S).cuda()
    gm.set_save_attn(None)
    gm.train(True)
    gb = _gpu_batch(make_batch(2, S, seed=9))

    def records(crit):
        KT = ops.KernelTimer
        KT.enabled, KT.records = True, []
        try:
            gm.zero_grad(set_to_none=True)
            losses, _ = forward_loss(gm, crit, gb)
            losses[0].backward()
            torch.cuda.synchronize()
            return [[r[0], r[6]] for r in KT.records]
        finally:
            KT.enabled, KT.records = False, []
            ops.SidePrep.join()

    crit = with_grad_diff(cu.build_reference_criterion(grad_diff_weight=None), None)
    assert type(crit.gen_loss) is cu.RoiMSE
    got = records(crit)
    assert calls == [] and len(got) == len(want), (len(calls), len(got), len(want))
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    on = records(with_grad_diff(cu.build_reference_criterion(), LAMBDA))        # the option on: the term runs, the model's launches stay
    assert calls == [1] and on == want
