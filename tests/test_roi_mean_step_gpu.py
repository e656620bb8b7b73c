"""The ROI-mean term on the GPU at module level and inside the 32^3 x 2 training step: WithRoiMean against its two terms,
nested with WithSSIM in both orders, weight updates reaching the term, graph replay against eager steps, and
train_dp(roi_mean_weight=...)."""
import os

import numpy as np
import pytest
import torch

import _roi_mean_plan as P
from _roi_loss_plan import rel_l2

pytestmark = pytest.mark.gpu

S = (32, 32, 32)
LAMBDA = 50.0        # the regional differences of an untrained model are O(1) and the RoiMSE term O(100): keeps the term visible


def _gpu_batch(b):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}


def _volumes(B=2, seed=53):
    """(B, 1, D, H, W) pred / gt / roi on the GPU: make_batch's tau and labels, pred = tau + noise + a bias that depends on the
    label (0.05 .. 0.41 in seven steps: the regional differences differ, all of one sign and away from 0)"""
    from coma_unet_amd.synthetic import make_batch
    b = make_batch(B, S, seed=seed)
    g = torch.Generator().manual_seed(seed)
    pred = b["tau"] + 0.2 * torch.randn(b["tau"].shape, generator=g) + 0.05 + 0.06 * torch.remainder(b["roi"], 7.0)
    return pred.cuda(), b["tau"].cuda(), b["roi"].cuda()


def _table():
    from coma_unet_amd.roi_tables import ROI_INDICES
    return list(ROI_INDICES), torch.full((len(ROI_INDICES),), 225.0, device="cuda")


@pytest.mark.parametrize("kind", list(P.KINDS))
def test_module_matches_the_restatement(kind):
    import coma_unet_amd as cu
    ids, w = _table()
    pred0, gt, roi = _volumes()
    gout = {"mean": torch.full((2,), 0.5), "sum": torch.ones(2), None: torch.ones(2)}
    for red in ("mean", "sum", None):
        crit = cu.RoiMeanLoss(w, ids, kind=kind, delta=P.DELTA, reduction=red)
        pred = pred0.clone().requires_grad_(True)
        loss = crit(pred, gt, roi)
        lref, _, gref, _ = P.loss_coef_grad64(P.KINDS[kind], pred0.permute(0, 2, 3, 4, 1), gt.permute(0, 2, 3, 4, 1),
                                              roi.permute(0, 2, 3, 4, 1), ids, w.double(), gout[red].cuda())
        want = lref.reshape(2, 1) if red is None else (lref.mean() if red == "mean" else lref.sum())
        assert loss.shape == want.shape and loss.dtype == torch.float32
        assert float(((loss.detach().double() - want).abs() / want.abs()).max()) <= P.LOSS_REL
        loss.sum().backward()
        assert pred.grad.shape == pred.shape
        e = rel_l2(pred.grad, gref.permute(0, 4, 1, 2, 3))
        assert e <= 1e-6, (kind, red, e)


@pytest.mark.parametrize("red", [None, "mean", "sum"])
def test_with_roi_mean_equals_the_two_terms(red):
    import coma_unet_amd as cu
    ids, w = _table()
    pred0, gt, roi = _volumes()
    lam = 0.75
    both = cu.WithRoiMean(cu.RoiRRMSE(w, ids, reduction=red), lam, kind="huber", delta=P.DELTA)
    assert both.batch_reduction == red and both.base.reduction == red
    vals, grads = [], []
    for term in (both, cu.RoiRRMSE(w, ids, reduction=red), cu.RoiMeanLoss(w, ids, kind="huber", delta=P.DELTA, reduction=red)):
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


@pytest.mark.parametrize("order", ["mean_over_ssim", "ssim_over_mean"])
def test_nests_with_ssim(order):
    import coma_unet_amd as cu
    ids, w = _table()
    pred0, gt, roi = _volumes()
    lm, ls, kw = 0.6, 0.4, dict(win_size=5, data_range=2.0)
    base = cu.RoiMSE(w, ids, reduction=None)
    if order == "mean_over_ssim":
        top = cu.WithRoiMean(cu.WithSSIM(base, ls, **kw), lm, kind="l1")
    else:
        top = cu.WithSSIM(cu.WithRoiMean(base, lm, kind="l1"), ls, **kw)
    assert top.batch_reduction is None
    vals, grads = [], []
    for term in (top, cu.RoiMSE(w, ids, reduction=None), cu.RoiMeanLoss(w, ids, kind="l1", reduction=None), cu.SSIMLoss(reduction=None, **kw)):
        p = pred0.clone().requires_grad_(True)
        v = term(p, gt, roi)
        v.sum().backward()
        vals.append(v.detach().double())
        grads.append(p.grad.double())
    want_v, want_g = vals[1] + lm * vals[2] + ls * vals[3], grads[1] + lm * grads[2] + ls * grads[3]
    assert vals[0].shape == (2, 1) and float(((vals[0] - want_v).abs() / want_v.abs()).max()) <= 1e-6
    assert rel_l2(grads[0], want_g) <= 1e-6
    top.batch_reduction = "mean"
    assert base.batch_reduction == "mean"
    v = top(pred0, gt, roi)
    assert v.dim() == 0 and abs(float(v) - float(want_v.mean())) <= 1e-6 * abs(float(want_v.mean()))


def test_weight_updates_reach_the_term():
    """The term follows the base loss's LIVE tables: an in-place change (its _version) or a replaced weights tensor changes
    the next loss; explicit tables do not follow the base; an unchanged table is not rebuilt."""
    import coma_unet_amd as cu
    ids, w = _table()
    w = 1.0 + torch.arange(len(ids), device="cuda", dtype=torch.float32)
    pred, gt, roi = _volumes()
    p5, g5, r5 = (t.permute(0, 2, 3, 4, 1) for t in (pred, gt, roi))
    base = cu.RoiMSE(w, ids, reduction=None)
    lam = 1.0e4                                               # the term dominates the sum it is read back from
    live = cu.WithRoiMean(base, lam, kind="l1")
    own = cu.WithRoiMean(base, lam, kind="l1", roi_weights=w.clone(), roi_indices=ids)
    term = lambda m: (m(pred, gt, roi).double() - base(pred, gt, roi).double()).reshape(-1) / lam
    ref = lambda ww: P.loss64(P.L1, p5, g5, r5, ids, ww.double())
    ok = lambda got, want: float(((got - want).abs() / want.abs()).max()) <= 2e-6       # (read back from a sum of fp32 losses)
    l0 = ref(w)
    assert ok(term(live), l0) and ok(term(own), l0)
    tab = live.roi_mean._tab
    term(live)
    assert live.roi_mean._tab is tab                          # no rebuild, no copy inside the step
    w[:12] *= 40.0                                            # in place: _version moves
    l1 = ref(w)
    assert float(((l1 - l0).abs() / l0).min()) > 1e-3         # the update matters
    assert ok(term(live), l1) and live.roi_mean._tab is not tab
    assert ok(term(own), l0)                                  # its own tables: untouched
    w2 = torch.flip(w, (0,)).contiguous()
    live.roi_weights = w2                                     # replaced through the wrapper: lands on the base
    assert base.roi_weights is w2 and ok(term(live), ref(w2))


def _static_model(dtype, seed=4):
    import coma_unet_amd as cu
    torch.manual_seed(seed)
    gm = cu.build_model(volume_shape=S, static_prompts=True, compute_dtype=dtype).cuda()
    gm.set_save_attn(None)
    gm.train(True)
    return gm


def test_gradient_at_the_prediction_matches_the_two_terms():
    """fp32 32^3 x 2 model with build_reference_criterion(roi_mean_weight=LAMBDA): the generative loss is RoiMSE + LAMBDA *
    the restatement, and what the loss hands back to the model at its own prediction is the sum of the two gradients."""
    import coma_unet_amd as cu
    from coma_unet_amd.roi_tables import ROI_INDICES
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import forward_loss
    gm = _static_model(torch.float32, seed=9)
    b = make_batch(2, S, seed=43)
    gb = _gpu_batch(b)
    gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
    crit = cu.build_reference_criterion("cuda", roi_mean_weight=LAMBDA)
    assert type(crit.gen_loss) is cu.WithRoiMean and crit.gen_loss.batch_reduction is None
    losses, outs = forward_loss(gm, crit, gb)
    seen = []
    outs[0].register_hook(lambda gr: seen.append(gr.detach().clone()))
    losses[0].backward()
    assert len(seen) == 1 and losses[1].shape == (2, 1)
    pred = outs[0].detach()
    p = pred.clone().requires_grad_(True)
    base = cu.RoiMSE(crit.gen_loss.roi_weights, ROI_INDICES, reduction=None)(p, gb["tau"], gb["roi"])
    base.sum().backward()
    to5 = lambda t: t.permute(0, 2, 3, 4, 1)
    w64 = torch.full((len(ROI_INDICES),), 225.0, dtype=torch.float64, device="cuda")
    lref, _, gref, _ = P.loss_coef_grad64(P.MSE, to5(pred), to5(gb["tau"]), to5(gb["roi"]), ROI_INDICES, w64,
                                          torch.ones(2, dtype=torch.float64, device="cuda"))
    want = base.detach().double().reshape(-1) + LAMBDA * lref
    assert float(((losses[1].detach().double().reshape(-1) - want).abs() / want).max()) <= 2e-6
    gwant = p.grad.double() + LAMBDA * gref.permute(0, 4, 1, 2, 3)
    e = rel_l2(seen[0], gwant.reshape(seen[0].shape))
    share = float((LAMBDA * gref).norm() / gwant.norm())
    print(f"gen loss {losses[1].reshape(-1).tolist()} (term {(LAMBDA * lref).tolist()}); gradient rel-L2 {e:.3e}, term's share {share:.3f}")
    assert e <= 2e-6 and share > 0.05


def test_graph_replay_matches_eager_steps_with_roi_mean():
    """test_roi_losses_step_gpu.test_graph_replay_matches_eager_steps_with_roi_rrmse's pattern and bounds (2e-2 on the losses,
    the parameters' total movement within 10 %, lr 1e-5, bf16 model) over three changing batches."""
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
        crit = cu.build_reference_criterion("cuda", roi_mean_weight=LAMBDA)
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


def test_train_dp_with_roi_mean_weight(tmp_path, monkeypatch):
    import coma_unet_amd as cu
    from coma_unet_amd import attn_unet_data_parallel as A
    from coma_unet_amd.synthetic import make_batch

    def loader(n, seed0, triplet):
        out, lookup = [], {}
        for i in range(n):
            bt = make_batch(2, S, seed=seed0 + i)
            ab = torch.tensor([1.0, 0.0])
            cov = bt["covars"].clone()
            cov[:, 0, 0] = ab
            paths = [f"/data/xnat/adni/{seed0 + i:03d}-S-{j:04d}/PET_2020-01-0{j + 1}_FTP/analysis/rnu.nii" for j in range(2)]
            for j in range(2):
                lookup[f"{seed0 + i:03d}-S-{j:04d}/PET_2020-01-0{j + 1}_FTP"] = bt["roi_pred_dicts"][j]
            item = (bt["mri"], bt["tau"], bt["roi"], (ab, cov), paths)
            out.append((item, item, item) if triplet else item)
        return out, lookup

    train, lk1 = loader(2, 70, True)
    val, lk2 = loader(1, 90, False)
    torch.manual_seed(11)
    m = cu.build_model(volume_shape=S).cuda()
    m.set_save_attn(None)
    m.train(True)
    crit = cu.build_reference_criterion()
    base = crit.gen_loss
    calls = []
    orig = base.calculate_new_weights
    base.calculate_new_weights = lambda errors, with_update=False: (calls.append(with_update), orig(errors, with_update))[1]
    seen = []
    fwd = cu.RoiMeanLoss.forward
    monkeypatch.setattr(cu.RoiMeanLoss, "forward", lambda self, pred, gt, roi: (seen.append(pred.requires_grad), fwd(self, pred, gt, roi))[1])
    losses = A.train_dp(m, crit, train, val, 1, 1e-3, save_path=str(tmp_path), cuda_id=0, roi_vecs_dict={**lk1, **lk2},
                        graph=False, val_iter=1, roi_mean_weight=LAMBDA, roi_mean_kwargs=dict(kind="huber", delta=0.5))
    assert isinstance(crit.gen_loss, cu.WithRoiMean) and crit.gen_loss.base is base and crit.gen_loss.roi_mean.kind == "huber"
    assert crit.gen_loss.roi_mean_weight == LAMBDA and crit.gen_loss.roi_mean.delta == 0.5
    assert base.batch_reduction is None and crit.gen_loss.batch_reduction is None
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert seen == [True, True]                          # the term ran in both training steps, on a prediction that takes gradients
    assert calls == [True]                               # the per-ROI weight update reached the base loss
    raw = torch.load(os.path.join(str(tmp_path), "checkpoints", "checkpoint_latest_epoch.pth"), map_location="cpu",
                     weights_only=True)
    assert set(raw) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "scheduler_state_dict"}
    assert set(raw["model_state_dict"]) == set(m.state_dict())
