"""The ROI-weighted loss classes on the GPU: criterions.RoiRSE / RoiRRMSE against what the reference's own classes gave
(tests/golden/roi_losses_ref.npz), RoiWeightedMSE against the fp64 restatement, WithSSIM over a new loss, and RoiRRMSE
inside the 32^3 x 2 training step (eager and graph-replayed)."""
import os

import numpy as np
import pytest
import torch

import _roi_loss_plan as P

pytestmark = pytest.mark.gpu

S = (32, 32, 32)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_losses_ref.npz")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _gpu_batch(b):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}


def _classes():
    import coma_unet_amd as cu
    return {"rse": cu.RoiRSE, "rrmse": cu.RoiRRMSE, "wmse": cu.RoiWeightedMSE}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("B", P.GOLDEN_B)
@pytest.mark.parametrize("name", ["rse", "rrmse", "wmse"])
def test_module_classes_reproduce_the_reference(name, B, dt):
    """The golden inputs are exact in bf16, so the loss is held to 1e-6 in both dtypes; the bf16 gradient is rounded once on
    the way out: rel-L2 <= 2^-9 + 1e-6."""
    g = np.load(GOLD)
    dtype, kind = DT[dt], P.KINDS[name]
    ids = g["roi_ids"].tolist()
    w64 = torch.from_numpy(g["weights"])
    w = w64.float().cuda()
    pred64, gt64, roi64 = (torch.from_numpy(g[f"in{B}_{k}"]) for k in ("pred", "gt", "roi"))
    ref_loss = P.loss64(kind, pred64, gt64, roi64, ids, w64)                      # (B,), == the golden scalars to 1e-12 (CPU test)
    for red in ("mean", "sum", None):
        crit = _classes()[name](w, ids, reduction=red)
        pred = pred64.to(dtype).cuda().requires_grad_(True)
        assert torch.equal(pred.detach().double().cpu(), pred64)
        loss = crit(pred, gt64.to(dtype).cuda(), roi64.float().cuda())
        gout = torch.full((B,), 1.0 / B if red == "mean" else 1.0, dtype=torch.float64)
        if red is None:
            assert loss.shape == (B, 1) and loss.dtype == torch.float32
            got, want = loss.detach().double().cpu().reshape(-1), ref_loss
            loss.sum().backward()
        else:
            assert loss.dim() == 0
            got, want = loss.detach().double().cpu().reshape(1), (ref_loss.mean() if red == "mean" else ref_loss.sum()).reshape(1)
            if name != "wmse":
                want_gold = float(g[f"{name}{B}_{red}"])
                assert abs(float(got) - want_gold) <= 1e-6 * abs(want_gold), (red, float(got), want_gold)
            loss.backward()
        assert float(((got - want).abs() / want.abs()).max()) <= P.LOSS_REL, (red, got, want)
        if name != "wmse":
            gref = torch.from_numpy(g[f"{name}{B}_grad_{'mean' if red == 'mean' else 'sum'}"])
        else:
            gref = P.loss_coef_grad64(kind, pred64, gt64, roi64, ids, w64, gout)[2]
        assert pred.grad.shape == pred.shape and pred.grad.dtype == dtype
        e = P.rel_l2(pred.grad.cpu(), gref)
        print(f"{name} B={B} {dt} reduction={red}: loss {got.tolist()} gradient rel-L2 {e:.3e}")
        assert e <= P.GRAD_REL_L2[dtype], (red, e)


def test_background_weight_and_weight_updates():
    """RoiWeightedMSE(background_weight=...) reaches the kernels; new weights reach the device tables when the weights tensor
    is replaced or changed in place (its _version), and only then."""
    g = np.load(GOLD)
    import coma_unet_amd as cu
    ids, w64 = g["roi_ids"].tolist(), torch.from_numpy(g["weights"])
    pred64, gt64, roi64 = (torch.from_numpy(g[f"in2_{k}"]) for k in ("pred", "gt", "roi"))
    args = (pred64.float().cuda(), gt64.float().cuda(), roi64.float().cuda())
    w = w64.float().cuda()
    for bg in (0.0, 3.5):
        crit = cu.RoiWeightedMSE(w, ids, reduction=None, background_weight=bg)
        ref = P.loss64(P.WMSE, pred64, gt64, roi64, ids, w64, bg)
        assert float(((crit(*args).double().cpu().reshape(-1) - ref).abs() / ref).max()) <= P.LOSS_REL
    crit = cu.RoiRRMSE(w, ids, reduction=None)
    crit(*args)
    tab = crit._tab
    crit(*args)
    assert crit._tab is tab                                   # no rebuild, no copy inside the step
    w[5] = 11.0                                               # in place: _version moves
    w64b = w64.clone()
    w64b[5] = 11.0
    ref = P.loss64(P.RRMSE, pred64, gt64, roi64, ids, w64b)
    assert float(((crit(*args).double().cpu().reshape(-1) - ref).abs() / ref).max()) <= P.LOSS_REL
    assert crit._tab is not tab


def test_with_ssim_equals_the_two_terms():
    g = np.load(GOLD)
    import coma_unet_amd as cu
    ids, w = g["roi_ids"].tolist(), torch.from_numpy(g["weights"]).float().cuda()
    gt, roi = torch.from_numpy(g["in3_gt"]).float().cuda(), torch.from_numpy(g["in3_roi"]).float().cuda()
    lam, kw = 0.75, dict(win_size=5, data_range=4.0)
    for red in (None, "mean"):
        grads, vals = [], []
        both = cu.WithSSIM(cu.RoiRRMSE(w, ids, reduction=red), lam, **kw)
        assert both.batch_reduction == red and both.base.reduction == red
        for term in (both, cu.RoiRRMSE(w, ids, reduction=red), cu.SSIMLoss(reduction=red, **kw)):
            p = torch.from_numpy(g["in3_pred"]).float().cuda().requires_grad_(True)
            v = term(p, gt, roi)
            v.sum().backward()
            grads.append(p.grad.double())
            vals.append(v.detach().double())
        assert vals[0].shape == ((3, 1) if red is None else ())
        want_v, want_g = vals[1] + lam * vals[2], grads[1] + lam * grads[2]
        assert float(((vals[0] - want_v).abs() / want_v.abs()).max()) <= 1e-6
        assert P.rel_l2(grads[0], want_g) <= 1e-6


def _static_model(dtype, seed=4):
    import coma_unet_amd as cu
    torch.manual_seed(seed)
    gm = cu.build_model(volume_shape=S, static_prompts=True, compute_dtype=dtype).cuda()
    gm.set_save_attn(None)
    gm.train(True)
    return gm


def test_gradient_at_the_prediction_matches_the_restatement():
    """fp32 32^3 x 2 model with build_reference_criterion(gen_loss="roi_rrmse"): what the loss hands back to the model at its
    own prediction is the restatement's autograd there (the other loss terms do not touch the prediction)."""
    import coma_unet_amd as cu
    from coma_unet_amd.roi_tables import ROI_INDICES
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import forward_loss
    gm = _static_model(torch.float32, seed=9)
    b = make_batch(2, S, seed=43)
    gb = _gpu_batch(b)
    gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
    crit = cu.build_reference_criterion("cuda", gen_loss="roi_rrmse")
    assert type(crit.gen_loss) is cu.RoiRRMSE and crit.gen_loss.batch_reduction is None
    losses, outs = forward_loss(gm, crit, gb)
    seen = []
    outs[0].register_hook(lambda gr: seen.append(gr.detach().clone()))
    losses[0].backward()
    assert len(seen) == 1 and losses[1].shape == (2, 1)
    w64 = torch.full((len(ROI_INDICES),), 225.0, dtype=torch.float64, device="cuda")
    lref, _, gref, _ = P.loss_coef_grad64(P.RRMSE, outs[0].detach(), gb["tau"], gb["roi"], ROI_INDICES, w64,
                                          torch.ones(2, dtype=torch.float64, device="cuda"))
    assert float(((losses[1].detach().double().reshape(-1) - lref).abs() / lref).max()) <= P.LOSS_REL
    e = P.rel_l2(seen[0], gref.reshape(seen[0].shape))
    print(f"gen loss {losses[1].reshape(-1).tolist()}; gradient at the prediction rel-L2 {e:.3e}")
    assert e <= P.GRAD_REL_L2[torch.float32]


def test_graph_replay_matches_eager_steps_with_roi_rrmse():
    """Bounds of test_model_gpu.test_graphed_step_matches_eager_steps (2e-2 on the losses, the parameters' total movement
    within 10 %, lr 1e-5, bf16 model), over three changing batches as test_ssim_loss_step_gpu does."""
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
        crit = cu.build_reference_criterion("cuda", gen_loss="roi_rrmse")
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
    # a parameter sample: both runs took 5 steps from the same start, and one Adam step moves a parameter by at most
    # lr (1 - beta1) / sqrt(1 - beta2) = 3.17 lr (Kingma & Ba, section 2.1) plus the decoupled decay lr wd |p|
    for n, pe in sample[0].items():
        assert float((sample[1][n] - pe).abs().max()) <= 2 * 5 * 1e-5 * (3.17 + 1e-2 * float(pe.abs().max())) + 1e-7, n
