"""The SSIM term inside the training step (32^3 x 2 model): one step against the CPU oracle plus lambda * (1 - oracle ssim3d)
by autograd, graph replay against eager steps, the bf16 step, and train_dp(ssim_weight=...)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

S = (32, 32, 32)
# At lambda = 1 the SSIM term's gradient w.r.t. the prediction has 0.012 of the norm of the RoiMSE term's on the oracle side
# (model seed 311, batch seed 37; computed on the CPU): lambda = 20 puts it at ~0.24, so that a broken SSIM backward cannot
# hide under the MSE gradient.  The test asserts the ratio.
LAMBDA = 20.0


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    n = b.norm()
    return float((a - b).norm() / n) if n > 0 else float((a - b).norm())


def _gpu_batch(b):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}


def _criterion(lam=LAMBDA):
    import coma_unet_amd as cu
    from coma_unet_amd.roi_tables import ROI_INDICES
    w = torch.full((len(ROI_INDICES),), 225.0, device="cuda")
    crit = cu.GenerativeContrastiveLoss(cu.RnCLoss(), cu.WithSSIM(cu.RoiMSE(w, ROI_INDICES, voxel_wise=False), lam),
                                        nn.TripletMarginLoss(1), regulatory_weight=0.0, ds_regulatory_weight=1.0)
    crit.gen_loss.batch_reduction = None
    return crit


def _oracle_total(model, b, lam, dt):
    """Oracle model + oracle criterion + lam * sum_b (1 - oracle ssim3d), everything differentiable by autograd."""
    from oracle.criterions_oracle import build_reference_criterion, train_step_loss
    from oracle.metrics_oracle import ssim3d
    res = model(b["mri"].to(dt), b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"].to(dt))
    losses = train_step_loss(res, b["tau"].to(dt), b["roi"].to(dt), b["covars"], build_reference_criterion())
    ssim_term = 1 - ssim3d(res[0], b["tau"])                         # (B,) fp64
    gen = losses[1].reshape(-1).double() + lam * ssim_term
    return losses[0] + lam * ssim_term.sum().to(losses[0].dtype), gen, res, ssim_term


def test_one_step_vs_oracle_with_ssim_term():
    """The comparisons and bounds of test_model_gpu.test_c1_forward_loss_backward_vs_oracle_and_golden, fp32, with the oracle
    (not the golden file, which has no SSIM term) as the reference for the loss values as well."""
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import forward_loss
    from oracle.coma_oracle import build_reference_model
    from oracle.criterions_oracle import build_reference_criterion
    from oracle.metrics_oracle import ssim3d
    torch.manual_seed(311)
    om = build_reference_model(volume_shape=S)
    om.set_save_attn(None)
    om.train(True)
    gm = cu.build_model(volume_shape=S).cuda()
    gm.load_state_dict(om.state_dict(), strict=True)
    gm.set_save_attn(None)
    gm.train(True)
    b = make_batch(2, S, seed=37)
    losses, outs = forward_loss(gm, _criterion(), _gpu_batch(b))
    losses[0].backward()
    # fp64 oracle
    o64 = copy.deepcopy(om).double()
    tot64, gen64, res64, ssim64 = _oracle_total(o64, b, LAMBDA, torch.float64)
    tot64.backward()
    # lambda is large enough for the SSIM gradient to matter (on the oracle side, w.r.t. the prediction)
    p = res64[0].detach().requires_grad_(True)
    g_mse = torch.autograd.grad(build_reference_criterion().gen_loss(p, b["tau"].double(), b["roi"].double()).sum(), p)[0]
    g_ssim = torch.autograd.grad(LAMBDA * (1 - ssim3d(p, b["tau"])).sum(), p)[0]
    ratio = float(g_ssim.norm() / g_mse.norm())
    print(f"|d ssim term / d pred| / |d RoiMSE / d pred| = {ratio:.3f} at lambda = {LAMBDA}")
    assert ratio >= 0.1
    assert rel(outs[0], res64[0]) < 1e-4
    assert rel(outs[1][-1], res64[1][-1]) < 1e-3
    assert abs(float(losses[0].detach()) - float(tot64.detach())) / float(tot64.detach()) < 1e-4
    assert losses[1].shape == (2, 1) and rel(losses[1].reshape(-1), gen64) < 1e-4
    # the fp32 CPU oracle's own distance from fp64 is the yardstick for the gradients
    tot32 = _oracle_total(om, b, LAMBDA, torch.float32)[0]
    tot32.backward()
    o32g, og = dict(om.named_parameters()), dict(o64.named_parameters())
    worst = worst_cpu = 0.0
    for n, prm in gm.named_parameters():
        r = og[n].grad
        assert (prm.grad is None) == (r is None), n
        if r is None or float(r.norm()) < 1e-4 * max(1.0, float(og[n].norm())):
            continue
        e, e_cpu = rel(prm.grad, r), rel(o32g[n].grad, r)
        worst, worst_cpu = max(worst, e), max(worst_cpu, e_cpu)
        assert e < max(3e-2, 4.0 * e_cpu), (n, e, e_cpu)
    print(f"worst relative gradient error vs fp64 oracle: HIP fp32 {worst:.2e}, CPU fp32 oracle {worst_cpu:.2e}")


def _static_model(dtype, seed=4):
    import coma_unet_amd as cu
    torch.manual_seed(seed)
    gm = cu.build_model(volume_shape=S, static_prompts=True, compute_dtype=dtype).cuda()
    gm.set_save_attn(None)
    gm.train(True)
    return gm


def test_graph_replay_matches_eager_steps_on_changing_batches():
    """Bound of test_model_gpu.test_graphed_step_matches_eager_steps (2e-2 on the loss, lr 1e-5, bf16 model)."""
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer, GraphedTrainStep
    raw = [make_batch(2, S, seed=s) for s in (29, 30, 31)]
    traj = []
    for graphed in (False, True):
        gm = _static_model(torch.bfloat16)
        gbs = []
        for b in raw:
            gb = _gpu_batch(b)
            gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
            gbs.append(gb)
        opt = make_optimizer(gm, 1e-5)
        crit = _criterion()
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
    print("eager", [t for t, _ in traj[0]], "graph", [t for t, _ in traj[1]])
    for (tg, gg), (te, ge) in zip(traj[1], traj[0]):
        assert np.isfinite(tg) and abs(tg - te) <= 2e-2 * abs(te)
        assert float((gg - ge).abs().max()) <= 2e-2 * float(ge.abs().max())
    assert len({round(t, 3) for t, _ in traj[1]}) == 3                         # the replays really saw three different batches


def test_bf16_step_runs_and_its_ssim_term_is_close_to_fp32():
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.train import train_step, make_optimizer
    b = make_batch(2, S, seed=41)
    terms = {}
    for dtype in (torch.float32, torch.bfloat16):
        gm = _static_model(dtype, seed=6)
        gb = _gpu_batch(b)
        gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
        crit = _criterion()
        losses, outs = train_step(gm, crit, make_optimizer(gm, 1e-5), gb)
        with torch.no_grad():
            term = crit.gen_loss.ssim(outs[0].detach(), gb["tau"]).reshape(-1).double().cpu()
        assert bool(torch.isfinite(losses[0])) and bool(torch.isfinite(losses[1]).all())
        terms[dtype] = term
    d = float((terms[torch.bfloat16] - terms[torch.float32]).abs().max())
    print(f"1 - ssim_b: fp32 {terms[torch.float32].tolist()}, bf16 {terms[torch.bfloat16].tolist()}, max difference {d:.2e}")
    assert d <= 1e-2


def test_train_dp_with_ssim_weight(tmp_path, monkeypatch):
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
    fwd = cu.SSIMLoss.forward
    monkeypatch.setattr(cu.SSIMLoss, "forward", lambda self, pred, gt, roi=None: (seen.append(pred.requires_grad), fwd(self, pred, gt, roi))[1])
    losses = A.train_dp(m, crit, train, val, 1, 1e-3, save_path=str(tmp_path), cuda_id=0, roi_vecs_dict={**lk1, **lk2},
                        graph=False, val_iter=1, ssim_weight=LAMBDA, ssim_kwargs=dict(win_size=7, kernel_type="uniform"))
    assert isinstance(crit.gen_loss, cu.WithSSIM) and crit.gen_loss.base is base and crit.gen_loss.ssim.win_size == 7
    assert base.batch_reduction is None and crit.gen_loss.batch_reduction is None
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert seen == [True, True]                          # the SSIM term ran in both training steps, on a prediction that takes gradients
    assert calls == [True]                               # the per-ROI weight update reached the base loss
    raw = torch.load(os.path.join(str(tmp_path), "checkpoints", "checkpoint_latest_epoch.pth"), map_location="cpu",
                     weights_only=True)
    assert set(raw) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "scheduler_state_dict"}
    assert set(raw["model_state_dict"]) == set(m.state_dict())
