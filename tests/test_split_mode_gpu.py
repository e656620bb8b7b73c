"""The split-bf16 mode at model level: compute_dtype=float32, conv_algo=4 (fp32 tensors; the thick stride-1 3x3x3 layers at
W >= 32 on the bf16 matrix pipe as a two-term split, csrc/conv_split.hip) against the fp32 CPU oracle at the headline size,
against the exact-fp32 mode over a few optimizer steps, and captured into a hipGraph.

The helpers restate those of test_baseline_configs_gpu.py (same oracle, same seeded batch, same initial weights); the
bounds of the 128^3 test are the ones the exact-fp32 mode is held to there, unchanged.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_KEYS = [
    "model.1.merge.conv.weight",                      # merge1  64 -> 32 at full resolution
    "model.0.conv.1.conv.weight",                     # head conv1 32 -> 32 (8 experts)
    "model.1.submodule.1.merge.conv.weight",          # merge2 128 -> 64
    "model.1.submodule.0.conv.0.conv.weight",         # enc1 conv0, stride 2
    "model.1.upconv.up.conv.weight",                  # up1, transposed
    "model.1.attention.W_g.0.conv.weight",            # gate 1x1x1
    "deep_modulator_3c.blocks.1.conv.weight",         # 16 -> 16 full-resolution tail
    "final_pred_head.conv.weight",
    "model.1.upconv.up.conv.routing.weight",
    "pos_dynamic_prompt",
]


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    n = b.norm()
    return float((a - b).norm() / n) if n > 0 else float((a - b).norm())


def _gpu_batch(b):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}


def _oracle_step(shape, B, seed):
    """fp32 CPU oracle forward + loss + backward -> (state_dict, batch, out, total, gen_vec, grads, proj4)."""
    from coma_unet_amd.synthetic import make_batch
    from oracle.coma_oracle import build_reference_model
    from oracle.criterions_oracle import build_reference_criterion, train_step_loss
    torch.manual_seed(seed)
    om = build_reference_model(volume_shape=shape, double_forward=False)   # one U-Net pass: train-mode outputs are those of two
    om.set_save_attn(None)
    om.train(True)
    sd = {k: v.clone() for k, v in om.state_dict().items()}
    b = make_batch(B, shape, seed=seed + 1)
    with torch.enable_grad():
        res = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        total, gen = train_step_loss(res, b["tau"], b["roi"], b["covars"], build_reference_criterion())[:2]
    total.backward()
    grads = {n: p.grad.clone() for n, p in om.named_parameters() if p.grad is not None}
    out = res[0].detach().clone()
    proj4 = res[1][-1].detach().clone()
    del om, res
    return sd, b, out, float(total), gen.detach().clone(), grads, proj4


def _gpu_model(shape, sd, dtype, **kw):
    import coma_unet_amd as cu
    gm = cu.build_model(volume_shape=shape, compute_dtype=dtype, **kw).cuda()
    gm.load_state_dict(sd, strict=True)
    gm.set_save_attn(None)
    gm.train(True)
    return gm


def test_128cubed_batch2_split_vs_oracle():
    """The headline size in split mode against the fp32 CPU oracle, with the exact-fp32 test's bounds: forward rel-L2 <= 1e-3,
    loss <= 1e-4, proj4 <= 1e-3, the ten GRAD_KEYS tensors <= 2e-2; and the step really ran both split kernels.
    Measured on an MI355X (this test's print): out rel-L2 3.2e-5, loss rel 1.3e-7, proj4 3.8e-5, worst of the gradient
    tensors 5.7e-3 (enc1 conv0) -- DESIGN.md section 3."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.train import forward_loss
    sd, b, out, total, gen, grads, proj4 = _oracle_step((128, 128, 128), 2, seed=1234)
    gm = _gpu_model((128, 128, 128), sd, torch.float32, conv_algo=4)
    KT = ops.KernelTimer
    KT.enabled, KT.records = True, []
    try:
        losses, outs = forward_loss(gm, cu.build_reference_criterion(), _gpu_batch(b))
        losses[0].backward()
        torch.cuda.synchronize()
        names = [r[6] for r in KT.records]
        kinds = {r[1] for r in KT.records}
    finally:
        KT.enabled, KT.records = False, []
        ops.SidePrep.join()
    n_halo = sum(n.startswith("conv_split_halo_k") for n in names)
    n_wgrad = sum(n.startswith("conv_split_wgrad_k") for n in names)
    print(f"split kernels in the step: {n_halo} x conv_split_halo_k, {n_wgrad} x conv_split_wgrad_k; classes {sorted(kinds)}")
    assert n_halo > 0 and n_wgrad > 0, sorted(set(names))
    assert "mfma-split" in kinds
    e_out = rel(outs[0], out)
    mae = float((outs[0].float().cpu() - out).abs().mean())
    e_loss = abs(float(losses[0]) - total) / abs(total)
    e_gen, e_proj = rel(losses[1], gen), rel(outs[1][-1], proj4)
    print(f"128^3 B=2 split: out rel-L2 {e_out:.3e}, voxel MAE {mae:.3e}, loss rel {e_loss:.3e}, gen {e_gen:.3e}, proj4 {e_proj:.3e}")
    got = dict(gm.named_parameters())
    errs = {}
    for k in GRAD_KEYS:
        if k not in grads:             # a prompt no sample of this batch selected: None on both sides
            assert got[k].grad is None, k
            continue
        errs[k] = rel(got[k].grad, grads[k])
        print(f"  grad {k}: rel {errs[k]:.3e}")
    assert e_out <= 1e-3
    assert e_loss <= 1e-4
    assert e_gen <= 1e-4
    assert e_proj <= 1e-3
    assert float(outs[0].min()) >= 0.0
    for k, e in errs.items():
        assert e <= 2e-2, (k, e)


def _steps(algo, graphed, S, b, n):
    import coma_unet_amd as cu
    from coma_unet_amd.train import train_step, make_optimizer, GraphedTrainStep
    torch.manual_seed(4)
    gm = cu.build_model(volume_shape=S, static_prompts=True, compute_dtype=torch.float32, conv_algo=algo).cuda()
    gm.set_save_attn(None)
    gm.train(True)
    gb = _gpu_batch(b)
    gb["roi_pred_dicts"] = gm._priors(b["roi_pred_dicts"], 2, torch.device("cuda"))
    opt = make_optimizer(gm, 1e-5)
    crit = cu.build_reference_criterion()
    if graphed:
        step = GraphedTrainStep(gm, crit, opt, gb, warmup=2)       # 2 eager warm-up steps inside
        ls = [float(step()[0][0]) for _ in range(n)]
    else:
        ls = [float(train_step(gm, crit, opt, gb)[0][0]) for _ in range(n + 2)][2:]
    torch.cuda.synchronize()
    return ls


def test_32cubed_split_follows_exact_and_graph_equals_eager():
    """32^3 x 2 (the full-resolution level is in the split kernels' scope): the loss sequence of conv_algo=4 follows that of
    conv_algo=0 from the same state (rel <= 1e-3), and a GraphedTrainStep replay equals the eager steps under conv_algo=4 to
    the tolerance of test_graphed_step_matches_eager_steps (2e-2)."""
    from coma_unet_amd import ops
    from coma_unet_amd.synthetic import make_batch
    S = (32, 32, 32)
    assert ops.pick_algo((2, 32, 32, 32, 32), torch.float32, 32, 3, 1, False, True, torch.device("cuda"), 4) == (4, 4)
    b = make_batch(2, S, seed=29)
    exact = _steps(0, False, S, b, 3)
    split = _steps(4, False, S, b, 3)
    graph = _steps(4, True, S, b, 3)
    print("exact", exact, "split", split, "split graphed", graph)
    for a, r in zip(split, exact):
        assert abs(a - r) <= 1e-3 * abs(r), (split, exact)
    for a, r in zip(graph, split):
        assert abs(a - r) <= 2e-2 * abs(r), (graph, split)
