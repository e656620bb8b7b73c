"""The pointwise mode at model level: compute_dtype=float32, conv_algo=7 (conv_algo=6 plus the attention gates' 1x1x1
convolutions W_g / W_x -- forward, data gradient, weight gradient -- on exact fp32 MFMA kernels of their own) against the fp32
CPU oracle, against the exact-fp32 mode over a few optimizer steps, captured into a hipGraph, and under inference.Predictor.

Helpers, GRAD_KEYS and bounds are those of test_split_thin_mode_gpu.py (same oracle, same seeded batch, same initial
weights).  At 32^3 the gate levels 1 (32 768 voxels, C = 32) and 2 (4096 voxels, C = 64) are in the kernels' scope (>= 4096
voxels per sample)."""
import pytest
import torch

from test_split_wide_mode_gpu import GRAD_KEYS, _gpu_batch, _gpu_model, _oracle_step, _steps, rel

pytestmark = pytest.mark.gpu


def test_32cubed_batch2_pointwise_vs_oracle():
    """32^3 x 2 under conv_algo=7 against the fp32 CPU oracle with the bounds of the exact-fp32 and split tests (forward
    rel-L2 <= 1e-3, loss <= 1e-4, GRAD_KEYS <= 2e-2); the step launches both pointwise kernels, and the thin split families
    conv_algo=6 adds still run."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.train import forward_loss
    S = (32, 32, 32)
    sd, b, out, total, gen, grads, proj4 = _oracle_step(S, 2, seed=1234)
    gm = _gpu_model(S, sd, torch.float32, conv_algo=7)
    KT = ops.KernelTimer
    KT.enabled, KT.records = True, []
    try:
        losses, outs = forward_loss(gm, cu.build_reference_criterion(), _gpu_batch(b))
        losses[0].backward()
        torch.cuda.synchronize()
        recs = [(r[0], r[6]) for r in KT.records if r[0].startswith("conv_")]
    finally:
        KT.enabled, KT.records = False, []
        ops.SidePrep.join()
    names = {n for _k, n in recs}
    print(f"convolution kernels of the step: {sorted(names)}")
    assert any(k == "conv_fwd" and n.startswith("conv_pw_f32_k<") for k, n in recs), sorted(names)
    assert any(k == "conv_dgrad" and n.startswith("conv_pw_f32_k<") for k, n in recs), sorted(names)
    assert any(n.startswith("conv_pw_f32_wgrad_k<") for n in names), sorted(names)
    assert any(n.startswith("conv_split_thin_k<") for n in names), sorted(names)
    e_out = rel(outs[0], out)
    e_loss = abs(float(losses[0]) - total) / abs(total)
    print(f"32^3 B=2 pointwise: out rel-L2 {e_out:.3e}, loss rel {e_loss:.3e}")
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
    for k, e in errs.items():
        assert e <= 2e-2, (k, e)


def test_64cubed_pointwise_follows_exact_and_graph_equals_eager():
    """64^3 x 2: the loss sequence of conv_algo=7 follows that of conv_algo=0 from the same state (rel <= 1e-3), and a
    GraphedTrainStep replay equals the eager steps under conv_algo=7 (2e-2): the figures of
    test_64cubed_thin_split_follows_exact_and_graph_equals_eager."""
    from coma_unet_amd import ops
    from coma_unet_amd.synthetic import make_batch
    S = (64, 64, 64)
    dev = torch.device("cuda")
    assert ops.pick_algo((2, 64, 64, 64, 32), torch.float32, 16, 1, 1, False, False, dev, 7) == (3, 3)      # gate level 1: W_g / W_x
    assert ops.pick_algo((2, 64, 64, 64, 16), torch.float32, 16, 3, 1, False, False, dev, 7) == (4, 4)      # 16 -> 16 tail layer, as 6
    b = make_batch(2, S, seed=29)
    exact = _steps(0, False, S, b, 3)
    pw = _steps(7, False, S, b, 3)
    graph = _steps(7, True, S, b, 3)
    print("exact", exact, "pointwise", pw, "pointwise graphed", graph)
    for a, r in zip(pw, exact):
        assert abs(a - r) <= 1e-3 * abs(r), (pw, exact)
    for a, r in zip(graph, pw):
        assert abs(a - r) <= 2e-2 * abs(r), (graph, pw)


def test_predictor_under_pointwise():
    """inference.Predictor on a conv_algo=7 model at 32^3 x 2, bounds of test_predictor_fp32_matches_oracle_and_plain_eval: the
    graph-replayed eval forward is within 1e-3 of the CPU oracle's eval output and within 1e-5 of the model's plain eval forward."""
    import coma_unet_amd as cu
    from test_predictor_gpu import _gpu, _model, _oracle
    _sd0, b1, _b2, e1 = _oracle()
    gm, eg = _model(torch.float32, 7)
    y = cu.Predictor(gm, _gpu(b1), graph=True)().clone()
    print(f"conv_algo=7: predictor vs oracle {rel(y, e1):.3e}, vs plain eval {rel(y, eg):.3e}")
    assert rel(y, e1) < 1e-3 and rel(y, eg) <= 1e-5
