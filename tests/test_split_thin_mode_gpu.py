"""The thin split mode at model level: compute_dtype=float32, conv_algo=6 (conv_algo=5 plus the few-channel full-resolution
layers -- the modulator tails, the 1 -> 32 head convolution, their data and weight gradients -- on the bf16 matrix pipe as a
two-term split) against the fp32 CPU oracle, against the exact-fp32 mode over a few optimizer steps, and captured into a
hipGraph.

Helpers, GRAD_KEYS and bounds are those of test_split_wide_mode_gpu.py (same oracle, same seeded batch, same initial
weights); 32^3 is the smallest volume whose full-resolution level the thin kernels take (W >= 32)."""
import pytest
import torch

from test_split_wide_mode_gpu import GRAD_KEYS, _gpu_batch, _gpu_model, _oracle_step, _steps, rel

pytestmark = pytest.mark.gpu


def test_32cubed_batch2_thin_split_vs_oracle():
    """32^3 x 2 under conv_algo=6 against the fp32 CPU oracle with the bounds of the exact-fp32 and split tests (forward
    rel-L2 <= 1e-3, loss <= 1e-4, GRAD_KEYS <= 2e-2); the step launches both thin split families and no conv_thin16f_*
    kernel (no class of the exact kernels' scope is left out of the split predicate)."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.train import forward_loss
    S = (32, 32, 32)
    sd, b, out, total, gen, grads, proj4 = _oracle_step(S, 2, seed=1234)
    gm = _gpu_model(S, sd, torch.float32, conv_algo=6)
    KT = ops.KernelTimer
    KT.enabled, KT.records = True, []
    try:
        losses, outs = forward_loss(gm, cu.build_reference_criterion(), _gpu_batch(b))
        losses[0].backward()
        torch.cuda.synchronize()
        names = {r[6] for r in KT.records if r[0].startswith("conv_")}
    finally:
        KT.enabled, KT.records = False, []
        ops.SidePrep.join()
    print(f"convolution kernels of the step: {sorted(names)}")
    assert any(n.startswith("conv_split_thin_k<") for n in names), sorted(names)
    assert any(n.startswith("conv_split_thin_wgrad_k<") for n in names), sorted(names)
    assert not any(n.startswith("conv_thin16f_") for n in names), sorted(names)
    e_out = rel(outs[0], out)
    e_loss = abs(float(losses[0]) - total) / abs(total)
    print(f"32^3 B=2 thin split: out rel-L2 {e_out:.3e}, loss rel {e_loss:.3e}")
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


def test_64cubed_thin_split_follows_exact_and_graph_equals_eager():
    """64^3 x 2: the loss sequence of conv_algo=6 follows that of conv_algo=0 from the same state (rel <= 1e-3), and a
    GraphedTrainStep replay equals the eager steps under conv_algo=6 (2e-2): the figures of
    test_64cubed_wide_split_follows_exact_and_graph_equals_eager."""
    from coma_unet_amd import ops
    from coma_unet_amd.synthetic import make_batch
    S = (64, 64, 64)
    dev = torch.device("cuda")
    assert ops.pick_algo((2, 64, 64, 64, 16), torch.float32, 16, 3, 1, False, False, dev, 6) == (4, 4)      # 16 -> 16 tail layer
    assert ops.pick_algo((2, 64, 64, 64, 16), torch.float32, 16, 3, 1, False, False, dev, 5) == (3, 3)
    b = make_batch(2, S, seed=29)
    exact = _steps(0, False, S, b, 3)
    split = _steps(6, False, S, b, 3)
    graph = _steps(6, True, S, b, 3)
    print("exact", exact, "thin split", split, "thin split graphed", graph)
    for a, r in zip(split, exact):
        assert abs(a - r) <= 1e-3 * abs(r), (split, exact)
    for a, r in zip(graph, split):
        assert abs(a - r) <= 2e-2 * abs(r), (graph, split)


def test_predictor_under_thin_split():
    """inference.Predictor on a conv_algo=6 model at 32^3 x 2, bounds of test_predictor_fp32_matches_oracle_and_plain_eval: the
    graph-replayed eval forward is within 1e-3 of the CPU oracle's eval output and within 1e-5 of the model's plain eval forward
    (the thin forward kernels without a statistics record)."""
    import coma_unet_amd as cu
    from test_predictor_gpu import _gpu, _model, _oracle
    _sd0, b1, _b2, e1 = _oracle()
    gm, eg = _model(torch.float32, 6)
    y = cu.Predictor(gm, _gpu(b1), graph=True)().clone()
    print(f"conv_algo=6: predictor vs oracle {rel(y, e1):.3e}, vs plain eval {rel(y, eg):.3e}")
    assert rel(y, e1) < 1e-3 and rel(y, eg) <= 1e-5
