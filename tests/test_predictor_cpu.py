"""Host side of the inference path (coma_unet_amd/inference.py) without a GPU."""
import pytest
import torch

from _gate_eval_ref import folded_gate64, gate_eval_ref64, randomize_gate


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("C", [32, 48])
def test_fold_gate_reproduces_fp64_eval_gate(C, bias):
    from coma_unet_amd import fold_gate
    from coma_unet_amd.attn_unet_data_parallel import ObservableAttentionBlock
    from coma_unet_amd.layers import Config
    torch.manual_seed(C + bias)
    blk = ObservableAttentionBlock(Config(), f_int=C // 2, f_g=C, f_l=C).double().eval()
    randomize_gate(blk, 3 * C + bias)
    if not bias:
        for seq in (blk.W_g, blk.W_x, blk.psi):
            seq[0].conv.bias = None
    g = torch.randn(2, C, 3, 4, 5, dtype=torch.float64)
    x = torch.randn(2, C, 3, 4, 5, dtype=torch.float64)
    att, psi = gate_eval_ref64(blk, g, x)
    fold = fold_gate(blk)
    assert fold["scale_g"].dtype == torch.float64 and fold["shift"].shape == (C // 2,) and fold["psi_ab"].shape == (2,)
    a2, p2 = folded_gate64(fold, blk.W_g[0].conv.weight.detach(), blk.W_x[0].conv.weight.detach(), g, x)
    assert float((a2 - att).abs().max()) < 1e-12 and float((p2 - psi).abs().max()) < 1e-12
    # the MFMA form's operands: 32 rows, exact zeros beyond F, the same numbers before their bf16 rounding
    F_ = C // 2
    assert fold["wg"].shape == (32, C) and fold["wg"].dtype == torch.bfloat16 and fold["shift32"].shape == (32,)
    for k in ("wg", "wx", "shift32", "w_psi32"):
        assert not fold[k][F_:].double().abs().any(), k
    want = fold["scale_g"][:, None] * blk.W_g[0].conv.weight.detach().reshape(F_, C)
    assert float((fold["wg"][:F_].double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())
    assert torch.equal(fold["shift32"][:F_], fold["shift"]) and torch.equal(fold["w_psi32"][:F_], fold["w_psi"])


def test_predictor_rejects_cpu_batch():
    import coma_unet_amd as cu
    from coma_unet_amd.synthetic import make_batch
    S = (16, 16, 16)
    model = cu.build_model(volume_shape=S)
    with pytest.raises(ValueError):
        cu.Predictor(model, make_batch(1, S, seed=0))


def test_eval_fused_is_off_by_default():
    from coma_unet_amd.layers import Config
    assert Config().eval_fused is False
