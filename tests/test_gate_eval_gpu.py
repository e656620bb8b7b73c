"""The eval-mode attention gate kernels (csrc/gate.hip: gate_eval_fwd_k, gate_eval_mfma_k) against the fp64 eval
composition of the gate, and against today's piecewise eval path on the same inputs.

Bounds (tests/test_ops_gpu.py's TOL): att and psi rel-L2 against fp64 below 2e-5 (fp32) / 2e-2 (bf16); in bf16 each new
kernel's error is at most 1.1 x the piecewise path's (the fused forms round fewer intermediates; the 10 % covers a
different summation order).  Both errors are printed.  Set-up as in AttentionLayer.forward: g is the upper and att the
lower channel half of one (B, D, H, W, 2C) buffer, and the g half must come back bit-identical.

The MFMA launcher caps a grid pass at 2048 blocks x 128 voxels per sample (conv_mfma_pw_k's cap), so 40 x 64 x 104 =
266 240 voxels is the smallest convenient grid above one pass (262 144)."""
import functools

import pytest
import torch

from _gate_eval_ref import gate_eval_ref64, randomize_gate

pytestmark = pytest.mark.gpu
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}
GRIDS = [(2, 4, 6, 8), (2, 3, 5, 7)]       # 105 voxels: no multiple of a wave's or a block's voxel step


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def _case(C, dtype, grid):
    """Block, inputs, the fp64 result and the piecewise eval path's errors: made once, shared, never modified."""
    from coma_unet_amd.attn_unet_data_parallel import ObservableAttentionBlock
    from coma_unet_amd.layers import Config
    B, D, H, W = grid
    torch.manual_seed(1000 * C + D)
    blk = ObservableAttentionBlock(Config(compute_dtype=dtype), f_int=C // 2, f_g=C, f_l=C).cuda().eval()
    randomize_gate(blk, C + D)
    g = torch.randn(B, D, H, W, C).to(dtype).cuda()
    x = torch.randn(B, D, H, W, C).to(dtype).cuda()
    ext = lambda t: t.permute(0, 4, 1, 2, 3)
    att64, psi64 = gate_eval_ref64(blk, ext(g), ext(x))
    blk.save_attn = True
    cat = _cat(g)
    with torch.no_grad():
        a_pw, p_pw = blk(g=cat[..., C:], x=x, out=cat[..., :C])          # today's eval path (cfg.eval_fused is False)
    blk.save_attn = None
    pw = (rel(ext(a_pw), att64), rel(ext(p_pw), psi64))
    return blk, g, x, att64, psi64, pw


def _cat(g):
    C = g.shape[4]
    cat = torch.zeros(tuple(g.shape[:4]) + (2 * C,), dtype=g.dtype, device=g.device)
    cat[..., C:] = g
    return cat


def _run_and_check(C, dtype, grid, want_psi, form, expect):
    from coma_unet_amd import fold_gate, inference, ops
    blk, g, x, att64, psi64, pw = _case(C, dtype, grid)
    cat = _cat(g)
    gv, out = cat[..., C:], cat[..., :C]
    assert ops.gate_eval_mfma_ok(gv, x, C // 2) == (expect == "mfma" or (dtype == torch.bfloat16 and C <= 64))
    before = dict(inference.counts)
    att, psi = inference.gate_eval(blk, gv, x, out=out, want_psi=want_psi, fold=fold_gate(blk), form=form)
    torch.cuda.synchronize()
    assert inference.counts[expect] == before[expect] + 1 and sum(inference.counts.values()) == sum(before.values()) + 1
    assert att.data_ptr() == out.data_ptr() and torch.equal(cat[..., C:], g), "foreign channels were touched"
    ext = lambda t: t.permute(0, 4, 1, 2, 3)
    e_att = rel(ext(att), att64)
    print(f"{expect} C={C} {dtype} {grid}: att rel-L2 {e_att:.3e} (piecewise {pw[0]:.3e})", end="")
    assert e_att < TOL[dtype]
    if dtype == torch.bfloat16:
        assert e_att <= 1.1 * pw[0]
    if want_psi:
        e_psi = rel(ext(psi), psi64)
        print(f"; psi {e_psi:.3e} (piecewise {pw[1]:.3e})")
        assert e_psi < TOL[dtype]
        if dtype == torch.bfloat16:
            assert e_psi <= 1.1 * pw[1]
    else:
        assert psi is None


@pytest.mark.parametrize("want_psi", [True, False])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [32, 64, 256])
def test_gate_eval_elementwise(C, dtype, grid, want_psi):
    # fp32 tensors and C = 256 must end up here on their own; bf16 C <= 64 would take the MFMA form and is forced
    form = "elementwise" if (dtype == torch.bfloat16 and C <= 64) else None
    _run_and_check(C, dtype, grid, want_psi, form, "elementwise")


@pytest.mark.parametrize("want_psi", [True, False])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("C", [32, 48, 64])         # 48: F = 24, three K steps and a partial row tile
def test_gate_eval_mfma(C, grid, want_psi):
    _run_and_check(C, torch.bfloat16, grid, want_psi, None, "mfma")


def test_gate_eval_mfma_more_than_one_grid_pass():
    _run_and_check(32, torch.bfloat16, (1, 40, 64, 104), True, None, "mfma")


def test_gate_eval_mfma_predicate_and_fallback():
    """0 for fp32 tensors, C = 128, C = 40 and a pitch that breaks 16-byte alignment; the Python layer then runs the
    element-wise kernel (asserted for C = 128 here and for fp32 / C = 256 in test_gate_eval_elementwise; C = 40 and the
    odd pitch are outside what the 1x1x1 convolution / gate kernels of the training path take, so only the answer is
    checked for them)."""
    from coma_unet_amd import ops
    mk = lambda C, dt, ld=None: torch.zeros(2, 4, 6, 8, ld or C, dtype=dt, device="cuda")[..., :C]
    bf, f32 = torch.bfloat16, torch.float32
    assert ops.gate_eval_mfma_ok(mk(32, bf), mk(32, bf), 16)
    assert ops.gate_eval_mfma_ok(mk(32, bf, 64), mk(32, bf), 16)
    assert not ops.gate_eval_mfma_ok(mk(32, f32), mk(32, f32), 16)
    assert not ops.gate_eval_mfma_ok(mk(128, bf), mk(128, bf), 64)
    assert not ops.gate_eval_mfma_ok(mk(40, bf), mk(40, bf), 20)
    assert not ops.gate_eval_mfma_ok(mk(32, bf, 68), mk(32, bf), 16)
    assert not ops.gate_eval_mfma_ok(mk(32, bf), mk(32, bf, 36), 16)
    _run_and_check(128, torch.bfloat16, GRIDS[1], True, None, "elementwise")
