"""inference.Predictor at 32^3, B = 2, with the oracle's weights after one training-mode forward (so that the running
statistics are not the initial ones).  Gate levels: 32^3 / C 32 and 16^3 / 64 (MFMA form in bf16), 8^3 / 128 and
4^3 / 256 (element-wise kernel).

Bounds: fp32 against the CPU oracle's eval output < 1e-3 (test_model_gpu.test_eval_mode_uses_double_updated_running_stats)
and against the model's own plain eval forward <= 1e-5; bf16 error against the oracle <= 1.1 x the plain eval forward's."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
S = (32, 32, 32)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _gpu(b):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}


def _call(m, b):
    return m(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])


@functools.lru_cache(maxsize=None)
def _oracle():
    """Oracle after one training-mode forward, in eval mode; its initial weights; two batches; its eval outputs."""
    from coma_unet_amd.synthetic import make_batch
    from oracle.coma_oracle import build_reference_model
    torch.manual_seed(5)
    om = build_reference_model(volume_shape=S)
    om.set_save_attn(None)
    om.train(True)
    sd0 = {k: v.clone() for k, v in om.state_dict().items()}
    b1, b2 = make_batch(2, S, seed=11), make_batch(2, S, seed=12)
    with torch.no_grad():
        _call(om, b1)
        om.eval()
        e1 = _call(om, b1)
    return sd0, b1, b2, e1


@functools.lru_cache(maxsize=None)
def _model(dtype, conv_algo=0):
    """The HIP model with the same history, in eval mode, and its plain eval output on batch 1 (never modified)."""
    import coma_unet_amd as cu
    sd0, b1, _b2, _e1 = _oracle()
    gm = cu.build_model(volume_shape=S, compute_dtype=dtype, conv_algo=conv_algo).cuda()
    gm.load_state_dict(sd0, strict=True)
    gm.set_save_attn(None)
    gm.train(True)
    with torch.no_grad():
        _call(gm, _gpu(b1))
        gm.eval()
        eg = _call(gm, _gpu(b1)).float().clone()
    return gm, eg


@pytest.mark.parametrize("conv_algo", [0, 4])
def test_predictor_fp32_matches_oracle_and_plain_eval(conv_algo):
    import coma_unet_amd as cu
    from coma_unet_amd import inference
    _sd0, b1, _b2, e1 = _oracle()
    gm, eg = _model(torch.float32, conv_algo)
    n0 = inference.counts["mfma"]
    y = cu.Predictor(gm, _gpu(b1), graph=True)().clone()
    assert tuple(y.shape) == (2, 1) + S
    print(f"conv_algo={conv_algo}: predictor vs oracle {rel(y, e1):.3e}, vs plain eval {rel(y, eg):.3e}")
    assert rel(y, e1) < 1e-3 and rel(y, eg) <= 1e-5
    assert inference.counts["mfma"] == n0, "fp32 tensors must not take the bf16 MFMA gate"


def test_predictor_bf16_no_worse_than_plain_eval():
    import coma_unet_amd as cu
    from coma_unet_amd import inference
    _sd0, b1, _b2, e1 = _oracle()
    gm, eg = _model(torch.bfloat16)
    n_m, n_e = inference.counts["mfma"], inference.counts["elementwise"]
    y = cu.Predictor(gm, _gpu(b1), graph=False)().float().clone()
    assert (inference.counts["mfma"] - n_m, inference.counts["elementwise"] - n_e) == (2, 2)
    e_pred, e_plain = rel(y, e1), rel(eg, e1)
    print(f"bf16: predictor vs oracle {e_pred:.3e}, plain eval forward vs oracle {e_plain:.3e}")
    assert e_pred <= 1.1 * e_plain
    yg = cu.Predictor(gm, _gpu(b1), graph=True)().float().clone()
    assert rel(yg, e1) <= 1.1 * e_plain


def test_graph_replay_reads_the_loaded_batch():
    import coma_unet_amd as cu
    _sd0, b1, b2, _e1 = _oracle()
    gm, _eg = _model(torch.float32)
    pg = cu.Predictor(gm, _gpu(b1), graph=True)
    pe = cu.Predictor(gm, _gpu(b1), graph=False)
    y1 = pg().clone()
    y2g = pg(_gpu(b2)).clone()                 # the list of prior dicts goes through model._priors
    y2e = pe(_gpu(b2)).clone()
    print(f"graph vs eager on batch 2: {rel(y2g, y2e):.3e}; batch 2 vs batch 1: {rel(y2g, y1):.3e}")
    assert rel(y2g, y2e) <= 1e-5
    assert rel(y2g, y1) > 1e-2, "the replay read stale inputs"


def test_model_state_untouched():
    import coma_unet_amd as cu
    _sd0, b1, _b2, _e1 = _oracle()
    gm, eg = _model(torch.float32)
    gb = _gpu(b1)
    gm.train(True)
    try:
        modes = [(m, m.training) for m in gm.modules()]
        sd = {k: v.clone() for k, v in gm.state_dict().items()}
        params = {k: v.detach().clone() for k, v in gm.named_parameters()}
        p = cu.Predictor(gm, gb, graph=True)
        for _ in range(3):
            p()
        pe = cu.Predictor(gm, gb, graph=False)
        pe()
        torch.cuda.synchronize()
        assert gm.training is True and all(m.training is t for m, t in modes)
        assert gm.cfg.eval_fused is False and gm.cfg.eval_stats is None and not gm.static_prompts
        now = gm.state_dict()
        assert list(now) == list(sd)
        for k, v in sd.items():
            assert torch.equal(now[k], v), k
        for k, v in gm.named_parameters():
            assert torch.equal(v.detach(), params[k]), k
    finally:
        gm.eval()
    with torch.no_grad():
        again = _call(gm, gb).float()
    assert rel(again, eg) <= 1e-5


def test_refresh_picks_up_new_running_statistics():
    import coma_unet_amd as cu
    _sd0, b1, _b2, _e1 = _oracle()
    gm, _eg = _model(torch.float32)
    p = cu.Predictor(gm, _gpu(b1), graph=True)
    y0 = p().clone()
    rv = gm.model[1].attention.W_g[1].running_var
    keep = rv.clone()
    try:
        rv.mul_(4.0)
        y_stale = p().clone()
        p.refresh()
        y1 = p().clone()
    finally:
        rv.copy_(keep)
    # two replays of one graph agree to the fp64 statistics atomics' reordering only (the graph-against-eager bound, 1e-5),
    # so "unchanged" is that bound and "changed" must stand clear of it (10 x)
    print(f"stale folds vs before: {rel(y_stale, y0):.3e}; after refresh() vs before: {rel(y1, y0):.3e}")
    assert rel(y_stale, y0) <= 1e-5, "the folds are made at construction / refresh(), not per call"
    assert rel(y1, y0) > 1e-4


def test_predictor_rejects_embeddings_out():
    import coma_unet_amd as cu
    _sd0, b1, _b2, _e1 = _oracle()
    gm = cu.build_model(volume_shape=S, embeddings_out=True).cuda()
    with pytest.raises(ValueError):
        cu.Predictor(gm, _gpu(b1))
