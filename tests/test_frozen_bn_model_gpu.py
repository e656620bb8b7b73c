"""Frozen-BatchNorm training end to end: the model with every BatchNorm3d frozen -- once by the torch idiom (the holder
modules in eval mode inside a train-mode model), once by model.freeze_batchnorm() -- against the CPU oracle frozen by the
idiom, at 32^3, B = 2, after the running statistics have been moved off (0, 1).

Tolerances are those of tests/test_model_gpu.py: forward and loss against the fp32 oracle within 1e-3; every gradient that is
not rounding noise (|r| < 1e-4 max(1, |p|)) against the fp64 oracle within max(3e-2, 4 x the fp32 CPU oracle's own error).  The
22 convolution biases that feed a frozen BatchNorm have real gradients now and none of them may fall under the noise rule.

Measured on an MI355X: forward rel-L2 2.0e-6, loss equal to the last digit, worst gradient 3.8e-3 ... 4.1e-3 from fp64 (the fp32
CPU oracle's own worst: 3.8e-3), smallest bias gradient norm 4.33e-4.  One scalar sits at the margin of the gradient rule: the
PReLU slope model.1.submodule.1.upconv.up.adn.A.weight (InstanceNorm + PReLU, not a frozen layer; |g| = 0.083) was 4.9e-2 off in
one of seven runs of test_frozen_step_matches_oracle (bound 3e-2: the CPU oracle's own error there is 6.9e-4) and within the bound
in the others.  Eight fresh runs of the step gave 0.0829 ... 0.0841 for it; the plain training step shows the same absolute
run-to-run spread on the same scalar (order of the fp32 split-K merges of the deep layers, amplified by the InstanceNorms at
2^3 ... 4^3 voxels).  The bound is left as it was set.
"""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn

import _step_state as ss

pytestmark = pytest.mark.gpu
S = (32, 32, 32)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "default_step_kernels_32.json")


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    n = b.norm()
    return float((a - b).norm() / n) if n > 0 else float((a - b).norm())


def _gpu_batch(b):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}


def _bns(m):
    return [x for x in m.modules() if isinstance(x, nn.BatchNorm3d)]


def _buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches_tracked" in k}


def _freeze(m, route):
    if route == "idiom":
        for x in _bns(m):
            x.eval()
    else:
        m.freeze_batchnorm()
    return m


_cache = {}


def _oracle():
    """The oracle with moved running statistics, frozen by the idiom, and its fp32 / fp64 step on the batch of seed 9."""
    if "o" not in _cache:
        from coma_unet_amd.synthetic import make_batch
        from oracle.coma_oracle import build_reference_model
        from oracle.criterions_oracle import build_reference_criterion, train_step_loss
        torch.manual_seed(321)
        om = build_reference_model(volume_shape=S)
        om.set_save_attn(None)
        om.train(True)
        w = make_batch(2, S, seed=5)
        with torch.no_grad():
            for _ in range(2):
                om(w["mri"], w["covars"], roi_pred_dicts=w["roi_pred_dicts"], sample_roi_mask=w["roi"])
        sd = copy.deepcopy(om.state_dict())
        _freeze(om, "idiom")
        b = make_batch(2, S, seed=9)
        o64 = copy.deepcopy(om).double()
        res = o64(b["mri"].double(), b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"].double())
        train_step_loss(res, b["tau"].double(), b["roi"].double(), b["covars"], build_reference_criterion())[0].backward()
        r32 = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        tot = train_step_loss(r32, b["tau"], b["roi"], b["covars"], build_reference_criterion())[0]
        tot.backward()
        assert all(torch.equal(v, sd[k]) for k, v in om.state_dict().items() if "running_" in k or "num_batches" in k)
        _cache["o"] = dict(sd=sd, b=b, out=r32[0].detach(), total=float(tot),
                           g32={n: (None if p.grad is None else p.grad.detach().clone()) for n, p in om.named_parameters()},
                           g64={n: (None if p.grad is None else p.grad.detach().clone()) for n, p in o64.named_parameters()},
                           p64={n: p.detach().clone() for n, p in o64.named_parameters()})
    return _cache["o"]


def _model(route, dtype=torch.float32, sd=None, **kw):
    import coma_unet_amd as cu
    gm = cu.build_model(volume_shape=S, compute_dtype=dtype, **kw).cuda()
    gm.load_state_dict(sd if sd is not None else _oracle()["sd"], strict=True)
    gm.set_save_attn(None)
    gm.train(True)
    return _freeze(gm, route) if route else gm


def _bias_names(gm):
    """The convolution biases that feed a BatchNorm inside the U-Net: 2 + 8 block convolutions, 3 per gate."""
    from coma_unet_amd.attn_unet_data_parallel import ObservableAttentionBlock
    out = []
    for name, m in gm.named_modules():
        if not name.startswith("model."):
            continue
        if getattr(m, "adn", None) is not None and isinstance(m.adn.N, nn.BatchNorm3d):
            out.append(name + ".conv.bias")
        if isinstance(m, ObservableAttentionBlock):
            out += [f"{name}.{k}.0.conv.bias" for k in ("W_g", "W_x", "psi")]
    return out


def _check_grads(gm, o, tag):
    og, o32, p64 = o["g64"], o["g32"], o["p64"]
    biases = _bias_names(gm)
    assert len(biases) == 22 and "model.0.conv.0.conv.bias" in biases and "model.0.conv.1.conv.bias" in biases, biases
    worst = worst_cpu = 0.0
    small = min((float(og[n].norm()), n) for n in biases)
    for n, p in gm.named_parameters():
        r = og[n]
        assert (p.grad is None) == (r is None), n
        if r is None or float(r.norm()) < 1e-4 * max(1.0, float(p64[n].norm())):
            assert n not in biases, (n, float(r.norm()))         # a bias in front of a frozen BatchNorm is no noise
            continue
        e, e_cpu = rel(p.grad, r), rel(o32[n], r)
        worst, worst_cpu = max(worst, e), max(worst_cpu, e_cpu)
        assert e < max(3e-2, 4.0 * e_cpu), (tag, n, e, e_cpu)
    print(f"{tag}: worst relative gradient error vs fp64 oracle: HIP fp32 {worst:.2e}, CPU fp32 oracle {worst_cpu:.2e}; "
          f"smallest bias gradient norm {small[0]:.2e} ({small[1]})")


@pytest.mark.parametrize("route", ["idiom", "switch"])
def test_frozen_step_matches_oracle(route):
    import coma_unet_amd as cu
    from coma_unet_amd.train import forward_loss
    o = _oracle()
    gm = _model(route)
    before = _buffers(gm)
    losses, outs = forward_loss(gm, cu.build_reference_criterion(), _gpu_batch(o["b"]))
    losses[0].backward()
    torch.cuda.synchronize()
    e_out, e_loss = rel(outs[0], o["out"]), abs(float(losses[0]) - o["total"]) / abs(o["total"])
    print(f"{route}: out rel-L2 {e_out:.2e}, loss rel {e_loss:.2e}")
    assert e_out < 1e-3 and e_loss < 1e-3
    _check_grads(gm, o, route)
    after = gm.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert gm.training and (route == "switch") == gm.cfg.frozen_bn == gm.cfg_heads.frozen_bn
    if route == "switch":      # sticky
        gm.eval()
        gm.train(True)
        assert gm.cfg.frozen_bn and all(m.training for m in _bns(gm))


def _records(gm, gb):
    """[(kind, kernel name)] of the bracketed launches of one forward + backward."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops
    from coma_unet_amd.train import forward_loss
    KT = ops.KernelTimer
    KT.enabled, KT.records = True, []
    try:
        gm.zero_grad(set_to_none=True)
        losses, _ = forward_loss(gm, cu.build_reference_criterion(), gb)
        losses[0].backward()
        torch.cuda.synchronize()
        return [[r[0], r[6]] for r in KT.records]
    finally:
        KT.enabled, KT.records = False, []
        ops.SidePrep.join()


def test_both_routes_launch_the_same_kernels():
    gb = _gpu_batch(_oracle()["b"])
    a, b = _records(_model("idiom"), gb), _records(_model("switch"), gb)
    assert a == b
    names = [n for _k, n in a]
    n_frozen = sum(n.startswith("norm_act_bwd_frozen_k") for n in names)
    n_gate_f, n_gate_b = sum(n.startswith("gate_frozen_fwd_k") for n in names), sum(n.startswith("gate_frozen_bwd_k") for n in names)
    n_train = sum(n.startswith("norm_bwd_partial_k") for n in names)
    print(f"frozen step: {len(a)} bracketed launches, {n_frozen} frozen norm backwards, {n_gate_f} + {n_gate_b} frozen gate passes, "
          f"{n_train} training-mode norm backwards (InstanceNorm)")
    assert n_gate_f == n_gate_b == 4 and n_frozen >= 10 + 2      # the 2 + 8 block BatchNorms and the heads that reach the loss
    plain = _records(_model(None), gb)
    assert not any(n.startswith(("norm_act_bwd_frozen_k", "gate_frozen")) for _k, n in plain)
    assert n_train == sum(n.startswith("norm_bwd_partial_k") for _k, n in plain) - n_frozen     # the InstanceNorm layers are untouched


def test_default_step_launches_what_the_parent_launched():
    """Nothing frozen: the bracketed launches of one default 32^3 step, kinds and kernel names in order, are the list
    recorded from the commit before frozen BatchNorm existed (tests/golden/default_step_kernels_32.json)."""
    with open(GOLD) as f:
        want = json.load(f)
    got = _records(_model(None), _gpu_batch(_oracle()["b"]))
    assert len(got) == len(want), (len(got), len(want))
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]


def test_three_frozen_adamw_steps_track_oracle():
    import coma_unet_amd as cu
    from coma_unet_amd.train import train_step, make_optimizer
    from oracle.coma_oracle import build_reference_model
    from oracle.criterions_oracle import build_reference_criterion, train_step_loss
    o = _oracle()
    om = build_reference_model(volume_shape=S)
    om.load_state_dict(o["sd"])
    om.set_save_attn(None)
    om.train(True)
    _freeze(om, "idiom")
    gm = _model("switch")
    before = _buffers(gm)
    b, gb = o["b"], _gpu_batch(o["b"])
    oopt, gopt = torch.optim.AdamW(om.parameters(), 1e-3), make_optimizer(gm, 1e-3)
    ocrit, gcrit = build_reference_criterion(), cu.build_reference_criterion()
    ol, gl = [], []
    for _ in range(3):
        oopt.zero_grad()
        res = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
        tot = train_step_loss(res, b["tau"], b["roi"], b["covars"], ocrit)[0]
        tot.backward()
        oopt.step()
        ol.append(float(tot))
        gm.train(True)                                            # what train_dp does every epoch: the switch survives it
        losses, _ = train_step(gm, gcrit, gopt, gb)
        gl.append(float(losses[0]))
    print("oracle losses", ol, "gpu losses", gl)
    assert abs(gl[0] - ol[0]) / ol[0] < 1e-4
    for a, r in zip(gl[1:], ol[1:]):
        assert abs(a - r) / r < 5e-2     # Adam's first steps are sign-like: noise-level grads flip +-lr
    after = gm.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def test_graphed_frozen_step_equals_eager_steps():
    """A GraphedTrainStep of the frozen model replayed three times against three eager frozen steps, compared per step and
    per tensor as tests/_step_state.py compares a stateful run with its reference (the fp32 bounds of that file): learning rate
    0 and that file's in-place perturbation of the weights in front of every step, so that step k is a function of
    (weights_k, batch) alone and no two steps see the same weights.  Capture and replay neither re-create the (mean, rstd)
    tables nor touch a running buffer."""
    import coma_unet_amd as cu
    from coma_unet_amd.train import train_step, make_optimizer, GraphedTrainStep
    o = _oracle()
    runs = {}
    for graphed in (False, True):
        gm = _model("switch", static_prompts=True)
        before = _buffers(gm)
        gb = _gpu_batch(o["b"])
        gb["roi_pred_dicts"] = gm._priors(o["b"]["roi_pred_dicts"], 2, torch.device("cuda"))
        opt = make_optimizer(gm, 0.0)
        crit = cu.build_reference_criterion()
        tabs = {id(m): (m.__dict__["_coma_frozen"]["mean"].data_ptr(), m.__dict__["_coma_frozen"]["rstd"].data_ptr()) for m in _bns(gm)}
        assert len(tabs) == 32
        seq = []
        if graphed:
            step = GraphedTrainStep(gm, crit, opt, gb, warmup=2)
        else:
            for _ in range(2):
                train_step(gm, crit, opt, gb)
            step = lambda: train_step(gm, crit, opt, gb)
        for k in (1, 2, 3):
            ss.perturb(gm, k)
            losses, _ = step()
            torch.cuda.synchronize()
            seq.append((ss.grads_of(gm), float(losses[0])))
        assert len({l for _g, l in seq}) == 3                     # three different steps
        for m in _bns(gm):
            ent = m.__dict__["_coma_frozen"]
            assert (ent["mean"].data_ptr(), ent["rstd"].data_ptr()) == tabs[id(m)]
        after = gm.state_dict()
        for k, v in before.items():
            assert torch.equal(after[k], v), k
        runs[graphed] = seq
    for i, ((ge, le), (gg, lg)) in enumerate(zip(runs[False], runs[True])):
        bad = ss.compare("fp32-auto", gg, ge, lg, le)
        print(f"step {i}: eager loss {le:.6f}, graph loss {lg:.6f}; {len(bad)} mismatches {bad[:6]}")
        assert not bad


def test_tables_follow_load_state_dict():
    """load_state_dict with other running statistics after freezing: the next forward uses them (the tables are refreshed
    in place), and agrees with the forward of a model that was given those statistics before it was frozen."""
    o = _oracle()
    gb = _gpu_batch(o["b"])
    run = lambda m: m(gb["mri"], gb["covars"], roi_pred_dicts=gb["roi_pred_dicts"], sample_roi_mask=gb["roi"])[0].detach().clone()
    gm = _model("switch")
    with torch.no_grad():
        out1 = run(gm)
    ptrs = [m.__dict__["_coma_frozen"]["mean"].data_ptr() for m in _bns(gm)]
    sd2 = {k: v.clone() for k, v in o["sd"].items()}
    for k in sd2:
        if k.endswith("running_mean"):
            sd2[k] = sd2[k] + 0.05
        elif k.endswith("running_var"):
            sd2[k] = sd2[k] * 1.3 + 0.01
    gm.load_state_dict(sd2, strict=True)
    assert gm.cfg.frozen_bn
    with torch.no_grad():
        out2 = run(gm)
        want = run(_model("idiom", sd=sd2))
    assert ptrs == [m.__dict__["_coma_frozen"]["mean"].data_ptr() for m in _bns(gm)]
    for m in _bns(gm):                                            # the tables hold exactly the new statistics
        ent = m.__dict__["_coma_frozen"]
        assert torch.equal(ent["mean"].view(-1), m.running_mean) and torch.equal(ent["rstd"].view(-1), torch.rsqrt(m.running_var + m.eps))
    # two forwards of one model differ by the order of the split-K merges (~1e-7): 1e-4, the loss bound of test_model_gpu.py
    assert rel(out2, want) < 1e-4, rel(out2, want)
    assert rel(out2, out1) > 1e-3


def test_mixed_gate_runs_piecewise_and_matches_oracle():
    """Only W_g's BatchNorm of every gate frozen (by the idiom, on both sides): the gates take the piecewise path, W_g's
    buffers stay, every other BatchNorm trains on batch statistics and moves its buffers as the oracle's do."""
    import coma_unet_amd as cu
    from coma_unet_amd.train import forward_loss
    from oracle.coma_oracle import build_reference_model
    from oracle.criterions_oracle import build_reference_criterion, train_step_loss
    o = _oracle()
    b = o["b"]
    om = build_reference_model(volume_shape=S)
    om.load_state_dict(o["sd"])
    om.set_save_attn(None)
    om.train(True)
    gm = _model(None)
    for m in (om, gm):
        hit = [x.eval() for n, x in m.named_modules() if n.endswith("attention.W_g.1")]
        assert len(hit) == 4
    o64 = copy.deepcopy(om).double()
    res = o64(b["mri"].double(), b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"].double())
    train_step_loss(res, b["tau"].double(), b["roi"].double(), b["covars"], build_reference_criterion())[0].backward()
    r32 = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
    tot = train_step_loss(r32, b["tau"], b["roi"], b["covars"], build_reference_criterion())[0]
    tot.backward()
    recs = _records(gm, _gpu_batch(b))
    assert not any(n.startswith("gate_frozen") for _k, n in recs)
    assert sum(n.startswith("norm_act_bwd_frozen_k") for _k, n in recs) == 4
    gm2 = _model(None)
    for n, x in gm2.named_modules():
        if n.endswith("attention.W_g.1"):
            x.eval()
    losses, outs = forward_loss(gm2, cu.build_reference_criterion(), _gpu_batch(b))
    losses[0].backward()
    torch.cuda.synchronize()
    assert rel(outs[0], r32[0]) < 1e-3 and abs(float(losses[0]) - float(tot)) / abs(float(tot)) < 1e-3
    # Gradients: 28 of the 32 BatchNorms train on the statistics of two volumes here, and in that regime single ill-conditioned
    # scalars (psi.1.bias, the merge PReLU slopes of the bottom levels) differ by 5e-2 ... 3e-1 between two runs of ONE step --
    # of the step as it was before this mode existed, too (the order of the fp32 split-K merges).  A per-tensor bound would test
    # that noise, so the rule of test_model_gpu.py is applied to the gradient as ONE vector over all parameters, and to the
    # tensors the frozen pieces themselves produce (W_g's BatchNorm affine pair and the W_g convolution bias in front of it).
    og, o32g = dict(o64.named_parameters()), dict(om.named_parameters())
    names = [n for n, p in gm2.named_parameters() if og[n].grad is not None]
    assert all((p.grad is None) == (og[n].grad is None) for n, p in gm2.named_parameters())
    cat = lambda f: torch.cat([f(n).detach().double().cpu().reshape(-1) for n in names])
    got, r64, r32 = cat(lambda n: dict(gm2.named_parameters())[n].grad), cat(lambda n: og[n].grad), cat(lambda n: o32g[n].grad)
    e, e_cpu = float((got - r64).norm() / r64.norm()), float((r32 - r64).norm() / r64.norm())
    print(f"mixed gate: whole gradient vs fp64 oracle: HIP fp32 {e:.2e}, CPU fp32 oracle {e_cpu:.2e}")
    assert e < max(3e-2, 4.0 * e_cpu), (e, e_cpu)
    gp = dict(gm2.named_parameters())
    for n in names:
        if "attention.W_g.1." in n or n.endswith("attention.W_g.0.conv.bias"):
            e, e_cpu = rel(gp[n].grad, og[n].grad), rel(o32g[n].grad, og[n].grad)
            print(f"  {n}: {e:.2e} (CPU fp32 {e_cpu:.2e})")
            assert e < max(3e-2, 4.0 * e_cpu), (n, e, e_cpu)
    osd, gsd = om.state_dict(), gm2.state_dict()
    for k, v in o["sd"].items():
        if "attention.W_g.1.running_" in k or "attention.W_g.1.num_batches" in k:
            assert torch.equal(gsd[k].cpu(), v) and torch.equal(osd[k], v), k
        elif "running_" in k:
            assert rel(gsd[k], osd[k]) < 1e-4 and not torch.equal(osd[k], v), k


def test_bf16_frozen_error_is_measured():
    """bf16 activations in the frozen mode: report the measured error instead of claiming the fp32 bound."""
    import coma_unet_amd as cu
    from coma_unet_amd.train import forward_loss
    o = _oracle()
    gm = _model("switch", dtype=torch.bfloat16)
    before = _buffers(gm)
    losses, outs = forward_loss(gm, cu.build_reference_criterion(), _gpu_batch(o["b"]))
    losses[0].backward()
    torch.cuda.synchronize()
    e = rel(outs[0].float(), o["out"])
    mae = float((outs[0].float().cpu() - o["out"]).abs().mean())
    print(f"bf16 frozen forward rel-L2 {e:.3e}, voxel MAE {mae:.3e}, loss {float(losses[0]):.5f} vs {o['total']:.5f}")
    assert e < 1e-1
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in gm.parameters())
    after = gm.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
