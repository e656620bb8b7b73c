"""What the frozen-BatchNorm GPU tests rest on, checked without a GPU: the fp64 restatements of tests/_frozen_plan.py against
torch autograd, that every GPU shape crosses the boundary it is listed for (by the plain-Python mirrors of the new kernels'
launch arithmetic, whose constants are looked up in the sources), and the torch idiom itself on the CPU oracle: BatchNorm3d
modules in eval mode inside a train-mode model run forward and backward without moving a running buffer."""
import os

import pytest
import torch
import torch.nn.functional as F

import _frozen_plan as FP
import _nonconv_plan as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coma_unet_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _act_f(z, act, slope):
    if act == "none":
        return z
    if act == "relu":
        return F.relu(z)
    if act == "prelu":
        return F.prelu(z, slope)
    if act == "leaky":
        return F.leaky_relu(z, 0.01)
    if act == "sigmoid":
        return torch.sigmoid(z)
    return F.relu(F.prelu(z, slope))


# ---------------------------------------------------------------------------------------------------------------------
# the mirrors' constants are the sources'; every shape crosses what it claims
# ---------------------------------------------------------------------------------------------------------------------
def test_frozen_launch_constants_still_in_the_sources():
    no, ga = _src("norm.hip"), _src("gate.hip")
    for needle in ("constexpr int BURST = sizeof(T) == 2 ? 8 : 2, LD = 2;", "RowsP rp = make_rows(x, COMA_NORM_BATCH, vec);",
                   "if (!want && pick_vec8(x) == 8 && pick_vec8(dy) == 8 && pick_vec8(dx) == 8) vec = 8;",
                   "rec_add(bsums, brs, (int64_t)k * p.C, &sh[0][0], p.C);"):
        assert needle in no, needle
    for needle in (f"int cap = {FP.GATE_FROZEN_CAP} / x->B; if (cap < 1) cap = 1;", "gate_blocks(p.e.V, (256 / p.e.cv) * 2, cap)",
                   "gate_frozen_vec(x->dtype, ts, 7, x->C, g1raw->C, 4)", f"constexpr int U = {FP.GATE_FROZEN_U};"):
        assert needle in ga, needle


def test_frozen_norm_shapes_cross_their_boundaries():
    B = 2
    rows = [r for r in NP.norm_f32_rows(B) if r[3] == "batch"]
    assert {r[1] for r in rows} == {1, 3, 16, 32, 96}
    seen_vec, below, past = set(), 0, 0
    for V, C, ld, _mode, _act, _aff, R_ in rows:
        assert R_ == V * B
        vec = FP.frozen_vec("f32", C, (ld, C, C), True)          # x pitched, dy contiguous, dx in a buffer of its own pitch
        seen_vec.add(vec)
        p = FP.frozen_norm_plan(R_, C, vec, "f32")
        assert p["blocks"] > 1 and p["trips"] > 1 and p["ragged_last"], (V, C, p)
        below += p["blocks"] == 5
        past += p["blocks"] == NP.ROWS_CAP
        if C % 4:
            assert ld != C                                        # a pitched tensor
    assert seen_vec == {1, 4} and below == 5 and past == 5
    dims, Bb, C = NP.NORM_BIG
    p = FP.frozen_norm_plan(NP.vol(dims) * Bb, C, 4, "f32")
    assert p["blocks"] == NP.ROWS_CAP and p["trips"] > 4 and p["ragged_rows"]
    vecs = set()
    for V, C, ld, _act in FP.FROZEN_BF16:
        for sums in (True, False):
            vec = FP.frozen_vec("bf16", C, (ld, C, C), sums)
            vecs.add((vec, sums))
            p = FP.frozen_norm_plan(V * B, C, vec, "bf16")
            assert p["blocks"] > 1 and p["ragged_last"] and ld != C, (V, C, vec, p)
            assert p["trips"] > 1 or p["masked_burst"], (V, C, vec, p)
    assert {v for v, s in vecs if not s} == {8, 4} and {v for v, s in vecs if s} == {4}
    assert {c[1] for c in FP.FROZEN_BF16} == {8, 32}
    V, C, ld = FP.FROZEN_ACT_SHAPE
    p = FP.frozen_norm_plan(V * B, C, FP.frozen_vec("f32", C, (ld, C, C), True), "f32")
    assert p["blocks"] > 1 and p["trips"] > 1 and p["ragged_last"] and p["cv"] != p["cvp"] and ld != C


def test_frozen_gate_shapes_cross_their_boundaries():
    by = {c[0]: c for c in FP.GATE_FROZEN}
    assert [(c[1], c[2], c[3], c[4]) for c in FP.GATE_FROZEN[:2]] == [(c[1], c[2], c[3], c[4]) for c in NP.GATE_BIG]
    for name in ("vec4", "vec1", "bf16"):
        _n, dims, B, C, F_, dt, vec = by[name]
        p = FP.gate_frozen_plan(NP.vol(dims), B, C, F_, vec)
        assert p["blocks"] == FP.GATE_FROZEN_CAP // B and p["trips"] > 1 and p["ragged"] and p["cv"] <= 64, (name, p)
    _n, dims, B, C, F_, dt, vec = by["bf16"]
    p8 = FP.gate_frozen_plan(NP.vol(dims), B, C, F_, 8)           # the forward runs 8 wide
    assert p8["blocks"] == FP.GATE_FROZEN_CAP // B and p8["trips"] > 1 and (C, F_) == (64, 32)
    _n, dims, B, C, F_, dt, vec = by["wide"]
    p = FP.gate_frozen_plan(NP.vol(dims), B, C, F_, vec)
    assert (dims, B, C, F_) == ((5, 6, 7), 2, 256, 128) and p["cv"] == 64 and p["blocks"] > 1 and p["half_live"], p


# ---------------------------------------------------------------------------------------------------------------------
# the restatements against torch autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("act", NP.NORM_ACTS)
def test_norm_frozen_restatement_matches_torch_autograd(act, affine):
    g = torch.Generator().manual_seed(len(act) + 10 * affine)
    B, C = 3, 5
    x = torch.randn((B, 4, 3, 6, C), generator=g, dtype=torch.float64) * 1.5 + 0.7
    dy = torch.randn(x.shape, generator=g, dtype=torch.float64)
    rm = torch.randn(C, generator=g, dtype=torch.float64) * 0.5 + 0.4
    rv = torch.rand(C, generator=g, dtype=torch.float64) * 2.0 + 0.3
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) if affine else None
    beta = torch.randn(C, generator=g, dtype=torch.float64) if affine else None
    slope = torch.tensor([-0.3 if act == "prelu_relu" else 0.2], dtype=torch.float64) if "prelu" in act else None
    mine = FP.norm_frozen64(x, dy, act, rm, rv, gamma, beta, slope)
    xe = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    ps = [None if t is None else t.clone().requires_grad_(True) for t in (gamma, beta, slope)]
    rm0, rv0 = rm.clone(), rv.clone()
    y = _act_f(F.batch_norm(xe, rm, rv, ps[0], ps[1], False, 0.1, 1e-5), act, ps[2])
    y.backward(dy.permute(0, 4, 1, 2, 3))
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    assert float((mine["y"] - cl(y.detach())).abs().max()) < 1e-12
    assert float((mine["dx"] - cl(xe.grad)).abs().max()) < 1e-12
    for nm, p_ in zip(("dgamma", "dbeta", "dslope"), ps):
        if p_ is not None:
            assert float((mine[nm] - p_.grad).abs().max()) < 1e-10, nm
    assert bool((mine["mag_y"] >= mine["z"].abs() - 1e-12).all()) and bool((mine["mag_dx"] >= mine["dx"].abs() - 1e-12).all())
    for nm in ("dgamma", "dbeta", "dslope"):
        assert bool((mine["mass"][nm] >= mine[nm].abs() - 1e-12).all()), nm
    km = mine["kink_mass"](torch.ones_like(x))
    assert all(bool((km[nm] >= 0).all()) and km[nm].shape == mine[nm].shape for nm in km)


def test_gate_frozen_restatement_matches_torch_autograd():
    g = torch.Generator().manual_seed(11)
    B, C, F_ = 2, 8, 4
    rn = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    x, g1, x1, datt = rn(B, 3, 4, 5, C), rn(B, 3, 4, 5, F_) * 1.3, rn(B, 3, 4, 5, F_) * 0.8, rn(B, 3, 4, 5, C)
    P = dict(gam_g=rn(F_).abs() + 0.5, bet_g=rn(F_) * 0.3, gam_x=rn(F_).abs() + 0.5, bet_x=rn(F_) * 0.3, w=rn(F_) * 0.5, b=rn(1) * 0.2,
             gam_p=rn(1).abs() + 0.5, bet_p=rn(1) * 0.3)
    S = dict(rm_g=rn(F_) * 0.4, rv_g=rn(F_).abs() + 0.3, rm_x=rn(F_) * 0.4, rv_x=rn(F_).abs() + 0.3, rm_p=rn(1) * 0.2, rv_p=rn(1).abs() + 0.3)
    mine = FP.gate_frozen64(x, g1, x1, P, S, datt)
    leaf = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    cf = lambda t: t.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    xe, ge, x1e = cf(x), cf(g1), cf(x1)
    S0 = {k: v.clone() for k, v in S.items()}
    bn = lambda t, n, ga, be: F.batch_norm(t, S["rm_" + n], S["rv_" + n], ga, be, False, 0.1, 1e-5)
    s = F.relu(bn(ge, "g", leaf["gam_g"], leaf["bet_g"]) + bn(x1e, "x", leaf["gam_x"], leaf["bet_x"]))
    pr = F.conv3d(s, leaf["w"].view(1, F_, 1, 1, 1), leaf["b"])
    psi = torch.sigmoid(bn(pr, "p", leaf["gam_p"], leaf["bet_p"]))
    att = xe * psi
    att.backward(datt.permute(0, 4, 1, 2, 3))
    assert all(torch.equal(S[k], S0[k]) for k in S)
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    tol = 1e-11
    assert float((mine["att"] - cl(att.detach())).abs().max()) < tol and float((mine["psi"] - cl(psi.detach())).abs().max()) < tol
    assert float((mine["dx"] - cl(xe.grad)).abs().max()) < tol
    assert float((mine["dg1"] - cl(ge.grad)).abs().max()) < tol and float((mine["dx1"] - cl(x1e.grad)).abs().max()) < tol
    for nm, key in (("dgam_g", "gam_g"), ("dbet_g", "bet_g"), ("dgam_x", "gam_x"), ("dbet_x", "bet_x"), ("dw", "w"), ("db", "b"),
                    ("dgam_p", "gam_p"), ("dbet_p", "bet_p")):
        assert float((mine[nm] - leaf[key].grad.reshape(mine[nm].shape)).abs().max()) < 1e-10, nm
        assert bool((mine["m_" + nm] >= mine[nm].abs() - 1e-12).all()), nm
    for a, v in (("A_att", "att"), ("A_dx", "dx"), ("A_dg1", "dg1"), ("A_dx1", "dx1"), ("kink_dg1", "dg1"), ("kink_dx1", "dx1")):
        assert bool((mine[a] >= 0).all()) and mine[a].shape == mine[v].shape
    assert bool((mine["A_dg1"] >= mine["dg1"].abs() - 1e-12).all()) and bool((mine["A_att"] >= mine["att"].abs() - 1e-12).all())
    nm_ = mine["near_mass"](torch.ones_like(mine["t"]))
    assert all(nm_[k].shape == mine[k].shape for k in nm_)


# ---------------------------------------------------------------------------------------------------------------------
# the idiom on the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_idiom_leaves_the_running_buffers_alone():
    """BatchNorm3d modules in eval mode inside the train-mode oracle at 32^3 x 2: forward, loss and backward run, every
    BatchNorm's affine parameters get a gradient, and no running buffer or step counter moves."""
    from coma_unet_amd.synthetic import make_batch
    from oracle.coma_oracle import build_reference_model
    from oracle.criterions_oracle import build_reference_criterion, train_step_loss
    S = (32, 32, 32)
    torch.manual_seed(321)
    om = build_reference_model(volume_shape=S)
    om.set_save_attn(None)
    om.train(True)
    with torch.no_grad():                                         # the running statistics away from (0, 1)
        w = make_batch(2, S, seed=5)
        om(w["mri"], w["covars"], roi_pred_dicts=w["roi_pred_dicts"], sample_roi_mask=w["roi"])
    bns = [m for m in om.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    assert len(bns) == 32                                          # 2 + 8 block, 12 gate, 10 projection-head BatchNorms
    for m in bns:
        m.eval()
    assert om.training
    before = {k: v.clone() for k, v in om.state_dict().items() if "running_" in k or "num_batches_tracked" in k}
    assert len(before) == 3 * len(bns) and any(float(v.float().abs().max()) not in (0.0, 1.0) for v in before.values())
    b = make_batch(2, S, seed=9)
    res = om(b["mri"], b["covars"], roi_pred_dicts=b["roi_pred_dicts"], sample_roi_mask=b["roi"])
    train_step_loss(res, b["tau"], b["roi"], b["covars"], build_reference_criterion())[0].backward()
    after = om.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    used = [m for m in bns if m.weight.grad is not None]
    assert len(used) >= 22 and all(bool(torch.isfinite(m.weight.grad).all()) for m in used)
