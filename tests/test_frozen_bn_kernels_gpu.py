"""The frozen-BatchNorm kernels against the fp64 restatements of tests/_frozen_plan.py: NormAct through a frozen BatchNorm
(coma_norm_act_fwd on the (mean, rstd) tables, norm_act_bwd_frozen_k) and the fused frozen gate (ops.GateFrozen:
gate_frozen_fwd_k / gate_frozen_bwd_k), past one block, one trip and one row chunk, on pitched tensors, with the running
statistics away from (0, 1).  test_frozen_bn_cpu.py asserts that every shape crosses what it is listed for.

Every output lives in a sentinel-guarded buffer, every element of every output is compared, and nothing is excluded: where a
pre-activation lies within its own rounding error of the activation's kink the bound grows by what the other branch moves.
Bounds have the form of test_nonconv_sizes_gpu._bound: u_out |ref| + (2 K 2^-24 + n 2^-53) A, with A the L1 mass of the terms
behind the element, K the fp32 roundings behind one term (counted from the kernel source at each call) and n the length of a
double-precision accumulation; bf16 tensors add one bf16 rounding of the mass per intermediate that is stored in bf16."""
import pytest
import torch
import torch.nn as nn

import _frozen_plan as FP
import _nonconv_plan as NP
from oracle import fp64_ref as R
from test_nonconv_sizes_gpu import DT, Guard, _bound, _free, _gen, _guarded_new, _ops, _pitched, _randn, _u

pytestmark = pytest.mark.gpu

REPORT = {}


def _frozen_bn(C, gen, grads=True):
    """An eval-mode nn.BatchNorm3d holder with running statistics away from (0, 1) -- the torch idiom."""
    bn = nn.BatchNorm3d(C).cuda()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=gen, device="cuda") * 0.5 + 0.3)
        bn.running_var.copy_(torch.rand(C, generator=gen, device="cuda") * 1.5 + 0.4)
        bn.weight.copy_(torch.rand(C, generator=gen, device="cuda") + 0.5)
        bn.bias.copy_(torch.randn(C, generator=gen, device="cuda") * 0.3)
        bn.num_batches_tracked.fill_(7)
    bn.weight.requires_grad_(grads)
    bn.bias.requires_grad_(grads)
    bn.eval()
    return bn


def _norm_frozen_case(V_or_dims, B, C, ld, act, grads, dt, tag):
    """layers.norm_act on an eval-mode BatchNorm3d inside a train-mode caller.  fp32 roundings behind one element, from the
    sources: the table rstd = rsqrt(running_var + eps) (the sum, rsqrt within 2 ulp: 3).  Forward (norm_act_fwd_k): sc = rstd
    gamma (1), sh = beta - mean sc (2), the fma (1), the activation's product (1), a margin of 2: K = 10 (+ 5 for the
    sigmoid's expf, sum, quotient).  Backward (norm_act_bwd_frozen_k): dz = dy act'(z) (1), gr = gamma rstd (1 + 3), dx = dz gr
    (1), a margin of 2: K = 8 (+ 6 for the sigmoid's derivative; what z's own error moves it by is part of the mass).  z =
    fma((x - mean) rstd, gamma, beta) carries K_Z = 8 roundings: where |z| <= 2 K_Z u mass the kernel may take the other
    branch and the bounds of dx and of the three sums grow by what that moves.  The sums add terms of xhat (5), dz (1) and
    their product (1) in double: K = 10 with the margin; bf16 sums 8 rows in fp32 first: K = 18."""
    ops, L = _ops()
    from coma_unet_amd import layers
    dtype, u = DT[dt], _u(DT[dt])
    dims = V_or_dims if isinstance(V_or_dims, tuple) else (1, 1, V_or_dims)
    xs = (B, *dims, C)
    gen = _gen("frozen_norm", tag)
    has_slope = act in ("prelu", "prelu_relu")
    x = _pitched(xs, ld, dtype, torch.randn(xs, generator=gen, device="cuda") * 1.5 + 0.7)
    dy = _randn(xs, gen, dtype)
    bn = _frozen_bn(C, gen, grads)
    slope = torch.tensor([-0.3 if act == "prelu_relu" else 0.2], device="cuda", requires_grad=grads) if has_slope else None
    ref = FP.norm_frozen64(x, dy, act, bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach(),
                           slope.detach() if slope is not None else None, bn.eps)
    run0 = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    cfg = layers.Config(compute_dtype=dtype)
    xg = x.detach().requires_grad_(True)
    align = 8 if dtype == torch.bfloat16 else 4
    yb = Guard(xs, dtype, ld + align, 0 if ld % align == 0 else 1)
    with _guarded_new(ops) as made:
        y = layers.norm_act(cfg, xg, bn, L.NORM_BATCH, NP.NORM_ACTS.index(act), slope, True, yb.t)
        y.backward(dy)
        torch.cuda.synchronize()
    assert yb.untouched() and len(made) >= 1 and all(g.untouched() for g in made)
    assert torch.equal(bn.running_mean, run0[0]) and torch.equal(bn.running_var, run0[1]) and torch.equal(bn.num_batches_tracked, run0[2])
    assert "_coma_frozen" in bn.__dict__                           # the (mean, rstd) tables of the holder were used
    sig = act == "sigmoid"
    st = {"y": R.check_elementwise(y, ref["y"], _bound(ref["y"], ref["mag_y"], 10 + 5 * sig, u), "y")}
    near = (ref["z"].abs() <= 2 * FP.K_Z * R.U_F32 * ref["mag_y"]).double()
    st["kinks"] = int(near.sum()) if act not in ("none", "sigmoid") else 0
    st["dx"] = R.check_elementwise(xg.grad, ref["dx"], _bound(ref["dx"], ref["mag_dx"], 8 + 6 * sig, u) + near * ref["kink"], "dx")
    nrow = x.numel() // C
    km = ref["kink_mass"](near)
    Ks = 10 + (8 if dtype == torch.bfloat16 else 0)
    for nm, p_ in (("dgamma", bn.weight), ("dbeta", bn.bias), ("dslope", slope)):
        if p_ is None:
            continue
        if not grads:
            assert p_.grad is None, nm
            continue
        st[nm] = R.check_elementwise(p_.grad, ref[nm], _bound(ref[nm], ref["mass"][nm], Ks, R.U_F32, nrow) + km[nm], nm)
    REPORT[f"frozen_norm-{tag}"] = st


@pytest.mark.parametrize("row", [r for r in NP.norm_f32_rows() if r[3] == "batch"], ids=lambda r: "-".join(str(v) for v in r[:3]))
def test_norm_frozen_f32_ragged_rows(row):
    """fp32, C in {1, 3, 16, 32, 96}, vec 4 and vec 1, pitched x: 5 row chunks with a short last one, and past the 1024-chunk
    cap with a ragged last chunk."""
    V, C, ld, _mode, act, _affine, _rows = row
    try:
        _norm_frozen_case(V, 2, C, ld, act, True, "f32", "-".join(str(v) for v in row[:3]))
    finally:
        _free()


def test_norm_frozen_f32_big():
    """81^3 x 32: every block walks its 519-row chunk in several bursts."""
    dims, B, C = NP.NORM_BIG
    try:
        _norm_frozen_case(dims, B, C, C + 4, "relu", True, "f32", "big")
    finally:
        _free()


@pytest.mark.parametrize("grads", [True, False], ids=["grads", "stream"])
@pytest.mark.parametrize("case", FP.FROZEN_BF16, ids=lambda c: f"c{c[1]}-ld{c[2]}")
def test_norm_frozen_bf16(case, grads):
    """bf16 twins: 16-byte vectors in the pure streaming form (no parameter gradient wanted), 8-byte ones with the sums."""
    V, C, ld, act = case
    try:
        _norm_frozen_case(V, 2, C, ld, act, grads, "bf16", f"bf16-{V}-{C}-{ld}-{grads}")
    finally:
        _free()


@pytest.mark.parametrize("grads", [True, False], ids=["grads", "stream"])
@pytest.mark.parametrize("act", NP.NORM_ACTS)
def test_norm_frozen_every_activation(act, grads):
    """All six activation codes, with the parameter gradients and as the pure streaming pass."""
    V, C, ld = FP.FROZEN_ACT_SHAPE
    try:
        _norm_frozen_case(V, 2, C, ld, act, grads, "f32", f"act-{act}-{grads}")
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# GateFrozen
# ---------------------------------------------------------------------------------------------------------------------
GATE_SUMS = (("dgam_g", "bn_g", "weight"), ("dbet_g", "bn_g", "bias"), ("dgam_x", "bn_x", "weight"), ("dbet_x", "bn_x", "bias"),
             ("dw", "conv", "weight"), ("db", "conv", "bias"), ("dgam_p", "bn_p", "weight"), ("dbet_p", "bn_p", "bias"))


def _gate_piecewise(ops, L, layers, cfg, mods, x, g1raw, x1raw, out):
    """The piecewise composition the model runs under COMA_FUSED_GATE=0 behind the two raw products."""
    g1 = layers.norm_act(cfg, g1raw, mods["bn_g"], L.NORM_BATCH, L.ACT_NONE, None, True)
    x1 = layers.norm_act(cfg, x1raw, mods["bn_x"], L.NORM_BATCH, L.ACT_NONE, None, True)
    s = ops.AddRelu.apply(g1, x1)
    psi = layers.norm_act(cfg, layers.conv_plain(cfg, s, mods["conv"], 1, 1, False), mods["bn_p"], L.NORM_BATCH, L.ACT_SIGMOID, None, True)
    return ops.GateMul.apply(x, psi, ops.Out(out)), psi


@pytest.mark.parametrize("case", FP.GATE_FROZEN, ids=lambda c: c[0])
def test_gate_frozen(case):
    """ops.GateFrozen with att written into the first C channels of a 2C-wide buffer and dx accumulated onto a Gaussian base
    (a GradFork buffer), against gate_frozen64 and against the piecewise path.  fp32 roundings behind one element, from
    gate.hip: the tables rstd_g, rstd_x (3 each), scg, scx (2), sh (5), the two fma's of t (2): 15 behind t -- where |t| <= 2 . 15 u
    mass the relu mask may differ and the bounds of dg1raw / dx1raw and of their sums grow by what the masked term moves;
    psi_raw: F fma's over the lanes and their tree (F + 1); a_p, b_p (7); the fma and the sigmoid (5); the product with x (1):
    K = F + 29 for att, psi and dx (+ 1 for the accumulate).  The backward adds the dot over C channels (C), dzp (3), dpr (1),
    d (1), the scaled outputs (1 + 4): K = C + F + 40 for dg1raw / dx1raw; the sums add 16 voxels in fp32 before they go to
    double: K = C + F + 56.  bf16: psi is stored in bf16 and read back by every consumer: one bf16 rounding of the mass.
    The piecewise path stores g1, x1, s, psi_raw, psi and, backward, dpsi, d(psi_raw), ds and d(g1) = d(x1): nine more
    roundings (bf16 ones on bf16 tensors) behind its outputs, three of them (g1, x1, their sum) behind the t its relu sees."""
    ops, L = _ops()
    from coma_unet_amd import layers
    name, dims, B, C, F_, dt, vec = case
    dtype, u = DT[dt], _u(DT[dt])
    bf = dtype == torch.bfloat16
    gen = _gen("gate_frozen", name)
    xs, fs = (B, *dims, C), (B, *dims, F_)
    al = 8 if bf else 4
    try:
        if vec == 1:      # channel slices at an odd offset: the scalar form
            mk = lambda shape, scale=1.0: Guard(shape, dtype, shape[-1] + 2, 1, fill=3.0e4).t.copy_(torch.randn(shape, generator=gen, device="cuda") * scale)
        else:
            mk = lambda shape, scale=1.0: _pitched(shape, shape[-1] + al, dtype, torch.randn(shape, generator=gen, device="cuda") * scale)
        x, g1, x1 = mk(xs), mk(fs, 1.3), mk(fs, 0.8)
        datt = _randn(xs, gen, dtype)
        base = _randn(xs, gen, dtype)
        mods = {"bn_g": _frozen_bn(F_, gen), "bn_x": _frozen_bn(F_, gen), "bn_p": _frozen_bn(1, gen), "conv": nn.Conv3d(F_, 1, 1).cuda()}
        with torch.no_grad():
            mods["conv"].weight.copy_(torch.randn(mods["conv"].weight.shape, generator=gen, device="cuda") * 0.5)
            mods["conv"].bias.copy_(torch.rand(1, generator=gen, device="cuda") * 0.4 - 0.2)
        P = dict(gam_g=mods["bn_g"].weight, bet_g=mods["bn_g"].bias, gam_x=mods["bn_x"].weight, bet_x=mods["bn_x"].bias,
                 w=mods["conv"].weight.reshape(-1), b=mods["conv"].bias, gam_p=mods["bn_p"].weight, bet_p=mods["bn_p"].bias)
        S = dict(rm_g=mods["bn_g"].running_mean, rv_g=mods["bn_g"].running_var, rm_x=mods["bn_x"].running_mean,
                 rv_x=mods["bn_x"].running_var, rm_p=mods["bn_p"].running_mean, rv_p=mods["bn_p"].running_var)
        ref = FP.gate_frozen64(x, g1, x1, {k: v.detach() for k, v in P.items()}, S, datt)
        run0 = {k: v.clone() for k, v in S.items()}
        cfg = layers.Config(compute_dtype=dtype)
        got = {}
        for path in ("fused", "piecewise"):
            for m in mods.values():
                m.zero_grad(set_to_none=True)
            xg, g1g, x1g = (t.detach().requires_grad_(True) for t in (x, g1, x1))
            fork = ops.GradFork()
            dxb = Guard(xs, dtype, C + al, 0)
            dxb.t.copy_(base)
            fork.buf = dxb.t
            xg._coma_fork = fork
            ab = Guard(xs, dtype, 2 * C, 0)                     # att: the first C channels of the concat buffer
            with _guarded_new(ops) as made:
                if path == "fused":
                    assert ops.gate_frozen_ok(xg, g1g, x1g, ab.t)
                    stats = tuple(layers.frozen_stats(mods[k]) for k in ("bn_g", "bn_x", "bn_p"))
                    att, psi = ops.GateFrozen.apply(xg, g1g, x1g, P["gam_g"], P["bet_g"], P["gam_x"], P["bet_x"], mods["conv"].weight,
                                                    mods["conv"].bias, P["gam_p"], P["bet_p"], stats, ops.Out(ab.t))
                    att.backward(datt)
                    dx = fork.buf
                    assert xg.grad is None and dx is dxb.t      # accumulated in place, handed to the fork
                else:
                    xg._coma_fork = None                          # (GateMul returns its gradient: added to the base here)
                    att, psi = _gate_piecewise(ops, L, layers, cfg, mods, xg, g1g, x1g, ab.t)
                    att.backward(datt)
                    dx = (base.float() + xg.grad.float()).to(dtype)
                torch.cuda.synchronize()
            assert ab.untouched() and dxb.untouched() and all(g.untouched() for g in made), path
            assert len(made) >= (3 if path == "fused" else 6), (path, len(made))      # fused: psi, dg1raw, dx1raw
            got[path] = dict(att=att.detach().clone(), psi=psi.detach().clone(), dx=dx.detach().clone(), dg1=g1g.grad.clone(), dx1=x1g.grad.clone(),
                             **{nm: getattr(mods[m], a).grad.reshape(-1).clone() for nm, m, a in GATE_SUMS})
            del ab, dxb, made
        assert all(torch.equal(S[k], run0[k]) for k in S)
        refdx = base.double() + ref["dx"]
        A_dx = base.double().abs() + ref["A_dx"]
        n = B * NP.vol(dims)
        ub = R.U_BF16 if bf else 0.0
        Kf, Kb = F_ + 29, C + F_ + 40

        def bounds(extra_k, stores, t_stores):
            """{output: bound}; extra_k more fp32 roundings and `stores` bf16-stored intermediates behind every quantity;
            t_stores of them behind t (the piecewise path forms s from the stored g1 and x1: its relu mask may differ
            wherever |t| is within those roundings)."""
            e = lambda A: stores * ub * A
            near = (ref["t"].abs() <= (2 * (15 + extra_k) * R.U_F32 + t_stores * ub) * ref["A_t"]).double()
            nm_ = ref["near_mass"](near)
            nearv = near.reshape(fs)
            b = {"att": _bound(ref["att"], ref["A_att"], Kf + extra_k, u) + e(ref["A_att"]),
                 "psi": _bound(ref["psi"], ref["A_psi"], Kf + extra_k, u) + e(ref["A_psi"]),
                 "dx": _bound(refdx, A_dx, Kf + 1 + extra_k, u) + e(A_dx)}
            for k in ("dg1", "dx1"):
                b[k] = _bound(ref[k], ref["A_" + k], Kb + extra_k, u) + e(ref["A_" + k]) + nearv * ref["kink_" + k]
            for k, _m, _a in GATE_SUMS:
                b[k] = _bound(ref[k], ref["m_" + k], Kb + 16 + extra_k, R.U_F32, n) + e(ref["m_" + k]) + nm_[k]
            return b, int(near.sum())

        (bf_, kinks), (bp_, kinks_pw) = bounds(0, 1, 0), bounds(9, 10, 3)
        want = {"att": ref["att"], "psi": ref["psi"], "dx": refdx, "dg1": ref["dg1"], "dx1": ref["dx1"], **{k: ref[k] for k, _m, _a in GATE_SUMS}}
        st = {"kinks": kinks, "kinks_pw": kinks_pw}
        for k, r_ in want.items():
            st[k] = R.check_elementwise(got["fused"][k].reshape(r_.shape), r_, bf_[k], f"fused {k}")
            st["pw_" + k] = R.check_elementwise(got["piecewise"][k].reshape(r_.shape), got["fused"][k].reshape(r_.shape).double(),
                                                bf_[k] + bp_[k], f"piecewise vs fused {k}")
        REPORT[f"gate_frozen-{name}"] = st
    finally:
        _free()


def test_zz_report():
    """Prints the measured worst ratio of every case that ran (to its bound)."""
    for k, v in REPORT.items():
        print("ROW", k, {a: (float(f"{b:.4g}") if isinstance(b, float) else b) for a, b in v.items()})
