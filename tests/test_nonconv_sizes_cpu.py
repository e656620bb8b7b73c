"""What test_nonconv_sizes_gpu.py rests on, checked without a GPU: that every shape of tests/_nonconv_plan.py really crosses
the boundary it is listed for (by the plain-Python mirrors of the launch arithmetic), that the caps the mirrors use are still
the ones in the .hip sources, and that each fp64 restatement agrees with an independent source on tiny inputs."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _nonconv_plan as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coma_unet_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------------
# the caps of the mirrors are the caps of the sources
# ---------------------------------------------------------------------------------------------------------------------
def test_cap_constants_still_in_the_sources():
    ew, me, no, nc, ga = (_src(n) for n in ("elementwise.hip", "metrics.hip", "norm.hip", "norm_common.h", "gate.hip"))
    T = NP.THREADS
    for text, needles in (
            (ew, [f"(total + {T - 1}) / {T}", f"if (nb > {NP.EW_CAP}) nb = {NP.EW_CAP};", f"#define LOSS_BLOCKS {NP.LOSS_BLOCKS}",
                  f"(V + {T} * 8 - 1) / ({T} * 8)", f"k += {NP.LOSS_FINALIZE_LANES}", f"if (gx > {NP.ZERO_GX}) gx = {NP.ZERO_GX};",
                  f"n > {NP.ZERO_GY} ? {NP.ZERO_GY} : n", f"ew_grid(vec4 ? (n + 3) / 4 : n)"]),
            (me, [f"(V + {T} * 16 - 1) / ({T} * 16)", f"if (nblk > {NP.EVAL_CAP}) nblk = {NP.EVAL_CAP};",
                  f"if (nb > {NP.EW_CAP}) nb = {NP.EW_CAP};"]),
            (nc, [f"p.ry * {NP.ROWS_PER_STEP}", f"{NP.ROWS_CAP} / p.G"]),
            (no, [f'"COMA_NORM_BLOCKS", {NP.NORM_BLOCKS}', f"constexpr int NORM_UNR = {NP.NORM_UNR};", f"k += {NP.LOSS_FINALIZE_LANES}",
                  "apply_blocks(p.V * p.cv, p.cv, NORM_UNR)", "apply_blocks(p.V * p.cv, p.cv, NORM_UNR / 2)"]),
            (ga, [f"{NP.GATE_MID_CAP} / g1->B", f"{NP.GATE_MID_CAP} / x->B", "gate_blocks(p.V, vpb * 2, cap)",
                  "gate_blocks(p.V, (256 / p.cv) * 2, cap)", f"gate_blocks(p.V * p.cv, 256 * 4, {NP.GATE_APPLY_CAP})",
                  f"gate_blocks(p.V * p.cv, 256 * 2, {NP.GATE_APPLY_CAP})"])):
        for n in needles:
            assert n in text, n


# ---------------------------------------------------------------------------------------------------------------------
# every case crosses its boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_elementwise_cases_pass_one_grid_pass():
    for name, dims, C, ldw, c_off, vec in NP.EW3_CASES:
        total = NP.vol(dims) * (C // vec)
        assert total > NP.EW_PASS and NP.ew_grid(total) == NP.EW_CAP and NP.passes(total, NP.ew_grid(total)) == 2, name
        assert total % NP.THREADS != 0, name                                      # a ragged last block
        assert (vec == 4) == (ldw % 4 == 0 and c_off % 4 == 0) and c_off + C <= ldw, name
    for name, dims, C, ldw, c_off, vec in NP.GATE_MUL_CASES:
        cv = C // vec
        total = NP.vol(dims) * cv
        assert cv <= 64 and cv & (cv - 1) == 0, name
        assert total > NP.EW_PASS and NP.passes(total, NP.ew_grid(total)) == 2, name
        assert (total % NP.THREADS == 0) == (name == "c32_even"), name            # dead lanes in the last block's shuffle
        assert (vec == 4) == (ldw % 4 == 0 and c_off % 4 == 0) and c_off + C <= ldw, name
    assert NP.vol(NP.GATE_MUL_CASES[1][1]) % 2 == 1
    for name, dims, C in NP.CAST_CASES:
        assert NP.vol(dims) * C > NP.EW_PASS, name
    assert {c[2] for c in NP.CAST_CASES} == {1, 3}                                # (cast_copy_k treats C == 1 apart)


def test_loss_eval_adamw_zero_cases():
    (mid, dm, _), (big, db, B) = NP.LOSS_CASES
    assert 2 < NP.loss_blocks(NP.vol(dm)) < NP.LOSS_FINALIZE_LANES and NP.vol(dm) % NP.LOSS_PER_BLOCK != 0
    V = NP.vol(db)
    assert V > NP.EW_PASS and V > NP.LOSS_BLOCKS * NP.LOSS_PER_BLOCK and B == 3
    assert NP.loss_blocks(V) == NP.LOSS_BLOCKS > NP.LOSS_FINALIZE_LANES and NP.passes(V, NP.LOSS_BLOCKS) > 8
    (_, d1, B1), (_, d2, B2) = NP.EVAL_CASES
    assert 1 < NP.eval_blocks(NP.vol(d1)) < NP.EVAL_CAP and B1 == 3
    assert NP.vol(d2) > NP.EVAL_CAP * NP.EVAL_PER_BLOCK and NP.eval_blocks(NP.vol(d2)) == NP.EVAL_CAP and B2 == 1
    (_, n4, o4), (_, n1, o1) = NP.ADAMW_CASES
    assert o4 == 0 and n4 % 4 == 3 and n4 // 4 > NP.EW_PASS and NP.ew_grid((n4 + 3) // 4) == NP.EW_CAP
    assert o1 % 4 != 0 and n1 > NP.EW_PASS and NP.ew_grid(n1) == NP.EW_CAP
    tab, n_buf, longest = NP.zero_ranges_table()
    gx, gy = NP.zero_grid(tab.shape[0], longest)
    assert tab.shape[0] > NP.ZERO_GY == gy and longest > NP.ZERO_GX * NP.THREADS and gx == NP.ZERO_GX
    assert int((tab[:, 1] == 0).sum()) > 10 and int((tab[:, 0] % 2 == 1).sum()) > 10
    ends = tab[:-1, 0] + tab[:-1, 1]
    assert bool((tab[1:, 0] > ends).all()) and int(tab[-1].sum()) < n_buf and int(tab[0, 0]) > 0      # sentinel cells between
    shape, spacing = NP.RESAMPLE_CASE
    out = [int(np.round(n * s / 2.0)) for n, s in zip(shape, spacing)]
    assert out[0] * out[1] * out[2] > NP.EW_PASS
    with open(os.path.join(ROOT, "tests", "test_input_pipeline.py")) as f:
        assert f"({shape}, {spacing})" in f.read()


def test_row_chunk_cases():
    B = 2
    for what, dt, C, ld, V in NP.colsum_rows(B):
        G = 1 if what == "bias" else B
        R_ = V * B if G == 1 else V
        vec = (8 if dt == "bf16" else 4) if (C % 8 == 0 and ld % 8 == 0) else 1
        p = NP.make_rows(R_, C, G, vec)
        cap = NP.ROWS_CAP // G
        assert p["nchunks"] > NP.LOSS_FINALIZE_LANES, (what, dt, C, V)         # colsum_finalize_k loops
        assert p["nchunks"] * p["ch"] > R_ >= (p["nchunks"] - 1) * p["ch"] + 1, (what, dt, C, V)   # ragged, non-empty last chunk
        assert p["nchunks"] == cap or NP.cdiv(R_, p["ry"] * NP.ROWS_PER_STEP) < cap
    caps = [NP.make_rows(V * B if w == "bias" else V, C, 1 if w == "bias" else B, 1)["nchunks"] for w, dt, C, ld, V in NP.colsum_rows(B) if C == 5]
    assert 1024 in caps and 512 in caps and min(caps) < 512
    rows = NP.norm_f32_rows(B)
    assert {r[1] for r in rows} == {1, 3, 16, 32, 96} and {NP.norm_f32_vec(r[1], r[2]) for r in rows} == {1, 4}
    for i, (V, C, ld, mode, act, affine, Rg) in enumerate(rows):
        G = 1 if mode == "batch" else B
        p = NP.make_rows(Rg, C, G, NP.norm_f32_vec(C, ld))
        assert p["nchunks"] * p["ch"] > Rg >= (p["nchunks"] - 1) * p["ch"] + 1, rows[i]
        assert p["nchunks"] == (5 if i % 2 == 0 else NP.ROWS_CAP // G), rows[i]
    assert {r[4] for r in rows} == set(NP.NORM_ACTS)
    # C = 3 and C = 96 make apply_blocks step its block count down to a multiple of the channel groups
    assert NP.apply_blocks(10 ** 7, 3, 4) % 3 == 0 and NP.apply_blocks(10 ** 7, 24, 4) % 3 == 0 and NP.apply_blocks(10 ** 7, 8, 4) == NP.NORM_BLOCKS


def test_apply_cap_cases():
    dims, B, C = NP.NORM_BIG
    V, cv = NP.vol(dims), C // 4
    assert V * cv > NP.NORM_BLOCKS * NP.THREADS * NP.NORM_UNR and NP.apply_blocks(V * cv, cv, NP.NORM_UNR) == NP.NORM_BLOCKS
    assert NP.apply_blocks(V * cv, cv, NP.NORM_UNR // 2) == NP.NORM_BLOCKS and V % 2 == 1
    for name, dims, B, C, F_, vec in NP.GATE_BIG:
        V, cvf, cvc = NP.vol(dims), F_ // vec, C // vec
        cap = NP.GATE_MID_CAP // B
        assert cvf <= 64 and cvc <= 64
        assert NP.cdiv(V, 2 * (256 // cvf)) > cap == NP.gate_blocks(V, 2 * (256 // cvf), cap), name          # mid forward
        assert NP.cdiv(V, 2 * (256 // cvc)) > cap, name                                                        # apply backward
        assert V * cvc > NP.GATE_APPLY_CAP * 256 * 4, name                                                     # apply forward
        assert V * cvf > NP.GATE_APPLY_CAP * 256 * 2, name                                                     # mid-backward apply
        assert NP.make_rows(V * B, F_, 1, vec)["nchunks"] > 500, name                                          # mid-backward partial: many chunks


# ---------------------------------------------------------------------------------------------------------------------
# the restatements against independent sources
# ---------------------------------------------------------------------------------------------------------------------
def test_adamw_recurrence_matches_torch_optim_in_double():
    g = torch.Generator().manual_seed(0)
    lr, b1, b2, eps, wd = (NP.f32(x) for x in NP.ADAMW_HP)
    p0 = torch.randn(1000, generator=g)
    pr = p0.double().clone().requires_grad_(True)
    opt = torch.optim.AdamW([pr], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    st = NP.adamw_init(p0)
    for t in range(1, 6):
        gr = torch.randn(1000, generator=g)
        pr.grad = gr.double()
        opt.step()
        info = NP.adamw_step(st, gr, t)
        assert float((st["p"] - pr.detach()).abs().max()) < 1e-13
        assert float((st["m"] - opt.state[pr]["exp_avg"]).abs().max()) < 1e-14
        assert float((st["v"] - opt.state[pr]["exp_avg_sq"]).abs().max()) < 1e-14
        # the bounds: positive, far below the update (lr), and the fp32 arithmetic of the step stays inside them
        assert 0 < float(st["bp"].max()) < 1e-5 and 0 <= info["bias_share"] <= 1
    # eps(bc): what fp32 1 - powf(beta, t) really loses stays below the stated relative error
    for b in (b1, b2):
        for t in range(1, 40):
            got = float(np.float32(1.0) - np.power(np.float32(b), np.float32(t)))
            bc1, bc2, e1, e2 = NP.adamw_bias_terms(b, b, t)
            assert abs(got - bc1) <= e1 * bc1
            assert abs(float(np.sqrt(np.float32(got))) - bc2 ** 0.5) <= e2 * bc2 ** 0.5


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def test_paint_and_loss_restatements_match_the_oracles():
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.roi_tables import ROI_INDICES, ROI_INDEX_TO_NAME
    from oracle.criterions_oracle import RoiMSE as ORoiMSE
    B, S = 3, (6, 7, 8)
    b = make_batch(B, S, seed=5)
    g = torch.Generator().manual_seed(1)
    pos, neg = torch.randn(S, generator=g), torch.randn(S, generator=g)
    prior = torch.tensor([[[d[ROI_INDEX_TO_NAME[i]]["loc"], d[ROI_INDEX_TO_NAME[i]]["std"]] for i in ROI_INDICES]
                          for d in b["roi_pred_dicts"]], dtype=torch.float32)
    abeta = torch.tensor([1.0, 0.0, 1.0])
    x = b["mri"].float()
    x[:, :, 0] = 0.0
    # the painting as attn_unet_data_parallel.py:630-651 writes it (the loop of tests/test_ops_gpu.py)
    suvr, sal = torch.zeros_like(x), torch.zeros_like(x)
    for bb in range(B):
        for i, idx in enumerate(ROI_INDICES):
            m = b["roi"][bb] == idx
            suvr[bb][m] = prior[bb, i, 0]
            sal[bb][m] = prior[bb, i, 1]
    suvr = torch.where(x < 1e-4, torch.zeros_like(suvr), suvr)
    sal = torch.where(x < 1e-4, torch.zeros_like(sal), sal)
    dyn = torch.stack([(pos if abeta[bb] == 1 else neg)[None] for bb in range(B)])
    want = _cl(torch.cat((dyn, sal, suvr), dim=1))
    got = NP.paint_ref(_cl(b["roi"].float()), _cl(x), prior, ROI_INDICES, abeta, pos, neg)
    assert torch.equal(got, want) and bool((want[..., 1] != 0).any())
    # RoiMSE: the oracle module and the reference's own numbers in the golden file
    w = torch.full((36,), 225.0)
    w[5] = 17.0
    pred = torch.rand((B, 1, *S), generator=g)
    orc = ORoiMSE(w.double(), ROI_INDICES)
    orc.batch_reduction = None
    lr_ = orc(pred.double(), b["tau"].double(), b["roi"].double())
    loss, mm, ms = NP.roi_mse_ref(_cl(pred), _cl(b["tau"].float()), _cl(b["roi"].float()), ROI_INDICES, w)
    assert float((loss - lr_.reshape(-1)).abs().max()) < 1e-12 * float(lr_.abs().max())
    gold = np.load(os.path.join(ROOT, "tests", "golden", "criterions_ref.npz"))
    gw = torch.from_numpy(gold["gcl_w"])
    for Bn in (1, 2, 3):
        t = lambda k: _cl(torch.from_numpy(gold[f"roimse{Bn}_{k}"]))
        loss, mm, ms = NP.roi_mse_ref(t("pred"), t("gt"), t("roi"), ROI_INDICES, gw)
        want = torch.from_numpy(gold[f"roimse{Bn}_loss"]).double().reshape(-1)
        assert float(((loss - want).abs() / want.abs()).max()) < 1e-5
        # the gradient the kernels are held to: gout * mask_mean * 2 / V * (pred - gt)
        gref = (t("pred").double() - t("gt").double()) * (mm * 2.0 / t("pred")[0].numel()).view(Bn, 1, 1, 1, 1)
        gwant = t("grad").double()
        assert float((gref - gwant).norm() / gwant.norm()) < 1e-5


def test_eval_stats_restatement_matches_the_metrics_oracle():
    from coma_unet_amd.synthetic import make_batch
    from coma_unet_amd.roi_tables import ROI_INDICES
    from oracle import metrics_oracle as mo
    B, S = 3, (12, 14, 16)
    b = make_batch(B, S, seed=0)
    g = torch.Generator().manual_seed(1)
    tau = b["tau"].double()
    pred = torch.clamp(tau + 0.2 * torch.randn(tau.shape, generator=g).double(), min=0.0)
    st, mass = NP.eval_stats_ref(_cl(pred), _cl(tau), _cl(b["roi"].float()), ROI_INDICES)
    assert bool((mass >= st.abs() - 1e-9).all())
    z = torch.zeros(len(ROI_INDICES), dtype=torch.float64)
    diff = pred - tau
    ref = mo.calc_roi_metrics(ROI_INDICES, None, z, z, z, z, z, tau, b["roi"].double(), pred, diff, torch.abs(diff / tau))
    r = st[:, :-1]
    n = r[..., 0]
    mine = ((r[..., 1] / n).sum(0), r[..., 6].sum(0), (r[..., 2] / (r[..., 4] - r[..., 3] ** 2 / n)).sum(0),
            torch.sqrt(r[..., 2] / r[..., 4]).sum(0), r[..., 7].sum(0))
    for name, a, w in zip(("mae", "mape", "rse", "wrrmse", "nonnan"), mine, ref):
        fin = torch.isfinite(w)
        assert torch.equal(fin, torch.isfinite(a)) and bool(fin.any()), name
        assert float(((a[fin] - w[fin]).abs() / (w[fin].abs() + 1e-12)).max()) < 1e-9, name
    gl = mo.batch_global_metrics(pred, tau)
    t = st[:, -1]
    V = float(n.new_tensor(S).prod())
    assert abs(float(t[:, 1].sum() / (B * V)) - float(gl["mae"])) < 1e-12
    assert abs(float(t[:, 6].sum() * 100) - float(gl["mape_sum"])) < 1e-9 * float(gl["mape_sum"]) and int(t[:, 7].sum()) == gl["mape_count"]
    assert abs(float((t[:, 2] / (t[:, 4] - t[:, 3] ** 2 / V)).mean()) - float(gl["rse"])) < 1e-10
    assert abs(float(torch.sqrt(t[:, 2] / t[:, 4]).mean()) - float(gl["rrmse"])) < 1e-12
    assert bool((t[:, 0] == V).all()) and abs(float(t[:, 5].sum()) - float(pred.sum())) < 1e-8


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


@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("act", NP.NORM_ACTS)
def test_norm_restatement_matches_torch_functional(act, mode):
    g = torch.Generator().manual_seed(len(act))
    B, C = 3, 5
    x = torch.randn((B, 4, 3, 6, C), generator=g, dtype=torch.float64) * 1.5 + 0.7
    dy = torch.randn(x.shape, generator=g, dtype=torch.float64)
    affine = mode == "batch"
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) if affine else None
    beta = torch.randn(C, generator=g, dtype=torch.float64) if affine else None
    slope = torch.tensor([-0.3 if act == "prelu_relu" else 0.2], dtype=torch.float64) if "prelu" in act else None
    mine = NP.norm_act64(x, dy, mode, act, gamma, beta, slope)
    xe = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    ps = [None if t is None else t.clone().requires_grad_(True) for t in (gamma, beta, slope)]
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    if mode == "batch":
        z = F.batch_norm(xe, rm, rv, ps[0], ps[1], True, 0.1, 1e-5)
    else:
        z = F.instance_norm(xe, None, None, None, None, True, 0.1, 1e-5)
    y = _act_f(z, act, ps[2])
    y.backward(dy.permute(0, 4, 1, 2, 3))
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    assert float((mine["y"] - cl(y.detach())).abs().max()) < 1e-12
    assert float((mine["dx"] - cl(xe.grad)).abs().max()) < 1e-12
    for nm, p_ in zip(("dgamma", "dbeta", "dslope"), ps):
        if p_ is not None:
            assert float((mine[nm] - p_.grad).abs().max()) < 1e-10, nm
    if mode == "batch":
        assert float((mine["running_mean"] - rm).abs().max()) < 1e-14 and float((mine["running_var"] - rv).abs().max()) < 1e-14
    assert bool((mine["mag_y"] >= mine["z"].abs() - 1e-12).all()) and bool((mine["mag_dx"] >= mine["dx"].abs() - 1e-12).all())
    for nm in ("dgamma", "dbeta", "dslope"):
        assert bool((mine["mass"][nm] >= mine[nm].abs() - 1e-12).all())


def test_gate_restatement_matches_torch_functional():
    g = torch.Generator().manual_seed(7)
    B, C, F_ = 2, 8, 4
    rn = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    x, g1, x1, datt = rn(B, 3, 4, 5, C), rn(B, 3, 4, 5, F_) * 1.3, rn(B, 3, 4, 5, F_) * 0.8, rn(B, 3, 4, 5, C)
    P = dict(gam_g=rn(F_).abs() + 0.5, bet_g=rn(F_) * 0.3, gam_x=rn(F_).abs() + 0.5, bet_x=rn(F_) * 0.3, w=rn(F_) * 0.5, b=rn(1) * 0.2,
             gam_p=rn(1).abs() + 0.5, bet_p=rn(1) * 0.3)
    mine = NP.gate64(x, g1, x1, P, datt)
    leaf = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    cf = lambda t: t.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    xe, ge, x1e = cf(x), cf(g1), cf(x1)
    run = {n: (torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)) for n, c in (("g", F_), ("x", F_), ("p", 1))}
    bn = lambda t, n, ga, be: F.batch_norm(t, run[n][0], run[n][1], ga, be, True, 0.1, 1e-5)
    s = F.relu(bn(ge, "g", leaf["gam_g"], leaf["bet_g"]) + bn(x1e, "x", leaf["gam_x"], leaf["bet_x"]))
    pr = F.conv3d(s, leaf["w"].view(1, F_, 1, 1, 1), leaf["b"])
    psi = torch.sigmoid(bn(pr, "p", leaf["gam_p"], leaf["bet_p"]))
    att = xe * psi
    att.backward(datt.permute(0, 4, 1, 2, 3))
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    tol = 1e-11
    assert float((mine["att"] - cl(att.detach())).abs().max()) < tol and float((mine["psi"] - cl(psi.detach())).abs().max()) < tol
    assert float((mine["dx"] - cl(xe.grad)).abs().max()) < tol
    assert float((mine["dg1"] - cl(ge.grad)).abs().max()) < tol and float((mine["dx1"] - cl(x1e.grad)).abs().max()) < tol
    for nm, key in (("dgam_g", "gam_g"), ("dbet_g", "bet_g"), ("dgam_x", "gam_x"), ("dbet_x", "bet_x"), ("dw", "w"),
                    ("dgam_p", "gam_p"), ("dbet_p", "bet_p")):
        assert float((mine[nm] - leaf[key].grad).abs().max()) < 1e-10, nm
        assert bool((mine["m_" + nm] >= mine[nm].abs() - 1e-12).all()), nm
    for n in ("g", "x", "p"):
        assert float((mine["rm_" + n] - run[n][0]).abs().max()) < 1e-13 and float((mine["rv_" + n] - run[n][1]).abs().max()) < 1e-12
    for a, v in (("A_att", "att"), ("A_dx", "dx"), ("A_dg1", "dg1"), ("A_dx1", "dx1")):
        assert bool((mine[a] >= 0).all()) and mine[a].shape == mine[v].shape
