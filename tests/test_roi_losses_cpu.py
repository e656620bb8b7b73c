"""What the ROI-weighted loss tests rest on, checked without a GPU: the fp64 restatement of tests/_roi_loss_plan.py against
the golden arrays the reference's own RoiRSE / RoiRRMSE produced (tests/make_roi_loss_golden.py), the kernels' one-pass
denominators against the two-pass ones, the launch-arithmetic mirror against the source and the cases against the
boundaries they are listed for, and the constructor / argument errors of the three classes."""
import os

import numpy as np
import pytest
import torch

import _roi_loss_plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "roi_losses_ref.npz")


def _gold():
    return np.load(GOLD)


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def test_golden_file_is_what_the_plan_describes():
    g = _gold()
    from coma_unet_amd.roi_tables import ROI_INDICES
    assert os.path.getsize(GOLD) < 100 * 1024
    assert g["roi_ids"].tolist() == list(ROI_INDICES)
    w = g["weights"]
    assert w.dtype == np.float64 and sorted(set(w.tolist())) == [7.5, 100.0, 225.0] and (w != 225.0).sum() == 2
    for B in P.GOLDEN_B:
        pred, gt, roi = P.golden_inputs(B, ROI_INDICES)
        for name, t in (("pred", pred), ("gt", gt), ("roi", roi)):
            a = g[f"in{B}_{name}"]
            assert a.dtype == np.float64 and a.shape == (B, 1) + P.GOLDEN_DIMS and np.array_equal(a, t.numpy()), (B, name)
        for t in (pred, gt):       # bf16-exact: one fixture serves every dtype
            assert torch.equal(t.to(torch.bfloat16).double(), t) and float(t.min()) >= 0 and float(t.max()) < 4
        labels = set(roi.reshape(-1).tolist())
        assert labels <= set(float(i) for i in ROI_INDICES) | set(float(i) for i in P.OTHER_LABELS)
    labels3 = set(torch.from_numpy(g["in3_roi"]).reshape(-1).tolist())
    assert set(float(i) for i in P.OTHER_LABELS) <= labels3


@pytest.mark.parametrize("B", P.GOLDEN_B)
@pytest.mark.parametrize("name", ["rse", "rrmse"])
def test_restatement_equals_the_reference_classes(name, B):
    g = _gold()
    kind = P.KINDS[name]
    ids, w = g["roi_ids"].tolist(), torch.from_numpy(g["weights"])
    pred, gt, roi = (torch.from_numpy(g[f"in{B}_{k}"]) for k in ("pred", "gt", "roi"))
    for red in ("mean", "sum"):
        gout = torch.full((B,), 1.0 / B if red == "mean" else 1.0, dtype=torch.float64)
        loss, coef, grad, den = P.loss_coef_grad64(kind, pred, gt, roi, ids, w, gout)
        tot = loss.mean() if red == "mean" else loss.sum()
        assert abs(float(tot) - float(g[f"{name}{B}_{red}"])) <= 1e-12 * abs(float(g[f"{name}{B}_{red}"]))
        assert _rel(grad, g[f"{name}{B}_grad_{red}"]) <= 1e-12
        # the closed form the backward kernel uses: coef w d
        closed = (gout * coef).view(B, 1, 1, 1, 1) * P.mask64(roi, ids, w) * (pred - gt)
        assert _rel(closed, g[f"{name}{B}_grad_{red}"]) <= 1e-12


@pytest.mark.parametrize("weights", ["mixed", "unit"])
def test_one_pass_denominators_equal_two_pass(weights):
    g = _gold()
    ids = g["roi_ids"].tolist()
    w = torch.from_numpy(g["weights"]) if weights == "mixed" else torch.ones(len(ids), dtype=torch.float64)
    for B in P.GOLDEN_B:
        gt, roi = torch.from_numpy(g[f"in{B}_gt"]), torch.from_numpy(g[f"in{B}_roi"])
        for kind in P.KINDS.values():
            two = P.terms64(kind, gt, gt, roi, ids, w)[1]
            one = P.one_pass_den64(kind, gt, roi, ids, w)
            assert _rel(one, two) <= 1e-12, (kind, B, _rel(one, two))
    if weights == "unit":       # m is the true mean: RSE's denominator is the plain sum of squares about it
        gt = torch.from_numpy(g["in3_gt"])
        flat = gt.reshape(3, -1)
        ref = ((flat - flat.mean(1, keepdim=True)) ** 2).sum(1)
        assert _rel(P.one_pass_den64(P.RSE, gt, torch.from_numpy(g["in3_roi"]), ids, w), ref) <= 1e-12


def test_mirror_constants_are_the_sources():
    with open(os.path.join(ROOT, "coma_unet_amd", "csrc", "roi_loss.hip")) as f:
        src = f.read()
    for needle in (f"RWL_BLOCKS = {P.RWL_BLOCKS}", "RWL_PER_BLOCK = 256 * 8", f"RWL_REC = {P.RWL_REC}",
                   "(V + RWL_PER_BLOCK - 1) / RWL_PER_BLOCK", f"i += {P.FINALIZE_LANES}", f"if (nb > {P.BWD_CAP}) nb = {P.BWD_CAP};",
                   "((v4 ? (p.V + 3) / 4 : p.V) + 255) / 256", "t->ld == 1 && t->sb % 4 == 0",
                   "(size_t)pred->B * RWL_BLOCKS * RWL_REC * sizeof(double)", "p.V >> 2"):
        assert needle in src, needle
    assert P.RWL_PER_BLOCK == 256 * 8 and P.ws_bytes(3) == 3 * 512 * 4 * 8
    # same grid arithmetic as loss_partial_k (tests/_nonconv_plan.py)
    import _nonconv_plan as NP
    for V in (1, 210, 2048, 2049, 36960, 1048576, 1056768, 2097152):
        assert P.fwd_blocks(V) == NP.loss_blocks(V)


def test_cases_cross_their_boundaries():
    cases = {c[0]: c for c in P.CASES}
    assert set(cases) >= {"tail", "mid", "cap", "pitched"}
    for es in (4, 2):
        _, dims, B, lay = cases["tail"]
        L = P.case_layout(dims, B, lay, es)
        V = P.vol(dims)
        assert dims == (5, 6, 7) and B == 3 and V == 210 and V % 4 != 0 and not L["vec"] and P.fwd_blocks(V) == 1 and V < P.THREADS
        assert L["pred"][1] % 4 != 0                      # misaligned sample strides
        _, dims, B, lay = cases["vtail"]
        L = P.case_layout(dims, B, lay, es)
        assert L["vec"] and P.vol(dims) % 4 == 2 and L["pred"][1] == 212
        _, dims, B, lay = cases["mid"]
        L = P.case_layout(dims, B, lay, es)
        V = P.vol(dims)
        assert dims == (32, 33, 35) and B == 3 and L["vec"] and 2 < P.fwd_blocks(V) < P.FINALIZE_LANES
        assert P.fwd_trips(V, True) == 2 and P.fwd_trips(V, False) == 8 and V % P.RWL_PER_BLOCK != 0
        assert not P.vec4_ok(1, V, 1)                     # the same volume one element off its base: scalar path
        _, dims, B, lay = cases["cap"]
        L = P.case_layout(dims, B, lay, es)
        V = P.vol(dims)
        assert dims == (64, 128, 129) and B == 2 and L["vec"] and V == 1056768 > P.RWL_BLOCKS * P.RWL_PER_BLOCK
        assert P.fwd_blocks(V) == P.RWL_BLOCKS and P.finalize_trips(V) == 8 > 1
        assert P.fwd_trips(V, True) == 3 and P.fwd_trips(V - P.RWL_PER_BLOCK * 8, True) == 2      # just past a trip boundary
        assert P.bwd_blocks(V, True) < P.BWD_CAP                                             # (one backward pass: 1032 blocks)
        _, dims, B, lay = cases["pitched"]
        L = P.case_layout(dims, B, lay, es)
        assert dims == cases["mid"][1] and B == 3 and not L["vec"] and L["pred"][0] * es == 16 and L["gt"][0] == 1
        assert P.fwd_trips(P.vol(dims), False) == 8


def test_bounds_sit_under_the_ceilings():
    V = P.vol((64, 128, 129))
    for kind in P.KINDS.values():
        assert P.rel_bound(P.K_LOSS[kind], V, amp=8.0) < P.LOSS_REL
        assert P.U_F32 + 2 * P.K_GRAD[kind] * P.U_F32 < P.GRAD_REL_L2[torch.float32]


def test_constructor_and_argument_errors():
    import coma_unet_amd as cu
    from coma_unet_amd import criterions as C
    from coma_unet_amd.roi_tables import ROI_INDICES
    w = torch.full((len(ROI_INDICES),), 225.0)
    for cls in (cu.RoiRSE, cu.RoiRRMSE, cu.RoiWeightedMSE):
        m = cls(w, ROI_INDICES)
        assert m.reduction == "mean" and m.batch_reduction == "mean" and m.voxel_wise is False and m.voxel_weights is None
        assert m.roi_indices is ROI_INDICES and m.roi_weights is w and m.scale_factor == 360
        m.batch_reduction = None
        assert m.reduction is None
        m.reduction = "sum"
        assert m.batch_reduction == "sum"
        assert cls(w, ROI_INDICES, None).batch_reduction is None and cls(w, ROI_INDICES, reduction="sum").reduction == "sum"
        new = m.calculate_new_weights(torch.rand(len(ROI_INDICES)), with_update=True)
        assert new.shape == w.shape and abs(float(new.norm()) - 360.0) < 1e-3 and m.roi_weights is w
        with pytest.raises(ValueError, match="reduction"):
            cls(w, ROI_INDICES, reduction="max")
        with pytest.raises(ValueError, match="weights"):
            cls(w[:5], ROI_INDICES)
        with pytest.raises(ValueError, match="ROI indices"):
            cls(torch.ones(65), list(range(65)))
        with pytest.raises(ValueError, match="ROI indices"):
            cls(torch.ones(0), [])
        z = torch.zeros(2, 1, 4, 4, 4)
        with pytest.raises(ValueError, match="ROI label volume"):
            m(z, z, None)
        with pytest.raises(ValueError, match="equal shape"):
            m(z, z[:, :, :3], z)
        with pytest.raises(ValueError, match="equal shape"):
            m(z[:, 0], z[:, 0], z[:, 0])
    with pytest.raises(TypeError):
        cu.RoiRSE(w, ROI_INDICES, "mean", 2.0)            # the reference's constructor: no background weight
    with pytest.raises(ValueError, match="background_weight"):
        cu.RoiWeightedMSE(w, ROI_INDICES, background_weight=float("nan"))
    assert cu.RoiWeightedMSE(w, ROI_INDICES, background_weight=0.0).background_weight == 0.0
    with pytest.raises(ValueError, match="gen_loss"):
        C.build_reference_criterion("cpu", gen_loss="roi_mae")
    for name, cls in (("roi_mse", cu.RoiMSE), ("roi_rse", cu.RoiRSE), ("roi_rrmse", cu.RoiRRMSE), ("roi_wmse", cu.RoiWeightedMSE)):
        crit = C.build_reference_criterion("cpu", gen_loss=name)
        assert type(crit.gen_loss) is cls and crit.gen_loss.batch_reduction is None
    assert type(C.build_reference_criterion("cpu").gen_loss) is cu.RoiMSE
    ws = cu.WithSSIM(cu.RoiRRMSE(w, ROI_INDICES), 0.5)
    ws.batch_reduction = None
    assert ws.base.reduction is None and ws.roi_weights is w and ws.voxel_wise is False
