"""What the ROI-mean loss tests rest on, checked without a GPU: the fp64 restatement of tests/_roi_mean_plan.py against the
oracle's ROI means, its autograd gradient against the closed form the backward kernel uses, the launch-arithmetic mirror
against the source and the cases against the boundaries they are listed for, the margins the inputs are built to keep, and
the constructor / wrapper behaviour of the Python classes (no kernel is called)."""
import os

import numpy as np
import pytest
import torch

import _roi_mean_plan as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c[0]: c for c in P.CASES}
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _rounded(case, pattern, tab, dtype):
    pred, gt, roi, ids, w = P.make_inputs(case, pattern, tab)
    return pred.to(dtype).double(), gt.to(dtype).double(), roi, ids, w


def test_restatement_equals_the_oracle_roi_means():
    """At unit weights the "mse" loss is the mean over present regions of (mean pred - mean gt)^2 of RoiCorrMetric's means."""
    from oracle.metrics_oracle import RoiCorrMetric
    pred, gt, roi, ids, _ = _rounded(CASES["tail"], "random", "roi36", torch.float32)
    to5 = lambda t: t.permute(0, 4, 1, 2, 3)
    m = RoiCorrMetric(ids)
    m.acc_roi_corr(to5(pred), to5(gt), to5(roi).double())
    pm, gm = np.array(m.pred_means, dtype=np.float64), np.array(m.gt_means, dtype=np.float64)      # (n_roi, B); nan where absent
    here = ~np.isnan(pm)
    assert here.sum() > 90 and here.shape == (36, 3)
    ref = np.array([np.mean(((pm - gm) ** 2)[here[:, b], b]) for b in range(3)])
    got = P.loss64(P.MSE, pred, gt, roi, ids, torch.ones(36, dtype=torch.float64))
    assert float(np.abs(got.numpy() - ref).max() / np.abs(ref).max()) <= 1e-12
    cnt, pm2, gm2 = P.region_means64(pred, gt, roi, ids)
    assert np.allclose(pm2.numpy().T[here], pm[here], rtol=1e-13, atol=0) and np.allclose(gm2.numpy().T[here], gm[here], rtol=1e-13, atol=0)
    assert bool(((cnt.numpy().T > 0) == here).all())


@pytest.mark.parametrize("kind", list(P.KINDS))
@pytest.mark.parametrize("pattern,tab", [("random", "randw"), ("absent", "roi36"), ("fractional", "wide64"), ("none", "roi36"),
                                         ("single", "one")])
def test_autograd_gradient_equals_the_closed_form(kind, pattern, tab):
    pred, gt, roi, ids, w = _rounded(CASES["tail"], pattern, tab, torch.float32)
    gout = torch.tensor([1.0, -2.0, 0.37], dtype=torch.float64)
    loss, coef, grad, (cnt, d) = P.loss_coef_grad64(P.KINDS[kind], pred, gt, roi, ids, w, gout)
    closed = P.closed_grad64(coef, gout, roi, ids)
    assert float((closed - grad).abs().max()) <= 1e-13 * max(float(grad.abs().max()), 1e-300)
    assert bool(torch.equal(closed == 0, grad == 0))
    if pattern == "none":
        assert float(loss.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0 and float(cnt.max()) == 0.0
    else:
        assert float(loss.min()) > 0.0
    if tab == "wide64":                        # the later copy of a duplicated id owns no voxel; the id past 4096 does
        assert float(cnt[:, P.DUP_SLOT].max()) == 0.0 and float(cnt[:, 3].min()) > 0 and float(cnt[:, 36].min()) > 0
        assert ids[36] == P.BIG_ID >= 4096 and ids[P.DUP_SLOT] == ids[3] and len(ids) == 64
        assert bool((roi == P.BIG_ID).any()) and bool((roi != roi.round()).any())         # fractional labels present
    if pattern == "absent":                    # a third of the table never occurs but for one voxel in sample 1
        assert int((cnt[0] == 0).sum()) == 12 and int((cnt[1] == 0).sum()) == 11 and int((cnt[1] == 1).sum()) == 1
    if tab == "randw":
        assert int((w == 0).sum()) == 2 and float(w.min()) == 0.0


def test_mirror_constants_are_the_sources():
    with open(os.path.join(ROOT, "coma_unet_amd", "csrc", "roi_mean.hip")) as f:
        src = f.read()
    for needle in (f"RM_BLOCKS = {P.RM_BLOCKS}", "RM_PER_BLOCK = 256 * 8", f"RM_WAVE_VOX = {P.RM_WAVE_VOX}", f"RM_SLOTS = {P.RM_SLOTS}",
                   "RM_REC = 3 * RM_SLOTS", f"RM_FIN_PARTS = {P.FIN_PARTS}", f"RM_BWD_BLOCKS = {P.BWD_CAP}",
                   "(V + RM_PER_BLOCK - 1) / RM_PER_BLOCK", "(int64_t)gridDim.x * 4 * RM_WAVE_VOX", "i += RM_FIN_PARTS",
                   "((v4 ? (p.V + 3) / 4 : p.V) + 255) / 256", "t->ld == 1 && t->sb % 4 == 0",
                   "(size_t)pred->B * RM_BLOCKS * RM_REC * sizeof(double)", "__launch_bounds__(256) void roi_mean_partial_k"):
        assert needle in src, needle
    for banned in ("atomicAdd", "atomic_", "atomicMin", "atomicMax", "atomicCAS"):     # the point of the kernel: no atomics of any kind
        assert banned not in src, banned
    assert P.RM_PER_BLOCK == 256 * 8 and P.RM_REC == 192 and P.ws_bytes(3) == 3 * 512 * 192 * 8
    with open(os.path.join(ROOT, "coma_unet_amd", "build.py")) as f:
        assert '"roi_mean.hip"' in f.read()


def test_cases_cross_their_boundaries():
    assert set(CASES) >= {"tail", "vtail", "mid", "cap", "pitched"}
    for es in (4, 2):
        _, dims, B, lay = CASES["tail"]
        V = P.vol(dims)
        assert V == 210 and V % 4 != 0 and not P.case_layout(dims, B, lay, es)["vec"] and P.fwd_blocks(V) == 1 and P.fwd_trips(V) == 1
        assert V < P.RM_WAVE_VOX                               # under one wave's trip: three waves of the block idle
        _, dims, B, lay = CASES["vtail"]
        assert P.case_layout(dims, B, lay, es)["vec"] and P.vol(dims) % 4 == 2          # a partly valid 4-voxel group
        _, dims, B, lay = CASES["mid"]
        V = P.vol(dims)
        assert P.case_layout(dims, B, lay, es)["vec"] and P.fwd_blocks(V) == 19 and P.fwd_trips(V) == 2 and V % P.RM_PER_BLOCK != 0
        assert 1 < P.finalize_trips(V) == 2 and P.fwd_blocks(V) % P.FIN_PARTS != 0     # uneven parts in the finalise
        assert not P.vec4_ok(1, V, 1)                          # the same volume one element off its base: scalar path
        _, dims, B, lay = CASES["cap"]
        V = P.vol(dims)
        assert P.case_layout(dims, B, lay, es)["vec"] and V > P.RM_BLOCKS * P.RM_PER_BLOCK and P.fwd_blocks(V) == P.RM_BLOCKS
        assert P.fwd_trips(V) == 3 and P.fwd_trips(V - P.RM_PER_BLOCK * 8) == 2 and P.finalize_trips(V) == 32
        assert P.bwd_blocks(V, True) < P.BWD_CAP
        _, dims, B, lay = CASES["pitched"]
        L = P.case_layout(dims, B, lay, es)
        assert dims == CASES["mid"][1] and not L["vec"] and L["pred"][0] * es == 16 and L["gt"][0] == 1
    for c in P.CASES:
        V = P.vol(c[1])
        assert P.sum_chain(V) + P.REF_CHAIN <= V or V == 210, c[0]      # what lets the statistics be held to V 2^-53
    combos = P.case_combos()
    assert {p for _, p, _ in combos} == set(P.PATTERNS) and {t for _, _, t in combos} == set(P.TABLES)
    assert {c[0] for c, _, _ in combos} == set(CASES)


def test_bounds_sit_under_the_ceilings():
    V = P.vol(CASES["cap"][1])
    assert P.scalar_bound(V, amp=P.AMP_MAX) < P.LOSS_REL
    assert P.K_CAST * P.U_F32 <= 2 * P.U_F32 and P.f64_terms(V, P.AMP_MAX) < 1e-10
    assert P.grad_bound(V, P.AMP_MAX, torch.float32) <= 4 * P.U_F32 + 1e-10
    assert P.grad_bound(V, P.AMP_MAX, torch.bfloat16) <= P.U_BF16 + 4 * P.U_F32 + 1e-10
    assert P.stats_bound(V) == V * P.U_F64


def _margins(case, pattern, tab, dt):
    pred, gt, roi, ids, w = _rounded(case, pattern, tab, DT[dt])
    cnt, pm, gm = P.region_means64(pred, gt, roi, ids)
    here = cnt > 0
    d = (pm - gm)[here].abs()
    return d, here, P.amplification(pred, gt, roi, ids)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_inputs_keep_their_margins(dt):
    """On the rounded inputs the restatement sees: every present region's |d| >= 1e-3 (the "l1" sign cannot flip) and
    ||d| - delta| >= 1e-3 (nor the huber branch), both huber branches are populated, `none` has nothing present, and the
    amplification the bounds use stays under the AMP_MAX the ceilings were checked at."""
    small = [c for c in P.case_combos() if c[0][0] in ("tail", "mid")]         # (vtail / pitched share these values)
    big = [c for c in P.case_combos() if c[0][0] == "cap"][:2]
    for case, pattern, tab in small + big:
        d, here, amp = _margins(case, pattern, tab, dt)
        what = (case[0], pattern, tab)
        if pattern == "none":
            assert d.numel() == 0, what
            continue
        assert d.numel() > 0 and float(d.min()) >= 1e-3 and float((d - P.DELTA).abs().min()) >= 1e-3, what
        assert amp <= P.AMP_MAX, (what, amp)
        if d.numel() >= 12:
            assert bool((d < P.DELTA).any()) and bool((d > P.DELTA).any()), what


def test_constructor_and_argument_errors():
    import coma_unet_amd as cu
    from coma_unet_amd import criterions as C
    from coma_unet_amd.roi_tables import ROI_INDICES
    w = torch.full((len(ROI_INDICES),), 225.0)
    m = cu.RoiMeanLoss(w, ROI_INDICES)
    assert m.reduction == "mean" and m.batch_reduction == "mean" and m.kind == "mse" and m.delta == 1.0
    assert m.roi_indices is ROI_INDICES and m.roi_weights is w
    m.batch_reduction = None
    assert m.reduction is None
    m.reduction = "sum"
    assert m.batch_reduction == "sum"
    assert cu.RoiMeanLoss(w, ROI_INDICES, "huber", 0.15, None).batch_reduction is None
    for bad, match in ((dict(reduction="max"), "reduction"), (dict(kind="l2"), "kind"), (dict(kind="huber", delta=0.0), "delta"),
                       (dict(kind="huber", delta=float("inf")), "delta"), (dict(kind="huber", delta=float("nan")), "delta")):
        with pytest.raises(ValueError, match=match):
            cu.RoiMeanLoss(w, ROI_INDICES, **bad)
    with pytest.raises(ValueError, match="weights"):
        cu.RoiMeanLoss(w[:5], ROI_INDICES)
    with pytest.raises(ValueError, match="ROI indices"):
        cu.RoiMeanLoss(torch.ones(65), list(range(65)))
    with pytest.raises(ValueError, match="ROI indices"):
        cu.RoiMeanLoss(torch.ones(0), [])
    z = torch.zeros(2, 1, 4, 4, 4)
    with pytest.raises(ValueError, match="ROI label volume"):
        m(z, z, None)
    with pytest.raises(ValueError, match="equal shape"):
        m(z, z[:, :, :3], z)
    base = cu.RoiMSE(w, ROI_INDICES)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="roi_mean_weight"):
            cu.WithRoiMean(base, bad)
    with pytest.raises(ValueError, match="batch_reduction"):
        cu.WithRoiMean(torch.nn.MSELoss(), 1.0)
    with pytest.raises(ValueError, match="both"):
        cu.WithRoiMean(base, 1.0, roi_weights=w)
    with pytest.raises(ValueError, match="ROI tables"):
        cu.WithRoiMean(cu.VoxelL1(), 1.0)
    with pytest.raises(ValueError, match="kind"):
        cu.WithRoiMean(base, 1.0, kind="l2")
    own = cu.WithRoiMean(cu.VoxelL1(), 1.0, roi_weights=w[:3], roi_indices=ROI_INDICES[:3])
    assert own.roi_mean.roi_weights.shape == (3,) and not own.live_tables
    assert cu.WithRoiMean(base, 0.0).roi_mean_weight == 0.0
    crit = C.build_reference_criterion("cpu", roi_mean_weight=0.25)
    assert type(crit.gen_loss) is cu.WithRoiMean and type(crit.gen_loss.base) is cu.RoiMSE and crit.gen_loss.batch_reduction is None
    assert crit.gen_loss.roi_mean_weight == 0.25 and crit.gen_loss.roi_mean.kind == "mse"
    assert type(C.build_reference_criterion("cpu").gen_loss) is cu.RoiMSE          # default: untouched


@pytest.mark.parametrize("order", ["mean_over_ssim", "ssim_over_mean"])
def test_attribute_forwarding_through_both_nestings(order):
    import coma_unet_amd as cu
    from coma_unet_amd.roi_tables import ROI_INDICES
    w = torch.full((len(ROI_INDICES),), 225.0)
    base = cu.RoiMSE(w, ROI_INDICES)
    if order == "mean_over_ssim":
        top = cu.WithRoiMean(cu.WithSSIM(base, 0.5), 0.25, kind="huber", delta=0.15)
        rm = top
    else:
        rm = cu.WithRoiMean(base, 0.25, kind="huber", delta=0.15)
        top = cu.WithSSIM(rm, 0.5)
    assert rm.roi_mean.kind == "huber" and rm.roi_mean.delta == 0.15 and rm.roi_mean.batch_reduction is None and rm.live_tables
    assert top.batch_reduction == "mean" and top.roi_weights is w and top.roi_indices is ROI_INDICES
    assert top.voxel_wise is False and top.voxel_weights is None and top.scale_factor == 360
    top.batch_reduction = None                                  # one shared attribute, all the way down
    assert base.batch_reduction is None and rm.batch_reduction is None and top.batch_reduction is None
    w2 = torch.ones(len(ROI_INDICES))
    top.roi_weights = w2
    assert base.roi_weights is w2 and rm.roi_weights is w2
    new = top.calculate_new_weights(torch.rand(len(ROI_INDICES)), with_update=True)
    assert new.shape == w2.shape and abs(float(new.norm()) - 360.0) < 1e-3 and top.update_weights(new) is None
    assert "roi_weights" not in rm.__dict__ and "batch_reduction" not in rm.__dict__
    assert [type(m_).__name__ for m_ in top.modules()].count("WithRoiMean") == 1


def test_train_loop_wraps_once_and_updates_in_place():
    import coma_unet_amd as cu
    from coma_unet_amd import criterions as C
    from coma_unet_amd.train_loop import with_roi_mean, with_ssim
    crit = C.build_reference_criterion("cpu")
    g0 = crit.gen_loss
    assert with_roi_mean(crit, None) is crit and crit.gen_loss is g0                # off: nothing is touched
    with_roi_mean(crit, 0.5, dict(kind="l1"))
    with_ssim(crit, 0.1)
    assert type(crit.gen_loss) is cu.WithSSIM and type(crit.gen_loss.base) is cu.WithRoiMean and crit.gen_loss.base.base is g0
    rm = crit.gen_loss.base
    with_roi_mean(crit, 0.75)
    with_ssim(crit, 0.2)
    assert crit.gen_loss.base is rm and rm.roi_mean_weight == 0.75 and rm.roi_mean.kind == "l1" and crit.gen_loss.ssim_weight == 0.2
    assert crit.gen_loss.batch_reduction is None and crit.gen_loss.roi_indices is g0.roi_indices
    # a criterion that already carries the SSIM wrapper: the term goes below it, and both are found again
    crit = C.build_reference_criterion("cpu")
    g0 = crit.gen_loss
    with_ssim(crit, 0.1)
    top = crit.gen_loss
    with_roi_mean(crit, 0.5)
    with_ssim(crit, 0.3)
    with_roi_mean(crit, 0.6)
    assert crit.gen_loss is top and type(top.base) is cu.WithRoiMean and top.base.base is g0
    assert top.ssim_weight == 0.3 and top.base.roi_mean_weight == 0.6
    assert [type(m_).__name__ for m_ in top.modules()].count("WithRoiMean") == 1
