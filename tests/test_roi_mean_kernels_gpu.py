"""coma_roi_mean_fwd / coma_roi_mean_bwd / coma_roi_region_stats (csrc/roi_mean.hip) through the C ABI: the cases x label
patterns x tables of tests/_roi_mean_plan.py x {fp32, bf16} x every kind, against the fp64 restatement evaluated on the very
same stored inputs.

Paths (asserted from the mirrored launch arithmetic in test_roi_mean_cpu.py):
  tail     V = 210, B = 3, dense: one block, one wave busy, sample stride no multiple of 4 -> SCALAR path
  vtail    the same volume at sample stride 212 -> VECTOR path, the last 4-voxel group half valid
  mid      (32, 33, 35), B = 3, dense -> VECTOR path, 19 blocks, 2 trips, 2 finalise trips over uneven parts
  cap      (64, 128, 129), B = 2 -> VECTOR path, the 512-block cap, 3 trips, 32 finalise trips
  pitched  mid's shape, pred / dpred at the 16-byte voxel pitch -> SCALAR path; pitch padding untouched
  mid, one element off its base (test_scalar_and_vector_paths_agree) -> SCALAR path on dense input

Bounds: counted from the kernel source (P.scalar_bound / P.grad_bound / P.stats_bound): loss and coef within 2 u + the fp64
terms (and the loss under 1e-6), the statistics within V 2^-53 with exact counts, dpred within 4 u (+ 2^-8 for bf16) per voxel,
exact zeros exact.  Everything is run twice and must repeat bitwise."""
import gc

import pytest
import torch

import _roi_mean_plan as P
from oracle import fp64_ref as R
from test_nonconv_sizes_gpu import Guard, _pitched
from test_roi_losses_kernels_gpu import Buf

pytestmark = pytest.mark.gpu

SENT = -7.0
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GOUT = [1.0, -2.0, 0.37]


def _L():
    from coma_unet_amd import _lib
    return _lib


def _inputs(case, pattern, tab, dtype, off=0):
    """-> pred, gt, roi views (values rounded to dtype), a maker of guarded dpred buffers, ids, w (fp32 cuda), vector path?"""
    name, dims, B, lay = case
    es = 2 if dtype == torch.bfloat16 else 4
    lo = P.case_layout(dims, B, lay, es)
    pv, gtv, lab, ids, w = P.make_inputs(case, pattern, tab)
    shape = (B, *dims, 1)
    if lay == "pitched":
        pred = _pitched(shape, lo["pred"][0], dtype, pv.cuda())
        mk_dp = lambda: Guard(shape, dtype, lo["pred"][0], 0)
    else:
        pb = Buf(B, dims, dtype, *lo["pred"], off, fill=3.0e4)
        pb.t.copy_(pv.cuda())
        pred = pb.t
        mk_dp = lambda: Buf(B, dims, dtype, *lo["pred"], off)
    gb, rb = Buf(B, dims, dtype, *lo["gt"], off, fill=3.0e4), Buf(B, dims, torch.float32, *lo["roi"], off, fill=17.0)
    gb.t.copy_(gtv.cuda())
    rb.t.copy_(lab.cuda())
    return pred, gb.t, rb.t, mk_dp, ids, w.float().cuda(), lo["vec"] and off % 4 == 0


def _ws(L, pred):
    return L.workspace(L.lib.coma_roi_mean_ws_bytes(L.ct(pred)), pred.device)


def _fwd(L, pred, gt, roi, ids_t, w, kind, delta=P.DELTA):
    B, n = pred.shape[0], ids_t.numel()
    res = torch.full((64 + B + B * n + 64,), SENT, device="cuda")
    loss, coef = res[64:64 + B], res[64 + B:64 + B + B * n].view(B, n)
    ws = _ws(L, pred)
    L.check(L.lib.coma_roi_mean_fwd(L.ct(pred), L.ct(gt), L.ct(roi), L.ptr(ids_t), L.ptr(w), n, kind, delta,
                                    L.ptr(loss), L.ptr(coef), L.ptr(ws), ws.numel(), L.stream()), "roi_mean_fwd")
    assert bool((res[:64] == SENT).all()) and bool((res[64 + B + B * n:] == SENT).all())
    return loss, coef


def _stats(L, pred, gt, roi, ids_t):
    B, n = pred.shape[0], ids_t.numel()
    res = torch.full((64 + B * n * 3 + 64,), SENT, dtype=torch.float64, device="cuda")
    st = res[64:64 + B * n * 3].view(B, n, 3)
    ws = _ws(L, pred)
    L.check(L.lib.coma_roi_region_stats(L.ct(pred), L.ct(gt), L.ct(roi), L.ptr(ids_t), n, L.ptr(st), L.ptr(ws), ws.numel(),
                                        L.stream()), "roi_region_stats")
    assert bool((res[:64] == SENT).all()) and bool((res[64 + B * n * 3:] == SENT).all())
    return st


def _bwd(L, roi, ids_t, gout, coef, dp):
    L.check(L.lib.coma_roi_mean_bwd(L.ct(roi), L.ptr(ids_t), ids_t.numel(), L.ptr(gout), L.ptr(coef), L.ct(dp.t), L.stream()),
            "roi_mean_bwd")
    assert dp.untouched()
    return dp.t


def _rel(got, ref):
    """max relative error over the non-zero reference entries; the zero ones must be exactly zero"""
    got, ref = got.double(), ref.double()
    zero = ref == 0
    assert bool((got[zero] == 0).all())
    return float(((got - ref).abs()[~zero] / ref.abs()[~zero]).max()) if bool((~zero).any()) else 0.0


def _check_stats(L, pred, gt, roi, ids, ids_t, what):
    V = pred[0].numel()
    st, st2 = _stats(L, pred, gt, roi, ids_t), _stats(L, pred, gt, roi, ids_t)
    assert torch.equal(st, st2), what                                            # bitwise repeatable
    cnt, sp, sg = P.region_sums64(pred, gt, roi, ids)
    assert torch.equal(st[..., 0], cnt), what                                    # counts are exact
    ep, eg = _rel(st[..., 1], sp), _rel(st[..., 2], sg)
    print(f"{what}: stats rel err sum pred {ep:.3e} sum gt {eg:.3e} (bound {P.stats_bound(V):.3e})")
    assert ep <= P.stats_bound(V) and eg <= P.stats_bound(V), (what, ep, eg)
    return st


def _check_kind(L, kind, pred, gt, roi, mk_dp, ids, ids_t, w, dtype, amp, what):
    """forward twice, backward twice, against the restatement.  -> (loss, coef, dpred)."""
    B, V = pred.shape[0], pred[0].numel()
    gout = torch.tensor(GOUT[:B], device="cuda")
    loss, coef = _fwd(L, pred, gt, roi, ids_t, w, kind)
    loss2, coef2 = _fwd(L, pred, gt, roi, ids_t, w, kind)
    assert torch.equal(loss, loss2) and torch.equal(coef, coef2), what          # bitwise repeatable
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(coef).all()), what
    lref, cref, gref, (cnt, d) = P.loss_coef_grad64(kind, pred, gt, roi, ids, w.double(), gout)
    here = cnt > 0
    if bool(here.any()):                                                         # the margins the bounds rest on
        assert float(d[here].abs().min()) >= 1e-3 and float((d[here].abs() - P.DELTA).abs().min()) >= 1e-3, what
    lerr, cerr = _rel(loss, lref), _rel(coef, cref)
    sb = P.scalar_bound(V, amp)
    print(f"{what}: loss rel err {lerr:.3e} coef rel err {cerr:.3e} (bound {sb:.3e}, amp {amp:.1f})")
    assert lerr <= min(sb, P.LOSS_REL) and cerr <= sb, (what, lerr, cerr, sb)
    dp = _bwd(L, roi, ids_t, gout, coef, mk_dp())
    dp2 = _bwd(L, roi, ids_t, gout, coef, mk_dp())
    assert torch.equal(dp, dp2), what
    assert torch.equal(dp == 0, gref == 0), what                                 # the exact zeros are exact
    worst = R.check_elementwise(dp, gref, P.grad_bound(V, amp, dtype) * gref.abs(), what + " dpred")
    print(f"{what}: dpred worst element / bound {worst:.3f}")
    return loss, coef, dp


def _run(L, case, pattern, tab, dtype, off=0, what=""):
    pred, gt, roi, mk_dp, ids, w, vec = _inputs(case, pattern, tab, dtype, off)
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    amp = P.amplification(pred, gt, roi, ids)
    assert amp <= P.AMP_MAX
    st = _check_stats(L, pred, gt, roi, ids, ids_t, what)
    outs = [_check_kind(L, kind, pred, gt, roi, mk_dp, ids, ids_t, w, dtype, amp, f"{what}-{n}") for n, kind in P.KINDS.items()]
    return st, outs, (pred, gt, roi, mk_dp, ids_t, w, vec)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case,pattern,tab", P.case_combos(), ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_loss_coef_gradient_and_stats_vs_fp64(case, pattern, tab, dt):
    L = _L()
    try:
        st, outs, (pred, gt, roi, _, ids_t, w, vec) = _run(L, case, pattern, tab, DT[dt], what=f"{case[0]}-{pattern}-{tab}-{dt}")
        assert vec == (case[0] in ("vtail", "mid", "cap"))                       # the path this case takes
        if pattern == "none":                                                    # nothing present: exactly 0, never NaN
            assert float(st.abs().max()) == 0.0
            for loss, coef, dp in outs:
                assert float(loss.abs().max()) == 0.0 and float(coef.abs().max()) == 0.0 and float(dp.abs().max()) == 0.0
        else:
            assert all(float(loss.min()) > 0.0 for loss, _, _ in outs)
        if pattern == "absent":                                                  # the one-voxel region, and the absent third
            assert int((st[1, :, 0] == 1).sum()) == 1 and int((st[0, :, 0] == 0).sum()) == 12
        if pattern == "fractional":
            assert bool((roi != roi.round()).any())
        if tab == "wide64" and pattern != "blocks":                              # the id past the 4096-entry table has voxels
            assert float(st[:, 36, 0].min()) > 0 and float(st[:, P.DUP_SLOT, 0].max()) == 0.0
    finally:
        gc.collect()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_scalar_and_vector_paths_agree(dt):
    """The same dense `mid` input 16-byte aligned (vector path) and one element off (scalar path): each within its bounds, and
    -- both paths give a lane the same four voxels, so they add in the same order -- bitwise equal to each other."""
    L = _L()
    case = next(c for c in P.CASES if c[0] == "mid")
    V = P.vol(case[1])
    res = []
    for off in (0, 1):
        res.append(_run(L, case, "random", "wide64", DT[dt], off, what=f"mid+{off}-{dt}"))
        pred, vec = res[-1][2][0], res[-1][2][6]
        assert vec == (off == 0) and (pred.data_ptr() % 16 == 0) == (off == 0)
    (sv, ov, _), (ss, os_, (_, _, roi_s, mk_dp, ids_t, _, _)) = res
    assert torch.equal(sv[..., 0], ss[..., 0])
    assert _rel(sv[..., 1], ss[..., 1]) <= 2 * P.stats_bound(V) and _rel(sv[..., 2], ss[..., 2]) <= 2 * P.stats_bound(V)
    gout = torch.tensor(GOUT[:3], device="cuda")
    for (lv, cv, dv), (ls, cs, _) in zip(ov, os_):
        sb = 2 * P.scalar_bound(V, P.AMP_MAX)
        assert _rel(lv, ls) <= sb and _rel(cv, cs) <= sb
        assert torch.equal(sv, ss) and torch.equal(lv, ls) and torch.equal(cv, cs)
        d2 = _bwd(L, roi_s, ids_t, gout, cv.clone(), mk_dp())                    # the scalar path from the VECTOR path's coef
        assert torch.equal(d2, dv)


@pytest.mark.parametrize("pattern", ["blocks", "random"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_region_stats_equal_eval_stats(dt, pattern):
    """roi_region_stats against the evaluation kernel's per-ROI bins: counts (slot 0) exactly, sum pred (slot 5) and sum gt
    (slot 3) within V 2^-53."""
    L = _L()
    from coma_unet_amd import metrics as M, ops
    case = next(c for c in P.CASES if c[0] == "mid")
    V = P.vol(case[1])
    pred, gt, roi, _, ids, _, _ = _inputs(case, pattern, "roi36", DT[dt])
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    st = ops.roi_region_stats(pred, gt, roi, ids_t)
    assert torch.equal(st, _stats(L, pred, gt, roi, ids_t))
    to5 = lambda t: t.permute(0, 4, 1, 2, 3)
    ev = M.eval_stats(to5(pred), to5(gt), to5(roi), ids)[:, :len(ids)]
    assert torch.equal(st[..., 0], ev[..., M.CNT]) and float(st[..., 0].sum()) > 0
    ep, eg = _rel(st[..., 1], ev[..., M.SP]), _rel(st[..., 2], ev[..., M.SG])
    print(f"region stats vs eval_stats {dt} {pattern}: sum pred {ep:.3e} sum gt {eg:.3e} (bound {P.stats_bound(V):.3e})")
    assert ep <= P.stats_bound(V) and eg <= P.stats_bound(V)


def test_argument_checks():
    L = _L()
    case = next(c for c in P.CASES if c[0] == "tail")
    pred, gt, roi, mk_dp, ids, w, _ = _inputs(case, "random", "roi36", torch.float32)
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    B, n = pred.shape[0], len(ids)
    loss, coef = torch.full((B,), SENT, device="cuda"), torch.full((B, n), SENT, device="cuda")
    st = torch.full((B, n, 3), SENT, dtype=torch.float64, device="cuda")
    ws = _ws(L, pred)
    assert L.lib.coma_roi_mean_ws_bytes(L.ct(pred)) == P.ws_bytes(B)
    s = L.stream()

    def fwd(p=pred, g=gt, r=roi, n=n, kind=0, delta=1.0, nbytes=None):
        return L.lib.coma_roi_mean_fwd(L.ct(p), L.ct(g), L.ct(r), L.ptr(ids_t), L.ptr(w), n, kind, delta, L.ptr(loss), L.ptr(coef),
                                       L.ptr(ws), ws.numel() if nbytes is None else nbytes, s)

    def stats(p=pred, g=gt, r=roi, n=n, nbytes=None):
        return L.lib.coma_roi_region_stats(L.ct(p), L.ct(g), L.ct(r), L.ptr(ids_t), n, L.ptr(st), L.ptr(ws),
                                           ws.numel() if nbytes is None else nbytes, s)

    two = torch.zeros(B, 5, 6, 7, 2, device="cuda")
    bad = [dict(n=0), dict(n=65), dict(kind=3), dict(kind=-1), dict(kind=2, delta=0.0), dict(kind=2, delta=-1.0),
           dict(kind=2, delta=float("inf")), dict(kind=2, delta=float("nan")), dict(nbytes=P.ws_bytes(B) - 1),
           dict(g=gt.bfloat16()), dict(r=roi.bfloat16()), dict(g=gt[:, :4]), dict(p=two), dict(r=two[..., :1]), dict(g=two[..., :1])]
    for kw in bad:
        assert fwd(**kw) == 1, kw
    for kw in (dict(n=0), dict(n=65), dict(nbytes=P.ws_bytes(B) - 1), dict(g=gt.bfloat16()), dict(r=roi.bfloat16()), dict(g=gt[:, :4])):
        assert stats(**kw) == 1, kw
    dp = mk_dp()
    gout = torch.ones(B, device="cuda")
    bwd = lambda d, r=roi, n=n: L.lib.coma_roi_mean_bwd(L.ct(r), L.ptr(ids_t), n, L.ptr(gout), L.ptr(coef), L.ct(d), s)
    assert bwd(dp.t[:, :4]) == 1 and bwd(dp.t, n=0) == 1 and bwd(dp.t, n=65) == 1 and bwd(dp.t, r=roi.bfloat16()) == 1
    assert bwd(two) == 1 and bwd(dp.t, r=two[..., :1]) == 1
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert bool((loss == SENT).all()) and bool((coef == SENT).all()) and bool((st == SENT).all()) and bool((dp.flat == SENT).all())
    with pytest.raises(L.ComaError, match="roi_mean_fwd"):
        L.check(fwd(kind=7), "roi_mean_fwd")
    assert fwd(kind=1, delta=0.0) == 0 and fwd(kind=2, delta=0.15) == 0 and stats() == 0          # (delta only matters for huber)
    coef.zero_()
    assert bwd(dp.t) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and float(st[..., 0].sum()) > 0
