"""coma_roi_wloss_fwd / coma_roi_wloss_bwd (csrc/roi_loss.hip) through the C ABI: every kind x {fp32, bf16} x the cases of
tests/_roi_loss_plan.py x two label tables, against the fp64 two-pass restatement evaluated on the very same stored inputs.

Paths (asserted from the mirrored launch arithmetic in test_roi_losses_cpu.py):
  tail     V = 210, B = 3, dense: one block, sample stride no multiple of 4 -> SCALAR path
  vtail    the same volume at sample stride 212 -> VECTOR path, 52 groups of 4 + 2 scalar tail voxels
  mid      (32, 33, 35), B = 3, dense -> VECTOR path, 19 blocks, 2 trips
  cap      (64, 128, 129), B = 2 -> VECTOR path, the 512-block cap, 3 trips, an 8-trip finalise loop
  pitched  mid's shape, pred / dpred at the 16-byte voxel pitch -> SCALAR path, 8 trips; pitch padding untouched
  mid, one element off its base (test_scalar_and_vector_paths_agree) -> SCALAR path on dense input

Bounds: counted from the kernel source (K_LOSS / K_COEF / K_GRAD of the plan), and the ceilings of the plan on top:
loss relative error <= 1e-6, gradient rel-L2 <= 1e-6 (fp32) and <= 2^-9 + 1e-6 (bf16)."""
import gc
import zlib

import pytest
import torch

import _roi_loss_plan as P
from oracle import fp64_ref as R
from test_nonconv_sizes_gpu import Guard, _pitched

pytestmark = pytest.mark.gpu

SENT = -7.0
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GOUT = [1.0, -2.0, 0.37]


def _L():
    from coma_unet_amd import _lib
    return _lib


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()))


class Buf:
    """(B, D, H, W, 1) view `t` of voxel pitch ld and sample stride sb, `off` elements behind a 64-cell header of a flat
    buffer filled with `fill`: everything outside the view must still hold `fill` after a kernel wrote `t`."""

    def __init__(self, B, dims, dtype, ld, sb, off=0, fill=SENT):
        D, H, W = dims
        self.fill = fill
        self.flat = torch.full((64 + off + B * sb + 64,), fill, dtype=dtype, device="cuda")
        self.geom = ((B, D, H, W, 1), (sb, H * W * ld, W * ld, ld, 1), 64 + off)
        self.t = self.flat.as_strided(*self.geom)

    def untouched(self):
        c = self.flat.clone()
        c.as_strided(*self.geom).fill_(self.fill)
        return bool((c == self.fill).all())


def _tables(table):
    """-> ids (list), w (fp32 cuda), label pools (every sample but #1, sample #1: NO listed label at all)."""
    from coma_unet_amd.roi_tables import ROI_INDICES
    if table == "roi36":
        ids, w = list(ROI_INDICES), P.mixed_weights(len(ROI_INDICES), torch.float32)
        pool = [float(i) for i in ids] * 2 + [0.0] * 12 + [2.0, 4999.0, 5000.0, 17.5]      # 0, >= 4096 and a fraction present
    else:
        ids, w = list(P.TEMPLATE_IDS), torch.ones(len(P.TEMPLATE_IDS))
        pool = [float(i) for i in range(0, 10)] + [4999.0]
    none = [0.0, 9.0, 4999.0, 3000.0]
    assert not set(none) & set(float(i) for i in ids)
    return ids, w.cuda(), torch.tensor(pool, device="cuda"), torch.tensor(none, device="cuda")


def _inputs(case, dtype, table, off=0):
    """-> pred, gt, roi views (values rounded to dtype), a maker of guarded dpred buffers, ids, w."""
    name, dims, B, lay = case
    es = 2 if dtype == torch.bfloat16 else 4
    lo = P.case_layout(dims, B, lay, es)
    gen = _gen("roi_wloss", name, table)              # (the same values for both dtypes and both offsets)
    shape = (B, *dims, 1)
    ids, w, pool, none = _tables(table)
    gtv = torch.rand(shape, generator=gen, device="cuda") + 0.25
    pv = gtv + 0.3 * torch.randn(shape, generator=gen, device="cuda")
    lab = pool[torch.randint(0, pool.numel(), shape, generator=gen, device="cuda")]
    lab[1] = none[torch.randint(0, none.numel(), shape[1:], generator=gen, device="cuda")]
    if lay == "pitched":
        pred = _pitched(shape, lo["pred"][0], dtype, pv)
        mk_dp = lambda: Guard(shape, dtype, lo["pred"][0], 0)
    else:
        pb = Buf(B, dims, dtype, *lo["pred"], off, fill=3.0e4)
        pb.t.copy_(pv)
        pred = pb.t
        mk_dp = lambda: Buf(B, dims, dtype, *lo["pred"], off)
    gb, rb = Buf(B, dims, dtype, *lo["gt"], off, fill=3.0e4), Buf(B, dims, torch.float32, *lo["roi"], off, fill=17.0)
    gb.t.copy_(gtv)
    rb.t.copy_(lab)
    return pred, gb.t, rb.t, mk_dp, ids, w, lo["vec"] and off % 4 == 0


def _fwd(L, pred, gt, roi, ids_t, w, kind, bg=1.0):
    B = pred.shape[0]
    res = torch.full((64 + 2 * B + 64,), SENT, device="cuda")
    loss, coef = res[64:64 + B], res[64 + B:64 + 2 * B]
    ws = L.workspace(L.lib.coma_roi_wloss_ws_bytes(L.ct(pred)), pred.device)
    L.check(L.lib.coma_roi_wloss_fwd(L.ct(pred), L.ct(gt), L.ct(roi), L.ptr(ids_t), L.ptr(w), ids_t.numel(), bg, kind,
                                     L.ptr(loss), L.ptr(coef), L.ptr(ws), ws.numel(), L.stream()), "roi_wloss_fwd")
    assert bool((res[:64] == SENT).all()) and bool((res[64 + 2 * B:] == SENT).all())
    return loss, coef


def _bwd(L, pred, gt, roi, ids_t, w, gout, coef, dp, bg=1.0):
    L.check(L.lib.coma_roi_wloss_bwd(L.ct(pred), L.ct(gt), L.ct(roi), L.ptr(ids_t), L.ptr(w), ids_t.numel(), bg, L.ptr(gout),
                                     L.ptr(coef), L.ct(dp.t), L.stream()), "roi_wloss_bwd")
    assert dp.untouched()
    return dp.t


def _check_kind(L, kind, pred, gt, roi, mk_dp, ids, w, dtype, what):
    """forward twice, backward twice, against the restatement.  -> (loss, coef, dpred)."""
    B = pred.shape[0]
    V = pred[0].numel()
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    gout = torch.tensor(GOUT[:B], device="cuda")
    loss, coef = _fwd(L, pred, gt, roi, ids_t, w, kind)
    loss2, coef2 = _fwd(L, pred, gt, roi, ids_t, w, kind)
    assert torch.equal(loss, loss2) and torch.equal(coef, coef2), what          # bitwise repeatable
    lref, cref, gref, den = P.loss_coef_grad64(kind, pred, gt, roi, ids, w.double(), gout)
    amp = P.den_mass64(kind, gt, roi, ids, w.double()) / den
    lerr = ((loss.double() - lref).abs() / lref.abs())
    cerr = ((coef.double() - cref).abs() / cref.abs())
    print(f"{what}: loss rel err {lerr.tolist()} coef rel err {cerr.tolist()} (mass(D) / D {amp.tolist()})")
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(coef).all()), what
    for b in range(B):
        assert float(lerr[b]) <= min(P.rel_bound(P.K_LOSS[kind], V, float(amp[b])), P.LOSS_REL), (what, b, float(lerr[b]))
        assert float(cerr[b]) <= P.rel_bound(P.K_COEF[kind], V, float(amp[b])), (what, b, float(cerr[b]))
    dp = _bwd(L, pred, gt, roi, ids_t, w, gout, coef, mk_dp())
    dp2 = _bwd(L, pred, gt, roi, ids_t, w, gout, coef, mk_dp())
    assert torch.equal(dp, dp2), what
    u_out = R.U_BF16 if dtype == torch.bfloat16 else R.U_F32
    extra = ((V + 8) * P.U_F64 * (1.0 + amp)).view(B, 1, 1, 1, 1)
    bound = u_out * gref.abs() + (2.0 * P.K_GRAD[kind] * P.U_F32 + extra) * gref.abs()
    worst = R.check_elementwise(dp, gref, bound, what + " dpred")
    l2 = max(P.rel_l2(dp[b], gref[b]) for b in range(B))
    print(f"{what}: dpred worst element / bound {worst:.3f}, rel-L2 {l2:.3e} (ceiling {P.GRAD_REL_L2[dtype]:.3e})")
    assert l2 <= P.GRAD_REL_L2[dtype], (what, l2)
    return loss, coef, dp


@pytest.mark.parametrize("table", ["roi36", "template"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c[0])
def test_loss_coef_and_gradient_vs_fp64(case, dt, table):
    L = _L()
    dtype = DT[dt]
    try:
        pred, gt, roi, mk_dp, ids, w, vec = _inputs(case, dtype, table)
        assert vec == (case[0] in ("vtail", "mid", "cap"))                       # the path this case takes
        assert float(roi.min()) == 0.0 and float(roi.max()) >= 4096.0             # labels 0 and >= 4096 present
        assert not any(bool((roi[1] == float(i)).any()) for i in ids)             # sample 1: no listed label at all
        for name, kind in P.KINDS.items():
            _check_kind(L, kind, pred, gt, roi, mk_dp, ids, w, dtype, f"{case[0]}-{dt}-{table}-{name}")
    finally:
        gc.collect()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_scalar_and_vector_paths_agree(dt):
    """The same dense `mid` input 16-byte aligned (vector path) and one element off (scalar path): dpred bitwise equal from
    the same coef; each path's own loss and coef within the bounds (their summation orders differ)."""
    L = _L()
    dtype = DT[dt]
    case = next(c for c in P.CASES if c[0] == "mid")
    outs = []
    for off in (0, 1):
        pred, gt, roi, mk_dp, ids, w, vec = _inputs(case, dtype, "roi36", off)
        assert vec == (off == 0) and (pred.data_ptr() % 16 == 0) == (off == 0)
        outs.append([_check_kind(L, kind, pred, gt, roi, mk_dp, ids, w, dtype, f"mid+{off}-{dt}-{n}") for n, kind in P.KINDS.items()])
        outs[-1].append((pred, gt, roi, mk_dp, ids, w))
    for k, kind in enumerate(P.KINDS.values()):
        lv, cv, dv = outs[0][k]
        ls, cs, ds = outs[1][k]
        assert float(((lv - ls).abs() / ls.abs()).max()) <= 2e-7 and float(((cv - cs).abs() / cs.abs()).max()) <= 2e-7
        # the scalar path's backward from the VECTOR path's coef: the same per-voxel values
        pred, gt, roi, mk_dp, ids, w = outs[1][3]
        ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
        gout = torch.tensor(GOUT[:3], device="cuda")
        d2 = _bwd(L, pred, gt, roi, ids_t, w, gout, cv.clone(), mk_dp())
        assert torch.equal(d2, dv), kind


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_unit_weights_equal_the_validation_metrics(dt):
    """With every weight 1, RoiRRMSE / RoiRSE per sample are the rrmse / rse terms of metrics.batch_global_metrics."""
    L = _L()
    from coma_unet_amd import metrics as M
    dtype = DT[dt]
    case = next(c for c in P.CASES if c[0] == "mid")
    pred, gt, roi, _, ids, w, _ = _inputs(case, dtype, "template")
    assert bool((w == 1).all())
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    to5 = lambda t: t.permute(0, 4, 1, 2, 3)                                      # (B, 1, D, H, W) view
    for name, key in (("rse", "rse"), ("rrmse", "rrmse")):
        loss, _ = _fwd(L, pred, gt, roi, ids_t, w, P.KINDS[name])
        for b in range(pred.shape[0]):
            m = M.batch_global_metrics(to5(pred[b:b + 1].contiguous()), to5(gt[b:b + 1].contiguous()),
                                       roi=to5(roi[b:b + 1].contiguous()), roi_indices=ids)
            ref = float(m[key])
            assert abs(float(loss[b]) - ref) <= 1e-6 * abs(ref), (name, b, float(loss[b]), ref)


def test_argument_checks():
    L = _L()
    case = next(c for c in P.CASES if c[0] == "tail")
    pred, gt, roi, mk_dp, ids, w, _ = _inputs(case, torch.float32, "roi36")
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    B = pred.shape[0]
    loss, coef = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    ws = L.workspace(L.lib.coma_roi_wloss_ws_bytes(L.ct(pred)), pred.device)
    assert L.lib.coma_roi_wloss_ws_bytes(L.ct(pred)) == P.ws_bytes(B)
    s = L.stream()

    def fwd(p=pred, g=gt, r=roi, n=len(ids), kind=0, nbytes=None):
        return L.lib.coma_roi_wloss_fwd(L.ct(p), L.ct(g), L.ct(r), L.ptr(ids_t), L.ptr(w), n, 1.0, kind, L.ptr(loss), L.ptr(coef),
                                        L.ptr(ws), ws.numel() if nbytes is None else nbytes, s)

    assert fwd() == 0
    bad = [dict(n=0), dict(n=65), dict(kind=3), dict(kind=-1), dict(nbytes=P.ws_bytes(B) - 1), dict(g=gt.bfloat16()),
           dict(r=roi.bfloat16()), dict(g=gt[:, :4]), dict(p=torch.zeros(B, 5, 6, 7, 2, device="cuda")),
           dict(r=torch.zeros(B, 5, 6, 7, 2, device="cuda")[..., :1]), dict(g=torch.zeros(B, 5, 6, 7, 2, device="cuda")[..., :1])]
    for kw in bad:
        assert fwd(**kw) == 1, kw
    dp = mk_dp()
    gout = torch.ones(B, device="cuda")
    bwd = lambda d, n=len(ids): L.lib.coma_roi_wloss_bwd(L.ct(pred), L.ct(gt), L.ct(roi), L.ptr(ids_t), L.ptr(w), n, 1.0,
                                                         L.ptr(gout), L.ptr(coef), L.ct(d), s)
    assert bwd(dp.t) == 0
    assert bwd(dp.t.bfloat16()) == 1 and bwd(dp.t[:, :4]) == 1 and bwd(dp.t, 0) == 1
    with pytest.raises(L.ComaError, match="roi_wloss_fwd"):
        L.check(fwd(kind=7), "roi_wloss_fwd")
    torch.cuda.synchronize()
