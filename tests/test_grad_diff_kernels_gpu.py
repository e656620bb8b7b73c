"""coma_grad_diff_fwd / coma_grad_diff_bwd (csrc/grad_diff.hip) through the C ABI, against the fp64 restatement of
tests/_grad_diff_plan.py evaluated on the very same stored inputs.

Shapes (P.CASES): tiny 3x4x5 (under one tile), edges 9x10x37 (1 / 2 / 5 voxels past a tile), flat 1x8x40 (no z pair), multi
40x40x72 (75 tiles: past the finalise's 64 lanes).  Layouts: dense, channel 0 of a (..., 4) fp32 / (..., 8) bf16 buffer, one
element off the base.  flat and multi take the 16-byte staging when dense and aligned; everything else stages by element.

Bounds: P.loss_bound / P.coef_bound / P.grad_bound, counted in the plan's docstring from the kernel's arithmetic (fp64 on the
staged values, one rounding per output).  Exact zeros are exact.  Everything is run twice and must repeat bitwise."""
import functools
import gc

import pytest
import torch

import _grad_diff_plan as P
from oracle import fp64_ref as R
from test_roi_losses_kernels_gpu import Buf

pytestmark = pytest.mark.gpu

SENT = -7.0
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
REPORT = {}


def _L():
    from coma_unet_amd import _lib
    return _lib


def _buf(B, dims, dtype, layout, fill=SENT):
    V = dims[0] * dims[1] * dims[2]
    if layout == "slice":
        ld = 4 if dtype == torch.float32 else 8
        return Buf(B, dims, dtype, ld, V * ld, 0, fill=fill)
    return Buf(B, dims, dtype, 1, V, 1 if layout == "off1" else 0, fill=fill)


def _place(vals, dtype, layout, fill=3.0e4):
    """(B, D, H, W) cpu values -> a (B, D, H, W, 1) device view in `layout` whose surroundings hold finite garbage"""
    B, dims = vals.shape[0], tuple(vals.shape[1:])
    b = _buf(B, dims, dtype, layout, fill)
    b.t.copy_(vals.cuda().unsqueeze(-1))
    return b.t


def _inputs(name, kind, mask, dtype, layout):
    """-> pred (in `layout`), gt, roi (dense, or one element off with "off1"; roi None without a mask), a maker of dpred buffers"""
    pv, gv, lab = (P.exact_inputs if kind == "exact" else P.random_inputs)(name, mask)
    _, dims, B = P.case(name)
    side = "off1" if layout == "off1" else "contig"
    pred, gt = _place(pv, dtype, layout), _place(gv, dtype, side)
    roi = None if mask is None else _place(lab, torch.float32, side, fill=17.0)
    return pred, gt, roi, lambda: _buf(B, dims, dtype, layout)


def _vec_paths(name, dtype, layout):
    """(pred, gt) staged 16 bytes at a time?"""
    _, dims, B = P.case(name)
    V, es = dims[0] * dims[1] * dims[2], 2 if dtype == torch.bfloat16 else 4
    off = 1 if layout == "off1" else 0
    ld = 1 if layout != "slice" else 16 // es
    return P.vec_ok(ld, V * ld, dims[2], off, es), P.vec_ok(1, V, dims[2], off, es)


@functools.lru_cache(maxsize=None)
def _ref(name, kind, mask, mode, alpha):
    """the restatement on the device, once per input set (exact inputs are the same numbers in fp32 and bf16)"""
    pv, gv, lab = (P.exact_inputs if kind == "exact" else P.random_inputs)(name, mask)
    B = pv.shape[0]
    gout = torch.tensor(P.GOUT[:B], dtype=torch.float64, device="cuda")
    roi = None if mask is None else lab.cuda()
    aw = P.AXIS_W[(mode, alpha)]
    loss, coef, grad = P.loss_coef_grad64(pv.cuda(), gv.cuda(), roi, P.MODES[mode], alpha, aw, gout)
    closed, amp, near = P.closed_grad_amp64(pv.cuda(), gv.cuda(), roi, P.MODES[mode], alpha, aw, gout)
    assert float((closed - grad).abs().max()) <= 1e-13 * max(float(amp.max()), 1e-300)
    return loss, coef, grad, amp, near


def _aw(mode, alpha):
    import ctypes
    return (ctypes.c_float * 3)(*P.AXIS_W[(mode, alpha)])


def _fwd(L, pred, gt, roi, mode, alpha, ws=None, nbytes=None):
    B = pred.shape[0]
    res = torch.full((64 + B + 3 * B + 64,), SENT, device="cuda")
    loss, coef = res[64:64 + B], res[64 + B:64 + 4 * B].view(B, 3)
    if ws is None:
        ws = L.workspace(L.lib.coma_grad_diff_ws_bytes(L.ct(pred)), pred.device)
    L.check(L.lib.coma_grad_diff_fwd(L.ct(pred), L.ct(gt), None if roi is None else L.ct(roi), P.MODES[mode], alpha, _aw(mode, alpha),
                                     L.ptr(loss), L.ptr(coef), L.ptr(ws), ws.numel() if nbytes is None else nbytes, L.stream()),
            "grad_diff_fwd")
    assert bool((res[:64] == SENT).all()) and bool((res[64 + 4 * B:] == SENT).all())
    return loss, coef


def _bwd(L, pred, gt, roi, mode, alpha, gout, coef, dp):
    L.check(L.lib.coma_grad_diff_bwd(L.ct(pred), L.ct(gt), None if roi is None else L.ct(roi), P.MODES[mode], alpha, L.ptr(gout),
                                     L.ptr(coef), L.ct(dp.t), L.stream()), "grad_diff_bwd")
    assert dp.untouched()
    return dp.t


def _rel(got, ref):
    """max relative error over the non-zero reference entries; the zero ones must be exactly zero"""
    got, ref = got.double(), ref.double()
    zero = ref == 0
    assert bool((got[zero] == 0).all())
    return float(((got - ref).abs()[~zero] / ref.abs()[~zero]).max()) if bool((~zero).any()) else 0.0


def _check(L, name, kind, mask, mode, alpha, dtype, layout, what, exclude_near=False):
    """forward twice, backward twice, against the restatement.  -> (loss, coef, dpred)"""
    pred, gt, roi, mk_dp = _inputs(name, kind, mask, dtype, layout)
    B, V = pred.shape[0], pred[0].numel()
    gout = torch.tensor(P.GOUT[:B], device="cuda")
    lref, cref, gref, amp, near = _ref(name, kind, mask, mode, alpha)
    loss, coef = _fwd(L, pred, gt, roi, mode, alpha)
    loss2, coef2 = _fwd(L, pred, gt, roi, mode, alpha)
    assert torch.equal(loss, loss2) and torch.equal(coef, coef2), what           # bitwise repeatable
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(coef).all()), what
    lerr, cerr = _rel(loss, lref), _rel(coef, cref)
    assert lerr <= P.loss_bound(V) and cerr <= P.coef_bound(), (what, lerr, cerr, P.loss_bound(V))
    dp = _bwd(L, pred, gt, roi, mode, alpha, gout, coef, mk_dp())
    dp2 = _bwd(L, pred, gt, roi, mode, alpha, gout, coef, mk_dp())
    assert torch.equal(dp, dp2), what
    got = dp[..., 0]
    bound = P.grad_bound(gref, amp, dtype)
    share = 0.0
    if exclude_near:        # |t| or |gp| within 1e-5 of a tie: a last-bit rounding may legitimately flip a sign there
        share = float(near.double().mean())
        assert share <= 1e-3, (what, share)
        flips = int(((got.double() - gref).abs() > bound)[near].sum())
        print(f"{what}: excluded share {share:.3e}; voxels off their bound among the excluded: {flips}")
        keep = ~near
        worst = R.check_elementwise(got[keep], gref[keep], bound[keep], what + " dpred")
    else:
        assert bool((got[amp == 0] == 0).all()), what                             # no live pair at the voxel: exactly 0
        worst = R.check_elementwise(got, gref, bound, what + " dpred")
    gl2 = P.rel_l2(got, gref) if float(gref.abs().max()) > 0 else 0.0
    print(f"{what}: loss rel err {lerr:.3e} (bound {P.loss_bound(V):.3e}) coef {cerr:.3e} dpred rel-L2 {gl2:.3e} worst / bound {worst:.3f}")
    key = (kind, str(dtype).split(".")[-1])
    old = REPORT.get(key, (0.0, 0.0, 0.0))
    REPORT[key] = (max(old[0], lerr), max(old[1], gl2), max(old[2], worst))
    return loss, coef, dp


@pytest.mark.parametrize("layout", P.LAYOUTS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", [c[0] for c in P.CASES])
def test_exact_inputs_vs_fp64(name, dt, layout):
    L = _L()
    _, dims, B = P.case(name)
    masks = (None, "brain", "zero") if B == 1 else (None, "brain")
    try:
        vp, vg = _vec_paths(name, DT[dt], layout)
        assert vg == (name in ("flat", "multi") and layout != "off1") and vp == (vg and layout == "contig")
        for mask in masks:
            for mode, alpha in P.CONFIGS:
                loss, coef, dp = _check(L, name, "exact", mask, mode, alpha, DT[dt], layout, f"{name}-{dt}-{layout}-{mask}-{mode}{alpha}")
                aw = P.AXIS_W[(mode, alpha)]
                if name == "flat":                                               # no z pair: coefficient 0, nothing NaN
                    assert float(coef[:, 0].abs().max()) == 0.0
                if aw[1] == 0.0:
                    assert float(coef[:, 1].abs().max()) == 0.0
                if mask == "zero" or (mask == "brain" and B > 1):                # an all-zero mask: loss 0, gradient 0
                    b = B - 1
                    assert float(loss[b]) == 0.0 and float(coef[b].abs().max()) == 0.0 and float(dp[b].abs().max()) == 0.0
                if mask != "zero":
                    assert float(loss[0]) > 0.0 and float(dp[0].abs().max()) > 0.0
        print("measured so far (max loss rel err, max dpred rel-L2, max worst/bound):", REPORT)
    finally:
        gc.collect()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("mask", [None, "brain"])
def test_random_inputs_vs_fp64(mask):
    """uniform [0, 4) fp32 at 40x40x72 x 2: alpha 2 (both modes) and signed alpha 1 everywhere; abs alpha 1 away from the ties
    (|t| <= 1e-5 or |gp| <= 1e-5 in fp64), whose share must stay under 1e-3."""
    L = _L()
    for mode, alpha in P.CONFIGS:
        _check(L, "multi", "random", mask, mode, alpha, torch.float32, "contig", f"random-{mask}-{mode}{alpha}",
               exclude_near=(mode, alpha) == ("abs", 1))
    print("measured (max loss rel err, max dpred rel-L2, max worst/bound):", REPORT)


@pytest.mark.parametrize("name", ["flat", "multi"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_scalar_and_vector_paths_agree_bitwise(dt, name):
    """Dense and aligned (16-byte staging and stores) against one element off (element-wise): both leave the same values in
    LDS and everything after reads LDS only -- the same bits."""
    L = _L()
    assert _vec_paths(name, DT[dt], "contig") == (True, True) and _vec_paths(name, DT[dt], "off1") == (False, False)
    for mask in (None, "brain"):
        for mode, alpha in (("abs", 1), ("signed", 2)):
            a = _check(L, name, "exact", mask, mode, alpha, DT[dt], "contig", f"{name}-vec-{dt}")
            b = _check(L, name, "exact", mask, mode, alpha, DT[dt], "off1", f"{name}-scalar-{dt}")
            c = _check(L, name, "exact", mask, mode, alpha, DT[dt], "slice", f"{name}-slice-{dt}")
            for x, y, z in zip(a, b, c):
                assert torch.equal(x, y) and torch.equal(x, z)
            assert a[2].data_ptr() % 16 == 0 and b[2].data_ptr() % 16 != 0


def test_exact_size_workspace_full_of_nan_gives_the_same_bits():
    L = _L()
    for name in ("edges", "multi"):
        _, dims, B = P.case(name)
        for mask in (None, "brain"):
            pred, gt, roi, _ = _inputs(name, "exact", mask, torch.float32, "contig")
            n = L.lib.coma_grad_diff_ws_bytes(L.ct(pred))
            assert n == P.ws_bytes(B, dims)
            guard = torch.full((64 + n + 64,), 0xFF, dtype=torch.uint8, device="cuda")      # all-ones bytes: NaN as doubles
            ws = guard[64:64 + n]
            assert bool(torch.isnan(ws.view(torch.float64)).all())
            want = _fwd(L, pred, gt, roi, "abs", 2)
            got = _fwd(L, pred, gt, roi, "abs", 2, ws=ws)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert bool((guard[:64] == 0xFF).all()) and bool((guard[64 + n:] == 0xFF).all())
            assert not bool(torch.isnan(ws.view(torch.float64)).any())                       # every record was written


def test_argument_checks():
    L = _L()
    pred, gt, roi, mk_dp = _inputs("edges", "exact", "brain", torch.float32, "contig")
    B = pred.shape[0]
    loss, coef = torch.full((B,), SENT, device="cuda"), torch.full((B, 3), SENT, device="cuda")
    ws = L.workspace(L.lib.coma_grad_diff_ws_bytes(L.ct(pred)), pred.device)
    need = P.ws_bytes(B, (9, 10, 37))
    s = L.stream()
    import ctypes
    ones = (ctypes.c_float * 3)(1.0, 1.0, 1.0)

    def fwd(p=pred, g=gt, r=roi, mode=0, alpha=1, aw=ones, wsp=L.ptr(ws), nbytes=ws.numel()):
        return L.lib.coma_grad_diff_fwd(L.ct(p), L.ct(g), None if r is None else L.ct(r), mode, alpha, aw, L.ptr(loss), L.ptr(coef),
                                        wsp, nbytes, s)

    two = torch.zeros(B, 9, 10, 37, 2, device="cuda")
    wide = torch.zeros(B, 9, 10, 37, 4, device="cuda")
    bad = [dict(wsp=None), dict(nbytes=need - 1), dict(nbytes=0), dict(p=two, g=two), dict(g=wide[..., :1]), dict(r=wide[..., :1]),
           dict(g=gt[:, :4]), dict(r=roi[:, :4]), dict(g=gt.bfloat16()), dict(r=roi.bfloat16()), dict(mode=2), dict(mode=-1),
           dict(alpha=0), dict(alpha=3), dict(aw=(ctypes.c_float * 3)(1.0, -1.0, 1.0)), dict(aw=(ctypes.c_float * 3)(1.0, float("nan"), 1.0)),
           dict(aw=None)]
    for kw in bad:
        assert fwd(**kw) == 1 and len(L.lib.coma_last_error()) > 0, kw
    dp = mk_dp()
    gout = torch.ones(B, device="cuda")

    def bwd(d, p=pred, g=gt, r=roi, mode=0, alpha=1):
        return L.lib.coma_grad_diff_bwd(L.ct(p), L.ct(g), None if r is None else L.ct(r), mode, alpha, L.ptr(gout), L.ptr(coef), L.ct(d), s)

    for kw in (dict(d=dp.t[:, :4]), dict(d=two), dict(d=dp.t.bfloat16()), dict(d=dp.t, mode=2), dict(d=dp.t, alpha=3), dict(d=dp.t, g=wide[..., :1]),
               dict(d=dp.t, r=wide[..., :1]), dict(d=dp.t, g=gt.bfloat16()), dict(d=dp.t, p=two, g=two)):
        assert bwd(**kw) == 1 and len(L.lib.coma_last_error()) > 0, kw
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert bool((loss == SENT).all()) and bool((coef == SENT).all()) and bool((dp.flat == SENT).all())
    with pytest.raises(L.ComaError, match="grad_diff_fwd"):
        L.check(fwd(alpha=7), "grad_diff_fwd")
    assert fwd(nbytes=need) == 0 and fwd(r=None) == 0
    coef.zero_()
    assert bwd(dp.t) == 0 and bwd(dp.t, r=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and float(dp.t.abs().max()) == 0.0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_graph_capture_replays_with_changed_inputs(dt):
    """forward + backward captured on a side stream; replayed after the inputs' CONTENTS changed; against eager calls bitwise"""
    L = _L()
    name, mask, mode, alpha = "edges", "brain", "abs", 1
    pred, gt, roi, mk_dp = _inputs(name, "exact", mask, DT[dt], "slice")
    B = pred.shape[0]
    gout = torch.tensor(P.GOUT[:B], device="cuda")
    loss, coef = torch.zeros(B, device="cuda"), torch.zeros(B, 3, device="cuda")
    dp = mk_dp()
    n = L.lib.coma_grad_diff_ws_bytes(L.ct(pred))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    aw = _aw(mode, alpha)

    def run():
        L.check(L.lib.coma_grad_diff_fwd(L.ct(pred), L.ct(gt), L.ct(roi), P.MODES[mode], alpha, aw, L.ptr(loss), L.ptr(coef), L.ptr(ws), n,
                                         L.stream()), "grad_diff_fwd")
        L.check(L.lib.coma_grad_diff_bwd(L.ct(pred), L.ct(gt), L.ct(roi), P.MODES[mode], alpha, L.ptr(gout), L.ptr(coef), L.ct(dp.t),
                                         L.stream()), "grad_diff_bwd")

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(), capture_error_mode="thread_local"):
        run()
    first = None
    for trial in range(2):
        if trial == 1:                                  # new contents in the same buffers: rolled volumes, other labels
            pred.copy_(pred.roll(3, 3).clone())
            gt.copy_(gt.roll(2, 1).clone())
            roi.copy_(roi.roll(1, 2).clone())
        loss.fill_(SENT); coef.fill_(SENT); dp.t.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        got = (loss.clone(), coef.clone(), dp.t.clone())
        loss.fill_(SENT); coef.fill_(SENT); dp.t.fill_(SENT)
        run()
        torch.cuda.synchronize()
        for x, y in zip(got, (loss, coef, dp.t)):
            assert torch.equal(x, y) and bool(torch.isfinite(x.float()).all())
        assert dp.untouched() and float(got[0][0]) > 0
        if first is None:
            first = got
    assert not torch.equal(first[0], got[0]) and not torch.equal(first[2], got[2])          # the replay saw the new contents
