"""The streaming kernels outside the convolution families (csrc/elementwise.hip, metrics.hip, norm.hip, the fp32 side of
gate.hip) past one block, one row chunk and one pass of their grid-stride loops: every entry point against a plain fp64 (or,
where one rounding is all there is, bit-exact fp32) restatement of the same operation on the very same rounded inputs.

The shapes come from tests/_nonconv_plan.py (test_nonconv_sizes_cpu.py asserts that each one crosses the boundary it is listed
for).  Every output lives in a buffer whose pitch padding and surroundings hold a sentinel that must survive, every element
of every output is compared, and the measured worst ratios are printed by test_zz_report (profiles/nonconv_sizes.txt).

Tolerances: `torch.equal` where the kernel rounds once; else |got - ref| <= u_out |ref| + (2 K 2^-24 + n 2^-53) A with A the
L1 mass of the terms behind the element, K the fp32 roundings behind one term (counted from the kernel source, stated at
each call) and n the length of a double-precision accumulation.  bf16 volumes are also held to a rel-L2 per slab.
"""
import contextlib
import gc
import os
import zlib

import pytest
import torch

import _nonconv_plan as NP
from oracle import fp64_ref as R

pytestmark = pytest.mark.gpu

SENT = -7.0
SLAB_TOL = 5e-3           # bf16 volumes: max over (sample, z-plane) slabs of rel-L2 (test_production_shapes_gpu.py)
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
REPORT = {}


def _ops():
    from coma_unet_amd import ops, _lib
    return ops, _lib


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()))


def _u(dtype):
    return R.U_BF16 if dtype == torch.bfloat16 else R.U_F32


class Guard:
    """A flat sentinel-filled buffer [64 cells | B * V * ld | 4096 cells] and the (B, D, H, W, C) view `t` of channels
    [c_off, c_off + C) of its middle: the pitch padding and both ends must still hold the sentinel after a kernel wrote `t`."""

    def __init__(self, shape, dtype, ld=None, c_off=0, fill=SENT):
        B, D, H, W, C = shape
        ld = ld or C
        assert c_off + C <= ld
        self.fill = fill
        self.flat = torch.full((64 + B * D * H * W * ld + 4096,), fill, dtype=dtype, device="cuda")
        self.geom = (tuple(shape), (D * H * W * ld, H * W * ld, W * ld, ld, 1), 64 + c_off)
        self.t = self.flat.as_strided(*self.geom)

    def untouched(self):
        c = self.flat.clone()
        c.as_strided(*self.geom).fill_(self.fill)
        return bool((c == self.fill).all())


class FlatGuard:
    """A 1-D view `t` of n cells at element offset `off` behind a 64-cell sentinel header, with a sentinel tail."""

    def __init__(self, n, dtype, off=0, fill=SENT):
        self.fill, self.lo, self.n = fill, 64 + off, n
        self.flat = torch.full((64 + off + n + 4096,), fill, dtype=dtype, device="cuda")
        self.t = self.flat[self.lo:self.lo + n]

    def untouched(self):
        return bool((self.flat[:self.lo] == self.fill).all()) and bool((self.flat[self.lo + self.n:] == self.fill).all())


def _pitched(shape, ld, dtype, src):
    """`src` copied into a (B, D, H, W, C) view of voxel pitch ld whose foreign lanes hold finite garbage."""
    g = Guard(shape, dtype, ld, 0, fill=3.0e4)
    g.t.copy_(src)
    return g.t


@contextlib.contextmanager
def _guarded_new(ops):
    """While active, every activation buffer the autograd wrappers allocate (ops._new: saved intermediates, gradients) is
    a Guard view of the pitch ops._new would have given it; -> the list of those guards."""
    guards, orig = [], ops._new

    def new(shape, dtype, device):
        if len(shape) != 5:
            return orig(shape, dtype, device)
        g = Guard(tuple(shape), dtype, (shape[4] + 7) // 8 * 8 if shape[4] % 8 else shape[4], 0)
        guards.append(g)
        return g.t

    ops._new = new
    try:
        yield guards
    finally:
        ops._new = orig


def _randn(shape, gen, dtype, scale=1.0):
    return (torch.randn(tuple(shape), generator=gen, device="cuda") * scale).to(dtype)


def _bound(ref, A, K, u_out, n=0):
    return u_out * ref.abs() + (2.0 * K * R.U_F32 + n * NP.U_F64) * A


def _put(name, **kv):
    REPORT[name] = kv


# ---------------------------------------------------------------------------------------------------------------------
# one rounding: add, add-relu, relu mask, copy, gate multiply, cast, batch sum, zero_ranges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", NP.EW3_CASES, ids=lambda c: c[0])
def test_ew3_add_relu_copy(case, dt):
    """ew3_k (coma_add with a batch-1 operand, the copy form, add_relu_fwd / bwd), more elements per sample than one pass of
    the 8192-block grid; the vec-1 form through a channel slice at an odd offset of a wider buffer."""
    ops, L = _ops()
    name, dims, C, ldw, c_off, _vec = case
    dtype, B = DT[dt], 2
    gen = _gen("ew3", name, dt)
    s = L.stream()
    try:
        a1 = _randn((1, *dims, C), gen, dtype)
        a, b = _randn((B, *dims, C), gen, dtype), _randn((B, *dims, C), gen, dtype)
        out = Guard((B, *dims, C), dtype, ldw, c_off)
        y = ops.AddBcast.apply(a1, b, ops.Out(out.t))
        assert torch.equal(y, (a1.float() + b.float()).to(dtype)) and out.untouched(), "add (broadcast)"
        out = Guard((B, *dims, C), dtype, ldw, c_off)
        ops.Copy.apply(b, ops.Out(out.t))
        assert torch.equal(out.t, b) and out.untouched(), "copy"
        out = Guard((B, *dims, C), dtype, ldw, c_off)
        L.check(L.lib.coma_add_relu_fwd(L.ct(a), L.ct(b), L.ct(out.t), s), "add_relu_fwd")
        want = (a.float() + b.float()).clamp_min(0).to(dtype)
        assert torch.equal(out.t, want) and out.untouched(), "add_relu_fwd"
        da = Guard((B, *dims, C), dtype, ldw, c_off)
        L.check(L.lib.coma_add_relu_bwd(L.ct(out.t), L.ct(b), L.ct(da.t), s), "add_relu_bwd")
        assert torch.equal(da.t, torch.where(want > 0, b, torch.zeros_like(b))) and da.untouched(), "add_relu_bwd"
        _put(f"ew3-{name}-{dt}", exact=True)
    finally:
        _free()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", NP.GATE_MUL_CASES, ids=lambda c: c[0])
def test_gate_mul(case, dt):
    """gate_mul_fwd_k / gate_mul_bwd_k past one pass, with dead lanes in the last block's shuffle (V * cv not a multiple of
    256), accumulate_dx 0 and 1.  out and dx (=) round once: bit-exact.  dx (+=): product and sum, K = 2.  dpsi: C products
    summed in fp32 over the lanes of a voxel, K = C."""
    ops, L = _ops()
    name, dims, C, ldw, c_off, _vec = case
    dtype, B, u = DT[dt], 2, _u(DT[dt])
    gen = _gen("gate_mul", name, dt)
    s = L.stream()
    try:
        x, dout = _randn((B, *dims, C), gen, dtype), _randn((B, *dims, C), gen, dtype)
        psi = torch.sigmoid(torch.randn((B, *dims, 1), generator=gen, device="cuda")).to(dtype)
        out = Guard((B, *dims, C), dtype, ldw, c_off)
        L.check(L.lib.coma_gate_mul_fwd(L.ct(x), L.ct(psi), L.ct(out.t), s), "gate_mul_fwd")
        assert torch.equal(out.t, (x.float() * psi.float()).to(dtype)) and out.untouched(), "gate_mul_fwd"
        del out
        prod = (dout.float() * psi.float())
        dref = (dout.double() * x.double()).sum(-1, keepdim=True)
        dmass = (dout.double() * x.double()).abs().sum(-1, keepdim=True)
        st = {}
        for acc in (0, 1):
            dx = Guard((B, *dims, C), dtype, ldw, c_off)
            dpsi = Guard((B, *dims, 1), dtype, 8, 0)
            base = _randn((B, *dims, C), gen, dtype)
            if acc:
                dx.t.copy_(base)
            L.check(L.lib.coma_gate_mul_bwd(L.ct(x), L.ct(psi), L.ct(dout), L.ct(dx.t), acc, L.ct(dpsi.t), s), "gate_mul_bwd")
            assert dx.untouched() and dpsi.untouched(), "gate_mul_bwd wrote outside its outputs"
            if acc == 0:
                assert torch.equal(dx.t, prod.to(dtype)), "dx (=)"
            else:
                ref = base.double() + dout.double() * psi.double()
                st["dx_acc"] = R.check_elementwise(dx.t, ref, _bound(ref, base.double().abs() + prod.double().abs(), 2, u), "dx (+=)")
            st[f"dpsi{acc}"] = R.check_elementwise(dpsi.t, dref, _bound(dref, dmass, C, u), "dpsi")
            if dtype == torch.bfloat16:
                st[f"slab{acc}"] = max(R.slab_rel_l2(dpsi.t, dref, 2), R.slab_rel_l2(dx.t, ref, 2) if acc else 0.0)
                assert st[f"slab{acc}"] < SLAB_TOL, st
            del dx, dpsi, base
        _put(f"gate_mul-{name}-{dt}", **st)
    finally:
        _free()


@pytest.mark.parametrize("case", NP.CAST_CASES, ids=lambda c: c[0])
def test_cast_copy_and_batch_sum(case):
    """cast_copy_k (fp32 -> bf16 into a pitch-8 buffer, bf16 -> fp32, both same-type forms) and batch_sum_k (B = 3,
    sequential fp32 adds) over more than 8192 * 256 elements: bit-exact."""
    ops, L = _ops()
    name, dims, C = case
    gen = _gen("cast", name)
    s = L.stream()
    try:
        src32 = _randn((1, *dims, C), gen, torch.float32)
        for sdt, ddt, lds, ldd in (("f32", "bf16", C, 8), ("bf16", "f32", 8, C), ("f32", "f32", C, 4), ("bf16", "bf16", 8, 8)):
            src = _pitched((1, *dims, C), lds, DT[sdt], src32)
            dst = Guard((1, *dims, C), DT[ddt], ldd, 0)
            L.check(L.lib.coma_cast_copy(L.ct(src), L.ct(dst.t), s), "cast_copy")
            assert torch.equal(dst.t, src.to(DT[ddt])) and dst.untouched(), (sdt, ddt)
            del src, dst
        for dt in ("f32", "bf16"):
            x = _randn((NP.BATCH_SUM_B, *dims, C), gen, DT[dt])
            dst = Guard((1, *dims, C), DT[dt], 8 if C == 1 else 4, 0)
            L.check(L.lib.coma_batch_sum(L.ct(x), L.ct(dst.t), s), "batch_sum")
            acc = x[0].float()
            for b in range(1, NP.BATCH_SUM_B):
                acc = acc + x[b].float()
            assert torch.equal(dst.t[0], acc.to(DT[dt])) and dst.untouched(), ("batch_sum", dt)
            del x, dst
        _put(f"cast_copy+batch_sum-{name}", exact=True)
    finally:
        _free()


def test_zero_ranges():
    """zero_ranges_k with more ranges than grid y (1024) and a range longer than one pass of grid x (64 * 256): exactly
    the cells of the ranges become zero, the sentinel cells between them stay."""
    ops, L = _ops()
    tab, n_buf, longest = NP.zero_ranges_table()
    try:
        buf = torch.full((n_buf,), SENT, device="cuda")
        want = buf.clone()
        for off, ln in tab.tolist():
            want[off:off + ln] = 0.0
        dtab = tab.cuda()
        L.check(L.lib.coma_zero_ranges(buf.data_ptr(), dtab.data_ptr(), tab.shape[0], longest, L.stream()), "zero_ranges")
        assert torch.equal(buf, want)
        _put("zero_ranges", exact=True, ranges=tab.shape[0], longest=longest)
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# ROI painting and the losses
# ---------------------------------------------------------------------------------------------------------------------
def _roi_volume(shape, gen):
    """fp32 labels: the 36 ROI ids, other integer labels (0, one below the table, one past the 4096-entry LUT), a fraction."""
    from coma_unet_amd.roi_tables import ROI_INDICES
    table = torch.tensor([float(i) for i in ROI_INDICES] * 2 + [0.0] * 12 + [3.0, 5000.0, 17.5], device="cuda")
    return table[torch.randint(0, table.numel(), tuple(shape), generator=gen, device="cuda")]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", NP.LOSS_CASES, ids=lambda c: c[0])
def test_roi_paint_and_losses(case, dt):
    """roi_paint_fwd / bwd, roi_mse_fwd / bwd, l1_fwd / bwd with B = 3 and mixed abeta: `mid` has 2 < nblk < 64 loss blocks,
    `big` passes the 8192-block grids, the 512-block loss cap and the 64-lane finalize loop."""
    ops, L = _ops()
    from coma_unet_amd.roi_tables import ROI_INDICES
    name, dims, B = case
    dtype, u = DT[dt], _u(DT[dt])
    V = NP.vol(dims)
    ld1 = 8 if dtype == torch.bfloat16 else 4            # (16-byte voxel pitch of the single-channel volumes)
    gen = _gen("loss", name, dt)
    s = L.stream()
    st = {}
    try:
        ids = torch.tensor(ROI_INDICES, dtype=torch.int32, device="cuda")
        roi = _roi_volume((B, *dims, 1), gen)
        xv = torch.rand((B, *dims, 1), generator=gen, device="cuda")
        xv = torch.where(torch.rand((B, *dims, 1), generator=gen, device="cuda") < 0.1, torch.zeros_like(xv), xv)
        x = _pitched((B, *dims, 1), ld1, dtype, xv)
        prior = torch.randn((B, len(ROI_INDICES), 2), generator=gen, device="cuda")
        abeta = torch.tensor([1.0, 0.0, 1.0], device="cuda")
        pos, neg = torch.randn(dims, generator=gen, device="cuda"), torch.randn(dims, generator=gen, device="cuda")
        # ---- paint forward: values are selected, then rounded once to the storage type
        out3 = Guard((B, *dims, 3), dtype, 4, 0)
        L.check(L.lib.coma_roi_paint_fwd(L.ct(roi), L.ct(x), L.ptr(prior), L.ptr(ids), ids.numel(), L.ptr(abeta), L.ptr(pos),
                                         L.ptr(neg), L.ct(out3.t), s), "roi_paint_fwd")
        assert torch.equal(out3.t, NP.paint_ref(roi, x, prior, ROI_INDICES, abeta, pos, neg).to(dtype)) and out3.untouched()
        del out3
        # ---- paint backward: dpos / dneg += the samples' gradients, B sequential fp32 adds and the "+=": K = B + 1
        d3 = _pitched((B, *dims, 3), 4, dtype, _randn((B, *dims, 3), gen, dtype))
        dpos, dneg = FlatGuard(V, torch.float32), FlatGuard(V, torch.float32)
        bp, bn = torch.randn(V, generator=gen, device="cuda"), torch.randn(V, generator=gen, device="cuda")
        dpos.t.copy_(bp)
        dneg.t.copy_(bn)
        L.check(L.lib.coma_roi_paint_bwd(L.ct(d3), L.ptr(abeta), L.ptr(dpos.t), L.ptr(dneg.t), s), "roi_paint_bwd")
        g0 = d3[..., 0].double().reshape(B, V)
        sel = (abeta == 1.0).double().view(B, 1)
        for nm, got, base, w in (("dpos", dpos, bp, sel), ("dneg", dneg, bn, 1 - sel)):
            ref = base.double() + (g0 * w).sum(0)
            st[nm] = R.check_elementwise(got.t, ref, _bound(ref, base.double().abs() + (g0.abs() * w).sum(0), B + 1, R.U_F32), nm)
            assert got.untouched(), nm
        del d3, dpos, dneg, g0
        # ---- losses
        gtv = torch.rand((B, *dims, 1), generator=gen, device="cuda")
        gt = gtv.to(dtype)
        pred = _pitched((B, *dims, 1), ld1, dtype, gtv + 0.3 * torch.randn((B, *dims, 1), generator=gen, device="cuda"))
        w = torch.full((len(ROI_INDICES),), 225.0, device="cuda")
        w[5], w[11] = 17.0, 7.5
        gout = torch.tensor([1.0, -2.0, 0.37], device="cuda")
        ws = L.workspace(L.lib.coma_loss_ws_bytes(L.ct(pred)), pred.device)
        res = FlatGuard(3 * B, torch.float32)
        loss, mm, l1 = res.t[:B], res.t[B:2 * B], res.t[2 * B:]
        L.check(L.lib.coma_roi_mse_fwd(L.ct(pred), L.ct(gt), L.ct(roi), L.ptr(ids), L.ptr(w), ids.numel(), L.ptr(loss), L.ptr(mm),
                                       L.ptr(ws), ws.numel(), s), "roi_mse_fwd")
        L.check(L.lib.coma_l1_fwd(L.ct(pred), L.ct(gt), L.ptr(l1), L.ptr(ws), ws.numel(), s), "l1_fwd")
        assert res.untouched()
        lref, mref, sref = NP.roi_mse_ref(pred, gt, roi, ROI_INDICES, w)
        d = (pred.double() - gt.double())
        l1ref = d.abs()[..., 0].mean(dim=(1, 2, 3))
        # d = pred - gt is formed in fp32 (one rounding) and enters the square twice: K = 2; |d|: K = 1; the mask weights are
        # summed exactly in double: K = 0.  All three accumulate V terms in double.
        st["loss"] = R.check_elementwise(loss, lref, _bound(lref, lref, 2, R.U_F32, V), "roi_mse loss")
        st["mask_mean"] = R.check_elementwise(mm, mref, _bound(mref, mref, 0, R.U_F32, V), "mask mean")
        st["l1"] = R.check_elementwise(l1, l1ref, _bound(l1ref, l1ref, 1, R.U_F32, V), "l1 loss")
        # backward.  roi_mse: scale = gout * (mask_mean * 2) / V -- the stored fp32 mask mean, a product, a division -- times the
        # fp32 d: K = 5.  l1: +-(gout / V): K = 2 (the sign of an fp32 difference is exact).
        dp = Guard((B, *dims, 1), dtype, ld1, 0)
        L.check(L.lib.coma_roi_mse_bwd(L.ct(pred), L.ct(gt), L.ptr(gout), L.ptr(mm), L.ct(dp.t), s), "roi_mse_bwd")
        ref = d * (gout.double() * mref * 2.0 / V).view(B, 1, 1, 1, 1)
        st["dpred_mse"] = R.check_elementwise(dp.t, ref, _bound(ref, ref.abs(), 5, u), "roi_mse dpred")
        assert dp.untouched()
        if dtype == torch.bfloat16:
            st["slab_mse"] = R.slab_rel_l2(dp.t, ref, 2)
            assert st["slab_mse"] < SLAB_TOL, st
        dp = Guard((B, *dims, 1), dtype, ld1, 0)
        L.check(L.lib.coma_l1_bwd(L.ct(pred), L.ct(gt), L.ptr(gout), L.ct(dp.t), s), "l1_bwd")
        ref = torch.sign(d) * (gout.double() / V).view(B, 1, 1, 1, 1)
        st["dpred_l1"] = R.check_elementwise(dp.t, ref, _bound(ref, ref.abs(), 2, u), "l1 dpred")
        assert dp.untouched()
        if dtype == torch.bfloat16:
            st["slab_l1"] = R.slab_rel_l2(dp.t, ref, 2)
            assert st["slab_l1"] < SLAB_TOL, st
        _put(f"paint+losses-{name}-{dt}", **st)
    finally:
        _free()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", NP.EVAL_CASES, ids=lambda c: c[0])
def test_eval_stats(case, dt):
    """eval_stats_k over several blocks per sample (the fp64 atomics across blocks) and past its 1024-block cap: every
    (sample, bin, k) entry.  fp32 roundings behind one term: counts, g, g^2, p none (exact in double); |d| one; d^2 two (the
    fp32 d enters twice); |d / g| two (d, the division)."""
    ops, L = _ops()
    from coma_unet_amd.roi_tables import ROI_INDICES
    name, dims, B = case
    dtype = DT[dt]
    V = NP.vol(dims)
    gen = _gen("eval", name, dt)
    try:
        ids = torch.tensor(ROI_INDICES, dtype=torch.int32, device="cuda")
        roi = _roi_volume((B, *dims, 1), gen)
        gtv = torch.rand((B, *dims, 1), generator=gen, device="cuda") + 0.05
        r = torch.rand((B, *dims, 1), generator=gen, device="cuda")
        gtv = torch.where(r < 0.03, torch.zeros_like(gtv), gtv)                       # tau == 0: inf and NaN ratios
        pv = (gtv + 0.2 * torch.randn((B, *dims, 1), generator=gen, device="cuda")).clamp_min(0.0)
        pv = torch.where(r < 0.015, torch.zeros_like(pv), pv)                          # ... half of them 0 / 0
        gt = gtv.to(dtype)
        pred = _pitched((B, *dims, 1), 2, dtype, pv)
        n = len(ROI_INDICES)
        out = FlatGuard(B * (n + 1) * 8, torch.float64)
        L.check(L.lib.coma_eval_stats(L.ct(pred), L.ct(gt), L.ct(roi), L.ptr(ids), n, L.ptr(out.t), L.stream()), "eval_stats")
        assert out.untouched()
        got = out.t.view(B, n + 1, 8)
        ref, mass = NP.eval_stats_ref(pred, gt, roi, ROI_INDICES)
        assert torch.equal(torch.isinf(got), torch.isinf(ref)) and not bool(torch.isnan(got).any())
        assert bool(torch.isinf(ref[:, :n, 6]).any()) and bool((ref[:, :, 7] < ref[:, :, 0]).any()), "the case must hold inf and NaN ratios"
        fin = ~torch.isinf(ref)
        z = torch.zeros_like(ref)
        got, ref, mass = torch.where(fin, got, z), torch.where(fin, ref, z), torch.where(fin, mass, z)
        assert torch.equal(got[..., 0], ref[..., 0]) and torch.equal(got[..., 7], ref[..., 7]), "counts"
        K = torch.tensor([0, 1, 2, 0, 0, 0, 2, 0], dtype=torch.float64, device="cuda")
        bound = 4 * NP.U_F64 * ref.abs() + (2.0 * K * R.U_F32 + V * NP.U_F64) * mass
        _put(f"eval_stats-{name}-{dt}", ratio=R.check_elementwise(got, ref, bound, "eval stats"))
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev_step", [False, True], ids=["host_step", "step_dev"])
@pytest.mark.parametrize("case", NP.ADAMW_CASES, ids=lambda c: c[0])
def test_adamw(case, dev_step):
    """adamw_k over more than one pass: the float4 path with a 3-element scalar tail, and the scalar path on slices that are
    not 16-byte aligned; three steps, with the host step count and with the device counter (host `step` then holds a wrong
    value: the device one must win).  m, v and the update p - p0 against the fp64 recurrence, each within the bound that
    _nonconv_plan.adamw_step carries along (the 1 - powf(beta, t) term included)."""
    ops, L = _ops()
    name, n, off = case
    gen = _gen("adamw", name)
    lr, b1, b2, eps, wd = NP.ADAMW_HP
    st = {}
    try:
        bufs = [FlatGuard(n, torch.float32, off) for _ in range(4)]
        p, g, m, v = (b.t for b in bufs)
        assert (p.data_ptr() % 16 == 0) == (off == 0)
        p.copy_(torch.randn(n, generator=gen, device="cuda"))
        m.zero_()
        v.zero_()
        p0 = p.clone()
        ref = NP.adamw_init(p0)
        step_dev = torch.zeros(1, dtype=torch.int32, device="cuda") if dev_step else None
        for t in (1, 2, 3):
            g.copy_(torch.randn(n, generator=gen, device="cuda") * (0.5 if t == 2 else 1.0))
            if dev_step:
                step_dev.fill_(t)
            ops.adamw_(p, g, m, v, lr, b1, b2, eps, wd, 7 if dev_step else t, step_dev)
            info = NP.adamw_step(ref, g, t)
            st[f"m{t}"] = R.check_elementwise(m, ref["m"], ref["bm"], f"m step {t}")
            st[f"v{t}"] = R.check_elementwise(v, ref["v"], ref["bv"], f"v step {t}")
            upd, upd_ref = p.double() - p0.double(), ref["p"] - p0.double()
            st[f"upd{t}"] = R.check_elementwise(upd, upd_ref, ref["bp"], f"p - p0 step {t}")
            st[f"upd_rel{t}"] = float(((upd - upd_ref).abs() / upd_ref.abs().clamp_min(1e-30)).median())
            small = p0.abs() < 1e-2          # there the roundings relative to |p| vanish: what is left is the error of s itself
            st[f"upd_rel_small_p{t}"] = float(((upd - upd_ref).abs() / upd_ref.abs().clamp_min(1e-30))[small].median())
            st[f"bias_share{t}"] = info["bias_share"]
            print(f"adamw {name} {'step_dev' if dev_step else 'host'} step {t}: worst ratio m {st[f'm{t}']:.3g} v {st[f'v{t}']:.3g} "
                  f"update {st[f'upd{t}']:.3g}; bound of the bias-correction term: bc1 {info['e_bc1']:.2e} sqrt(bc2) {info['e_bc2s']:.2e}")
            del upd, upd_ref
        assert all(b.untouched() for b in bufs)
        _put(f"adamw-{name}-{'step_dev' if dev_step else 'host_step'}", **st)
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# column sums: spatial mean, conv bias gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", NP.colsum_rows(), ids=lambda r: "-".join(str(v) for v in r))
def test_spatial_mean_and_bias_gradient(row):
    """stats_partial_k's per-chunk partial rows + colsum_finalize_k with more than 64 chunks (below the 1024 / G cap, ragged
    last chunk) and past the cap, on pitched tensors: coma_spatial_mean (instance rows) and the bias gradient of
    coma_conv_wgrad (batch rows, or per-sample).  fp32 terms go straight to fp64: K = 0; bf16 terms are summed in fp32 over
    bursts of 8 rows first: K = 8."""
    ops, L = _ops()
    what, dt, C, ld, V = row
    dtype, B = DT[dt], 2
    gen = _gen("colsum", row)
    s = L.stream()
    K = 8 if dtype == torch.bfloat16 else 0
    try:
        x = _pitched((B, 1, 1, V, C), ld, dtype, torch.randn((B, 1, 1, V, C), generator=gen, device="cuda") + 0.25)
        xd = x.double().reshape(B, V, C)
        if what == "mean":
            out = FlatGuard(B * C, torch.float32)
            ws = L.workspace(L.lib.coma_norm_ws_bytes(L.ct(x)), x.device)
            L.check(L.lib.coma_spatial_mean(L.ct(x), L.ptr(out.t), L.ptr(ws), ws.numel(), s), "spatial_mean")
            ref, mass, n = xd.mean(1), xd.abs().mean(1), V
        else:
            ps = what == "bias_ps"
            x1 = ops._new((B, 1, 1, V, 1), dtype, x.device)
            x1.copy_(torch.randn((B, 1, 1, V, 1), generator=gen, device="cuda"))
            d = ops._desc(1, 1, 0, ps, 0)
            out = FlatGuard((B if ps else 1) * C, torch.float32)
            dwk = torch.zeros(((B if ps else 1), 1, C, 1), device="cuda")
            nws = max(L.lib.coma_conv_wgrad_ws_bytes(d, L.ct(x1), L.ct(x)), L.lib.coma_norm_ws_bytes(L.ct(x)))
            ws = L.workspace(nws, x.device)
            L.check(L.lib.coma_conv_wgrad(d, L.ct(x1), L.ct(x), L.ptr(dwk), L.ptr(out.t), L.ptr(ws), ws.numel(), 0, s), "conv_wgrad")
            ref, mass, n = (xd.sum(1), xd.abs().sum(1), V) if ps else (xd.sum((0, 1)), xd.abs().sum((0, 1)), B * V)
        assert out.untouched()
        ratio = R.check_elementwise(out.t.view(ref.shape), ref, _bound(ref, mass, K, R.U_F32, n), what)
        _put("colsum-" + "-".join(str(v) for v in row), ratio=ratio)
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# NormAct fp32
# ---------------------------------------------------------------------------------------------------------------------
def _norm_case(V_or_dims, B, C, ld, mode, act, affine, tag):
    """fp32 roundings behind one element, from norm_act_fwd_k / norm_act_bwd_apply_k: y = act(fma(x, sc, sh)) with mean and
    rstd rounded from double (2), sc = rstd gamma (1), sh = beta - mean sc (2), the fma (1), the activation's product (1), a
    margin of 2: K = 9 (+ 5 for the sigmoid's expf, sum, quotient).  dx = rstd gamma (dz - s1 - xhat s2): xhat (2 + the 2 of
    mean, rstd), z (2), dz (1), s1 / s2 rounded from double (2), xhat s2 (1), two differences (2), two products (2), a
    margin of 2: K = 16 (+ 6 for the sigmoid's derivative).  Where |z| is below its own rounding error the kernel may take
    the other branch of the activation: there the bound of dx grows by the jump of the slope times |dy| rstd |gamma|.
    The three parameter sums add terms of about 8 roundings in double: K = 10."""
    ops, L = _ops()
    dims = V_or_dims if isinstance(V_or_dims, tuple) else (1, 1, V_or_dims)
    xs = (B, *dims, C)
    gen = _gen("norm", tag)
    has_slope = act in ("prelu", "prelu_relu")
    x = _pitched(xs, ld, torch.float32, torch.randn(xs, generator=gen, device="cuda") * 1.5 + 0.7)
    dy = torch.randn(xs, generator=gen, device="cuda")
    gamma = (torch.rand(C, generator=gen, device="cuda") + 0.5) if affine else None
    beta = (torch.randn(C, generator=gen, device="cuda") * 0.3) if affine else None
    slope = torch.tensor([-0.3 if act == "prelu_relu" else 0.2], device="cuda") if has_slope else None
    ref = NP.norm_act64(x, dy, mode, act, gamma, beta, slope)
    xg = x.detach().requires_grad_(True)
    gg, bg, sg = (None if t is None else t.clone().requires_grad_(True) for t in (gamma, beta, slope))
    rm = torch.zeros(C, device="cuda") if (affine and mode == "batch") else None
    rv = torch.ones(C, device="cuda") if (affine and mode == "batch") else None
    yb = Guard(xs, torch.float32, ld + 4, 0 if ld % 4 == 0 else 1)
    code = {"batch": L.NORM_BATCH, "instance": L.NORM_INSTANCE}[mode]
    with _guarded_new(ops) as made:
        y = ops.NormAct.apply(xg, gg, bg, sg, rm, rv, code, NP.NORM_ACTS.index(act), 0.1, 1e-5, True, ops.Out(yb.t))
        y.backward(dy)
        torch.cuda.synchronize()
    assert yb.untouched() and len(made) >= 1 and all(g.untouched() for g in made)
    sig = act == "sigmoid"
    st = {"y": R.check_elementwise(y, ref["y"], _bound(ref["y"], ref["mag_y"], 9 + 5 * sig, R.U_F32), "y")}
    near = (ref["z"].abs() <= 2 * 8 * R.U_F32 * ref["mag_y"]).double()
    st["kinks"] = int(near.sum()) if act not in ("none", "sigmoid") else 0
    st["dx"] = R.check_elementwise(xg.grad, ref["dx"], _bound(ref["dx"], ref["mag_dx"], 16 + 6 * sig, R.U_F32) + near * ref["kink"], "dx")
    nrow = x.numel() // C
    for nm, got in (("dgamma", gg), ("dbeta", bg), ("dslope", sg)):
        if got is not None:
            st[nm] = R.check_elementwise(got.grad, ref[nm], _bound(ref[nm], ref["mass"][nm], 10, R.U_F32, nrow), nm)
    if rm is not None:
        # (1 - momentum) * old + momentum * float(statistic): K = 4 over the two terms
        for nm, got, old in (("running_mean", rm, 0.0), ("running_var", rv, 0.9)):
            st[nm] = R.check_elementwise(got, ref[nm], _bound(ref[nm], old + (ref[nm] - old).abs(), 4, R.U_F32), nm)
    _put(f"norm_f32-{tag}", **st)


@pytest.mark.parametrize("row", NP.norm_f32_rows(), ids=lambda r: "-".join(str(v) for v in r[:6]))
def test_norm_act_f32_ragged_rows(row):
    """NormAct forward + backward in fp32 (stats_partial_k and norm_bwd_partial_k with their fp32 burst widths, both apply
    kernels) at row counts with a ragged last chunk below and past the 1024 / G chunk cap, vec 4 and vec 1."""
    V, C, ld, mode, act, affine, _rows = row
    try:
        _norm_case(V, 2, C, ld, mode, act, affine, "-".join(str(v) for v in row[:6]))
    finally:
        _free()


@pytest.mark.parametrize("mode,act", [("batch", "relu"), ("instance", "prelu")])
def test_norm_act_f32_over_apply_caps(mode, act):
    """One fp32 shape past the 4096-block caps of both apply kernels (4 and 2 voxels per thread and trip)."""
    dims, B, C = NP.NORM_BIG
    try:
        _norm_case(dims, B, C, C, mode, act, mode == "batch", f"big-{mode}-{act}")
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# GateFused fp32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NP.GATE_BIG, ids=lambda c: c[0])
def test_gate_fused_f32(case):
    """ops.GateFused in fp32 past the block caps of all five kernels (mid forward and apply backward: 1024 / B blocks of
    2 * 256 / cv voxels; apply forward and mid-backward apply: 4096 blocks), 16-byte vectors and, through slices at an odd
    channel offset, the scalar form.  fp32 roundings behind one element, from gate.hip: s = relu(fma(g, scg, fma(x, scx, sh)))
    with scg, scx, sh from rounded statistics: 8; psi_raw: F fma's over the lanes + the bias: F + 2; BN_psi's affine map: 6;
    the sigmoid: 4; the product with x: 1 -- K = F + 21 for att, psi and dx.  The backward adds the dot over C channels, dz
    (3), d(psi_raw) (8), the relu mask and w (1), the BatchNorm backward (10): K = C + F + 43 for dg1raw / dx1raw and the
    parameter sums.  Where |s| is below its own rounding error the relu mask may differ: the bound of dg1raw / dx1raw grows
    there by what the masked term moves."""
    ops, L = _ops()
    name, dims, B, C, F_, vec = case
    gen = _gen("gate", name)
    xs, fs = (B, *dims, C), (B, *dims, F_)
    off = 0 if vec == 4 else 1
    s = L.stream()
    try:
        mk = lambda shape, scale=1.0: _pitched(shape, shape[-1] + 4, torch.float32, torch.randn(shape, generator=gen, device="cuda") * scale) \
            if off == 0 else Guard(shape, torch.float32, shape[-1] + 2, 1, fill=3.0e4).t.copy_(torch.randn(shape, generator=gen, device="cuda") * scale)
        x, g1, x1 = mk(xs), mk(fs, 1.3), mk(fs, 0.8)
        datt = torch.randn(xs, generator=gen, device="cuda")
        un = lambda n, lo, hi: torch.rand(n, generator=gen, device="cuda") * (hi - lo) + lo
        P = dict(gam_g=un(F_, 0.5, 1.5), bet_g=un(F_, -0.3, 0.3), gam_x=un(F_, 0.5, 1.5), bet_x=un(F_, -0.3, 0.3),
                 w=torch.randn(F_, generator=gen, device="cuda") * 0.5, b=un(1, -0.2, 0.2), gam_p=un(1, 0.5, 1.5), bet_p=un(1, -0.3, 0.3))
        ref = NP.gate64(x, g1, x1, P, datt)
        sums = []
        for t in (g1, x1):
            rec = ops.stat_record(1, F_, 2, t.device)
            L.check(L.lib.coma_norm_stats(L.ct(t), L.NORM_BATCH, L.ptr(rec), s), "norm_stats")
            sums.append(rec)
        leaf = {k: v.clone().requires_grad_(k != "b") for k, v in P.items()}
        xg, g1g, x1g = (t.detach().requires_grad_(True) for t in (x, g1, x1))
        run = [torch.zeros(F_, device="cuda"), torch.ones(F_, device="cuda"), torch.zeros(F_, device="cuda"), torch.ones(F_, device="cuda"),
               torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")]
        ab = Guard(xs, torch.float32, C + (4 if off == 0 else 2), off)
        with _guarded_new(ops) as made:
            att, psi = ops.GateFused.apply(xg, g1g, x1g, sums[0], sums[1], leaf["gam_g"], leaf["bet_g"], leaf["gam_x"], leaf["bet_x"],
                                           leaf["w"], leaf["b"], leaf["gam_p"], leaf["bet_p"], tuple(run), 0.1, (1e-5, 1e-5, 1e-5), ops.Out(ab.t))
            att.backward(datt)
            torch.cuda.synchronize()
        assert ab.untouched() and len(made) >= 7 and all(g.untouched() for g in made)   # s, psi_raw, psi, dx, dz, dg1raw, dx1raw
        Kf, Kb = F_ + 21, C + F_ + 43
        st = {"att": R.check_elementwise(att, ref["att"], _bound(ref["att"], ref["A_att"], Kf, R.U_F32), "att"),
              "psi": R.check_elementwise(psi, ref["psi"], _bound(ref["psi"], ref["A_psi"], Kf, R.U_F32), "psi"),
              "dx": R.check_elementwise(xg.grad, ref["dx"], _bound(ref["dx"], ref["A_dx"], Kf, R.U_F32), "dx")}
        near = (ref["t"].abs() <= 2 * 8 * R.U_F32 * ref["A_t"]).double().reshape(fs)
        st["kinks"] = int(near.sum())
        for nm, got in (("dg1", g1g.grad), ("dx1", x1g.grad)):
            st[nm] = R.check_elementwise(got, ref[nm], _bound(ref[nm], ref["A_" + nm], Kb, R.U_F32) + near * ref["kink_" + nm], nm)
        n = B * NP.vol(dims)
        for nm, key in (("dgam_g", "gam_g"), ("dbet_g", "bet_g"), ("dgam_x", "gam_x"), ("dbet_x", "bet_x"), ("dw", "w"),
                        ("dgam_p", "gam_p"), ("dbet_p", "bet_p")):
            st[nm] = R.check_elementwise(leaf[key].grad, ref[nm], _bound(ref[nm], ref["m_" + nm], Kb, R.U_F32, n), nm)
        for i, nm in enumerate(("rm_g", "rv_g", "rm_x", "rv_x", "rm_p", "rv_p")):
            old = 0.9 if nm.startswith("rv") else 0.0
            st[nm] = R.check_elementwise(run[i], ref[nm], _bound(ref[nm], old + (ref[nm] - old).abs(), 4, R.U_F32), nm)
        _put(f"gate_f32-{name}", **st)
    finally:
        _free()


def test_zz_report():
    """Prints the measured worst ratio of every case that ran (to its bound; `exact` where the comparison is bit-exact)."""
    for k, v in REPORT.items():
        print("ROW", k, {a: (float(f"{b:.4g}") if isinstance(b, float) else b) for a, b in v.items()})
    out = os.environ.get("NONCONV_SIZES_REPORT")
    if out:
        with open(out, "w") as f:
            for k, v in REPORT.items():
                f.write("ROW %s %s\n" % (k, {a: (float(f"{b:.4g}") if isinstance(b, float) else b) for a, b in v.items()}))
