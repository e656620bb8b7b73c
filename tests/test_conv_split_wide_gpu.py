"""The wide split (coma_conv_desc.algo = 5; csrc/conv_split.hip): the stride-2 families on the bf16 matrix pipe as a two-term
split, through the C ABI against the fp64 references of oracle/fp64_ref.py.

  tfwd   -- transposed stride-2 forward (the up-convolutions)                 conv_split_tconv_k
  dgrad  -- data gradient of a stride-2 convolution (the same kernel, form 1)  conv_split_tconv_k
  wgrad  -- weight gradient of a stride-2 convolution                          conv_split_wgrad2_k<0>
  twgrad -- weight gradient of a transposed stride-2 convolution               conv_split_wgrad2_k<1>

Helpers, operands (Gaussian fp32, not bf16-exact; finite garbage in foreign lanes) and the two checks (per-element bound
elem_bound(ref, A, 3K, 2^-24) + 2^-14 A; max slab rel-L2 <= 1e-4) are those of test_conv_split_gpu.py, shared through
tests/_split_abi.py; the exact kernels (algo = 0) run through the same assertions as the control.

A case is (B, coarse D, H, W, coarse channels, fine channels, coarse pitch, fine pitch, odd): the coarse grid is the dense
side (tiles of 2 x 4 x 32 voxels for the transposed kernel, 1 x 2 x 32 for the weight gradients), the fine grid is
2 x coarse, or 2 x coarse - 1 with `odd` for the two operations whose fine side is a convolution's INPUT (dgrad, wgrad).
"""
import pytest
import torch

from oracle import fp64_ref as R
from _split_abi import SLAB_TOL, _buf, _check, _free, _gen, _ops, _rand, _weights

pytestmark = pytest.mark.gpu

CASES = [
    (2, 3, 5, 33, 64, 32, 64, 32, False),
    (1, 3, 6, 40, 32, 32, 32, 32, True),
    (2, 2, 4, 32, 128, 64, 128, 64, False),
    (1, 3, 5, 34, 32, 32, 64, 96, True),       # both sides channel slices of wider buffers
]
_ids = lambda c: "x".join(str(int(v)) for v in c)
WHATS = ["tfwd", "dgrad", "wgrad", "twgrad"]
NEW = {"tfwd": "conv_split_tconv_k", "dgrad": "conv_split_tconv_k", "wgrad": "conv_split_wgrad2_k<0>", "twgrad": "conv_split_wgrad2_k<1>"}
OLD = {"tfwd": "conv_mfma_tconv_k<float", "dgrad": "conv_mfma_tconv_k<float", "wgrad": "conv_f32_wgrad16_k<2, 0>",
       "twgrad": "conv_f32_wgrad16_k<2, 1>"}


def _grids(case, fine_is_input):
    B, D, H, W, cc, cf, cld, fld, odd = case
    o = 1 if (odd and fine_is_input) else 0
    return (B, D, H, W), (B, 2 * D - o, 2 * H - o, 2 * W - o)


def _foreign_untouched(buf, shape, ld, c, fill):
    if ld > c:
        assert bool((buf.as_strided(tuple(shape[:4]) + (ld - c,), buf.stride(), buf.storage_offset() + c) == fill).all()), \
            "foreign lanes of the output written"


def _tfwd(case, ps, algo, key, norm=None, has_bias=False):
    """transposed forward: x coarse (cc channels) -> y fine (cf channels)"""
    ops, L = _ops()
    B, D, H, W, cc, cf, cld, fld, odd = case
    cg, fg = _grids(case, False)
    gen = _gen("tfwd", case, ps, key)
    x = _rand(cg + (cc,), cld, gen)
    wk = _weights(B if ps else 1, cf, cc, gen)
    bias = torch.randn(((B, cf) if ps else (cf,)), generator=gen, device="cuda") * 0.5 if has_bias else None
    ybuf = _buf(fg + (cf,), fld, -7.0)
    d = ops._desc(3, 2, 1, ps, algo)
    picked = L.lib.coma_conv_pick_algo(d, L.ct(x), L.ct(ybuf))
    y, sums = ops._conv_fwd(x, wk, bias, 3, 2, 1, ps, algo, ops.Out(ybuf), norm)
    kernel = L.lib.coma_last_kernel().decode()
    _foreign_untouched(ybuf, fg, fld, cf, -7.0)
    ref, A = R.conv_fwd(x.double(), wk.double(), None if bias is None else bias.double(), 3, 2, True)
    return dict(y=y, ref=ref, A=A, sums=sums, kernel=kernel, picked=picked, K=27 * cc + 1)


def _dgrad(case, ps, algo, key, accumulate=False):
    """data gradient of the stride-2 convolution fine (cf) -> coarse (cc): the transposed form on (dy coarse -> dx fine)"""
    ops, L = _ops()
    B, D, H, W, cc, cf, cld, fld, odd = case
    cg, fg = _grids(case, True)
    gen = _gen("dgrad", case, ps, key)
    dy = _rand(cg + (cc,), cld, gen)
    wk_d = _weights(B if ps else 1, cc, cf, gen).transpose(2, 3).contiguous()      # [Bw, 27, fine channels, coarse channels]
    dx = _buf(fg + (cf,), fld, -7.0)
    base = None
    if accumulate:
        base = torch.randn(fg + (cf,), generator=gen, device="cuda")
        dx.copy_(base)
    dd, cdy, cdx = ops._desc(3, 2, 1, ps, algo), L.ct(dy), L.ct(dx)
    picked = L.lib.coma_conv_pick_algo(dd, cdy, cdx)
    acc_ok = L.lib.coma_conv_accumulate_ok(dd, cdy, cdx)
    ws = L.workspace(L.lib.coma_conv_fwd_ws_bytes(dd, cdy, cdx), dy.device)
    flags = L.ACCUMULATE if accumulate else 0
    L.check(L.lib.coma_conv_fwd_ws(dd, cdy, L.ptr(wk_d), L.F32, None, cdx, L.ptr(ws), ws.numel(), flags, L.stream()), "coma_conv_fwd_ws(dgrad)")
    kernel = L.lib.coma_last_kernel().decode()
    _foreign_untouched(dx, fg, fld, cf, -7.0)
    ref, A = R.conv_dgrad(dy.double(), wk_d.double().transpose(2, 3), fg[1:4], 3, 2, False)
    if accumulate:
        ref = ref + base.double()          # (A stays the convolution's: the epilogue's addition is the bound's |base| term)
    return dict(y=dx, ref=ref, A=A, kernel=kernel, picked=picked, K=27 * cc + 1, acc_ok=acc_ok,
                base=None if base is None else base.double())


def _wgrad(case, ps, algo, key, transposed=False):
    """wgrad: stride-2 convolution x fine (cf) -> dy coarse (cc); twgrad: transposed, x coarse (cc) -> dy fine (cf)"""
    ops, L = _ops()
    B, D, H, W, cc, cf, cld, fld, odd = case
    cg, fg = _grids(case, not transposed)
    gen = _gen("wgrad", case, ps, key, transposed)
    if transposed:
        x, dy, cin, cout = _rand(cg + (cc,), cld, gen), _rand(fg + (cf,), fld, gen), cc, cf
    else:
        x, dy, cin, cout = _rand(fg + (cf,), fld, gen), _rand(cg + (cc,), cld, gen), cf, cc
    form = 1 if transposed else 0
    picked = L.lib.coma_conv_wgrad_algo(ops._desc(3, 2, form, ps, algo), L.ct(x), L.ct(dy))
    _, dwk, _ = ops._conv_bwd(x, None, dy, 3, 2, form, ps, algo, (B if ps else 1, 27, cout, cin), False, True, 0, None)
    kernel = L.lib.coma_last_kernel().decode()
    ref, A = R.conv_wgrad(x.double(), dy.double(), 3, 2, transposed, ps)
    return dict(y=dwk, ref=ref, A=A, kernel=kernel, picked=picked, K=D * H * W * (1 if ps else B))


_RUN = {"tfwd": _tfwd, "dgrad": _dgrad, "wgrad": _wgrad, "twgrad": lambda c, ps, a, k: _wgrad(c, ps, a, k, True)}


# ---------------------------------------------------------------------------------------------------------------------
# 1. dispatch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_dispatch_in_scope(case, ps):
    """algo = 5 answers 4 and launches the new kernels; algo = 4 and algo = 0 answer 3 and launch the exact kernels."""
    try:
        with torch.no_grad():
            for what in WHATS:
                r5 = _RUN[what](case, ps, 5, "dispatch")
                assert r5["picked"] == 4, (what, r5["picked"])
                assert r5["kernel"].startswith(NEW[what]), (what, r5["kernel"])
                for algo in (4, 0):
                    r = _RUN[what](case, ps, algo, "dispatch")
                    assert r["picked"] == 3, (what, algo, r["picked"])
                    assert r["kernel"].startswith(OLD[what]), (what, algo, r["kernel"])
    finally:
        _free()


# out-of-scope problems: (name, x shape, Cout, stride, dtype, launches compared).  "s2fwd": the forward of a stride-2
# convolution stays on the gather kernel although its data gradient and weight gradient are in scope.
OUT_OF_SCOPE = [
    ("coarseW16", (2, 4, 16, 32, 32), 32, 2, torch.float32, "fdw"),
    ("s2fwd", (2, 4, 8, 64, 32), 64, 2, torch.float32, "f"),
    ("C8", (1, 4, 8, 64, 8), 8, 2, torch.float32, "fdw"),
    ("bf16", (2, 4, 8, 64, 32), 64, 2, torch.bfloat16, "fdw"),
    ("stride1", (2, 4, 8, 32, 32), 32, 1, torch.float32, "fdw"),
]


@pytest.mark.parametrize("prob", OUT_OF_SCOPE, ids=lambda p: p[0])
def test_dispatch_out_of_scope(prob):
    """On each problem algo = 5 answers what algo = 4 answers and launches the same kernels; the stride-1 problem still
    reaches conv_split_halo_k / conv_split_wgrad_k."""
    ops, L = _ops()
    name, xs, cout, stride, dt, which = prob
    B, cin = xs[0], xs[4]
    ys = (B, *R.out_grid(xs[1:4], 3, stride, False), cout)
    try:
        with torch.no_grad():
            gen = _gen("oos", prob[:4])
            x = (torch.randn(xs, generator=gen, device="cuda")).to(dt)
            dy = (torch.randn(ys, generator=gen, device="cuda")).to(dt)
            wk = _weights(1, cout, cin, _gen("oosw", prob[:4]))
            wdt = lambda a: torch.bfloat16 if a == 2 else torch.float32
            got = {}
            for algo in (4, 5):
                a_f, a_d = ops.pick_algo(xs, dt, cout, 3, stride, False, False, x.device, algo)
                a_w = L.lib.coma_conv_wgrad_algo(ops._desc(3, stride, 0, False, algo), L.ct(x), L.ct(dy))
                picks, kernels = [], []
                if "f" in which:
                    ops._conv_fwd(x, wk.to(wdt(a_f)), None, 3, stride, 0, False, algo, None, None)
                    picks.append(a_f); kernels.append(L.lib.coma_last_kernel().decode())
                if "d" in which:
                    ops._conv_bwd(x, wk.transpose(2, 3).contiguous().to(wdt(a_d)), dy, 3, stride, 0, False, algo,
                                  (1, 27, cout, cin), True, False, 0, None)
                    picks.append(a_d); kernels.append(L.lib.coma_last_kernel().decode())
                if "w" in which:
                    ops._conv_bwd(x, None, dy, 3, stride, 0, False, algo, (1, 27, cout, cin), False, True, 0, None)
                    picks.append(a_w); kernels.append(L.lib.coma_last_kernel().decode())
                torch.cuda.synchronize()
                got[algo] = (picks, kernels)
            assert got[5] == got[4], (got[5], got[4])
            assert not any(k.startswith(("conv_split_tconv_k", "conv_split_wgrad2_k")) for k in got[5][1]), got[5][1]
            if name == "stride1":
                assert got[5][0] == [4, 4, 4], got[5][0]
                assert got[5][1][0].startswith("conv_split_halo_k") and got[5][1][1].startswith("conv_split_halo_k") and \
                    got[5][1][2].startswith("conv_split_wgrad_k"), got[5][1]
            else:
                assert all(a != 4 for a in got[5][0]), got[5][0]
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# 2. element bound and slab rel-L2, the new kernels and the exact-fp32 control
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [5, 0], ids=["split", "exact-control"])
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("what", WHATS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kernel_matches_fp64(case, what, ps, algo):
    try:
        with torch.no_grad():
            r = _RUN[what](case, ps, algo, "parity")
            assert r["picked"] == (4 if algo == 5 else 3), r["picked"]
            assert r["kernel"].startswith(NEW[what] if algo == 5 else OLD[what]), r["kernel"]
            _check(r, f"{what} {_ids(case)} ps={ps} algo={algo}")
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# 3. accumulate, statistics, COMA_ZEROED_OUT
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [5, 0], ids=["split", "exact-control"])
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_dgrad_accumulates(case, ps, algo):
    """COMA_ACCUMULATE: the result is prior content + reference within the same bound (+ 2^-24 |prior| for the epilogue's
    addition); coma_conv_accumulate_ok and the scratch query agree between algo 0 and 5."""
    ops, L = _ops()
    try:
        with torch.no_grad():
            r = _dgrad(case, ps, algo, "accum", accumulate=True)
            assert r["acc_ok"] == 1
            assert r["kernel"].startswith(NEW["dgrad"] if algo == 5 else OLD["dgrad"]), r["kernel"]
            _check(r, f"dgrad+= {_ids(case)} ps={ps} algo={algo}")
            B, D, H, W, cc, cf, cld, fld, odd = case
            cg, fg = _grids(case, True)
            dy, dx = _buf(cg + (cc,), cld, 0.0), _buf(fg + (cf,), fld, 0.0)
            d5, d0 = ops._desc(3, 2, 1, ps, 5), ops._desc(3, 2, 1, ps, 0)
            assert L.lib.coma_conv_accumulate_ok(d5, L.ct(dy), L.ct(dx)) == L.lib.coma_conv_accumulate_ok(d0, L.ct(dy), L.ct(dx)) == 1
            assert L.lib.coma_conv_fwd_ws_bytes(d5, L.ct(dy), L.ct(dx)) == L.lib.coma_conv_fwd_ws_bytes(d0, L.ct(dy), L.ct(dx))
    finally:
        _free()


@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("norm", ["batch", "instance"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_bias_and_stats(case, norm, ps):
    """Transposed forward with bias and the {sum, sumsq} record out of coma_conv_fwd_norm_stats: the output meets both checks
    and the statistics describe the STORED output (bounds of test_conv_split_gpu.test_forward_bias_and_fused_stats:
    1e-5 (1 + max |mean|) and rel 1e-5 on rstd)."""
    ops, L = _ops()
    B, cf = case[0], case[5]
    try:
        with torch.no_grad():
            mode = L.NORM_BATCH if norm == "batch" else L.NORM_INSTANCE
            r = _tfwd(case, ps, 5, "stats", norm=mode, has_bias=True)
            assert r["picked"] == 4 and r["kernel"].startswith(NEW["tfwd"]), (r["picked"], r["kernel"])
            _check(r, f"tfwd+bias+{norm} {_ids(case)} ps={ps}")
            vox = r["y"].shape[1] * r["y"].shape[2] * r["y"].shape[3]
            G = B if mode == L.NORM_INSTANCE else 1
            n = vox * (1 if G == B else B)
            mean, rstd = ops.stats_from_sums(r["sums"], G, cf, n, 1e-5)
            yf = r["y"].double()
            red = (1, 2, 3) if G == B else (0, 1, 2, 3)
            m_ref = yf.mean(red).reshape(mean.shape)
            v_ref = yf.var(red, unbiased=False).reshape(mean.shape)
            assert float((mean.double() - m_ref).abs().max()) < 1e-5 * (1.0 + float(m_ref.abs().max()))
            assert float(((rstd.double() - (v_ref + 1e-5).rsqrt()).abs() / (v_ref + 1e-5).rsqrt()).max()) < 1e-5
    finally:
        _free()


@pytest.mark.parametrize("form", [0, 1], ids=["stride2", "transposed"])
def test_wgrad_zeroed_out_flag(form):
    """COMA_ZEROED_OUT: the kernel adds into a caller-zeroed dwk and gives the same result as with its own memset."""
    ops, L = _ops()
    gen = _gen("zeroed", form)
    coarse = torch.randn((2, 3, 4, 32, 32), generator=gen, device="cuda")
    fine = torch.randn((2, 6, 8, 64, 32), generator=gen, device="cuda")
    x, dy = (fine, coarse) if form == 0 else (coarse, fine)
    d = ops._desc(3, 2, form, True, 5)
    assert L.lib.coma_conv_wgrad_algo(d, L.ct(x), L.ct(dy)) == 4
    ws = L.workspace(L.lib.coma_conv_wgrad_ws_bytes(d, L.ct(x), L.ct(dy)), x.device)
    a = torch.full((2, 27, 32, 32), 5.0, device="cuda")
    b = torch.zeros((2, 27, 32, 32), device="cuda")
    L.check(L.lib.coma_conv_wgrad(d, L.ct(x), L.ct(dy), L.ptr(a), None, L.ptr(ws), ws.numel(), 0, L.stream()), "wgrad")
    assert L.lib.coma_last_kernel().decode().startswith("conv_split_wgrad2_k")
    L.check(L.lib.coma_conv_wgrad(d, L.ct(x), L.ct(dy), L.ptr(b), None, L.ptr(ws), ws.numel(), L.ZEROED_OUT, L.stream()), "wgrad")
    torch.cuda.synchronize()
    ref, _ = R.conv_wgrad(x.double(), dy.double(), 3, 2, form == 1, True)
    assert R.slab_rel_l2(a, ref, 2) <= SLAB_TOL and R.slab_rel_l2(b, ref, 2) <= SLAB_TOL
    _free()


# ---------------------------------------------------------------------------------------------------------------------
# 4. production shapes: the eight launches of the 128^3 x 2 step that fall in scope, once each at full size
# ---------------------------------------------------------------------------------------------------------------------
PRODUCTION = [
    ("tfwd", (2, 32, 32, 32, 128, 64, 128, 64, False)),       # up2: 128 -> 64 from 32^3
    ("tfwd", (2, 64, 64, 64, 64, 32, 64, 32, False)),         # up1: 64 -> 32 from 64^3
    ("dgrad", (2, 32, 32, 32, 128, 64, 128, 64, False)),      # enc2 conv0: dy 128 channels at 32^3 -> 64 channels at 64^3
    ("dgrad", (2, 64, 64, 64, 64, 32, 64, 32, False)),        # enc1 conv0: dy 64 channels at 64^3 -> 32 channels at 128^3
    ("wgrad", (2, 32, 32, 32, 128, 64, 128, 64, False)),      # enc2 conv0: 64 -> 128 at 64^3
    ("wgrad", (2, 64, 64, 64, 64, 32, 64, 32, False)),        # enc1 conv0: 32 -> 64 at 128^3
    ("twgrad", (2, 32, 32, 32, 128, 64, 128, 64, False)),     # up2
    ("twgrad", (2, 64, 64, 64, 64, 32, 64, 32, False)),       # up1
]


@pytest.mark.parametrize("row", PRODUCTION, ids=lambda r: f"{r[0]}-{r[1][1]}cubed-{r[1][4]}to{r[1][5]}")
def test_production_shape(row):
    """Persistent tile loops, the prefetch across tiles and passes and the 262k / 32k-voxel reductions only run at full
    size (per-sample weights, as the CondConv layers of the step; reference computed in slabs by fp64_ref)."""
    what, case = row
    ops, L = _ops()
    try:
        with torch.no_grad():
            if what == "tfwd":
                r = _tfwd(case, True, 5, "prod", norm=L.NORM_INSTANCE, has_bias=True)
            elif what == "dgrad":
                r = _dgrad(case, True, 5, "prod", accumulate=True)
            else:
                r = _RUN[what](case, True, 5, "prod")
            assert r["picked"] == 4 and r["kernel"].startswith(NEW[what]), (r["picked"], r["kernel"])
            _check(r, f"{what} production {_ids(case)}")
    finally:
        _free()
