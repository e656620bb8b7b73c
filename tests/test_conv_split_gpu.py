"""The split-bf16 convolution kernels (coma_conv_desc.algo = 4; csrc/conv_split.hip) through the C ABI against the fp64
references of oracle/fp64_ref.py.

fp32 tensors and fp32 kernel-layout weights; inside the kernels every operand is a = a_hi + a_lo + r with
a_hi = bf16(a), a_lo = bf16(a - a_hi) and a product is a_hi b_hi + a_hi b_lo + a_lo b_hi (three bf16 MFMAs, fp32
accumulation).  Operands here are Gaussian fp32, NOT bf16-exact: bf16-exact inputs have lo == 0 and would pass with
the cross terms missing.

Two checks per case:
  * worst-case per-element bound, cannot fail on a correct kernel:
        |got - ref| <= 2^-24 |ref| + (2^-14 + 2 (3K) 2^-24) A,    A = |x| (*) |w| + |b|,
    K = products per output.  2^-14 A: the dropped terms a_lo b_lo + r_a b + a r_b are below 3.03 * 2^-16 |a||b| per
    product (|r| <= 2^-16 |a|, |a_lo| <= 2^-8 (1 + 2^-8) |a|); 3K: three exact fp32 products accumulated per term.
  * max slab rel-L2 <= 1e-4 (the project's WGRAD_SLAB_TOL).  Measured on the CPU with a torch emulation of the split
    (tests/test_split_cpu.py): a correct split is 4.4e-6 (22x below), one that drops a cross term is 1.66e-3 (16x above).
    The exact-fp32 kernels (algo = 0) are held to the same assertion as the control.
"""
import pytest
import torch

from oracle import fp64_ref as R
from _split_abi import SLAB_TOL, _buf, _check, _free, _gen, _ops, _rand, _weights

pytestmark = pytest.mark.gpu

# (B, D, H, W, Cin, Cout, x pitch, y pitch): small enough for a CPU-side fp64 reference in seconds, each crossing a tile edge
# (tiles are 2 x 4 x 32 voxels, 32 output channels, 16-channel chunks)
CASES = [
    (2, 6, 10, 32, 32, 32, 32, 32),
    (1, 5, 7, 40, 64, 32, 64, 32),
    (2, 4, 4, 32, 128, 64, 128, 64),
    (1, 3, 9, 33, 32, 48, 64, 64),      # both sides channel slices of wider buffers, N not a multiple of 32
]
_ids = lambda c: "x".join(str(v) for v in c)


def _tensors(case):
    B, D, H, W, cin, cout, xld, yld = case
    return (B, D, H, W, cin), (B, D, H, W, cout), xld, yld


def _fwd(case, ps, algo, norm, has_bias, key):
    """-> dict(y, ref, A, sums, kernel, picked, ybuf)"""
    ops, L = _ops()
    xs, ys, xld, yld = _tensors(case)
    B, cin, cout = xs[0], xs[4], ys[4]
    gen = _gen("fwd", case, ps, key)
    x = _rand(xs, xld, gen)
    wk = _weights(B if ps else 1, cout, cin, gen)
    bias = torch.randn(((B, cout) if ps else (cout,)), generator=gen, device="cuda") * 0.5 if has_bias else None
    ybuf = _buf(ys, yld, -7.0)
    picked = L.lib.coma_conv_pick_algo(ops._desc(3, 1, 0, ps, algo), L.ct(x), L.ct(ybuf))
    y, sums = ops._conv_fwd(x, wk, bias, 3, 1, 0, ps, algo, ops.Out(ybuf), norm)
    kernel = L.lib.coma_last_kernel().decode()
    if yld > cout:
        assert bool((ybuf.as_strided(ys[:4] + (yld - cout,), ybuf.stride(), ybuf.storage_offset() + cout) == -7.0).all()), \
            "foreign lanes of the output written"
    ref, A = R.conv_fwd(x.double(), wk.double(), None if bias is None else bias.double(), 3, 1, False)
    return dict(y=y, ref=ref, A=A, sums=sums, kernel=kernel, picked=picked, K=27 * cin + 1)


def _dgrad(case, ps, algo, key):
    ops, L = _ops()
    xs, ys, xld, yld = _tensors(case)
    B, cin, cout = xs[0], xs[4], ys[4]
    gen = _gen("dgrad", case, ps, key)
    dy = _rand(ys, yld, gen)
    wk_d = _weights(B if ps else 1, cout, cin, gen).transpose(2, 3).contiguous()      # [Bw, 27, Cin, Cout]
    dx = _buf(xs, xld, -7.0)
    dd, cdy, cdx = ops._desc(3, 1, 1, ps, algo), L.ct(dy), L.ct(dx)      # data gradient = the transposed form on (dy -> dx)
    picked = L.lib.coma_conv_pick_algo(dd, cdy, cdx)
    ws = L.workspace(L.lib.coma_conv_fwd_ws_bytes(dd, cdy, cdx), dy.device)
    L.check(L.lib.coma_conv_fwd_ws(dd, cdy, L.ptr(wk_d), L.F32, None, cdx, L.ptr(ws), ws.numel(), 0, L.stream()), "coma_conv_fwd_ws(dgrad)")
    kernel = L.lib.coma_last_kernel().decode()
    if xld > cin:
        assert bool((dx.as_strided(xs[:4] + (xld - cin,), dx.stride(), dx.storage_offset() + cin) == -7.0).all()), \
            "foreign lanes of the output written"
    ref, A = R.conv_dgrad(dy.double(), wk_d.double().transpose(2, 3), xs[1:4], 3, 1, False)
    return dict(y=dx, ref=ref, A=A, kernel=kernel, picked=picked, K=27 * cout)


def _wgrad(case, ps, algo, key):
    ops, L = _ops()
    xs, ys, xld, yld = _tensors(case)
    B, cin, cout = xs[0], xs[4], ys[4]
    gen = _gen("wgrad", case, ps, key)
    x = _rand(xs, xld, gen)
    dy = _rand(ys, yld, gen)
    picked = L.lib.coma_conv_wgrad_algo(ops._desc(3, 1, 0, ps, algo), L.ct(x), L.ct(dy))
    _, dwk, _ = ops._conv_bwd(x, None, dy, 3, 1, 0, ps, algo, (B if ps else 1, 27, cout, cin), False, True, 0, None)
    kernel = L.lib.coma_last_kernel().decode()
    ref, A = R.conv_wgrad(x.double(), dy.double(), 3, 1, False, ps)
    return dict(y=dwk, ref=ref, A=A, kernel=kernel, picked=picked, K=xs[1] * xs[2] * xs[3] * (1 if ps else B))


_RUN = {"fwd": lambda c, ps, a, k: _fwd(c, ps, a, None, False, k), "dgrad": _dgrad, "wgrad": _wgrad}


# ---------------------------------------------------------------------------------------------------------------------
# 1. dispatch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_dispatch_in_scope(case, ps):
    """algo = 4 resolves to 4 and launches the split kernels; algo = 0 resolves to 3 on the same problems."""
    try:
        with torch.no_grad():
            for what, prefix in (("fwd", "conv_split_halo_k"), ("dgrad", "conv_split_halo_k"), ("wgrad", "conv_split_wgrad_k")):
                r4 = _RUN[what](case, ps, 4, "dispatch")
                assert r4["picked"] == 4, (what, r4["picked"])
                assert r4["kernel"].startswith(prefix), (what, r4["kernel"])
                r0 = _RUN[what](case, ps, 0, "dispatch")
                assert r0["picked"] == 3, (what, r0["picked"])
                assert not r0["kernel"].startswith("conv_split"), (what, r0["kernel"])
    finally:
        _free()


# out-of-scope problems: (name, x shape, Cout, stride, dtype)
OUT_OF_SCOPE = [
    ("W16", (2, 4, 16, 16, 32), 32, 1, torch.float32),
    ("stride2", (2, 4, 8, 64, 32), 64, 2, torch.float32),
    ("C8", (1, 4, 8, 32, 8), 8, 1, torch.float32),
    ("bf16", (2, 4, 8, 32, 32), 32, 1, torch.bfloat16),
]


@pytest.mark.parametrize("prob", OUT_OF_SCOPE, ids=lambda p: p[0])
def test_dispatch_out_of_scope(prob):
    """Outside the split kernels' scope algo = 4 answers what algo = 0 answers and launches the same kernel."""
    ops, L = _ops()
    _, xs, cout, stride, dt = prob
    B, cin = xs[0], xs[4]
    og = R.out_grid(xs[1:4], 3, stride, False)
    ys = (B, *og, cout)
    try:
        with torch.no_grad():
            gen = _gen("oos", prob)
            x = (torch.randn(xs, generator=gen, device="cuda")).to(dt)
            dy = (torch.randn(ys, generator=gen, device="cuda")).to(dt)
            got = {}
            for algo in (0, 4):
                a_f, a_d = ops.pick_algo(xs, dt, cout, 3, stride, False, False, x.device, algo)
                a_w = L.lib.coma_conv_wgrad_algo(ops._desc(3, stride, 0, False, algo), L.ct(x), L.ct(dy))
                wdt = lambda a: torch.bfloat16 if a == 2 else torch.float32
                wk = _weights(1, cout, cin, _gen("oosw", prob))
                y, _ = ops._conv_fwd(x, wk.to(wdt(a_f)), None, 3, stride, 0, False, algo, None, None)
                k_f = L.lib.coma_last_kernel().decode()
                dx, _, _ = ops._conv_bwd(x, wk.transpose(2, 3).contiguous().to(wdt(a_d)), dy, 3, stride, 0, False, algo,
                                         (1, 27, cout, cin), True, False, 0, None)
                k_d = L.lib.coma_last_kernel().decode()
                _, dwk, _ = ops._conv_bwd(x, None, dy, 3, stride, 0, False, algo, (1, 27, cout, cin), False, True, 0, None)
                k_w = L.lib.coma_last_kernel().decode()
                torch.cuda.synchronize()
                got[algo] = ((a_f, a_d, a_w), (k_f, k_d, k_w))
            assert got[4][0] == got[0][0], (got[4][0], got[0][0])
            assert all(a != 4 for a in got[4][0])
            assert got[4][1] == got[0][1], (got[4][1], got[0][1])
            assert not any(k.startswith("conv_split") for k in got[4][1])
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# 2. + 3. element bound and slab rel-L2, split kernels and the exact-fp32 control
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [4, 0], ids=["split", "exact-control"])
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("what", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kernel_matches_fp64(case, what, ps, algo):
    try:
        with torch.no_grad():
            r = _RUN[what](case, ps, algo, "parity")
            assert r["picked"] == (4 if algo == 4 else 3), r["picked"]
            _check(r, f"{what} {_ids(case)} ps={ps} algo={algo}")
    finally:
        _free()


@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("norm", ["batch", "instance"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_bias_and_fused_stats(case, norm, ps):
    """Forward with bias and the fused {sum, sumsq} record: the output meets both checks and the statistics describe the
    STORED output (bounds of test_gather_kernel_fused_stats: 1e-5 (1 + max |mean|) and rel 1e-5 on rstd)."""
    ops, L = _ops()
    B, cout = case[0], case[5]
    vox = case[1] * case[2] * case[3]
    try:
        with torch.no_grad():
            mode = L.NORM_BATCH if norm == "batch" else L.NORM_INSTANCE
            r = _fwd(case, ps, 4, mode, True, "stats")
            assert r["picked"] == 4 and r["kernel"].startswith("conv_split_halo_k"), (r["picked"], r["kernel"])
            _check(r, f"fwd+bias+{norm} {_ids(case)} ps={ps}")
            G = B if mode == L.NORM_INSTANCE else 1
            n = vox * (1 if G == B else B)
            mean, rstd = ops.stats_from_sums(r["sums"], G, cout, n, 1e-5)
            yf = r["y"].double()
            red = (1, 2, 3) if G == B else (0, 1, 2, 3)
            m_ref = yf.mean(red).reshape(mean.shape)
            v_ref = yf.var(red, unbiased=False).reshape(mean.shape)
            assert float((mean.double() - m_ref).abs().max()) < 1e-5 * (1.0 + float(m_ref.abs().max()))
            assert float(((rstd.double() - (v_ref + 1e-5).rsqrt()).abs() / (v_ref + 1e-5).rsqrt()).max()) < 1e-5
    finally:
        _free()


def test_contracts_kept():
    """Scratch and accumulate queries under algo 4: no forward scratch, no accumulate epilogue (as the halo kernels), the
    weight gradient asks for what algo 0 asks for."""
    ops, L = _ops()
    x = torch.zeros((2, 4, 8, 32, 32), device="cuda")
    y = torch.zeros((2, 4, 8, 32, 64), device="cuda")
    for ps in (False, True):
        d4, d0 = ops._desc(3, 1, 0, ps, 4), ops._desc(3, 1, 0, ps, 0)
        assert L.lib.coma_conv_pick_algo(d4, L.ct(x), L.ct(y)) == 4
        assert L.lib.coma_conv_accumulate_ok(d4, L.ct(x), L.ct(y)) == 0
        assert L.lib.coma_conv_fwd_ws_bytes(d4, L.ct(x), L.ct(y)) == L.lib.coma_conv_fwd_ws_bytes(d0, L.ct(x), L.ct(y)) == 0
        assert L.lib.coma_conv_wgrad_algo(d4, L.ct(x), L.ct(y)) == 4
        assert L.lib.coma_conv_wgrad_ws_bytes(d4, L.ct(x), L.ct(y)) == L.lib.coma_conv_wgrad_ws_bytes(d0, L.ct(x), L.ct(y))
        assert L.lib.coma_conv_wgrad_zs_bytes(d4, L.ct(x), L.ct(y)) == 0


def test_wgrad_zeroed_out_flag():
    """COMA_ZEROED_OUT: the kernel adds into a caller-zeroed dwk and gives the same result as with its own memset."""
    ops, L = _ops()
    gen = _gen("zeroed")
    x = torch.randn((2, 4, 8, 32, 32), generator=gen, device="cuda")
    dy = torch.randn((2, 4, 8, 32, 32), generator=gen, device="cuda")
    d = ops._desc(3, 1, 0, True, 4)
    ws = L.workspace(L.lib.coma_conv_wgrad_ws_bytes(d, L.ct(x), L.ct(dy)), x.device)
    a = torch.full((2, 27, 32, 32), 5.0, device="cuda")
    b = torch.zeros((2, 27, 32, 32), device="cuda")
    L.check(L.lib.coma_conv_wgrad(d, L.ct(x), L.ct(dy), L.ptr(a), None, L.ptr(ws), ws.numel(), 0, L.stream()), "wgrad")
    L.check(L.lib.coma_conv_wgrad(d, L.ct(x), L.ct(dy), L.ptr(b), None, L.ptr(ws), ws.numel(), L.ZEROED_OUT, L.stream()), "wgrad")
    torch.cuda.synchronize()
    ref, _ = R.conv_wgrad(x.double(), dy.double(), 3, 1, False, True)
    assert R.slab_rel_l2(a, ref, 2) <= SLAB_TOL and R.slab_rel_l2(b, ref, 2) <= SLAB_TOL


# ---------------------------------------------------------------------------------------------------------------------
# 5. production shape: 128^3 x 2, once each
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("chans", [(32, 32), (64, 32)], ids=["32to32", "64to32"])
def test_production_shape(chans, what):
    """The persistent tile loop, the chunk prefetch across tiles and the 2M-voxel reduction only run at full size
    (per-sample weights, as the CondConv layers of the step; reference computed in slabs by fp64_ref)."""
    cin, cout = chans
    case = (2, 128, 128, 128, cin, cout, cin, cout)
    try:
        with torch.no_grad():
            if what == "fwd":
                ops, L = _ops()
                r = _fwd(case, True, 4, L.NORM_INSTANCE, True, "prod")
            else:
                r = _RUN[what](case, True, 4, "prod")
            assert r["picked"] == 4 and r["kernel"].startswith("conv_split_"), (r["picked"], r["kernel"])
            _check(r, f"{what} 128^3 x 2 {cin}->{cout}")
    finally:
        _free()
