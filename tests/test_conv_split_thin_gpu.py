"""The thin split (coma_conv_desc.algo = 6; csrc/conv_split.hip): the few-channel full-resolution 3x3x3 layers (C <= 16 and
N <= 16, or C <= 8 and N <= 32, W >= 32) on v_mfma_f32_16x16x32_bf16 as a two-term split, through the C ABI against the fp64
references of oracle/fp64_ref.py.

  fwd   -- forward                                    conv_split_thin_k<CP, NB>
  dgrad -- data gradient (the same kernel, form 1)    conv_split_thin_k<CP, NB>
  wgrad -- weight gradient                            conv_split_thin_wgrad_k<CP, NB>

Helpers, operands (Gaussian fp32, not bf16-exact; finite garbage in foreign lanes) and the two checks (per-element bound
elem_bound(ref, A, 3K, 2^-24) + 2^-14 A; max slab rel-L2 <= 1e-4) are those of test_conv_split_gpu.py, shared through
tests/_split_abi.py; the exact kernels (algo = 0: conv_thin16f_k / conv_thin16f_wgrad_k) run through the same assertions as the
control.

A problem is (what, a, n): the launch reads `a` channels and writes `n` (fwd: x -> y; dgrad: dy -> dx; wgrad: x has `a`
channels, dy has `n`).  Tiles are 2 x 4 x 32 voxels; a launch has a budget of 512 blocks (256 for the weight-gradient instances
that run one block per CU) shared by the samples, each block walking a run of consecutive tile ids (8 z-tiles per id group:
ids past the grid exist).  The grids:
  (1, 2, 4, 32)    exactly one tile
  (2, 3, 5, 33)    partial tiles on every axis, the last x tile holds one voxel
  (1, 17, 42, 72)  3 x 11 x 16 = 528 ids against 512 blocks: every block walks two ids, some past the grid (four per block
                   where the budget is 256)
  (2, 32, 40, 64)  320 ids against 256 blocks per sample: the prefetch across tiles runs with per-sample weights
"""
import pytest
import torch

from oracle import fp64_ref as R
from _split_abi import SLAB_TOL, _buf, _check, _free, _gen, _ops, _rand, _weights

pytestmark = pytest.mark.gpu

GRIDS = [(1, 2, 4, 32), (2, 3, 5, 33), (1, 17, 42, 72), (2, 32, 40, 64)]

# one problem per kernel instance: all four grids
INSTANCES = [
    ("fwd", 16, 16), ("fwd", 8, 8), ("fwd", 1, 32), ("fwd", 5, 32), ("dgrad", 16, 16),
    ("wgrad", 16, 16), ("wgrad", 8, 8), ("wgrad", 1, 32), ("wgrad", 4, 32),
]
# the step's remaining channel pairs and the edge pairs: the one-tile grid and the partial-tile grid
OTHERS = [
    ("fwd", 3, 16), ("fwd", 16, 1), ("fwd", 2, 8), ("fwd", 8, 1), ("fwd", 9, 16),
    ("dgrad", 16, 3), ("dgrad", 1, 16), ("dgrad", 8, 2), ("dgrad", 1, 8), ("dgrad", 8, 8),
    ("wgrad", 3, 16), ("wgrad", 16, 1), ("wgrad", 2, 8), ("wgrad", 8, 1), ("wgrad", 9, 16),
]


def _pitch(c):
    """The natural pitch: 8 channels for 1..3 (and 5), else the next multiple of 4."""
    return 8 if c <= 8 and c not in (4, 8) else (c + 3) // 4 * 4


def _case(prob, grid, lda=None, ldn=None):
    what, a, n = prob
    return (what, a, n) + tuple(grid) + (lda or _pitch(a), ldn or _pitch(n))


CASES = [_case(p, g) for p in INSTANCES for g in GRIDS] + [_case(p, g) for p in OTHERS for g in GRIDS[:2]] + [
    _case(("fwd", 16, 16), GRIDS[1], 32, 48),          # both sides channel slices of wider buffers
    _case(("dgrad", 8, 2), GRIDS[1], 24, 16),
    _case(("wgrad", 16, 16), GRIDS[1], 32, 48),
]
_ids = lambda c: "-".join(str(v) for v in c)


def _cp_nb(what, a, n):
    return (16 if a > 8 else 8), (2 if n > 16 else 1)


def _new_name(what, a, n):
    return ("conv_split_thin_wgrad_k" if what == "wgrad" else "conv_split_thin_k") + "<%d, %d>" % _cp_nb(what, a, n)


def _old_name(what):
    return "conv_thin16f_wgrad_k<" if what == "wgrad" else "conv_thin16f_k<"


def _foreign_untouched(buf, shape, ld, c, fill):
    if ld > c:
        assert bool((buf.as_strided(tuple(shape[:4]) + (ld - c,), buf.stride(), buf.storage_offset() + c) == fill).all()), \
            "foreign lanes of the output written"


def _fwd(case, ps, algo, key, norm=None, has_bias=False):
    ops, L = _ops()
    what, a, n, B, D, H, W, lda, ldn = case
    g = (B, D, H, W)
    gen = _gen("fwd", case, ps, key)
    x = _rand(g + (a,), lda, gen)
    wk = _weights(B if ps else 1, n, a, gen)
    bias = torch.randn(((B, n) if ps else (n,)), generator=gen, device="cuda") * 0.5 if has_bias else None
    ybuf = _buf(g + (n,), ldn, -7.0)
    picked = L.lib.coma_conv_pick_algo(ops._desc(3, 1, 0, ps, algo), L.ct(x), L.ct(ybuf))
    y, sums = ops._conv_fwd(x, wk, bias, 3, 1, 0, ps, algo, ops.Out(ybuf), norm)
    kernel = L.lib.coma_last_kernel().decode()
    _foreign_untouched(ybuf, g, ldn, n, -7.0)
    ref, A = R.conv_fwd(x.double(), wk.double(), None if bias is None else bias.double(), 3, 1, False)
    return dict(y=y, ref=ref, A=A, sums=sums, kernel=kernel, picked=picked, K=27 * a + 1)


def _dgrad(case, ps, algo, key):
    """data gradient of the convolution n -> a channels: the transposed form on (dy with a channels -> dx with n channels)"""
    ops, L = _ops()
    what, a, n, B, D, H, W, lda, ldn = case
    g = (B, D, H, W)
    gen = _gen("dgrad", case, ps, key)
    dy = _rand(g + (a,), lda, gen)
    wk_d = _weights(B if ps else 1, a, n, gen).transpose(2, 3).contiguous()      # [Bw, 27, n (layer input), a (layer output)]
    dx = _buf(g + (n,), ldn, -7.0)
    dd, cdy, cdx = ops._desc(3, 1, 1, ps, algo), L.ct(dy), L.ct(dx)
    picked = L.lib.coma_conv_pick_algo(dd, cdy, cdx)
    assert L.lib.coma_conv_accumulate_ok(dd, cdy, cdx) == 0
    assert L.lib.coma_conv_fwd_ws_bytes(dd, cdy, cdx) == 0
    L.check(L.lib.coma_conv_fwd_ws(dd, cdy, L.ptr(wk_d), L.F32, None, cdx, None, 0, 0, L.stream()), "coma_conv_fwd_ws(dgrad)")
    kernel = L.lib.coma_last_kernel().decode()
    _foreign_untouched(dx, g, ldn, n, -7.0)
    ref, A = R.conv_dgrad(dy.double(), wk_d.double().transpose(2, 3), (D, H, W), 3, 1, False)
    return dict(y=dx, ref=ref, A=A, kernel=kernel, picked=picked, K=27 * a)


def _wgrad(case, ps, algo, key):
    ops, L = _ops()
    what, a, n, B, D, H, W, lda, ldn = case
    g = (B, D, H, W)
    gen = _gen("wgrad", case, ps, key)
    x = _rand(g + (a,), lda, gen)
    dy = _rand(g + (n,), ldn, gen)
    picked = L.lib.coma_conv_wgrad_algo(ops._desc(3, 1, 0, ps, algo), L.ct(x), L.ct(dy))
    _, dwk, _ = ops._conv_bwd(x, None, dy, 3, 1, 0, ps, algo, (B if ps else 1, 27, n, a), False, True, 0, None)
    kernel = L.lib.coma_last_kernel().decode()
    ref, A = R.conv_wgrad(x.double(), dy.double(), 3, 1, False, ps)
    return dict(y=dwk, ref=ref, A=A, kernel=kernel, picked=picked, K=D * H * W * (1 if ps else B))


_RUN = {"fwd": _fwd, "dgrad": _dgrad, "wgrad": _wgrad}


# ---------------------------------------------------------------------------------------------------------------------
# 1. dispatch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("prob", INSTANCES + OTHERS, ids=_ids)
def test_dispatch_in_scope(prob, ps):
    """algo = 6 answers 4 and launches the new kernels; algo = 5, 4 and 0 answer 3 and launch the exact kernels."""
    case = _case(prob, GRIDS[1])
    what, a, n = prob
    try:
        with torch.no_grad():
            r6 = _RUN[what](case, ps, 6, "dispatch")
            assert r6["picked"] == 4, (prob, r6["picked"])
            assert r6["kernel"].startswith(_new_name(*prob)), (prob, r6["kernel"])
            for algo in (5, 4, 0):
                r = _RUN[what](case, ps, algo, "dispatch")
                assert r["picked"] == 3, (prob, algo, r["picked"])
                assert r["kernel"].startswith(_old_name(what)), (prob, algo, r["kernel"])
    finally:
        _free()


# out-of-scope problems: (name, x shape, Cout, ksize, stride, dtype)
OUT_OF_SCOPE = [
    ("C32", (2, 4, 8, 32, 32), 32, 3, 1, torch.float32),
    ("stride2", (2, 4, 8, 64, 32), 64, 3, 2, torch.float32),
    ("W16C8", (2, 4, 16, 16, 8), 8, 3, 1, torch.float32),
    ("bf16", (2, 4, 8, 32, 16), 16, 3, 1, torch.bfloat16),
    ("1x1x1", (2, 4, 8, 32, 16), 8, 1, 1, torch.float32),
    ("16to32", (1, 4, 8, 32, 16), 32, 3, 1, torch.float32),
]


@pytest.mark.parametrize("prob", OUT_OF_SCOPE, ids=lambda p: p[0])
def test_dispatch_out_of_scope(prob):
    """On each problem algo = 6 answers what algo = 5 answers and launches the same kernels, none of them a thin split one;
    the thick stride-1 problem still reaches conv_split_halo_k / conv_split_wgrad_k."""
    ops, L = _ops()
    name, xs, cout, ksize, stride, dt = prob
    B, cin = xs[0], xs[4]
    ys = (B, *R.out_grid(xs[1:4], ksize, stride, False), cout)
    taps = ksize ** 3
    try:
        with torch.no_grad():
            gen = _gen("oos", prob[:5])
            x = (torch.randn(xs, generator=gen, device="cuda")).to(dt)
            dy = (torch.randn(ys, generator=gen, device="cuda")).to(dt)
            wk = (torch.randn((1, taps, cout, cin), generator=gen, device="cuda") * (1.0 / (taps * cin) ** 0.5)).contiguous()
            wdt = lambda a: torch.bfloat16 if a == 2 else torch.float32
            got = {}
            for algo in (5, 6):
                a_f, a_d = ops.pick_algo(xs, dt, cout, ksize, stride, False, False, x.device, algo)
                a_w = L.lib.coma_conv_wgrad_algo(ops._desc(ksize, stride, 0, False, algo), L.ct(x), L.ct(dy))
                kernels = []
                ops._conv_fwd(x, wk.to(wdt(a_f)), None, ksize, stride, 0, False, algo, None, None)
                kernels.append(L.lib.coma_last_kernel().decode())
                ops._conv_bwd(x, wk.transpose(2, 3).contiguous().to(wdt(a_d)), dy, ksize, stride, 0, False, algo,
                              (1, taps, cout, cin), True, False, 0, None)
                kernels.append(L.lib.coma_last_kernel().decode())
                ops._conv_bwd(x, None, dy, ksize, stride, 0, False, algo, (1, taps, cout, cin), False, True, 0, None)
                kernels.append(L.lib.coma_last_kernel().decode())
                torch.cuda.synchronize()
                got[algo] = ([a_f, a_d, a_w], kernels)
            assert got[6] == got[5], (got[6], got[5])
            assert not any(k.startswith("conv_split_thin") for k in got[6][1]), got[6][1]
            if name == "C32":
                assert got[6][0] == [4, 4, 4], got[6][0]
                assert got[6][1][0].startswith("conv_split_halo_k") and got[6][1][1].startswith("conv_split_halo_k") and \
                    got[6][1][2].startswith("conv_split_wgrad_k"), got[6][1]
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# 2. element bound and slab rel-L2, the new kernels and the exact-fp32 control
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [6, 0], ids=["split", "exact-control"])
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kernel_matches_fp64(case, ps, algo):
    what, a, n = case[:3]
    try:
        with torch.no_grad():
            r = _RUN[what](case, ps, algo, "parity")
            assert r["picked"] == (4 if algo == 6 else 3), r["picked"]
            assert r["kernel"].startswith(_new_name(what, a, n) if algo == 6 else _old_name(what)), r["kernel"]
            _check(r, f"{_ids(case)} ps={ps} algo={algo}")
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# 3. bias and statistics, the zeroed flags
# ---------------------------------------------------------------------------------------------------------------------
STATS_CASES = [_case(("fwd", 16, 16), GRIDS[1]), _case(("fwd", 8, 8), GRIDS[1]), _case(("fwd", 1, 32), GRIDS[1]),
               _case(("fwd", 3, 16), GRIDS[1], 8, 32), _case(("fwd", 16, 16), GRIDS[2]), _case(("fwd", 5, 32), GRIDS[3])]


@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("norm", ["batch", "instance"])
@pytest.mark.parametrize("case", STATS_CASES, ids=_ids)
def test_forward_bias_and_stats(case, norm, ps):
    """Forward with bias and the {sum, sumsq} record out of coma_conv_fwd_norm_stats: the output meets both checks and the
    statistics describe the STORED output (bounds of test_conv_split_wide_gpu.test_forward_bias_and_stats:
    1e-5 (1 + max |mean|) and rel 1e-5 on rstd), whichever way the statistics are produced."""
    ops, L = _ops()
    what, a, n, B = case[:4]
    try:
        with torch.no_grad():
            mode = L.NORM_BATCH if norm == "batch" else L.NORM_INSTANCE
            r = _fwd(case, ps, 6, "stats", norm=mode, has_bias=True)
            assert r["picked"] == 4 and r["kernel"].startswith(_new_name(what, a, n)), (r["picked"], r["kernel"])
            _check(r, f"fwd+bias+{norm} {_ids(case)} ps={ps}")
            vox = r["y"].shape[1] * r["y"].shape[2] * r["y"].shape[3]
            G = B if mode == L.NORM_INSTANCE else 1
            cnt = vox * (1 if G == B else B)
            mean, rstd = ops.stats_from_sums(r["sums"], G, n, cnt, 1e-5)
            yf = r["y"].double()
            red = (1, 2, 3) if G == B else (0, 1, 2, 3)
            m_ref = yf.mean(red).reshape(mean.shape)
            v_ref = yf.var(red, unbiased=False).reshape(mean.shape)
            assert float((mean.double() - m_ref).abs().max()) < 1e-5 * (1.0 + float(m_ref.abs().max()))
            assert float(((rstd.double() - (v_ref + 1e-5).rsqrt()).abs() / (v_ref + 1e-5).rsqrt()).max()) < 1e-5
    finally:
        _free()


@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("pair", [(16, 16), (8, 8), (1, 32)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_wgrad_zeroed_flags(pair, ps):
    """COMA_ZEROED_OUT / COMA_ZEROED_WS: with a caller-zeroed dwk and replica scratch the kernel gives the same result as with
    its own memsets; coma_conv_wgrad_ws_bytes under algo 6 is the replica workspace algo 0 asks for."""
    ops, L = _ops()
    a, n = pair
    B, D, H, W = GRIDS[1]
    gen = _gen("zeroed", pair, ps)
    x = _rand((B, D, H, W, a), _pitch(a), gen)
    dy = _rand((B, D, H, W, n), _pitch(n), gen)
    d6, d0 = ops._desc(3, 1, 0, ps, 6), ops._desc(3, 1, 0, ps, 0)
    assert L.lib.coma_conv_wgrad_algo(d6, L.ct(x), L.ct(dy)) == 4
    nws = L.lib.coma_conv_wgrad_ws_bytes(d6, L.ct(x), L.ct(dy))
    Bw = B if ps else 1
    assert nws == L.lib.coma_conv_wgrad_ws_bytes(d0, L.ct(x), L.ct(dy)) and nws >= 4 * 64 * Bw * 27 * n * a
    assert L.lib.coma_conv_wgrad_zs_bytes(d6, L.ct(x), L.ct(dy)) == L.lib.coma_conv_wgrad_zs_bytes(d0, L.ct(x), L.ct(dy))
    ws1 = torch.full((nws,), 0x55, dtype=torch.uint8, device="cuda")          # (garbage: the kernel's own memsets clear it)
    ws2 = torch.zeros((nws,), dtype=torch.uint8, device="cuda")
    g1 = torch.full((Bw, 27, n, a), 5.0, device="cuda")
    g2 = torch.zeros((Bw, 27, n, a), device="cuda")
    L.check(L.lib.coma_conv_wgrad(d6, L.ct(x), L.ct(dy), L.ptr(g1), None, L.ptr(ws1), nws, 0, L.stream()), "wgrad")
    assert L.lib.coma_last_kernel().decode().startswith("conv_split_thin_wgrad_k")
    L.check(L.lib.coma_conv_wgrad(d6, L.ct(x), L.ct(dy), L.ptr(g2), None, L.ptr(ws2), nws, L.ZEROED_OUT | L.ZEROED_WS, L.stream()), "wgrad")
    torch.cuda.synchronize()
    ref, _ = R.conv_wgrad(x.double(), dy.double(), 3, 1, False, ps)
    assert R.slab_rel_l2(g1, ref, 2) <= SLAB_TOL and R.slab_rel_l2(g2, ref, 2) <= SLAB_TOL
    _free()


# ---------------------------------------------------------------------------------------------------------------------
# 4. production shapes: the distinct thin launches of the 128^3 x 2 step, once each at full size
# ---------------------------------------------------------------------------------------------------------------------
# (what, a, n, per-sample weights): per-sample only where the layer is a CondConv (the 1 -> 32 head)
PRODUCTION = [
    ("fwd", 3, 16, False), ("fwd", 16, 16, False), ("fwd", 16, 1, False), ("fwd", 2, 8, False), ("fwd", 8, 8, False),
    ("fwd", 8, 1, False), ("fwd", 1, 32, True),
    ("dgrad", 16, 3, False), ("dgrad", 16, 16, False), ("dgrad", 1, 16, False), ("dgrad", 8, 2, False), ("dgrad", 8, 8, False),
    ("dgrad", 1, 8, False),
    ("wgrad", 3, 16, False), ("wgrad", 16, 16, False), ("wgrad", 16, 1, False), ("wgrad", 2, 8, False), ("wgrad", 8, 8, False),
    ("wgrad", 8, 1, False), ("wgrad", 1, 32, True),
]


@pytest.mark.parametrize("row", PRODUCTION, ids=lambda r: f"{r[0]}-{r[1]}to{r[2]}")
def test_production_shape(row):
    """Thirty-two tile ids per block, the prefetch across all of them and the 4-million-voxel reductions of the shared-weight
    gradients only exist at full size (reference computed in slabs by fp64_ref)."""
    what, a, n, ps = row
    case = _case((what, a, n), (2, 128, 128, 128))
    ops, L = _ops()
    try:
        with torch.no_grad():
            if what == "fwd":
                r = _fwd(case, ps, 6, "prod", norm=L.NORM_INSTANCE if ps else L.NORM_BATCH, has_bias=True)
            else:
                r = _RUN[what](case, ps, 6, "prod")
            assert r["picked"] == 4 and r["kernel"].startswith(_new_name(what, a, n)), (r["picked"], r["kernel"])
            _check(r, f"{what} production {_ids(case)}")
    finally:
        _free()
