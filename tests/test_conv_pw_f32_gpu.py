"""The pointwise kernels (coma_conv_desc.algo = 7; csrc/conv_pw_f32.hip): the 1x1x1 stride-1 fp32 layers with several channels
on both sides on the exact fp32 MFMA, through the C ABI against the fp64 references of oracle/fp64_ref.py (k = 1).

  fwd   -- forward                                    conv_pw_f32_k<C / 8, ceil(N / 32)>
  dgrad -- data gradient (the same kernel, form 1)    conv_pw_f32_k<C / 8, ceil(N / 32)>
  wgrad -- weight gradient                            conv_pw_f32_wgrad_k<ceil(N / 32), ceil(C / 32), TV>

Operands as in tests/_split_abi.py (Gaussian fp32; finite garbage in the foreign lanes of the inputs, a sentinel in those of
the outputs).  The kernels are exact fp32, so the per-element bound has no split term: elem_bound(ref, A, K, 2^-24[, base])
with K = C + 1 (forward with bias), C (no bias, data gradient) or the voxels summed (weight gradient); and the max slab
rel-L2 <= 1e-4.  The kernels these problems run on under algo = 6 go through the same assertions as the control:
conv_mfma_gather_k<*, 0, float> where C % 16 == 0 and N % 32 == 0, conv_direct_fwd_k<float, ...> for every other channel
pair (the fp32 gather kernel takes no other), conv_f32_wgrad_k<0, 1> for the weight gradient.

A problem is (what, a, n): the launch reads `a` channels and writes `n` (fwd: x -> y; dgrad: dy -> dx; wgrad: x has `a`
channels, dy has `n`).

Forward / data gradient: a wave owns 32 voxels, a block four waves, and the grid-stride loop runs under a cap of what the
chip holds at once: CUs x resident blocks of the instance (256 x 1 .. 4 on an MI355X: 4 for <1, 1>, 3 for <2..4, 1>, 2 for
<5..8, 1> and <1..4, 2>, 1 for <5..8, 2>), shared by the samples -- 1024 to 4096 wave tiles per pass.  The grids (B, D, H, W):
  (1, 16, 16, 16)   4096 voxels, the minimum: 128 whole wave tiles
  (2, 16, 17, 17)   4624 voxels: the last wave tile holds 16 voxels; per-sample weights with batch 2
  (1, 32, 64, 65)   133 120 voxels = 4160 wave tiles: under the 4096-tile cap 64 waves walk two tiles (the prefetch across
                    tiles) and the rest one; under 3072 some walk two and some one; under 2048 / 1024 every wave walks
                    two to five
Weight gradient: an LDS tile is TV = 128 voxels (one accumulator tile) or 64 (two to four), a launch has a budget of 2048
blocks (PW_F32_WGRAD_BLOCKS) shared by the samples, each block walking a run of consecutive tiles.  With at least 4096 voxels
per sample no sample is a single tile; on the same grids:
  (1, 16, 16, 16)   whole tiles only, one per block (the double buffer never flips)
  (2, 16, 17, 17)   4624 = 36 x 128 + 16 = 72 x 64 + 16: a partial last tile
  (1, 64, 64, 65)   2080 / 4160 tiles against 2048 blocks: every block walks two / three tiles (both LDS buffers)
                    (weight-gradient problems only)
"""
import pytest
import torch

from oracle import fp64_ref as R
from _split_abi import SLAB_TOL, _buf, _free, _gen, _ops, _rand

pytestmark = pytest.mark.gpu

GRIDS = [(1, 16, 16, 16), (2, 16, 17, 17), (1, 32, 64, 65)]
WGRAD_BIG = (1, 64, 64, 65)

# one problem per kernel instance: all three grids (the third is WGRAD_BIG for the weight gradient).  Forward instances <G, NT>, G = 1..8, NT = 1, 2 (among them the step's
# 32 -> 16 and the edges C = 8, 24, 64, N = 5, 20, 64); the four weight-gradient instances.  (The step's forward 64 -> 32 did
# not beat conv_mfma_gather_k in profiles/pointwise_f32.txt and is outside the predicate: OUT_OF_SCOPE below.)
INSTANCES = [
    ("fwd", 8, 5), ("fwd", 16, 32), ("fwd", 24, 20), ("fwd", 32, 16), ("fwd", 40, 8), ("fwd", 48, 24), ("fwd", 56, 12), ("fwd", 64, 16),
    ("fwd", 8, 64), ("fwd", 16, 40), ("fwd", 24, 36), ("fwd", 32, 64), ("fwd", 40, 33), ("fwd", 48, 48), ("fwd", 56, 64), ("fwd", 64, 64),
    ("wgrad", 32, 16), ("wgrad", 64, 32), ("wgrad", 32, 64), ("wgrad", 64, 64),
]
# the step's data gradients (16 -> 32 of the 32 -> 16 layers, 32 -> 64 of the 64 -> 32 layers) and the remaining edges: the
# first two grids
OTHERS = [
    ("dgrad", 16, 32), ("dgrad", 32, 16), ("dgrad", 32, 64),
    ("fwd", 8, 4), ("dgrad", 8, 5),
    ("wgrad", 8, 4), ("wgrad", 24, 20), ("wgrad", 16, 32),
]


def _case(prob, grid, lda=None, ldn=None):
    what, a, n = prob
    return (what, a, n) + tuple(grid) + (lda or a, ldn or n)


CASES = [_case(p, g if not (p[0] == "wgrad" and g == GRIDS[2]) else WGRAD_BIG) for p in INSTANCES for g in GRIDS] + [_case(p, g) for p in OTHERS for g in GRIDS[:2]] + [
    _case(("fwd", 32, 16), GRIDS[1], 48, 24),          # both sides channel slices of wider buffers
    _case(("fwd", 8, 5), GRIDS[1], 16, 8),             # rows allow 16-byte stores, the channel count does not
    _case(("dgrad", 16, 32), GRIDS[1], 24, 48),
    _case(("wgrad", 32, 16), GRIDS[1], 48, 24),
]
_ids = lambda c: "-".join(str(v) for v in c)


def _weights1(Bw, cout, cin, gen):
    """Gaussian fp32 kernel-layout weights of a 1-tap kernel wk[Bw, 1, Cout, Cin], outputs O(1)."""
    return (torch.randn((Bw, 1, cout, cin), generator=gen, device="cuda") * (1.0 / cin ** 0.5)).contiguous()


def _new_name(what, a, n):
    if what == "wgrad":
        tn, tc = (n + 31) // 32, (a + 31) // 32
        return "conv_pw_f32_wgrad_k<%d, %d, %d>" % (tn, tc, 128 if tn + tc == 2 else 64)
    return "conv_pw_f32_k<%d, %d>" % (a // 8, (n + 31) // 32)


def _old_picked(what, a, n):
    return 3 if what == "wgrad" or (a % 16 == 0 and n % 32 == 0) else 1


def _old_name(what, a, n):
    if what == "wgrad":
        return "conv_f32_wgrad_k<"
    return "conv_mfma_gather_k<" if a % 16 == 0 and n % 32 == 0 else "conv_direct_fwd_k<float"


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
    wk = _weights1(B if ps else 1, n, a, gen)
    bias = torch.randn(((B, n) if ps else (n,)), generator=gen, device="cuda") * 0.5 if has_bias else None
    ybuf = _buf(g + (n,), ldn, -7.0)
    d = ops._desc(1, 1, 0, ps, algo)
    picked = L.lib.coma_conv_pick_algo(d, L.ct(x), L.ct(ybuf))
    acc_ok, nws = L.lib.coma_conv_accumulate_ok(d, L.ct(x), L.ct(ybuf)), L.lib.coma_conv_fwd_ws_bytes(d, L.ct(x), L.ct(ybuf))
    y, sums = ops._conv_fwd(x, wk, bias, 1, 1, 0, ps, algo, ops.Out(ybuf), norm)
    kernel = L.lib.coma_last_kernel().decode()
    _foreign_untouched(ybuf, g, ldn, n, -7.0)
    ref, A = R.conv_fwd(x.double(), wk.double(), None if bias is None else bias.double(), 1, 1, False)
    return dict(y=y, ref=ref, A=A, sums=sums, kernel=kernel, picked=picked, acc_ok=acc_ok, nws=nws, K=a + (1 if has_bias else 0))


def _dgrad(case, ps, algo, key, accumulate=False):
    """data gradient of the convolution n -> a channels: the transposed form on (dy with a channels -> dx with n channels);
    accumulate: COMA_ACCUMULATE onto a Gaussian base."""
    ops, L = _ops()
    what, a, n, B, D, H, W, lda, ldn = case
    g = (B, D, H, W)
    gen = _gen("dgrad", case, ps, key)
    dy = _rand(g + (a,), lda, gen)
    wk_d = _weights1(B if ps else 1, a, n, gen).transpose(2, 3).contiguous()      # [Bw, 1, n (layer input), a (layer output)]
    dx = _buf(g + (n,), ldn, -7.0)
    base = None
    if accumulate:
        base = torch.randn(g + (n,), generator=gen, device="cuda")
        dx.copy_(base)
    dd, cdy, cdx = ops._desc(1, 1, 1, ps, algo), L.ct(dy), L.ct(dx)
    picked = L.lib.coma_conv_pick_algo(dd, cdy, cdx)
    acc_ok, nws = L.lib.coma_conv_accumulate_ok(dd, cdy, cdx), L.lib.coma_conv_fwd_ws_bytes(dd, cdy, cdx)
    ws = torch.zeros((max(nws, 16),), dtype=torch.uint8, device="cuda")
    L.check(L.lib.coma_conv_fwd_ws(dd, cdy, L.ptr(wk_d), L.F32, None, cdx, L.ptr(ws), nws, L.ACCUMULATE if accumulate else 0, L.stream()),
            "coma_conv_fwd_ws(dgrad)")
    kernel = L.lib.coma_last_kernel().decode()
    _foreign_untouched(dx, g, ldn, n, -7.0)
    ref, A = R.conv_dgrad(dy.double(), wk_d.double().transpose(2, 3), (D, H, W), 1, 1, False)
    if accumulate:
        ref = ref + base.double()
    return dict(y=dx, ref=ref, A=A, kernel=kernel, picked=picked, acc_ok=acc_ok, nws=nws, K=a, base=None if base is None else base.double())


def _wgrad(case, ps, algo, key):
    ops, L = _ops()
    what, a, n, B, D, H, W, lda, ldn = case
    g = (B, D, H, W)
    gen = _gen("wgrad", case, ps, key)
    x = _rand(g + (a,), lda, gen)
    dy = _rand(g + (n,), ldn, gen)
    picked = L.lib.coma_conv_wgrad_algo(ops._desc(1, 1, 0, ps, algo), L.ct(x), L.ct(dy))
    _, dwk, _ = ops._conv_bwd(x, None, dy, 1, 1, 0, ps, algo, (B if ps else 1, 1, n, a), False, True, 0, None)
    kernel = L.lib.coma_last_kernel().decode()
    ref, A = R.conv_wgrad(x.double(), dy.double(), 1, 1, False, ps)
    return dict(y=dwk, ref=ref, A=A, kernel=kernel, picked=picked, K=D * H * W * (1 if ps else B))


_RUN = {"fwd": _fwd, "dgrad": _dgrad, "wgrad": _wgrad}


def _check(r, what):
    bound = R.elem_bound(r["ref"], r["A"], r["K"], u_out=R.U_F32, base=r.get("base"))
    ratio = R.check_elementwise(r["y"], r["ref"], bound, what)
    slab = R.slab_rel_l2(r["y"], r["ref"], 2)
    print(f"{what}: kernel {r['kernel']}, worst ratio to the element bound {ratio:.3g}, max slab rel-L2 {slab:.3g}")
    assert slab <= SLAB_TOL, (what, slab)
    return ratio, slab


# ---------------------------------------------------------------------------------------------------------------------
# 1. dispatch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("prob", INSTANCES + OTHERS, ids=_ids)
def test_dispatch_in_scope(prob, ps):
    """algo = 7 answers 3 (fp32 kernel-layout weights), launches the new kernels, can accumulate and needs no forward
    scratch; algo = 6 and 0 launch the kernels they launched before."""
    case = _case(prob, GRIDS[1])
    what, a, n = prob
    try:
        with torch.no_grad():
            r7 = _RUN[what](case, ps, 7, "dispatch")
            assert r7["picked"] == 3, (prob, r7["picked"])
            assert r7["kernel"].startswith(_new_name(*prob)), (prob, r7["kernel"])
            if what != "wgrad":
                assert r7["acc_ok"] == 1 and r7["nws"] == 0, (prob, r7["acc_ok"], r7["nws"])
            for algo in (6, 0):
                r = _RUN[what](case, ps, algo, "dispatch")
                assert r["picked"] == _old_picked(*prob), (prob, algo, r["picked"])
                assert r["kernel"].startswith(_old_name(*prob)), (prob, algo, r["kernel"])
    finally:
        _free()


# problems just outside the scope: (name, x shape, Cout, ksize, dtype, the directions that are outside)
OUT_OF_SCOPE = [
    ("C72", (2, 16, 16, 16, 72), 32, 1, torch.float32, ("fwd", "dgrad", "wgrad")),
    ("C64N32", (2, 16, 16, 16, 64), 32, 1, torch.float32, ("fwd",)),  # (the class that lost to the gather kernel; 32 -> 64 and 32 x 64 inside)
    ("C48N32", (2, 16, 16, 16, 48), 32, 1, torch.float32, ("fwd",)),
    ("C12", (2, 16, 16, 16, 12), 8, 1, torch.float32, ("fwd",)),      # (its data gradient 8 -> 12 and its weight gradient 8 x 12 are inside)
    ("4095voxels", (2, 15, 13, 21, 32), 16, 1, torch.float32, ("fwd", "dgrad", "wgrad")),
    ("ksize3", (2, 16, 16, 16, 32), 32, 3, torch.float32, ("fwd", "dgrad", "wgrad")),
    ("bf16", (2, 16, 16, 16, 32), 16, 1, torch.bfloat16, ("fwd", "dgrad", "wgrad")),
    ("N1", (2, 16, 16, 16, 32), 1, 1, torch.float32, ("fwd", "dgrad", "wgrad")),      # conv_point1
]


@pytest.mark.parametrize("prob", OUT_OF_SCOPE, ids=lambda p: p[0])
def test_dispatch_out_of_scope(prob):
    """On each problem algo = 7 answers what algo = 6 answers and launches the same kernel, none of them a pointwise one, in
    every direction that is outside the predicates; a direction that is inside runs the new kernel."""
    ops, L = _ops()
    name, xs, cout, ksize, dt, outside = prob
    B, cin = xs[0], xs[4]
    ys = (B, *R.out_grid(xs[1:4], ksize, 1, False), cout)
    taps = ksize ** 3
    try:
        with torch.no_grad():
            gen = _gen("oos", prob[:4])
            x = (torch.randn(xs, generator=gen, device="cuda")).to(dt)
            dy = (torch.randn(ys, generator=gen, device="cuda")).to(dt)
            wk = (torch.randn((1, taps, cout, cin), generator=gen, device="cuda") * (1.0 / (taps * cin) ** 0.5)).contiguous()
            wdt = lambda a: torch.bfloat16 if a == 2 else torch.float32
            got = {}
            for algo in (6, 7):
                a_f, a_d = ops.pick_algo(xs, dt, cout, ksize, 1, False, False, x.device, algo)
                a_w = L.lib.coma_conv_wgrad_algo(ops._desc(ksize, 1, 0, False, algo), L.ct(x), L.ct(dy))
                kernels = {}
                ops._conv_fwd(x, wk.to(wdt(a_f)), None, ksize, 1, 0, False, algo, None, None)
                kernels["fwd"] = (a_f, L.lib.coma_last_kernel().decode())
                ops._conv_bwd(x, wk.transpose(2, 3).contiguous().to(wdt(a_d)), dy, ksize, 1, 0, False, algo,
                              (1, taps, cout, cin), True, False, 0, None)
                kernels["dgrad"] = (a_d, L.lib.coma_last_kernel().decode())
                ops._conv_bwd(x, None, dy, ksize, 1, 0, False, algo, (1, taps, cout, cin), False, True, 0, None)
                kernels["wgrad"] = (a_w, L.lib.coma_last_kernel().decode())
                torch.cuda.synchronize()
                got[algo] = kernels
            print(name, got)
            for what in ("fwd", "dgrad", "wgrad"):
                assert not got[6][what][1].startswith("conv_pw_f32"), got[6]
                if what in outside:
                    assert got[7][what] == got[6][what], (what, got[7], got[6])
                else:
                    assert got[7][what][0] == 3 and got[7][what][1].startswith("conv_pw_f32"), (what, got[7])
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# 2. element bound and slab rel-L2, the new kernels and the control
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [7, 6], ids=["pointwise", "control"])
@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_kernel_matches_fp64(case, ps, algo):
    what, a, n = case[:3]
    try:
        with torch.no_grad():
            r = _RUN[what](case, ps, algo, "parity")
            assert r["picked"] == (3 if algo == 7 else _old_picked(what, a, n)), r["picked"]
            assert r["kernel"].startswith(_new_name(what, a, n) if algo == 7 else _old_name(what, a, n)), r["kernel"]
            _check(r, f"{_ids(case)} ps={ps} algo={algo}")
    finally:
        _free()


# ---------------------------------------------------------------------------------------------------------------------
# 3. accumulate, bias and statistics, the zeroed flags
# ---------------------------------------------------------------------------------------------------------------------
ACC_CASES = [_case(("dgrad", 16, 32), GRIDS[1]), _case(("dgrad", 32, 64), GRIDS[1]), _case(("dgrad", 32, 16), GRIDS[1]),
             _case(("dgrad", 8, 5), GRIDS[1]), _case(("dgrad", 8, 5), GRIDS[1], 8, 8), _case(("dgrad", 24, 20), GRIDS[1], 32, 32),
             _case(("dgrad", 64, 64), GRIDS[0]), _case(("dgrad", 16, 32), GRIDS[2])]


@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("case", ACC_CASES, ids=_ids)
def test_accumulate(case, ps):
    """COMA_ACCUMULATE onto a Gaussian base (the data gradients of W_g / W_x land in GradFork buffers): 16-byte
    read-modify-write where the rows allow, scalar otherwise; the base enters the bound.  The control runs wherever the
    old kernel of the problem can accumulate (the gather kernel)."""
    what, a, n = case[:3]
    try:
        with torch.no_grad():
            r = _dgrad(case, ps, 7, "acc", accumulate=True)
            assert r["picked"] == 3 and r["acc_ok"] == 1 and r["kernel"].startswith(_new_name(what, a, n)), (r["picked"], r["kernel"])
            _check(r, f"accumulate {_ids(case)} ps={ps} algo=7")
            if _old_picked(what, a, n) == 3:
                r = _dgrad(case, ps, 6, "acc", accumulate=True)
                assert r["kernel"].startswith(_old_name(what, a, n)), r["kernel"]
                _check(r, f"accumulate {_ids(case)} ps={ps} algo=6")
    finally:
        _free()


STATS_CASES = [_case(("fwd", 32, 16), GRIDS[1]), _case(("fwd", 16, 32), GRIDS[1]), _case(("fwd", 8, 5), GRIDS[1]),
               _case(("fwd", 32, 64), GRIDS[1]), _case(("fwd", 24, 20), GRIDS[1], 48, 24), _case(("fwd", 64, 16), GRIDS[0]),
               _case(("fwd", 32, 16), GRIDS[2])]


@pytest.mark.parametrize("ps", [False, True], ids=["shared", "persample"])
@pytest.mark.parametrize("norm", ["batch", "instance"])
@pytest.mark.parametrize("case", STATS_CASES, ids=_ids)
def test_forward_bias_and_stats(case, norm, ps):
    """Forward with bias and the {sum, sumsq} record out of coma_conv_fwd_norm_stats: the output meets both checks and the
    statistics describe the STORED output (bounds of test_conv_split_thin_gpu.test_forward_bias_and_stats:
    1e-5 (1 + max |mean|) and rel 1e-5 on rstd)."""
    ops, L = _ops()
    what, a, n, B = case[:4]
    try:
        with torch.no_grad():
            mode = L.NORM_BATCH if norm == "batch" else L.NORM_INSTANCE
            r = _fwd(case, ps, 7, "stats", norm=mode, has_bias=True)
            assert r["picked"] == 3 and r["kernel"].startswith(_new_name(what, a, n)), (r["picked"], r["kernel"])
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
@pytest.mark.parametrize("pair", [(32, 16), (64, 64), (8, 4)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_wgrad_zeroed_flags(pair, ps):
    """COMA_ZEROED_OUT / COMA_ZEROED_WS: with a caller-zeroed dwk and replica scratch the kernel gives the same result as
    with its own memsets on dirty buffers; coma_conv_wgrad_ws_bytes / _zs_bytes under algo 7 name the replica scratch."""
    ops, L = _ops()
    a, n = pair
    B, D, H, W = GRIDS[1]
    try:
        gen = _gen("zeroed", pair, ps)
        x = _rand((B, D, H, W, a), a, gen)
        dy = _rand((B, D, H, W, n), n, gen)
        d7 = ops._desc(1, 1, 0, ps, 7)
        assert L.lib.coma_conv_wgrad_algo(d7, L.ct(x), L.ct(dy)) == 3
        nws = L.lib.coma_conv_wgrad_ws_bytes(d7, L.ct(x), L.ct(dy))
        Bw = B if ps else 1
        assert nws >= 4 * 64 * Bw * n * a
        assert L.lib.coma_conv_wgrad_zs_bytes(d7, L.ct(x), L.ct(dy)) == 4 * 64 * Bw * n * a
        ws1 = torch.full((nws,), 0x55, dtype=torch.uint8, device="cuda")          # (garbage: the kernel's own memsets clear it)
        ws2 = torch.zeros((nws,), dtype=torch.uint8, device="cuda")
        g1 = torch.full((Bw, 1, n, a), 5.0, device="cuda")
        g2 = torch.zeros((Bw, 1, n, a), device="cuda")
        L.check(L.lib.coma_conv_wgrad(d7, L.ct(x), L.ct(dy), L.ptr(g1), None, L.ptr(ws1), nws, 0, L.stream()), "wgrad")
        assert L.lib.coma_last_kernel().decode().startswith("conv_pw_f32_wgrad_k")
        L.check(L.lib.coma_conv_wgrad(d7, L.ct(x), L.ct(dy), L.ptr(g2), None, L.ptr(ws2), nws, L.ZEROED_OUT | L.ZEROED_WS, L.stream()), "wgrad")
        torch.cuda.synchronize()
        ref, A = R.conv_wgrad(x.double(), dy.double(), 1, 1, False, ps)
        K = D * H * W * (1 if ps else B)
        for g_, tag in ((g1, "own memsets"), (g2, "zeroed flags")):
            R.check_elementwise(g_, ref, R.elem_bound(ref, A, K, u_out=R.U_F32), f"wgrad {pair} ps={ps} {tag}")
            assert R.slab_rel_l2(g_, ref, 2) <= SLAB_TOL
    finally:
        _free()
