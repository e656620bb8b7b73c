"""The batched weight preparation (coma_weight_prep_batch / coma_routing_fwd_batch: every layer of a forward pass in one
launch) against the per-layer entry points it replaces in ops.PrepAhead.  The batched kernels run the per-layer kernels'
arithmetic per output element (same tiles, same fmaf order over the experts), so every comparison is torch.equal.  Every
output buffer is longer than the output and pre-filled with a sentinel: the padding must come back intact.

The expert scatter of the backward (coma_weight_prep_bwd) runs small layers with the experts across blockIdx.y: checked
against the fp64 einsum with the per-element bounds of test_prep_weights_e8_largest_layer_matches_fp64, below and above
the block-count threshold between the two forms."""

import pytest
import torch

from oracle import fp64_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
PAD = 67          # elements behind every output


def _L():
    from coma_unet_amd import _lib
    return _lib


def _buf(n, dtype):
    return torch.full((n + PAD,), SENTINEL, dtype=dtype, device="cuda")


# (A, B, taps, transposed, E, Bw, dtype of out[0] or None, dtype of out[1] or None)
F, H = torch.float32, torch.bfloat16
TABLE = [
    (32, 32, 27, 0, 8, 2, H, H),
    (16, 3, 27, 0, 8, 3, F, F),           # tile edges with B < 16
    (1, 8, 27, 0, 1, 1, H, F),
    (40, 24, 27, 0, 8, 1, F, H),          # no multiple of 16 either way
    (32, 64, 27, 1, 8, 2, H, H),          # transposed
    (16, 32, 1, 0, 8, 3, H, F),
    (1, 32, 1, 0, 1, 1, F, None),         # only the first layout
    (32, 1, 1, 1, 8, 2, None, H),         # only the second layout
    (24, 40, 27, 0, 8, 2, None, H),
    (48, 16, 27, 1, 1, 1, F, None),
    (20, 30, 1, 0, 8, 1, F, H),           # 600 pairs: more than one run of 256
]


def _make(rows, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    cases = []
    for A, B, taps, tr, E, Bw, d0, d1 in rows:
        master = torch.randn((E, A, B, taps), generator=gen, device="cuda") * 0.05
        r = torch.rand((Bw, E), generator=gen, device="cuda") if E > 1 else None
        cases.append({"row": (A, B, taps, tr, E, Bw, d0, d1), "master": master, "r": r})
    return cases


def _per_layer(case):
    """The per-layer entry points into fresh sentinel-filled buffers -> (out0, out1)."""
    L = _L()
    A, B, taps, tr, E, Bw, d0, d1 = case["row"]
    m, r = case["master"], case["r"]
    n = Bw * taps * A * B
    o0 = _buf(n, d0) if d0 is not None else None
    o1 = _buf(n, d1) if d1 is not None else None
    st = L.stream()
    if taps == 27:
        L.check(L.lib.coma_weight_prep_pair(L.ptr(m), L.ptr(r), E, Bw, A, B, L.ptr(o0), L.dtype_code(d0) if o0 is not None else 0,
                                            L.ptr(o1), L.dtype_code(d1) if o1 is not None else 0, st), "coma_weight_prep_pair")
    else:
        se = A * B
        if o0 is not None:      # [Bw][1][A][B]: n = a, c = b
            L.check(L.lib.coma_weight_prep(L.ptr(m), L.ptr(r), E, Bw, A, B, 1, se, B, 1, L.ptr(o0), L.dtype_code(d0), st), "coma_weight_prep")
        if o1 is not None:      # [Bw][1][B][A]: n = b, c = a
            L.check(L.lib.coma_weight_prep(L.ptr(m), L.ptr(r), E, Bw, B, A, 1, se, 1, B, L.ptr(o1), L.dtype_code(d1), st), "coma_weight_prep")
    return o0, o1


def _batched(cases):
    L = _L()
    items = (L.WprepItem * len(cases))()
    outs = []
    for it, case in zip(items, cases):
        A, B, taps, tr, E, Bw, d0, d1 = case["row"]
        n = Bw * taps * A * B
        o0 = _buf(n, d0) if d0 is not None else None
        o1 = _buf(n, d1) if d1 is not None else None
        it.master, it.r = L.ptr(case["master"]), L.ptr(case["r"])
        it.E, it.Bw, it.A, it.B, it.taps, it.transposed = E, Bw, A, B, taps, tr
        for k, o in enumerate((o0, o1)):
            if o is not None:
                it.out[k], it.dtype[k] = L.ptr(o), L.dtype_code(o.dtype)
        outs.append((o0, o1))
    L.check(L.lib.coma_weight_prep_batch(items, len(cases), L.stream()), "coma_weight_prep_batch")
    torch.cuda.synchronize()
    return outs


def _same(cases, outs):
    for case, got in zip(cases, outs):
        want = _per_layer(case)
        torch.cuda.synchronize()
        A, B, taps, tr, E, Bw, d0, d1 = case["row"]
        n = Bw * taps * A * B
        for k in range(2):
            if want[k] is None:
                assert got[k] is None
                continue
            assert torch.equal(got[k][n:], torch.full_like(got[k][n:], SENTINEL)), (case["row"], k, "padding overwritten")
            assert not bool((want[k][:n] == SENTINEL).any()), (case["row"], k, "the per-layer call left elements unwritten")
            assert torch.equal(got[k], want[k]), (case["row"], k, float((got[k].float() - want[k].float()).abs().max()))


def test_batch_mix_equals_per_layer_entry_points():
    cases = _make(TABLE, 11)
    _same(cases, _batched(cases))


def test_batch_mix_chunks_a_long_table():
    """70 tiny items: more than one kernel-argument block."""
    rows = []
    for i in range(70):
        if i % 3 == 2:
            rows.append((4 + i % 5, 3 + i % 4, 1, i % 2, 8, 1 + i % 2, F, H))
        else:
            rows.append((3 + i % 17, 5 + i % 3, 27, i % 2, 8 if i % 4 else 1, (1 + i % 3) if i % 4 else 1, H if i % 2 else F, F))
    cases = _make(rows, 12)
    _same(cases, _batched(cases))


def test_batch_mix_rejects_bad_items():
    L = _L()
    case = _make([(8, 8, 27, 0, 8, 2, F, F)], 13)[0]
    o = _buf(2 * 27 * 64, F)
    it = (L.WprepItem * 1)()
    it[0].master, it[0].r = L.ptr(case["master"]), None          # E = 8 without routing weights
    it[0].E, it[0].Bw, it[0].A, it[0].B, it[0].taps = 8, 2, 8, 8, 27
    it[0].out[0] = L.ptr(o)
    assert L.lib.coma_weight_prep_batch(it, 1, L.stream()) != 0
    it[0].r, it[0].taps = L.ptr(torch.rand((2, 8), device="cuda")), 9
    assert L.lib.coma_weight_prep_batch(it, 1, L.stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(o, torch.full_like(o, SENTINEL))
    assert L.lib.coma_weight_prep_batch(None, 0, L.stream()) == 0


# (B, NC, E, N, with bias_mix)
ROUTES = [(1, 5, 8, 32, True), (2, 6, 8, 300, True), (3, 5, 8, 1, True), (2, 5, 8, 16, False), (3, 6, 4, 700, True),
          (1, 6, 8, 64, False)]


def _routing(rows, seed):
    L = _L()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    items = (L.RoutingItem * len(rows))()
    keep, got, want = [], [], []
    for it, (B, NC, E, N, with_bm) in zip(items, rows):
        cov = torch.randn((B, NC), generator=gen, device="cuda")
        Wr = torch.randn((E, NC), generator=gen, device="cuda")
        br = torch.randn((E,), generator=gen, device="cuda")
        be = torch.randn((E, N), generator=gen, device="cuda")
        keep.append((cov, Wr, br, be))
        g = (_buf(B * E, F), _buf(B * N, F) if with_bm else None)
        w = (_buf(B * E, F), _buf(B * N, F) if with_bm else None)
        it.cov, it.Wr, it.br, it.bias_e, it.r, it.bias_mix = L.ptr(cov), L.ptr(Wr), L.ptr(br), L.ptr(be), L.ptr(g[0]), L.ptr(g[1])
        it.B, it.NC, it.E, it.N = B, NC, E, N
        L.check(L.lib.coma_routing_fwd(L.ptr(cov), B, NC, L.ptr(Wr), L.ptr(br), E, L.ptr(be), N, L.ptr(w[0]), L.ptr(w[1]), L.stream()),
                "coma_routing_fwd")
        got.append(g)
        want.append(w)
    L.check(L.lib.coma_routing_fwd_batch(items, len(rows), L.stream()), "coma_routing_fwd_batch")
    torch.cuda.synchronize()
    for row, g, w in zip(rows, got, want):
        B, NC, E, N, with_bm = row
        for k, n in ((0, B * E), (1, B * N)):
            if w[k] is None:
                continue
            assert torch.equal(g[k][n:], torch.full_like(g[k][n:], SENTINEL)), (row, k, "padding overwritten")
            assert not bool((w[k][:n] == SENTINEL).any())
            assert torch.equal(g[k], w[k]), (row, k)


def test_batch_routing_equals_per_layer_entry_point():
    _routing(ROUTES, 21)


def test_batch_routing_chunks_a_long_table():
    _routing([(1 + i % 3, 5 + i % 2, 8, 1 + 37 * (i % 9), i % 5 != 0) for i in range(70)], 22)


def test_prep_ahead_batches_its_launches(monkeypatch):
    """A replayed forward of PrepAhead makes one batched routing call and at most two batched mix calls, every per-entry
    _prep_fwd still goes through the module attribute, and the prepared weights equal the per-layer launches'."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops, synthetic
    L = _L()
    S = (16, 16, 16)
    torch.manual_seed(0)
    model = cu.build_model(volume_shape=S, conv_algo=1).to("cuda:0")      # (the deterministic direct kernels)
    model.set_save_attn(None)
    model.train(True)
    b = synthetic.make_batch(2, S, seed=3)
    gb = {k: (v.to("cuda:0") if torch.is_tensor(v) else v) for k, v in b.items()}

    def forward():
        with torch.no_grad():
            out = model(gb["mri"], gb["covars"], roi_pred_dicts=gb["roi_pred_dicts"], sample_roi_mask=gb["roi"])
        torch.cuda.synchronize()
        return out[0].float().clone()

    monkeypatch.setattr(ops.PrepAhead, "batch", True)
    monkeypatch.setattr(ops.PrepAhead, "live", 0)          # (an earlier test's forward without a backward keeps the buffers "in use")
    forward()                                   # records the plan
    calls = {"prep": 0, "mix": 0, "route": 0, "pair": 0}
    real_prep, real_mix, real_route, real_pair = ops._prep_fwd, L.lib.coma_weight_prep_batch, L.lib.coma_routing_fwd_batch, L.lib.coma_weight_prep_pair

    def prep(*a, **k):
        calls["prep"] += 1
        return real_prep(*a, **k)

    class Lib:
        def __getattr__(self, name):
            fn = getattr(L.lib, name)
            key = {"coma_weight_prep_batch": "mix", "coma_routing_fwd_batch": "route", "coma_weight_prep_pair": "pair"}.get(name)
            if key is None:
                return fn

            def counted(*a):
                calls[key] += 1
                return fn(*a)
            return counted

    monkeypatch.setattr(ops, "_prep_fwd", prep)
    monkeypatch.setattr(ops, "lib", Lib())
    used = ops.PrepAhead.used
    y_batch = forward()
    assert ops.PrepAhead.used - used >= 20 and calls["prep"] == ops.PrepAhead.used - used
    assert calls["route"] == 1 and 1 <= calls["mix"] <= 2 and calls["pair"] == 0, calls
    monkeypatch.setattr(ops.PrepAhead, "batch", False)
    y_layer = forward()
    assert calls["pair"] > 0 and calls["route"] == 1
    assert torch.equal(y_batch, y_layer)


# (cin, cout, transposed): 32 -> 32 (4 blocks of 256 pairs), 3 -> 16 (a fifth of a block), 64 -> 32 transposed (8 blocks) run
# the expert-split form; 128 -> 130 is 65 blocks, one more than the threshold, and its last block is partial
SCATTER = [(32, 32, 0), (3, 16, 0), (64, 32, 1), (128, 130, 0)]


@pytest.mark.parametrize("Bw", [1, 2])
@pytest.mark.parametrize("cin,cout,tr", SCATTER)
def test_expert_scatter_matches_fp64(cin, cout, tr, Bw):
    L = _L()
    E = 8
    gen = torch.Generator(device="cuda").manual_seed(31 + cin + Bw)
    wshape = (cin, cout) if tr else (cout, cin)
    master = torch.randn((E, *wshape, 27), generator=gen, device="cuda") * 0.05
    r = torch.rand((Bw, E), generator=gen, device="cuda")
    dwk = torch.randn((Bw, 27, cout, cin), generator=gen, device="cuda")
    nm = master.numel()
    dmaster, dr = _buf(nm, F), _buf(Bw * E, F)
    se = cout * cin * 27
    sn, sc = (27, cout * 27) if tr else (cin * 27, 27)
    L.check(L.lib.coma_weight_prep_bwd(L.ptr(dwk), L.ptr(master), L.ptr(r), E, Bw, cout, cin, 27, se, sn, sc, L.ptr(dmaster), L.ptr(dr),
                                       0, L.stream()), "coma_weight_prep_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dmaster[nm:], torch.full_like(dmaster[nm:], SENTINEL)), "dmaster: padding overwritten"
    assert torch.equal(dr[Bw * E:], torch.full_like(dr[Bw * E:], SENTINEL)), "dr: padding overwritten"
    m, rd = master.double(), r.double()
    dmix = dwk.double().permute(0, 2, 3, 1)                 # [b][cout][cin][27]
    if tr:
        dmix = dmix.transpose(1, 2)
    dm_ref = torch.einsum("be,b...->e...", rd, dmix)
    dm_abs = torch.einsum("be,b...->e...", rd.abs(), dmix.abs())
    ratio_dm = R.check_elementwise(dmaster[:nm].view_as(master), dm_ref, R.elem_bound(dm_ref, dm_abs, Bw, u_out=R.U_F32), "dmaster")
    dr_ref = torch.einsum("b...,e...->be", dmix, m)
    dr_abs = torch.einsum("b...,e...->be", dmix.abs(), m.abs())
    ratio_dr = R.check_elementwise(dr[:Bw * E].view(Bw, E), dr_ref, R.elem_bound(dr_ref, dr_abs, m[0].numel(), u_out=R.U_F32), "dr")
    print(f"scatter {cin}->{cout}{' T' if tr else ''} Bw={Bw}: worst ratio to the bound dmaster {ratio_dm:.3g}, dr {ratio_dr:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# fragment-ordered weights: straight out of the batched mix, and into the wide two-group kernel (COMA_WK_FRAG)
# ---------------------------------------------------------------------------------------------------------------------
def _to_frag(p):
    """wk [Bw][27][N][C] -> [Bw][N / 32][C / 16][27][lane = (n & 31) + 32 * ((c >> 3) & 1)][c & 7], flattened per sample."""
    Bw, T, N, C = p.shape
    return p.view(Bw, T, N // 32, 32, C // 16, 2, 8).permute(0, 2, 4, 1, 5, 3, 6).contiguous().view(Bw, T, N, C)


@pytest.mark.parametrize("N,C", [(32, 64), (64, 128)])
def test_batch_mix_writes_fragment_order(N, C):
    """Both orientations in one table: out[0] of a master [E][N][C][27], out[1] of a master [E][C][N][27]."""
    L = _L()
    rows = [(N, C, 27, 0, 8, 2, H, H), (C, N, 27, 1, 8, 2, H, H)]
    cases = _make(rows, 41 + N)
    plain = [_per_layer(c) for c in cases]
    items = (L.WprepItem * 2)()
    n = 2 * 27 * N * C
    got = []
    for k, (it, case) in enumerate(zip(items, cases)):
        A, B, taps, tr, E, Bw, d0, d1 = case["row"]
        o0, o1 = _buf(n, H), _buf(n, H)
        it.master, it.r = L.ptr(case["master"]), L.ptr(case["r"])
        it.E, it.Bw, it.A, it.B, it.taps, it.transposed = E, Bw, A, B, taps, tr
        it.out[0], it.out[1], it.dtype[0], it.dtype[1] = L.ptr(o0), L.ptr(o1), L.BF16, L.BF16
        it.frag = 1 << k                      # item 0: out[0] ([N][C]) in fragment order; item 1: out[1] ([B][A] = [N][C])
        got.append((o0, o1))
    L.check(L.lib.coma_weight_prep_batch(items, 2, L.stream()), "coma_weight_prep_batch")
    torch.cuda.synchronize()
    for k in range(2):
        for o in range(2):
            want = plain[k][o].clone()
            if o == k:
                want[:n] = _to_frag(plain[k][o][:n].view(2, 27, N, C)).reshape(-1)
            assert torch.equal(got[k][o], want), (k, o)          # (the padding behind the output included)
    # what the fragment order cannot take is refused
    items[0].dtype[0] = L.F32
    assert L.lib.coma_weight_prep_batch(items, 1, L.stream()) != 0
    items[0].dtype[0], items[0].A = L.BF16, N - 16
    assert L.lib.coma_weight_prep_batch(items, 1, L.stream()) != 0


def _conv_pair(xs, n_out, form, per_sample, seed):
    """coma_conv_fwd_ws on plain weights + workspace against fragment-ordered weights + COMA_WK_FRAG."""
    L = _L()
    from coma_unet_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(xs, generator=gen, device="cuda").bfloat16()
    Bw = xs[0] if per_sample else 1
    wk = (torch.randn((Bw, 27, n_out, xs[4]), generator=gen, device="cuda") * 0.05).bfloat16()
    d = L.ConvDesc(3, 1, 1, form, int(per_sample), 0)
    ys = []
    for arm in ("plain", "frag"):
        y = torch.full((*xs[:4], n_out), SENTINEL, dtype=H, device="cuda")
        cx, cy = L.ct(x), L.ct(y)
        nb = L.lib.coma_conv_wk_frag_bytes(d, cx, cy)
        assert nb == wk.numel() * 2 == L.lib.coma_conv_fwd_ws_bytes(d, cx, cy)
        if arm == "plain":
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            L.check(L.lib.coma_conv_fwd_ws(d, cx, L.ptr(wk), L.BF16, None, cy, L.ptr(ws), nb, 0, L.stream()), "coma_conv_fwd_ws")
        else:
            wf = _to_frag(wk)
            L.check(L.lib.coma_conv_fwd_ws(d, cx, L.ptr(wf), L.BF16, None, cy, None, 0, L.WK_FRAG, L.stream()), "coma_conv_fwd_ws")
        assert "conv_mfma_duo_k" in L.lib.coma_last_kernel().decode(), arm
        torch.cuda.synchronize()
        ys.append(y)
    assert not bool((ys[0] == SENTINEL).any())
    assert torch.equal(ys[0], ys[1])


def test_wk_frag_forward_and_data_gradient_equal_plain_weights():
    _conv_pair((2, 4, 8, 32, 64), 32, 0, True, 51)       # forward, per-sample weights
    _conv_pair((2, 4, 8, 32, 64), 32, 1, True, 52)       # data-gradient form
    _conv_pair((1, 4, 8, 16, 64), 32, 0, False, 53)      # the 16-wide tile, shared weights


def test_wk_frag_with_fused_statistics_equals_plain_weights():
    L = _L()
    gen = torch.Generator(device="cuda").manual_seed(54)
    xs, n_out = (2, 4, 8, 32, 64), 32
    x = torch.randn(xs, generator=gen, device="cuda").bfloat16()
    wk = (torch.randn((2, 27, n_out, 64), generator=gen, device="cuda") * 0.05).bfloat16()
    d = L.ConvDesc(3, 1, 1, 0, 1, 0)
    ys = []
    for arm in ("plain", "frag"):
        y = torch.full((*xs[:4], n_out), SENTINEL, dtype=H, device="cuda")
        sums = torch.zeros(8 * 2 * n_out * 2, dtype=torch.float64, device="cuda")      # COMA_STAT_REPLICAS records, instance norm
        cx, cy = L.ct(x), L.ct(y)
        nb = L.lib.coma_conv_fwd_ws_bytes(d, cx, cy)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        w, flags = (wk, 0) if arm == "plain" else (_to_frag(wk), L.WK_FRAG)
        L.check(L.lib.coma_conv_fwd_norm_stats(d, cx, L.ptr(w), L.BF16, None, cy, L.NORM_INSTANCE, L.ptr(sums),
                                               L.ptr(ws) if arm == "plain" else None, nb if arm == "plain" else 0, flags, L.stream()),
                "coma_conv_fwd_norm_stats")
        assert "conv_mfma_duo_k<1" in L.lib.coma_last_kernel().decode(), arm
        torch.cuda.synchronize()
        ys.append((y, sums.view(8, -1).sum(0)))
    assert torch.equal(ys[0][0], ys[1][0])
    assert torch.allclose(ys[0][1], ys[1][1], rtol=1e-12, atol=0)          # (fp64 atomics: the order of the adds is free)


def test_wk_frag_is_refused_where_the_wide_kernel_does_not_run():
    L = _L()
    gen = torch.Generator(device="cuda").manual_seed(55)
    xs = (2, 4, 8, 32, 32)                                # C = 32: the two-group kernel stages the plain layout
    x = torch.randn(xs, generator=gen, device="cuda").bfloat16()
    wk = (torch.randn((2, 27, 32, 32), generator=gen, device="cuda") * 0.05).bfloat16()
    y = torch.full((*xs[:4], 32), SENTINEL, dtype=H, device="cuda")
    d = L.ConvDesc(3, 1, 1, 0, 1, 0)
    assert L.lib.coma_conv_wk_frag_bytes(d, L.ct(x), L.ct(y)) == 0
    assert L.lib.coma_conv_fwd_ws(d, L.ct(x), L.ptr(wk), L.BF16, None, L.ct(y), None, 0, L.WK_FRAG, L.stream()) != 0
    sums = torch.zeros(8 * 2 * 32 * 2, dtype=torch.float64, device="cuda")
    assert L.lib.coma_conv_fwd_norm_stats(d, L.ct(x), L.ptr(wk), L.BF16, None, L.ct(y), L.NORM_INSTANCE, L.ptr(sums), None, 0,
                                          L.WK_FRAG, L.stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, SENTINEL)) and not bool(sums.any())


def test_prep_ahead_hands_fragment_order_to_the_thick_layers():
    """bf16 model on a 32^3 grid: the replayed forward + backward launch no duo_relayout_k (its scratch query is never
    answered by a launch: every C >= 64 two-group layer gets COMA_WK_FRAG) and give the losses of the per-layer path."""
    import coma_unet_amd as cu
    from coma_unet_amd import ops, synthetic
    from coma_unet_amd.train import train_step, make_optimizer
    S = (32, 32, 32)
    b = synthetic.make_batch(2, S, seed=5)
    losses, flagged = {}, {}
    was = ops.PrepAhead.batch
    real_fwd = ops._conv_fwd
    try:
        for mode in (True, False):
            ops.PrepAhead.batch = mode
            torch.manual_seed(1)
            model = cu.build_model(volume_shape=S, compute_dtype=torch.bfloat16, static_prompts=True).to("cuda:0")
            model.set_save_attn(None)
            model.train(True)
            gb = {k: (v.to("cuda:0") if torch.is_tensor(v) else v) for k, v in b.items()}
            gb["roi_pred_dicts"] = model._priors(b["roi_pred_dicts"], 2, torch.device("cuda:0"))
            opt = make_optimizer(model, 0.0)
            crit = cu.build_reference_criterion("cuda:0")
            count = [0]

            def counting(*a, **k):
                count[0] += bool(k.get("frag", False))
                return real_fwd(*a, **k)
            ops._conv_fwd = counting
            ls = [float(train_step(model, crit, opt, gb)[0][0]) for _ in range(3)]
            torch.cuda.synchronize()
            losses[mode], flagged[mode] = ls, count[0]
    finally:
        ops.PrepAhead.batch = was
        ops._conv_fwd = real_fwd
    print("fragment-ordered forward calls:", flagged, "losses:", losses)
    assert flagged[True] > 0 and flagged[False] == 0
    # the same kernels on the same values in both arms; what differs is the order of the fp32 / fp64 atomic merges of the bf16
    # step: 4 x the repeat spread of its loss (2.4e-4, profiles/step_state_noise.py RECORDED["bf16-auto"])
    assert all(abs(a - c) <= 1e-3 * abs(c) for a, c in zip(losses[True], losses[False])), losses
