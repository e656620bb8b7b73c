"""What test_conv_ws_gpu.py rests on, checked without a GPU: that the constants and expressions tests/_conv_ws_plan.py mirrors
are still the ones in the .hip / .h sources, that every case of its tables crosses the boundary it is listed for (by the
mirrors, and by the library's own host-side queries on tensors of the same shape), and that the fp64 references the GPU
side compares against agree with torch.nn.functional's fp64 convolutions and their autograd on tiny inputs."""
import os

import pytest
import torch
import torch.nn.functional as F

import _conv_ws_plan as P
from oracle import fp64_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coma_unet_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name) if not name.startswith("include") else os.path.join(ROOT, name)) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------------
# the mirrors are the sources
# ---------------------------------------------------------------------------------------------------------------------
def test_mirrored_expressions_still_in_the_sources():
    (lb, sb, ab), (lf, sf, af) = P.KSPLIT_BF16, P.KSPLIT_F32
    for name, needles in (
            ("conv_mfma.hip", [
                f"if (blocks >= {lf} || nsteps < {sf}) return 1;", f"long ks = {af} / blocks;",
                f"if (blocks >= {lb} || nsteps < {sb}) return 1;", f"long ks = {ab} / blocks;",
                f"if (ks > {P.KSPLIT_MAX}) ks = {P.KSPLIT_MAX};", "if (ks > nsteps / 4) ks = nsteps / 4;", "return ks < 2 ? 1 : (int)ks;",
                "const int BM = BN == 128 ? 128 : 256, LCK = f32 ? 4 : 5;", "g.gy = (long)(N / BN) * (mode == 1 ? 8 : 1);",
                "gather_ksplit(g.gx * g.gy * B, (mode == 1 ? 1 : taps) * (C >> LCK), f32)",
                "if (p.ksplit > 1 && ws && ws_bytes >= sizeof(float) * (size_t)B * Vout * p.N) {", "} else p.ksplit = 1;",
                "if (stats && p.ksplit == 1 && !p.accum) { p.stats = stats; *stats_chunks = 1; }",
                "const size_t bytes = sizeof(float) * (size_t)y->B * t_vox(y) * y->C;", "if (bytes > ((size_t)64 << 20)) return 0;",
                "const int BN = y->C % 128 == 0 ? 128 : y->C % 64 == 0 ? 64 : 32;",
                "else if (halo_ok(d, x, y)) return duo_frag_bytes(d, x, y);",
                "if (x->W < 16 && x->C % 32 == 0 && y->C % 32 == 0) return false;",
                "return d->ksize == 3 && d->stride == 1 && x->W >= 8 && (long)x->H * x->W >= 32 &&",
                "(x->C >= 8 || y->C >= 8 || x->C * y->C >= 8);", "x->C % 16 == 0 && y->C >= 16 &&",
                "x->W >= 32 && x->C <= 16 &&", "y->C <= (x->C > 8 ? 16 : 32)",
                "d->ksize == 1 && d->stride == 1 && x->C >= 8 && x->C <= 64 && x->C % 8 == 0 && y->C >= 4 && y->C <= 64 &&",
                "t_vox(x) >= 4096;", "if (x->C % 32 || y->C % 32) return false;", "if (x->C % 16 || y->C % 32) return false;",
                "return d->form == 0 && d->stride == 1 && (d->ksize == 3 || d->ksize == 1) && x->dtype == COMA_BF16 && dy->dtype == COMA_BF16 &&",
                "(wgrad2_ok(d, x, dy) || x->dtype == COMA_F32) && wsz <= WGRAD_REP_MAX_ELEMS ? sizeof(float) * wsz * WGRAD_NREP : 0;",
                "wgrad_replica_sum_k, dim3((unsigned)((wsz + 31) / 32)), dim3(256), 0, s, rep, WGRAD_NREP, wsz, dwk"]),
            ("conv_duo.hip", [
                "x->dtype != COMA_BF16 || d->ksize != 3 || d->stride != 1 || x->W < 16) return 0;",
                "if (x->C < 64 || x->C % 16 || y->C % 32) return 0;", "return (size_t)(d->per_sample_w ? x->B : 1) * 27 * y->C * x->C * 2;",
                "if (duo_frag_bytes(d, x, y) == 0 || x->C <= 32 || x->C % 32) return false;", "x->D <= 510 && x->H <= 510 && x->W <= 510;",
                "(wk_frag || (ws && ws_bytes >= frag_bytes && aligned16(ws)))"]),
            ("conv_tconv.hip", ["if (d->form != 1 || d->stride != 2 || d->ksize != 3 || x->dtype != y->dtype) return false;",
                                "ck = 64 / es;", "if (x->W < 32 || x->C % ck || y->C % 32) return false;"]),
            ("conv_mfma.h", [
                f"#define WGRAD_NREP {P.WGRAD_NREP}", f"#define WGRAD_REP_MAX_ELEMS {P.WGRAD_REP_MAX_ELEMS}",
                "return (long)d->ksize * d->ksize * d->ksize * dy->C * x->C * (d->per_sample_w ? x->B : 1);",
                "allow && wsz <= WGRAD_REP_MAX_ELEMS && ws && ws_bytes >= sizeof(float) * wsz * WGRAD_NREP;",
                "zeroed & (replicas ? COMA_ZEROED_WS : COMA_ZEROED_OUT)", "sizeof(float) * wsz * r.nrep"]),
            ("conv_wgrad.hip", ["wgrad_replicas(wsz, dwk, ws, ws_bytes, s, zeroed | COMA_ZEROED_OUT, !pl.p.plain);"]),
            ("norm.hip", [f"return (size_t){P.NORM_WS_ROWS} * x->C * sizeof(double2) + 256;"]),
            ("api.hip", ["size_t a = coma_norm_ws_bytes(dy);", "return a > b ? a : b;", "zeroed &= ~COMA_ZEROED_WS;",
                         "COMA_CHECK(ws && ws_bytes >= coma_norm_ws_bytes(dy),",
                         "return coma_conv_fwd_ws(d, x, wk, wk_dtype, bias, y, nullptr, 0, 0, stream);"]),
            ("include/coma_unet.h", [f"#define COMA_STAT_REPLICAS {P.STAT_REPLICAS}", "a smaller or NULL ws runs the unsplit kernel",
                                     "enum { COMA_ZEROED_OUT = 1, COMA_ZEROED_WS = 2,"])):
        text = _src(name)
        for n in needles:
            assert n in text, (name, n)


# ---------------------------------------------------------------------------------------------------------------------
# every case crosses its boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_cases_cross_their_boundaries():
    names = [c.name for c in P.FWD_CASES]
    assert len(set(names)) == len(names)
    for c in P.FWD_CASES:
        nws = P.fwd_ws_bytes(c)
        od = P.out_dims(c.dims, c.k, c.stride, c.form)
        if c.kind == "gather":
            assert P.gather_problem(c) is not None and not P.tconv_ok(c), c.name
            assert P.case_ksplit(c) == c.ksplit > 1, (c.name, P.case_ksplit(c))
            assert nws == 4 * c.B * P.vol(od) * c.cout > 0, c.name
        elif c.kind == "duo":
            assert P.halo_ok(c) and P.duo_wide_ok(c) and c.dims[2] >= 32, c.name
            assert nws == P.duo_frag_bytes(c) == (c.B if c.ps else 1) * 27 * c.cout * c.cin * 2 > 0 and nws % 16 == 0, c.name
        else:
            assert P.halo_ok(c) and nws == 0 and P.duo_frag_bytes(c) == 0, c.name
        assert 2 * c.B * max(P.vol(c.dims) * (c.cin + 16), P.vol(od) * (c.cout + 16)) * 4 < 2 << 20, c.name     # "under 2 MB"
    # the listed figures
    assert P.case_blocks(P.FWD["gather_s1-bf16"]) == 2 and P.case_blocks(P.FWD["gather_s1-f32"]) == 2
    tr = P.FWD["gather_tr"]
    assert P.gather_problem(tr)[1] == 1 and tr.dims[2] < 32 and (1 * (tr.cin >> 5)) == 16          # mode 1, 16 K steps
    assert not P.pw_ok(P.FWD["gather_k1"]) and P.FWD["gather_k1"].cin > 64
    assert P.fwd_ws_bytes(P.FWD["duo_wide-ps"]) == 2 * P.fwd_ws_bytes(P.FWD["duo_wide"])
    assert P.FWD["duo_ragged"].dims[2] % 32 != 0 and P.FWD["duo_ragged"].cin % 64 != 0
    # one step to either side of each threshold of gather_ksplit
    assert P.gather_ksplit(384, 64, False) == 1 and P.gather_ksplit(256, 64, False) == 2 and P.gather_ksplit(2, 15, False) == 1
    assert P.gather_ksplit(192, 64, True) == 1 and P.gather_ksplit(128, 64, True) == 2 and P.gather_ksplit(2, 7, True) == 1


def test_wgrad_cases_cross_their_boundaries():
    names = [c.name for c in P.WGRAD_CASES]
    assert len(set(names)) == len(names)
    for name, wsz in P.WSZ.items():
        assert P.wgrad_out_elems(P.WGRAD[name]) == wsz, name
    larger = {}
    for c in P.WGRAD_CASES:
        wsz, rep = P.wgrad_out_elems(c), P.conv_mfma_wgrad_ws_bytes(c)
        assert (rep > 0) == c.rep == (wsz <= P.WGRAD_REP_MAX_ELEMS), c.name
        assert rep in (0, 4 * wsz * P.WGRAD_NREP), c.name
        assert P.wgrad_ws_bytes(c) == max(P.norm_ws_bytes(c.cout), rep), c.name
        larger[c.name] = "replica" if rep > P.norm_ws_bytes(c.cout) else "norm"
        if c.kernel in ("conv_thin16_wgrad_k", "conv_mfma_wgrad2_k", "conv_thin16f_wgrad_k", "conv_split_thin_wgrad_k"):
            assert c.dims[2] >= 32 and c.dims[2] % 32 != 0, c.name                      # W >= 32, ragged
        if c.kernel == "conv_f32_wgrad_k" and c.k == 3:
            assert c.dims[2] < 32, c.name                                               # neither thin16f nor wgrad16
        if c.kernel == "conv_pw_f32_wgrad_k":
            assert P.vol(c.dims) >= 4096 and c.algo == 7, c.name
        assert 2 * c.B * P.vol(c.dims) * (max(c.cin, c.cout) + 8) * 4 < 2 << 20, c.name
    # with a bias gradient both orders of the two sizes occur
    assert larger["thin16_w"] == "replica" and larger["wgrad2"] == "replica" and larger["planned_f32"] == "replica"
    assert larger["wgrad2_k1"] == "norm" and larger["planned_f32_k1"] == "norm" and larger["pw_f32"] == "norm"
    assert larger["over_ps3"] == "norm" and larger["over_32x32"] == "norm"
    assert P.WGRAD["over_ps3"].B == 3 and P.wgrad_out_elems(P.WGRAD["thin16_w-ps"]) <= P.WGRAD_REP_MAX_ELEMS
    for n in P.ARENA_CASES:
        assert n in P.FWD or n in P.WGRAD, n


def _tensors(c, cin, cout, dims, od):
    from coma_unet_amd import _lib as L
    dt = L.BF16 if c.dt == "bf16" else L.F32
    mk = lambda d_, ch: L.Tensor(None, dt, c.B, d_[0], d_[1], d_[2], ch, ch, P.vol(d_) * ch)
    return mk(dims, cin), mk(od, cout)


def test_library_queries_answer_what_the_mirrors_answer():
    """The host-side size queries need no device: on contiguous tensors of each case's shape (no data pointer) they name the
    bytes the mirrors name."""
    from coma_unet_amd import _lib as L
    for c in P.FWD_CASES:
        d = L.ConvDesc(c.k, c.stride, (c.k - 1) // 2, c.form, int(c.ps), 0)
        x, y = _tensors(c, c.cin, c.cout, c.dims, P.out_dims(c.dims, c.k, c.stride, c.form))
        assert L.lib.coma_conv_pick_algo(d, x, y) == (2 if c.dt == "bf16" else 3), c.name
        assert L.lib.coma_conv_fwd_ws_bytes(d, x, y) == P.fwd_ws_bytes(c), c.name
        assert L.lib.coma_conv_accumulate_ok(d, x, y) == (1 if c.kind == "gather" else 0), c.name
    for c in P.WGRAD_CASES:
        d = L.ConvDesc(c.k, c.stride, (c.k - 1) // 2, c.form, int(c.ps), c.algo)
        x, dy = _tensors(c, c.cin, c.cout, c.dims, c.dims)
        want = 4 if c.algo == 6 else (2 if c.dt == "bf16" else 3)
        assert L.lib.coma_conv_wgrad_algo(d, x, dy) == want, c.name
        assert L.lib.coma_conv_wgrad_zs_bytes(d, x, dy) == P.conv_mfma_wgrad_ws_bytes(c), c.name
        assert L.lib.coma_conv_wgrad_ws_bytes(d, x, dy) == P.wgrad_ws_bytes(c), c.name
        assert L.lib.coma_norm_ws_bytes(dy) == P.norm_ws_bytes(c.cout), c.name


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 references against torch.nn.functional
# ---------------------------------------------------------------------------------------------------------------------
def _ext(t):            # (B, D, H, W, C) -> (B, C, D, H, W)
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _int(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("transposed,per_sample", [(False, False), (True, True)])
def test_fp64_references_against_functional_autograd(transposed, per_sample):
    """conv_fwd / conv_dgrad / conv_wgrad (3x3x3, stride 2, odd grids) against conv3d / conv_transpose3d and their autograd
    in fp64: the stride-2 convolution with shared weights and a bias, the transposed one with per-sample weights."""
    g = torch.Generator().manual_seed(5 + int(transposed))
    B, cin, cout, dims, k = 2, 3, 4, (3, 5, 4), 3
    Bw = B if per_sample else 1
    x = torch.randn((B, *dims, cin), generator=g, dtype=torch.float64)
    wk = torch.randn((Bw, k ** 3, cout, cin), generator=g, dtype=torch.float64)
    bias = torch.randn((B, cout) if per_sample else (cout,), generator=g, dtype=torch.float64)
    xe = _ext(x).requires_grad_(True)
    wkr = wk.clone().requires_grad_(True)
    outs = []
    for b in range(B):
        w_b, b_b = wkr[b if per_sample else 0], (bias[b] if per_sample else bias)
        if transposed:      # conv_transpose3d weights are (Cin, Cout, k, k, k)
            wt = w_b.permute(2, 1, 0).reshape(cin, cout, k, k, k)
            outs.append(F.conv_transpose3d(xe[b:b + 1], wt, b_b, stride=2, padding=1, output_padding=1))
        else:
            wt = w_b.permute(1, 2, 0).reshape(cout, cin, k, k, k)
            outs.append(F.conv3d(xe[b:b + 1], wt, b_b, stride=2, padding=1))
    ye = torch.cat(outs, 0)
    gy = torch.randn(ye.shape, generator=g, dtype=torch.float64)
    ye.backward(gy)
    y, A = R.conv_fwd(x, wk, bias, k, 2, transposed)
    assert y.shape == _int(ye).shape and torch.allclose(y, _int(ye.detach()), rtol=1e-12, atol=1e-12)
    assert bool((A >= y.abs() - 1e-12).all())
    dx, Ad = R.conv_dgrad(_int(gy), wk, dims, k, 2, transposed)
    assert torch.allclose(dx, _int(xe.grad), rtol=1e-12, atol=1e-12) and bool((Ad >= dx.abs() - 1e-12).all())
    dw, Aw = R.conv_wgrad(x, _int(gy), k, 2, transposed, per_sample)
    assert dw.shape == wk.shape and torch.allclose(dw, wkr.grad, rtol=1e-12, atol=1e-12) and bool((Aw >= dw.abs() - 1e-12).all())
