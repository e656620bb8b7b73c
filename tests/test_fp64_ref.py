"""The full-size fp64 reference (oracle/fp64_ref.py) against torch's own fp64 conv3d / conv_transpose3d autograd: the
production-shape GPU tests are only as trustworthy as this restatement.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

from oracle import fp64_ref as R


def _kernel_layout(w, transposed):
    """torch weight (per sample: leading B) -> kernel layout [Bw, taps, Cout, Cin]."""
    if transposed:                          # (B, Cin, Cout, k, k, k)
        w = w.transpose(1, 2)
    B, co, ci = w.shape[:3]
    return w.reshape(B, co, ci, -1).permute(0, 3, 1, 2).contiguous()


CASES = [(k, s, tr, ps) for k in (1, 3) for s in (1, 2) for tr in (False, True) for ps in (False, True)
         if not (k == 1 and s == 2)]


@pytest.mark.parametrize("dims", [(5, 6, 7), (4, 3, 9)])
@pytest.mark.parametrize("k,s,tr,ps", CASES)
def test_tap_sum_reference_matches_torch_autograd(k, s, tr, ps, dims):
    B, cin, cout = 2, 3, 5
    g = torch.Generator().manual_seed(k * 100 + s * 10 + tr * 2 + ps + sum(dims))
    p = (k - 1) // 2
    x = torch.randn((B, cin, *dims), generator=g, dtype=torch.float64)
    wshape = (cin, cout, k, k, k) if tr else (cout, cin, k, k, k)
    w = torch.randn(((B if ps else 1), *wshape), generator=g, dtype=torch.float64)
    bias = torch.randn(((B, cout) if ps else (cout,)), generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)

    def conv(xb, wb, bb):
        if tr:
            return F.conv_transpose3d(xb, wb, bb, stride=s, padding=p, output_padding=s - 1)
        return F.conv3d(xb, wb, bb, stride=s, padding=p)

    yr = torch.cat([conv(xr[i:i + 1], wr[i if ps else 0], bias[i] if ps else bias) for i in range(B)], 0)
    gy = torch.randn(yr.shape, generator=g, dtype=torch.float64)
    yr.backward(gy)

    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
    wk = _kernel_layout(w, tr)
    y, A = R.conv_fwd(cl(x), wk, bias, k, s, tr)
    assert y.shape == cl(yr).shape and A.shape == y.shape
    assert float((y - cl(yr.detach())).abs().max()) < 1e-12 * float(A.max())
    # the magnitude tensor is the same operation on absolute values
    yabs = torch.cat([conv(x[i:i + 1].abs(), w[i if ps else 0].abs(), (bias[i] if ps else bias).abs()) for i in range(B)], 0)
    assert float((A - cl(yabs)).abs().max()) < 1e-12 * float(A.max())
    dx, Adx = R.conv_dgrad(cl(gy), wk, dims, k, s, tr)
    assert float((dx - cl(xr.grad)).abs().max()) < 1e-12 * float(Adx.max())
    dw, Adw = R.conv_wgrad(cl(x), cl(gy), k, s, tr, ps)
    want = _kernel_layout(wr.grad, tr)
    assert dw.shape == want.shape
    assert float((dw - want).abs().max()) < 1e-12 * float(Adw.max())


def test_elem_bound_and_slab_checks_catch_one_wrong_tile():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn((2, 64, 16, 16, 32), generator=g, dtype=torch.float64)
    A = ref.abs() + 1.0
    got = ref.bfloat16().double()
    bound = R.elem_bound(ref, A, 27 * 32)
    assert R.check_elementwise(got, ref, bound) <= 1.0
    assert R.slab_rel_l2(got, ref, 2) < 5e-3
    bad = got.clone()
    bad[1, 5, :4, :2] *= 1.3                   # one 4 x 2 x 32 tile 30 % off
    with pytest.raises(AssertionError):
        R.check_elementwise(bad, ref, bound)
    assert R.slab_rel_l2(bad, ref, 2) > 5e-3
    assert float((bad - ref).norm() / ref.norm()) < 5e-3       # (what a global rel-L2 bound lets through)


@pytest.mark.parametrize("mode", ["batch", "instance"])
@pytest.mark.parametrize("act", ["none", "relu", "prelu", "leaky", "sigmoid", "prelu_relu"])
def test_norm_act_reference_matches_autograd(mode, act):
    g = torch.Generator().manual_seed(len(act))
    B, C = 2, 3
    x = torch.randn((B, 4, 5, 6, C), generator=g, dtype=torch.float64)
    dy = torch.randn(x.shape, generator=g, dtype=torch.float64)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    slope = torch.tensor([-0.3], dtype=torch.float64)
    aff = mode == "batch"
    out = R.norm_act_ref(x, dy, mode, act, gamma if aff else None, beta if aff else None,
                         slope if act in ("prelu", "prelu_relu") else None)
    xe = x.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    gr, br, sr = (t.clone().requires_grad_(True) for t in (gamma, beta, slope))
    if aff:
        z = F.batch_norm(xe, None, None, gr, br, True, 0.1, 1e-5)
    else:
        z = F.instance_norm(xe, eps=1e-5)
    y = R.act_ref(z, act, sr)
    y.backward(dy.permute(0, 4, 1, 2, 3))
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    assert float((out["y"] - cl(y.detach())).abs().max()) < 1e-12
    assert float((out["dx"] - cl(xe.grad)).abs().max()) < 1e-10
    if aff:
        assert float((out["dgamma"] - gr.grad).abs().max()) < 1e-10
        assert float((out["dbeta"] - br.grad).abs().max()) < 1e-10
        m = x.mean((0, 1, 2, 3))
        assert float((out["running_mean"] - 0.1 * m).abs().max()) < 1e-12
    if act in ("prelu", "prelu_relu"):
        assert float((out["dslope"] - sr.grad).abs().max()) < 1e-10
    assert bool((out["mag_y"] >= out["y"].abs() * 0 + 0).all()) and out["mag_dx"].shape == x.shape
