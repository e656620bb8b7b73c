"""Split-bf16 mode, the part that needs no GPU: the construction-time check of Config, and a torch emulation of the split
arithmetic (operands split with .to(bfloat16), three F.conv3d calls -- not a kernel) that pins the 1e-4 slab tolerance of
tests/test_conv_split_gpu.py to the reference arithmetic: the three-term form meets it, the one-term form and the forms
with a cross term left out do not."""
import pytest
import torch
import torch.nn.functional as F

from oracle import fp64_ref as R

SLAB_TOL = 1e-4


def test_config_rejects_split_with_bf16_tensors():
    from coma_unet_amd.layers import Config
    with pytest.raises(ValueError):
        Config(compute_dtype=torch.bfloat16, conv_algo=4)
    assert Config(compute_dtype=torch.float32, conv_algo=4).conv_algo == 4
    assert Config(compute_dtype=torch.bfloat16, conv_algo=0).conv_algo == 0


def test_algo_name_registered():
    from coma_unet_amd import ops
    assert ops._ALGO_NAMES[4] == "mfma-split"
    assert ops.conv_class("mfma-split", 32, 32) == "mfma-split"


def _split(a):
    hi = a.to(torch.bfloat16).float()                 # round to nearest even
    lo = (a - hi).to(torch.bfloat16).float()
    return hi, lo


def _conv(x, w):
    return F.conv3d(x.double(), w.double(), padding=1)     # (products of bf16 values are exact; fp64 accumulation stands in for fp32)


@pytest.mark.parametrize("chans", [(32, 32), (64, 32), (256, 128)], ids=lambda c: f"{c[0]}to{c[1]}")
def test_split_emulation_pins_the_tolerance(chans):
    cin, cout = chans
    g = torch.Generator().manual_seed(100 + cin)
    x = torch.randn((2, cin, 4, 12, 12), generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) / (27 * cin) ** 0.5
    ref = _conv(x, w)
    xh, xl = _split(x)
    wh, wl = _split(w)
    slab = lambda y: R.slab_rel_l2(y.permute(0, 2, 3, 4, 1), ref.permute(0, 2, 3, 4, 1), 2)     # (sample, z-plane) slabs
    three = slab(_conv(xh, wh) + _conv(xh, wl) + _conv(xl, wh))
    no_wlo = slab(_conv(xh, wh) + _conv(xl, wh))
    no_xlo = slab(_conv(xh, wh) + _conv(xh, wl))
    one = slab(_conv(xh, wh))
    print(f"{cin}->{cout}: three terms {three:.3g}, without x_hi*w_lo {no_wlo:.3g}, without x_lo*w_hi {no_xlo:.3g}, one term {one:.3g}")
    assert three <= SLAB_TOL / 10            # a correct split has an order of magnitude of room
    assert no_wlo > 10 * SLAB_TOL and no_xlo > 10 * SLAB_TOL and one > 10 * SLAB_TOL
    # the per-product bound of the dropped terms: max |err| / (|x| (*) |w|) stays below 2^-14
    A = _conv(x.abs(), w.abs())
    got = _conv(xh, wh) + _conv(xh, wl) + _conv(xl, wh)
    assert float(((got - ref).abs() / A).max()) < 2.0 ** -14


def test_truncation_would_not_meet_the_per_product_bound():
    """Round-to-nearest-even is required: |a - hi - lo| <= 2^-16 |a|; truncating both conversions gives ~2^-14."""
    g = torch.Generator().manual_seed(7)
    a = torch.randn(1 << 16, generator=g)
    hi, lo = _split(a)
    assert float(((a - hi - lo).abs() / a.abs()).max()) <= 2.0 ** -16
    trunc = lambda t: (t.view(torch.int32) & -65536).view(torch.float32)
    th = trunc(a)
    tl = trunc(a - th)
    assert float(((a - th - tl).abs() / a.abs()).max()) > 2.0 ** -16
