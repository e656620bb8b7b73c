"""Target smoothing without a GPU: the fp64 plan (tests/_smooth_plan.py) pinned against scipy's gaussian_filter and torch's
conv2d, the tap formulas, the presets, the argument guards and the exported symbols."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _smooth_plan as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode,boundary", [("nearest", "nearest"), ("constant", "zeros")])
def test_plan_matches_scipy_gaussian_filter(mode, boundary):
    from scipy.ndimage import gaussian_filter
    from coma_unet_amd.smooth import gaussian_taps
    vol = np.random.default_rng(0).random((5, 7, 9))
    w = gaussian_taps(2.0, approx="sampled")
    assert w.size == 17
    got = sp.smooth64(vol, (w, w, w), boundary)
    ref = gaussian_filter(vol, sigma=2.0, mode=mode, cval=0.0, truncate=4.0)
    err = float(np.abs(got - ref).max())
    print(f"{mode}: max abs {err:.2e}")
    assert err <= 1e-14


def test_reference_preset_is_the_in_plane_filter_not_the_3d_one():
    """`smoothing(tau.squeeze(0))` on (1, D, H, W): MONAI takes D for the channel axis -> a depthwise 2-D filter over (H, W)."""
    from coma_unet_amd.smooth import GaussianSmooth3D
    g = GaussianSmooth3D.reference()
    assert g.axes == ("y", "x") and g.taps[0] is None and g.boundary == "zeros" and g.radius == 4
    D, H, W = 5, 7, 9
    vol = np.random.default_rng(1).random((D, H, W))
    wy, wx = g.taps64["y"], g.taps64["x"]
    got = sp.smooth64(vol, (None, wy, wx), "zeros")
    kern = torch.from_numpy(np.outer(wy, wx))[None, None].repeat(D, 1, 1, 1)
    ref = F.conv2d(torch.from_numpy(vol)[None], kern, padding=4, groups=D)[0].numpy()
    err = float(np.abs(got - ref).max())
    three_d = sp.smooth64(vol, (wy, wy, wx), "zeros")
    print(f"vs depthwise conv2d: {err:.2e}; vs the 3-D filter: {np.abs(got - three_d).max():.2e}")
    assert err <= 1e-14
    assert float(np.abs(got - three_d).max()) > 1e-2


def test_taps():
    from coma_unet_amd.smooth import gaussian_taps
    w = gaussian_taps(1.0)
    assert w.dtype == np.float64 and w.size == 9 and abs(w.sum() - 0.99999320) <= 1e-8
    assert np.array_equal(w, w[::-1]) and np.all(w > 0)
    # the formula, term by term
    t = 0.70710678
    assert w[4] == 0.5 * (math.erf(t * 0.5) - math.erf(-t * 0.5))
    assert w[0] == 0.5 * (math.erf(t * -3.5) - math.erf(t * -4.5))
    assert gaussian_taps(2.0).size == 17
    assert gaussian_taps(0.05).size == 3                          # tail = int(max(0.2, 0.5) + 0.5) = 1
    s = gaussian_taps(1.0, approx="sampled")
    assert s.size == 9 and abs(s.sum() - 1.0) <= 1e-15
    assert np.allclose(s, np.exp(-0.5 * np.arange(-4, 5) ** 2.0) / np.exp(-0.5 * np.arange(-4, 5) ** 2.0).sum(), rtol=0, atol=1e-17)


def test_from_fwhm():
    from coma_unet_amd.smooth import GaussianSmooth3D
    g = GaussianSmooth3D.from_fwhm(2, (1, 1, 1))
    assert g.axes == ("z", "y", "x") and g.approx == "sampled" and g.boundary == "nearest"
    for a in g.axes:
        assert abs(g.sigma[a] - 0.8493) <= 5e-5 and g.taps64[a].size == 7
    assert all(t.dtype == np.float32 and t.size == 7 for t in g.taps)
    h = GaussianSmooth3D.from_fwhm(2, (1.0, 2.0, 0.5))           # spacing is (x, y, z); sigma is kept per (z, y, x)
    assert abs(h.sigma["x"] - 0.8493) <= 5e-5 and abs(h.sigma["y"] - 0.42466) <= 5e-5 and abs(h.sigma["z"] - 1.69865) <= 5e-5


def test_taps_are_rounded_once_from_fp64():
    from coma_unet_amd.smooth import GaussianSmooth3D, gaussian_taps
    g = GaussianSmooth3D(sigma=(1.5, 0.7), axes=("z", "x"))
    assert g.taps[1] is None
    assert np.array_equal(g.taps[0], gaussian_taps(1.5).astype(np.float32))
    assert np.array_equal(g.taps[2], gaussian_taps(0.7).astype(np.float32))


def test_value_errors():
    from coma_unet_amd.smooth import GaussianSmooth3D, gaussian_taps, as_smoother
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            gaussian_taps(bad)
        with pytest.raises(ValueError):
            GaussianSmooth3D(sigma=bad)
    with pytest.raises(ValueError):
        gaussian_taps(1.0, approx="fft")
    with pytest.raises(ValueError):
        GaussianSmooth3D(sigma=2.2)                               # radius 9 at truncation 4
    GaussianSmooth3D(sigma=2.0)                                   # radius 8: the cap itself is fine
    with pytest.raises(ValueError):
        GaussianSmooth3D(sigma=(1.0, 1.0, 1.0))                   # three sigmas for two axes
    with pytest.raises(ValueError):
        GaussianSmooth3D(axes=("y", "y"))
    with pytest.raises(ValueError):
        GaussianSmooth3D(boundary="reflect")
    g = GaussianSmooth3D.reference()
    with pytest.raises(ValueError):
        g(torch.zeros(4, 4, 4, dtype=torch.float64))              # not fp32
    with pytest.raises(ValueError):
        g(torch.zeros(4, 4, 4, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        g(torch.zeros(4, 4, 8)[:, :, ::2])                        # not contiguous
    with pytest.raises(ValueError):
        g(torch.zeros(4, 4))                                      # not a volume
    with pytest.raises(ValueError):
        g(torch.zeros(2, 2, 4, 4, 4))                             # more than one channel
    with pytest.raises(ValueError):
        g(torch.zeros(4, 4, 4))                                   # fp32, contiguous, but on the host: there is no CPU path
    with pytest.raises(TypeError):
        as_smoother("yes")


def test_as_smoother():
    from coma_unet_amd.smooth import GaussianSmooth3D, as_smoother
    assert as_smoother(None) is None
    g = as_smoother(True)
    assert isinstance(g, GaussianSmooth3D) and g.axes == ("y", "x") and g.sigma == {"y": 1.0, "x": 1.0}
    d = as_smoother({"sigma": 0.8, "axes": ("z", "y", "x"), "approx": "sampled", "boundary": "nearest"})
    assert d.axes == ("z", "y", "x") and d.boundary == "nearest" and d.taps64["z"].size == 7
    assert as_smoother(g) is g
    import coma_unet_amd as cu
    assert cu.GaussianSmooth3D is GaussianSmooth3D


def test_symbols_declared_bound_and_tile_exported():
    from coma_unet_amd import _lib as L
    from coma_unet_amd import smooth as S
    header = open(os.path.join(ROOT, "include", "coma_unet.h")).read()
    for name in ("coma_gauss_smooth3d", "coma_gauss_smooth3d_tile"):
        assert re.search(r"\b%s\(" % name, header) and name in L.SIGNATURES and hasattr(L.lib, name)
    assert L.lib.coma_abi_version() == 3
    macro = {m: int(v) for m, v in re.findall(r"#define (COMA_SMOOTH_\w+) (\d+)", header)}
    assert macro["COMA_SMOOTH_MAX_RADIUS"] == S.MAX_RADIUS == 8 and macro["COMA_SMOOTH_SMALL_RADIUS"] == S.SMALL_RADIUS
    assert (macro["COMA_SMOOTH_ZEROS"], macro["COMA_SMOOTH_NEAREST"]) == (S.ZEROS, S.NEAREST)
    assert S.TILE == (macro["COMA_SMOOTH_TILE_Z"], macro["COMA_SMOOTH_TILE_Y"], macro["COMA_SMOOTH_TILE_X"])
    assert S.tile(4, False) == S.tile(8, False) == S.TILE and S.TILE_LARGE_RADIUS == (S.TILE[0] // 2,) + S.TILE[1:]
    assert "smooth.hip" in __import__("coma_unet_amd.build", fromlist=["SOURCES"]).SOURCES


def test_contract_plan_stays_inside_the_counted_bound():
    """The fp32 restatement of the kernel's arithmetic against the fp64 one: inside `bound`, and not by orders of magnitude
    (a bound that nothing comes near would not be checking anything)."""
    from coma_unet_amd.smooth import gaussian_taps
    vol = sp.volume((2, 11, 13, 17), seed=4)
    for sigma, boundary in ((1.0, "zeros"), (2.0, "nearest")):
        w = gaussian_taps(sigma)
        taps = (w, w, w)
        err = float(np.abs(sp.smooth32(vol, taps, boundary).astype(np.float64) - sp.smooth64(vol, taps, boundary)).max())
        b = sp.bound(taps, float(np.abs(vol).max()))
        first_order = 3 * (w.size + 1) * 2.0 ** -24 * float(np.abs(vol).max())
        print(f"sigma {sigma}: err {err:.3e}, bound {b:.3e}, first-order figure {first_order:.3e}")
        assert err <= b
        assert b <= 1.001 * first_order
        assert err >= b / 200
