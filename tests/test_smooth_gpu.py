"""coma_gauss_smooth3d on the GPU against tests/_smooth_plan.py: inside the counted fp32 bound of the fp64 restatement AND bit for
bit the fp32 restatement of the arithmetic contract; volumes shorter than the halo, tile edges, per-axis taps, misaligned
buffers, impulses, the fused resample source, the error statuses."""
import numpy as np
import pytest
import torch

import _smooth_plan as sp

pytestmark = pytest.mark.gpu

MODES = {"zeros": 0, "nearest": 1}


def _taps(sigma):
    from coma_unet_amd.smooth import gaussian_taps
    return gaussian_taps(sigma)


def _run(vol, taps, boundary, **kw):
    from coma_unet_amd.smooth import smooth
    out = smooth(vol, [None if w is None else np.asarray(w).astype(np.float32) for w in taps], MODES[boundary], **kw)
    torch.cuda.synchronize()
    return out


def _check(vol, taps, boundary, got=None, what=""):
    """got (default: one launch on `vol`) against both restatements; returns the error against fp64."""
    if got is None:
        got = _run(torch.from_numpy(vol).cuda(), taps, boundary)
    got = got.cpu().numpy()
    assert got.shape == vol.shape and got.dtype == np.float32
    want64 = sp.smooth64(vol, taps, boundary)
    err = float(np.abs(got.astype(np.float64) - want64).max())
    b = sp.bound(taps, float(np.abs(vol).max()))
    exact = sp.smooth32(vol, taps, boundary)
    differ = int(np.count_nonzero(got != exact))
    print(f"{what}{vol.shape} {boundary}: max abs vs fp64 {err:.3e} (bound {b:.3e}); voxels differing from the fp32 contract: {differ}")
    assert err <= b
    assert differ == 0
    return err


@pytest.mark.parametrize("boundary", ["zeros", "nearest"])
@pytest.mark.parametrize("sigma", [1.0, 2.0])                   # radius 4 and radius 8
@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 3, 3, 3)])
def test_volume_shorter_than_the_halo(shape, sigma, boundary):
    w = _taps(sigma)
    assert w.size == {1.0: 9, 2.0: 17}[sigma]
    _check(sp.volume(shape, seed=sum(shape)), (w, w, w), boundary)


@pytest.mark.parametrize("boundary", ["zeros", "nearest"])
def test_per_axis_taps_and_unaligned_buffers(boundary):
    """z radius 2, y skipped, x radius 8 on W = 37 (scalar stores), then the same on buffers whose base is only 4-byte
    aligned, and W = 36 with an aligned and a misaligned output (16-byte stores / scalar stores)."""
    taps = (sp.ASYM[0], None, _taps(2.0))
    vol = sp.volume((2, 19, 21, 37), seed=7)
    _check(vol, taps, boundary)
    from coma_unet_amd.smooth import smooth
    for shape in ((2, 19, 21, 37), (1, 9, 10, 36)):
        vol = sp.volume(shape, seed=8)
        n = vol.size
        src = torch.zeros(n + 1, device="cuda")
        src[1:] = torch.from_numpy(vol).cuda().reshape(-1)
        dst = torch.full((n + 5,), float("nan"), device="cuda")
        view_in, view_out = src[1:].view(shape), dst[1:n + 1].view(shape)
        assert view_in.data_ptr() % 16 == 4 and view_out.data_ptr() % 16 == 4 and view_in.is_contiguous()
        got = _run(view_in, taps, boundary, out=view_out)
        _check(vol, taps, boundary, got, "unaligned ")
        assert torch.isnan(dst[0]) and torch.isnan(dst[n + 1:]).all()          # nothing written outside the view
    vol = sp.volume((1, 9, 10, 36), seed=9)
    _check(vol, taps, boundary, what="aligned, W % 4 == 0 ")


@pytest.mark.parametrize("boundary", ["zeros", "nearest"])
@pytest.mark.parametrize("k", [1, 2])
def test_tile_edges(k, boundary):
    """tile + 1 and 2 tile + 3 voxels per axis: a last tile of one and of three voxels, interior tiles whose halo is all data."""
    from coma_unet_amd.smooth import TILE, TILE_LARGE_RADIUS
    assert TILE_LARGE_RADIUS[0] < TILE[0]           # (the shapes below are past one tile of either instantiation)
    shape = (1,) + tuple(k * t + (1 if k == 1 else 3) for t in TILE)
    vol = sp.volume(shape, seed=10 + k)
    w4 = _taps(1.0)
    _check(vol, (w4, w4, w4), boundary, what="3-D radius 4 ")
    _check(vol, (None, w4, w4), boundary, what="reference preset ")
    if k == 1:
        w8 = _taps(2.0)
        _check(vol, (w8, w8, w8), boundary, what="3-D radius 8 ")
        _check(vol, (None, w8, w8), boundary, what="in-plane radius 8 ")


def test_impulses_give_the_clipped_outer_product():
    """Unit impulses at the eight corners and the centre, three different asymmetric tap vectors: out[i] = w[p - i + r] per axis,
    clipped by the volume.  A swapped, reversed or shifted axis cannot pass.  Exact: with a single non-zero input every
    chain is one product."""
    D, H, W = 6, 7, 11
    wz, wy, wx = (np.asarray(w).astype(np.float32) for w in sp.ASYM)
    pts = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)] + [(D // 2, H // 2, W // 2)]
    vol = np.zeros((len(pts), D, H, W), dtype=np.float32)
    want = np.zeros_like(vol)
    for b, (pz, py, px) in enumerate(pts):
        vol[b, pz, py, px] = 1.0
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    kz, ky, kx = pz - z + wz.size // 2, py - y + wy.size // 2, px - x + wx.size // 2
                    if 0 <= kz < wz.size and 0 <= ky < wy.size and 0 <= kx < wx.size:
                        want[b, z, y, x] = wz[kz] * np.float32(wy[ky] * wx[kx])           # x pass, then y, then z
    got = _run(torch.from_numpy(vol).cuda(), (wz, wy, wx), "zeros").cpu().numpy()
    assert np.array_equal(got, want)
    assert np.count_nonzero(want[-1]) == wz.size * wy.size * wx.size           # the centre impulse is not clipped
    assert np.array_equal(want, sp.smooth32(vol, (wz, wy, wx), "zeros"))         # (and the plan agrees with the hand count)


def test_reference_preset_is_slice_local_and_matches_the_plan():
    from coma_unet_amd.smooth import GaussianSmooth3D
    g = GaussianSmooth3D.reference()
    vol = sp.volume((1, 6, 12, 40), seed=20)
    a = torch.from_numpy(vol).cuda()
    b = a.clone()
    b[0, 2] += 1.0
    ga, gb = g(a), g(b)
    torch.cuda.synchronize()
    changed = [bool((ga[0, z] != gb[0, z]).any()) for z in range(6)]
    assert changed == [False, False, True, False, False, False]
    _check(vol, (None, g.taps64["y"], g.taps64["x"]), "zeros", ga, "reference() ")
    # every accepted layout gives the same numbers in its own shape
    for view in (a[0], a, a[:, None], torch.cat([a, b])):
        out = g(view)
        assert out.shape == view.shape and torch.equal(out.reshape(-1, 6, 12, 40)[0], ga[0])
    n = GaussianSmooth3D.from_fwhm(2, (1, 1, 1))
    _check(vol, tuple(n.taps64[k] for k in "zyx"), "nearest", n(a), "from_fwhm() ")


def test_bitwise_identities_and_repeatability():
    from coma_unet_amd.smooth import GaussianSmooth3D
    vol = torch.from_numpy(sp.volume((2, 9, 10, 37), seed=21)).cuda()
    assert torch.equal(_run(vol, (None, None, None), "zeros"), vol)                     # every axis skipped: a copy
    assert torch.equal(GaussianSmooth3D(axes=())(vol), vol)
    one = np.array([1.0])
    for boundary in MODES:
        assert torch.equal(_run(vol, (one, one, one), boundary), vol)                   # taps [1.0]
        assert torch.equal(_run(vol, (None, one, None), boundary), vol)
    w = _taps(1.0)
    first = _run(vol, (w, w, w), "nearest")
    assert torch.equal(_run(vol, (w, w, w), "nearest"), first)                          # two runs of the same launch


@pytest.mark.parametrize("shape,spacing", [((9, 10, 11), (3.0, 3.4, 2.9)), ((30, 33, 35), (1.2, 0.9375, 1.5))])
def test_fused_source_is_bitwise_the_two_step_result(shape, spacing):
    from coma_unet_amd import input_pipeline as P
    from coma_unet_amd.smooth import GaussianSmooth3D
    rng = np.random.default_rng(sum(shape))
    v = rng.normal(size=shape).astype(np.float32)
    v[0, 0, 0] = np.nan; v[-1, -1, -1] = np.inf; v[1, 2, 3] = -np.inf
    dv = torch.from_numpy(v).cuda()
    two = P.resample_nearest(dv, spacing, default_value=8.0)
    assert two.shape != dv.shape
    for g in (GaussianSmooth3D.reference(), GaussianSmooth3D.from_fwhm(2, (2, 2, 2)), GaussianSmooth3D(sigma=2.0, axes=("z", "y", "x")),
              GaussianSmooth3D(axes=())):
        want = g(two)
        got = g.resampled(dv, spacing, P.NEW_SPACING, default_value=8.0)
        torch.cuda.synchronize()
        assert got.shape == want.shape and torch.isfinite(want).all()
        assert torch.equal(got, want), (g.axes, g.boundary)
    raw = GaussianSmooth3D.reference().resampled(dv, spacing, P.NEW_SPACING, default_value=8.0, nan_to_num=False)
    keep = P.resample_nearest(dv, spacing, default_value=8.0, nan_to_num=False)
    want = GaussianSmooth3D.reference()(keep)
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(raw), torch.isnan(want)) and torch.equal(torch.nan_to_num(raw), torch.nan_to_num(want))
    # prepare_sample: tau through the fused launch, MRI and ROI exactly as without the option
    roi = torch.from_numpy((rng.random(size=shape) > 0.3).astype(np.float32) * 17).cuda()
    m0, t0, r0 = P.prepare_sample(dv, dv + 1, roi, spacing)
    m1, t1, r1 = P.prepare_sample(dv, dv + 1, roi, spacing, smoothing=True)
    torch.cuda.synchronize()
    assert torch.equal(m0, m1) and torch.equal(r0, r1) and t1.shape == t0.shape
    assert torch.equal(t1, GaussianSmooth3D.reference()(t0))
    m2, t2, r2 = P.prepare_sample(dv, dv + 1, roi, spacing, resize=False, smoothing=True)
    assert torch.equal(t2, GaussianSmooth3D.reference()(torch.nan_to_num(dv + 1)[None]))


def test_error_statuses_launch_nothing():
    from coma_unet_amd._lib import ComaError
    from coma_unet_amd.smooth import smooth
    vol = torch.from_numpy(sp.volume((1, 4, 5, 8), seed=22)).cuda()
    out = torch.full_like(vol, -1.0)

    def refused(taps, src=vol, dst=out, boundary=0):
        with pytest.raises(ComaError):
            smooth(src, taps, boundary, out=dst)
        torch.cuda.synchronize()
        assert bool((out == -1.0).all())

    refused((None, None, np.ones(19, dtype=np.float32) / 19))          # radius 9
    refused((np.ones(4, dtype=np.float32), None, None))                # an even count
    refused((None, np.ones(3, dtype=np.float32), None), boundary=2)    # no such boundary mode
    w = np.ones(3, dtype=np.float32)
    buf = torch.zeros(2 * vol.numel() - 1, device="cuda")
    a, b = buf[:vol.numel()].view(vol.shape), buf[vol.numel() - 1:].view(vol.shape)      # one shared voxel
    with pytest.raises(ComaError):
        smooth(a, (None, None, w), 0, out=b)
    with pytest.raises(ComaError):
        smooth(vol, (None, None, w), 0, out=vol)
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
