"""coma_augment_warp on the GPU against the fp64 plan (tests/_augment_plan.py): B = 2 with a different transform per sample at
20 x 24 x 28 and at 33 x 21 x 70 (W no multiple of 4: scalar tail and misaligned rows; wider than one wave; three tiles along
x, several along y and z).  The launch neither caps its grid nor loops over tiles (one block per 4 x 8 x 32 tile, grid.x up
to 2^31 - 1), so there is no large case."""
import functools

import numpy as np
import pytest
import torch

import _augment_plan as ap

pytestmark = pytest.mark.gpu

SEED = 0x5DEECE66D1234567


def _params(shape, ts=(ap.T1, ap.T2), intensity=((1, 0, 1, 0), (1, 0, 1, 0))):
    from coma_unet_amd.augment import matrix, pack_params
    return np.stack([pack_params(matrix(*t, shape=shape), *i) for t, i in zip(ts, intensity)])


@functools.lru_cache(maxsize=None)
def _vols(shape):
    v = ap.volumes(2, shape, seed=sum(shape))
    for a in v:
        a.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _disp(shape, grid):
    d = np.random.default_rng(sum(grid)).uniform(-2, 2, (2, 3) + grid).astype(np.float32)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _plan_plain(shape):
    """T1 / T2 without elastic part or intensity change: shared by the transform, noise and sigma = 0 cases."""
    return ap.warp(*_vols(shape), _params(shape))


def _run(vols, params, disp=None, seed=0):
    from coma_unet_amd.augment import warp
    dev = [torch.from_numpy(np.array(v)).cuda() for v in vols]           # (a copy: the shared volumes are read-only)
    out = warp(*dev, params, None if disp is None else np.ascontiguousarray(disp), seed)
    torch.cuda.synchronize()
    for d, v in zip(dev, vols):
        assert np.array_equal(d.cpu().numpy(), v)                     # the inputs are only read
    return [o.cpu().numpy() for o in out]


def _check_against_plan(got, plan, vols, name):
    """Case 3's checks: labels exact outside the half-integer band (either neighbour inside it, band <= 1.5 %), trilinear outputs
    within 1e-4 (fp32 coordinate error 2e-5 x slope <= 1 per axis x 3 axes, rounded up).  The MRI is compared where the label
    agrees with the plan's: where a band voxel took the other neighbour the mask may differ, and the label rule covers it."""
    gm, gt, gr = got
    errs = []
    for b in range(2):
        bad_out, bad_in, share = ap.label_check(gr[b], vols[2][b], plan["s"][b])
        et = float(np.abs(gt[b] - plan["tau"][b]).max())
        same = gr[b] == plan["roi"][b]
        em = float(np.abs(gm[b] - plan["mri"][b])[same].max())
        print(f"{name} sample {b}: label mismatches outside band {bad_out}, unexplained inside {bad_in}, band {share * 100:.2f} %; "
              f"tau max abs {et:.2e}, mri max abs {em:.2e}")
        assert bad_out == 0 and bad_in == 0
        assert share <= 0.015
        assert et <= 1e-4 and em <= 1e-4
        assert np.count_nonzero(gr[b]) > 0.3 * gr[b].size and np.count_nonzero(gt[b]) > 0.3 * gt[b].size
        errs.append(max(et, em))
    return max(errs)


@pytest.mark.parametrize("shape", ap.SHAPES)
def test_identity_is_bitwise(shape):
    from coma_unet_amd.augment import IDENTITY
    mri, tau, roi = _vols(shape)
    gm, gt, gr = _run((mri, tau, roi), np.tile(IDENTITY, (2, 1)), seed=SEED)
    assert np.array_equal(gt, tau) and np.array_equal(gr, roi)
    assert np.array_equal(gm, mri * (roi != 0)) and np.count_nonzero(roi == 0) > 0


def _flip_shift(vol, flips, t):
    """out[o] = vol[F o + t] (F: mirror the flipped axes about the centre), zeros shifted in: plain slicing."""
    v = np.flip(vol, axis=[a for a in range(3) if flips[a]]) if any(flips) else vol
    out = np.zeros_like(vol)
    dst, src = [], []
    for a, n in enumerate(vol.shape):
        # flipped axis: source index (n - 1 - o) + t = flipped-array index o - t; plain axis: o + t
        d = -t[a] if flips[a] else t[a]
        lo, hi = max(0, -d), min(n, n - d)
        dst.append(slice(lo, hi)), src.append(slice(lo + d, hi + d))
    out[tuple(dst)] = v[tuple(src)]
    return out


@pytest.mark.parametrize("shape", ap.SHAPES)
def test_flips_and_integer_shifts_are_bitwise(shape):
    from coma_unet_amd.augment import matrix, pack_params
    mri, tau, roi = _vols(shape)
    cases = [((True, False, False), (0, 0, 0)), ((False, True, False), (0, 0, 0)), ((False, False, True), (0, 0, 0)),
             ((False, False, False), (3, -2, 5)), ((True, True, True), (-1, 4, -7)), ((False, False, True), (0, 0, 13))]
    for (f0, t0), (f1, t1) in zip(cases[0::2], cases[1::2]):
        params = np.stack([pack_params(matrix(translate_zyx=t, flips=f, shape=shape)) for f, t in ((f0, t0), (f1, t1))])
        gm, gt, gr = _run((mri, tau, roi), params)
        for b, (f, t) in enumerate(((f0, t0), (f1, t1))):
            wr = _flip_shift(roi[b], f, t)
            assert np.array_equal(gr[b], wr), (f, t)
            assert np.array_equal(gt[b], _flip_shift(tau[b], f, t)), (f, t)
            assert np.array_equal(gm[b], _flip_shift(mri[b], f, t) * (wr != 0)), (f, t)
            assert np.count_nonzero(wr) > 0


@pytest.mark.parametrize("shape", ap.SHAPES)
def test_affine_transforms_match_the_plan(shape):
    import torch.nn.functional as F
    vols = _vols(shape)
    got = _run(vols, _params(shape))
    err = _check_against_plan(got, _plan_plain(shape), vols, f"affine {shape}")
    # for scale: fp32 grid_sample's own distance from the fp64 plan on the same coordinates
    D, H, W = shape
    s = _plan_plain(shape)["s"][0]
    grid = torch.from_numpy(np.stack([2 * s[2] / (W - 1) - 1, 2 * s[1] / (H - 1) - 1, 2 * s[0] / (D - 1) - 1], axis=-1))[None].float()
    ref32 = F.grid_sample(torch.from_numpy(vols[1][0].copy())[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    print(f"affine {shape}: kernel max abs error {err:.2e}; fp32 grid_sample (CPU) vs fp64 plan "
          f"{float(np.abs(ref32[0, 0].numpy() - _plan_plain(shape)['tau'][0]).max()):.2e}")


@pytest.mark.parametrize("grid", [(2, 2, 2), (3, 4, 5)])
@pytest.mark.parametrize("shape", ap.SHAPES)
def test_elastic_matches_the_plan(shape, grid):
    vols, disp = _vols(shape), _disp(shape, grid)
    params = _params(shape, ts=(ap.T1, ap.T1))
    got = _run(vols, params, disp)
    plan = ap.warp(*vols, params, disp)
    _check_against_plan(got, plan, vols, f"elastic {grid} {shape}")
    assert float(np.abs(plan["s"][0] - ap.source_coords(params[0, :12], shape)).max()) > 1.0       # the grid did move voxels


def test_oversized_control_grid_is_refused():
    from coma_unet_amd import _lib as L
    from coma_unet_amd.augment import warp
    shape = ap.SHAPES[0]
    dev = [torch.from_numpy(v.copy()).cuda() for v in _vols(shape)]
    out = [torch.full_like(d, -7.0) for d in dev]
    params = torch.from_numpy(_params(shape)).cuda()
    for g in ((9, 2, 2), (2, 2, 9), (1, 2, 2)):
        disp = torch.zeros((2, 3) + g, device="cuda")
        with pytest.raises(ValueError):
            warp(*dev, params, disp, 0, out)
        # and the C entry itself, behind the Python check
        rc = L.lib.coma_augment_warp(*(L.ptr(t) for t in dev), *(L.ptr(t) for t in out), 2, *shape, L.ptr(params), L.ptr(disp), *g, 0,
                                     L.stream())
        assert rc == 1 and b"control grid" in L.lib.coma_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in out)                     # nothing was launched
    warp(*dev, params, torch.zeros((2, 3, 8, 8, 8), device="cuda"), 0, out)       # 8 points per axis: the largest staged grid
    torch.cuda.synchronize()
    plan = _plan_plain(shape)
    assert float(np.abs(out[1].cpu().numpy() - plan["tau"]).max()) <= 1e-4


@pytest.mark.parametrize("shape", ap.SHAPES)
def test_intensity_matches_the_plan(shape):
    vols = _vols(shape)
    params = _params(shape, intensity=((1.1, 0.05, 0.8, 0.0), (0.9, -0.03, 1.25, 0.0)))
    gm, gt, gr = _run(vols, params)
    plan = ap.warp(*vols, params)
    for b in range(2):
        same = gr[b] == plan["roi"][b]
        top = float(np.abs(plan["mri"][b]).max())
        e = float(np.abs(gm[b] - plan["mri"][b])[same].max()) / top
        print(f"intensity {shape} sample {b}: max abs error / max {e:.2e} (max {top:.3f})")
        assert top > 0.5 and e <= 1e-5
    assert np.array_equal(gt, _run(vols, _params(shape))[1])             # tau is only resampled


@pytest.mark.parametrize("shape", ap.SHAPES)
def test_mri_is_zero_wherever_the_warped_roi_is(shape):
    vols = _vols(shape)
    params = _params(shape, intensity=((1.0, 0.3, 1.0, 0.2), (1.2, -0.4, 0.7, 0.1)))
    gm, gt, gr = _run(vols, params, _disp(shape, (3, 4, 5)), seed=SEED)
    bg = gr == 0
    assert bg.any() and not bg.all()
    assert not gm[bg].any()
    assert np.count_nonzero(gm[~bg]) > 0.99 * np.count_nonzero(~bg)


@pytest.mark.parametrize("shape", ap.SHAPES)
def test_noise(shape):
    mri, tau, roi = _vols(shape)
    D, H, W = shape
    sig = (0.5, 0.25)                                                     # powers of two: sigma * n is one exact rounding of n
    params = _params(shape, intensity=((1, 0, 1, sig[0]), (1, 0, 1, sig[1])))
    zero = np.zeros_like(mri)
    a = _run((zero, tau, roi), params, seed=SEED)
    b = _run((zero, tau, roi), params, seed=SEED)
    c = _run((zero, tau, roi), params, seed=SEED + 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))               # same seed: bitwise
    assert not np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
    idx = np.arange(D * H * W, dtype=np.uint64).reshape(shape)
    for s in range(2):
        fg = a[2][s] != 0
        N = int(fg.sum())
        n = a[0][s].astype(np.float64) / sig[s]                           # mri == 0: the output IS sigma * n
        want = ap.normal(SEED, s, idx)
        e = float(np.abs(n - want)[fg].max())
        mean, std = float(n[fg].mean()), float(n[fg].std())
        pair = fg[:, :, 1:] & fg[:, :, :-1]
        lag = float((n[:, :, 1:] * n[:, :, :-1])[pair].mean())
        print(f"noise {shape} sample {s}: N {N}; max |n - plan| {e:.2e}; mean {mean:+.4f} (5/sqrt N {5 / np.sqrt(N):.4f}); std {std:.4f}; "
              f"lag-1 {lag:+.4f}")
        assert N > 3000
        assert e <= 1e-5
        assert abs(mean) <= 5 / np.sqrt(N) and abs(std - 1) <= 5 / np.sqrt(2 * N)
        assert abs(lag) <= 5 / np.sqrt(N)
        assert not a[0][s][~fg].any()
    # sigma = 0: the generator is out of the picture, whatever the seed -- bitwise the noise-free output
    plain = _run((mri, tau, roi), _params(shape), seed=SEED)
    again = _run((mri, tau, roi), _params(shape), seed=SEED + 99)
    assert all(np.array_equal(x, y) for x, y in zip(plain, again))
    noisy = _run((mri, tau, roi), params, seed=SEED)
    fg = noisy[2] != 0
    assert float(np.abs(noisy[0] - plain[0])[fg].std()) > 0.1 and np.array_equal(noisy[1], plain[1])


def test_misuse_raises_and_launches_nothing():
    from coma_unet_amd._lib import ComaError
    from coma_unet_amd.augment import warp
    shape = ap.SHAPES[0]
    mri, tau, roi = [torch.from_numpy(v.copy()).cuda() for v in _vols(shape)]
    params = torch.from_numpy(_params(shape)).cuda()
    keep = [t.clone() for t in (mri, tau, roi)]
    out = [torch.full_like(t, -7.0) for t in (mri, tau, roi)]
    err = (ValueError, TypeError, ComaError)
    with pytest.raises(err):                                              # non-contiguous input
        warp(mri.transpose(2, 3), tau.transpose(2, 3), roi.transpose(2, 3), params, None, 0, None)
    with pytest.raises(err):
        warp(mri[:, :, :, ::2], tau[:, :, :, ::2], roi[:, :, :, ::2], params, None, 0, None)
    with pytest.raises(err):                                              # out aliasing in
        warp(mri, tau, roi, params, None, 0, (mri, out[1], out[2]))
    with pytest.raises(err):
        warp(mri, tau, roi, params, None, 0, (out[0], roi, out[2]))
    big = torch.full((mri.numel() + 64,), -7.0, device="cuda")
    with pytest.raises(err):                                              # two outputs overlapping each other
        warp(mri, tau, roi, params, None, 0, (big[:mri.numel()].view_as(mri), big[64:].view_as(mri), out[2]))
    with pytest.raises(err):                                              # mismatched shapes
        warp(mri, tau[:1], roi, params, None, 0, None)
    with pytest.raises(err):
        warp(mri, tau, roi[:, :-1].contiguous(), params, None, 0, None)
    with pytest.raises(err):
        warp(mri, tau, roi, params[:1], None, 0, None)
    with pytest.raises(err):
        warp(mri, tau, roi, params, None, 0, (out[0][:1], out[1], out[2]))
    with pytest.raises(err):
        warp(mri.cpu(), tau.cpu(), roi.cpu(), params, None, 0, None)
    with pytest.raises(err):
        warp(mri.double(), tau.double(), roi.double(), params, None, 0, None)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (mri, tau, roi)))
    assert all(bool((o == -7.0).all()) for o in out) and bool((big == -7.0).all())


def test_augment3d_call_shapes_identity_and_out():
    from coma_unet_amd.augment import Augment3D, IDENTITY
    shape = ap.SHAPES[0]
    mri, tau, roi = [torch.from_numpy(v.copy()).cuda().unsqueeze(1) for v in _vols(shape)]           # (B, 1, D, H, W) as train_dp has them
    aug = Augment3D(rotate_deg=8.0, translate_vox=2.0, mri_shift=(-0.1, 0.1), noise_sigma=(0.01, 0.02), elastic_grid=(4, 4, 4),
                    elastic_sigma_vox=1.5, seed=5)
    twin = Augment3D(rotate_deg=8.0, translate_vox=2.0, mri_shift=(-0.1, 0.1), noise_sigma=(0.01, 0.02), elastic_grid=(4, 4, 4),
                     elastic_sigma_vox=1.5, seed=5)
    got = aug(mri, tau, roi)
    assert all(g.shape == mri.shape and g.is_contiguous() for g in got) and got[0].data_ptr() != mri.data_ptr()
    params, disp = aug.last_params
    want = twin.sample_params(2, shape)
    assert np.array_equal(params, want[0]) and np.array_equal(disp, want[1])
    plan = ap.warp(*_vols(shape), params, disp)
    assert float(np.abs(got[1][:, 0].cpu().numpy() - plan["tau"]).max()) <= 1e-4
    # given parameters, into given buffers: the same numbers except the noise (its seed follows the call count)
    out = tuple(torch.empty_like(t) for t in (mri, tau, roi))
    res = aug(mri, tau, roi, params=params, disp=disp, out=out)
    assert all(r is o for r, o in zip(res, out)) and torch.equal(out[1], got[1]) and torch.equal(out[2], got[2])
    assert not torch.equal(out[0], got[0]) and float((out[0] - got[0]).abs().max()) < 0.3
    # an all-identity batch launches nothing and returns its inputs; with out= it is a copy
    ident = np.tile(IDENTITY, (2, 1))
    same = aug(mri, tau, roi, params=ident)
    assert same[0] is mri and same[1] is tau and same[2] is roi
    assert Augment3D(p=0.0, seed=1)(mri, tau, roi)[0] is mri
    res = aug(mri, tau, roi, params=ident, out=out)
    assert torch.equal(out[0], mri) and torch.equal(out[1], tau) and torch.equal(out[2], roi) and res[0] is out[0]
    # a Prefetcher sample: (1, D, H, W)
    one = aug(mri[0], tau[0], roi[0])
    assert one[0].shape == mri[0].shape
