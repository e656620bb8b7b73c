"""Augmentation without a GPU: the fp64 plan (tests/_augment_plan.py) pinned against torch's grid_sample / interpolate and a
published Philox vector, Augment3D.matrix, the parameter sampler and its resumable state, and the exported symbols."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _augment_plan as ap

SHAPE = ap.SHAPES[0]


def _matrix(t, shape=SHAPE):
    from coma_unet_amd.augment import matrix
    return matrix(*t, flips=(False, False, False), shape=shape)


def _grid(s, shape):
    """Source voxel coordinates (3, D, H, W) in (z, y, x) -> grid_sample's normalised (1, D, H, W, 3) grid in (x, y, z)."""
    D, H, W = shape
    g = np.stack([2 * s[2] / (W - 1) - 1, 2 * s[1] / (H - 1) - 1, 2 * s[0] / (D - 1) - 1], axis=-1)
    return torch.from_numpy(g)[None]


@pytest.mark.parametrize("name", ["T1", "T2"])
def test_plan_matches_grid_sample(name):
    A = _matrix(getattr(ap, name))
    mri, tau, roi = ap.volumes(1, SHAPE, seed=3)
    s = ap.source_coords(A.reshape(-1), SHAPE)
    grid = _grid(s, SHAPE)
    vol = torch.from_numpy(tau[0].astype(np.float64))[None, None]
    ref = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0].numpy()
    got = ap.trilinear(tau[0], s)
    err = float(np.abs(got - ref).max())
    lab = torch.from_numpy(roi[0].astype(np.float64))[None, None]
    ref_n = F.grid_sample(lab, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0, 0].numpy()
    got_n = ap.nearest(roi[0], s)
    mism = int(np.count_nonzero(got_n.astype(np.float64) != ref_n))
    inside = float(np.mean((ref != 0)))
    print(f"{name}: trilinear max abs {err:.2e}; nearest mismatches {mism}; non-zero share {inside:.2f}; "
          f"half-band share {ap.near_half(s).mean() * 100:.2f} %")
    assert inside > 0.5 and np.count_nonzero(ref_n) > 0
    assert err <= 1e-12
    assert mism == 0


def test_plan_elastic_matches_interpolate():
    rng = np.random.default_rng(5)
    for g in ((2, 2, 2), (3, 4, 5), (8, 8, 8)):
        disp = rng.uniform(-2, 2, (3,) + g)
        ref = F.interpolate(torch.from_numpy(disp)[None], size=SHAPE, mode="trilinear", align_corners=True)[0].numpy()
        got = ap.elastic_u(disp, SHAPE)
        assert got.shape == (3,) + SHAPE
        assert float(np.abs(got - ref).max()) <= 1e-12, g


def test_half_band_share_is_small():
    """The share of voxels the label comparison leaves to 'either neighbour' (DESIGN.md section 4): <= 1.5 % for T1 / T2."""
    for shape in ap.SHAPES:
        for t in (ap.T1, ap.T2):
            share = float(ap.near_half(ap.source_coords(_matrix(t, shape).reshape(-1), shape)).mean())
            print(f"{shape}: {share * 100:.2f} %")
            assert share <= 0.015


def test_matrix_identity_flips_and_centre():
    from coma_unet_amd.augment import matrix, pack_params, IDENTITY
    shape = (33, 21, 70)
    A = matrix((0, 0, 0), (1, 1, 1), (0, 0, 0), (False, False, False), shape)
    assert A.dtype == np.float64 and np.array_equal(A, np.eye(3, 4)) and not np.signbit(A).any()
    assert np.array_equal(pack_params(A), IDENTITY)
    # flips + integer translations: exact signed permutations, s = (size - 1) - o + t on a flipped axis
    A = matrix((0, 0, 0), (1, 1, 1), (3, -2, 5), (True, False, True), shape)
    want = np.array([[-1, 0, 0, 32 + 3], [0, 1, 0, -2], [0, 0, -1, 69 + 5]], dtype=np.float64)
    assert np.array_equal(A, want)
    for ax in range(3):
        fl = [False] * 3
        fl[ax] = True
        A = matrix(flips=fl, shape=shape)
        want = np.eye(3, 4)
        want[ax, ax], want[ax, 3] = -1, shape[ax] - 1
        assert np.array_equal(A, want)
    # the centre maps to centre + translation, whatever the rotation and scale
    c = (np.array(shape) - 1) / 2
    for t in (ap.T1, ap.T2):
        A = matrix(*t, flips=(False, True, False), shape=shape)
        assert np.allclose(A[:, :3] @ c + A[:, 3], c + np.array(t[2]), atol=1e-12)
    # a pure rotation is orthonormal, a pure scale divides
    R = matrix((20, -30, 40), shape=shape)[:, :3]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and np.linalg.det(R) > 0
    assert np.array_equal(matrix(scale_zyx=(2, 4, 0.5), shape=shape)[:, :3], np.diag([0.5, 0.25, 2.0]))
    with pytest.raises(ValueError):
        matrix(scale_zyx=(1, 0, 1))


def test_sampler_is_reproducible_resumable_and_in_range():
    from coma_unet_amd.augment import Augment3D, IDENTITY, matrix
    kw = dict(rotate_deg=(10, 5, 0), scale=(0.9, 1.1), translate_vox=4.0, flip_axes=(1,), elastic_grid=(3, 4, 5), elastic_sigma_vox=2.0,
              mri_scale=(0.9, 1.1), mri_shift=(-0.05, 0.05), mri_gamma=(0.8, 1.25), noise_sigma=(0.0, 0.03), p=0.7, seed=11)
    a, b = Augment3D(**kw), Augment3D(**kw)
    seq_a = [a.sample_params(2, SHAPE) for _ in range(4)]
    seq_b = [b.sample_params(2, SHAPE) for _ in range(2)]
    for (pa, da), (pb, db) in zip(seq_a, seq_b):
        assert pa.dtype == np.float32 and pa.shape == (2, 16) and da.shape == (2, 3, 3, 4, 5) and da.dtype == np.float32
        assert np.array_equal(pa, pb) and np.array_equal(da, db)
    # the state_dict round trip (through torch.save / weights_only load, as a checkpoint does) continues the sequence
    import io
    buf = io.BytesIO()
    torch.save({"augment_state": b.state_dict()}, buf)
    buf.seek(0)
    c = Augment3D(**{**kw, "seed": 999})
    c.load_state_dict(torch.load(buf, weights_only=True)["augment_state"])
    for pa, da in seq_a[2:]:
        pc, dc = c.sample_params(2, SHAPE)
        assert np.array_equal(pa, pc) and np.array_equal(da, dc)
    assert not np.array_equal(Augment3D(**{**kw, "seed": 12}).sample_params(2, SHAPE)[0], seq_a[0][0])
    # p = 0: identities, and the stream still advances as with p = 1
    z = Augment3D(**{**kw, "p": 0.0})
    pz, dz = z.sample_params(3, SHAPE)
    assert np.array_equal(pz, np.tile(IDENTITY, (3, 1))) and not dz.any() and Augment3D.is_identity(pz, dz)
    one = Augment3D(**{**kw, "p": 1.0})
    one.sample_params(3, SHAPE)
    assert z.rng.bit_generator.state == one.rng.bit_generator.state
    # ranges: |det| of the linear part = 1 / (sz sy sx); intensity parameters inside their ranges; some flips, some not
    r = Augment3D(**{**kw, "p": 1.0, "seed": 3})
    P, Dp = r.sample_params(200, SHAPE)
    assert not Augment3D.is_identity(P, Dp)
    det = np.linalg.det(P[:, :12].reshape(-1, 3, 4)[:, :, :3].astype(np.float64))
    assert np.all(np.abs(det) <= 1 / 0.9 ** 3 + 1e-5) and np.all(np.abs(det) >= 1 / 1.1 ** 3 - 1e-5)
    assert (det < 0).any() and (det > 0).any()                      # the y flip happens for some samples only
    c0 = (np.array(SHAPE) - 1) / 2
    shift = np.einsum("bij,j->bi", P[:, :12].reshape(-1, 3, 4)[:, :, :3].astype(np.float64), c0) + P[:, [3, 7, 11]] - c0
    assert np.all(np.abs(shift) <= 4.0 + 1e-4)
    for col, (lo, hi) in zip((12, 13, 14, 15), ((0.9, 1.1), (-0.05, 0.05), (0.8, 1.25), (0.0, 0.03))):
        assert P[:, col].min() >= np.float32(lo) and P[:, col].max() <= np.float32(hi) and P[:, col].std() > 0
    assert abs(float(Dp.std()) - 2.0) < 0.1
    # no rotation about x was asked for: with unit scale and no flip the x axis row / column stay put
    q = Augment3D(rotate_deg=(10, 0, 0), scale=(1, 1), translate_vox=0, seed=1).sample_params(1, SHAPE)[0][0, :12].reshape(3, 4)
    assert q[0, 0] == 1 and q[0, 1] == 0 and q[0, 2] == 0 and q[1, 0] == 0 and q[2, 0] == 0 and q[1, 2] != 0
    assert Augment3D(seed=0).sample_params(1)[1] is None
    for bad in (dict(p=1.5), dict(scale=(1.1, 0.9)), dict(flip_axes=(3,)), dict(elastic_grid=(9, 4, 4), elastic_sigma_vox=1.0),
                dict(noise_sigma=(-0.1, 0.1)), dict(mri_gamma=(0.0, 1.0))):
        with pytest.raises(ValueError):
            Augment3D(**bad)


def test_philox_known_answer():
    """Random123's known-answer vector for philox4x32-10 with an all-zero counter and key (kat_vectors)."""
    def words(c, k):
        return [int(w) for w in ap.philox4x32_10(*c, *k)]
    assert words((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    got = ap.philox4x32_10(np.array([0, 0]), 0, 0, 0, 0, 0)          # vectorised over the counter
    assert [int(w[1]) for w in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def test_plan_normal_is_standard_normal():
    n = ap.normal(0x1234567890ABCDEF, 1, np.arange(200000))
    N = n.size
    assert abs(n.mean()) <= 5 / np.sqrt(N) and abs(n.std() - 1) <= 5 / np.sqrt(2 * N)
    assert abs(np.mean(n[1:] * n[:-1])) <= 5 / np.sqrt(N)
    assert np.array_equal(n, ap.normal(0x1234567890ABCDEF, 1, np.arange(200000)))
    assert not np.array_equal(n, ap.normal(0x1234567890ABCDEF, 0, np.arange(200000)))
    assert not np.array_equal(n[:10], ap.normal(0x1234567890ABCDEE, 1, np.arange(10)))
    big = ap.normal(7, 0, np.array([5, 5 + (1 << 32)], dtype=np.uint64))                     # the high counter word counts
    assert big[0] != big[1]


def test_symbol_and_export():
    import coma_unet_amd as cu
    from coma_unet_amd._lib import lib, SIGNATURES
    assert hasattr(lib, "coma_augment_warp") and "coma_augment_warp" in SIGNATURES
    assert hasattr(cu, "Augment3D")
    from coma_unet_amd.augment import Augment3D
    assert cu.Augment3D is Augment3D


def test_train_dp_and_prefetcher_take_no_augmenter_by_default():
    import inspect
    from coma_unet_amd.augment import as_augmenter, Augment3D
    from coma_unet_amd.input_pipeline import Prefetcher
    assert inspect.signature(Prefetcher.__init__).parameters["augment"].default is None
    assert as_augmenter(None) is None
    a = Augment3D(seed=4)
    assert as_augmenter(a, rank=3) is a
    d = as_augmenter(dict(rotate_deg=5.0, seed=4), rank=3)
    assert isinstance(d, Augment3D) and d.seed == 7 and float(d.rotate_deg[0]) == 5.0
    with pytest.raises(TypeError):
        as_augmenter("yes")
