"""fp64 restatement of the augmentation warp (include/coma_unet.h `coma_augment_warp`, DESIGN.md section 4 "Augmentation"),
written from the specification, numpy only.  The GPU tests judge the kernel against this; test_augment_cpu.py pins this
against torch's grid_sample / interpolate and a published Philox vector.

Per output voxel o = (z, y, x) of sample b:  s = A_b (z, y, x, 1)^T + u_b(o);  roi_out = roi[floor(s + 0.5)] (0 outside);
tau_out = trilinear(tau, s) with zero padding;  mri_out = scale * g(trilinear(mri, s)) + shift + sigma * n, zeroed where
roi_out == 0."""
import numpy as np

NPARAM = 16
# the transforms the tests share: (rotation deg about z, y, x), (scale z, y, x), (translation z, y, x)
T1 = ((7.0, -5.0, 4.0), (1.05, 0.95, 1.0), (1.3, -2.1, 0.7))
T2 = ((-12.0, 9.0, 15.0), (0.9, 1.1, 1.07), (-3.4, 2.2, 5.1))
SHAPES = ((20, 24, 28), (33, 21, 70))
HALF_BAND = 1e-3            # |coordinate - half-integer| below which a label may be either neighbour


def volumes(B, shape, seed):
    """(mri, tau, roi) float32 (B, D, H, W): mri / tau uniform in [0, 1), labels out of a few integer ids in 4^3-ish blocks
    with a background of zeros around an ellipsoid."""
    rng = np.random.default_rng(seed)
    D, H, W = shape
    mri = rng.random((B, D, H, W)).astype(np.float32)
    tau = rng.random((B, D, H, W)).astype(np.float32)
    ids = np.array([2, 17, 18, 1003, 2035, 53], dtype=np.float32)
    blocks = rng.integers(0, len(ids), (B, (D + 3) // 4, (H + 3) // 4, (W + 3) // 4))
    lab = ids[blocks].repeat(4, 1).repeat(4, 2).repeat(4, 3)[:, :D, :H, :W]
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    inside = ((z - (D - 1) / 2) / (0.45 * D)) ** 2 + ((y - (H - 1) / 2) / (0.45 * H)) ** 2 + ((x - (W - 1) / 2) / (0.45 * W)) ** 2 <= 1
    roi = np.where(inside[None], lab, np.float32(0)).astype(np.float32)
    return mri, tau, np.ascontiguousarray(roi)


def elastic_u(disp_b, shape):
    """disp_b: (3, gz, gy, gx) -> u (3, D, H, W): trilinear, control point i of an axis at output index i (size-1)/(g-1)."""
    disp_b = np.asarray(disp_b, dtype=np.float64)
    g = disp_b.shape[1:]
    idx, frac = [], []
    for n, gn in zip(shape, g):
        c = np.arange(n, dtype=np.float64) * ((gn - 1) / (n - 1)) if n > 1 else np.zeros(n)
        i0 = np.minimum(np.floor(c).astype(np.int64), gn - 2)
        idx.append(i0)
        frac.append(c - i0)
    iz, iy, ix = np.meshgrid(*idx, indexing="ij")
    fz, fy, fx = np.meshgrid(*frac, indexing="ij")
    u = np.zeros((3,) + tuple(shape))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (fz if dz else 1 - fz) * (fy if dy else 1 - fy) * (fx if dx else 1 - fx)
                u += w[None] * disp_b[:, iz + dz, iy + dy, ix + dx]
    return u


def source_coords(A, shape, disp_b=None):
    """A: 12 values (3 x 4 row-major, (z, y, x)).  -> s (3, D, H, W) float64."""
    A = np.asarray(A, dtype=np.float64).reshape(3, 4)
    D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    s = np.stack([A[r, 0] * z + A[r, 1] * y + A[r, 2] * x + A[r, 3] for r in range(3)])
    if disp_b is not None:
        s = s + elastic_u(disp_b, shape)
    return s


def trilinear(vol, s):
    """Zero padding: a corner outside the volume contributes 0 (grid_sample padding_mode='zeros', align_corners=True)."""
    vol = np.asarray(vol, dtype=np.float64)
    D, H, W = vol.shape
    f = np.floor(s)
    t = s - f
    i = f.astype(np.int64)
    out = np.zeros(s.shape[1:])
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cz, cy, cx = i[0] + dz, i[1] + dy, i[2] + dx
                ok = (cz >= 0) & (cz < D) & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
                w = (t[0] if dz else 1 - t[0]) * (t[1] if dy else 1 - t[1]) * (t[2] if dx else 1 - t[2])
                out += np.where(ok, w * vol[np.clip(cz, 0, D - 1), np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)], 0.0)
    return out


def nearest(vol, s, offset=(0, 0, 0)):
    """vol[floor(s + 0.5) + offset] per axis, 0 outside."""
    D, H, W = vol.shape
    n = np.floor(s + 0.5).astype(np.int64)
    cz, cy, cx = n[0] + offset[0], n[1] + offset[1], n[2] + offset[2]
    ok = (cz >= 0) & (cz < D) & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
    return np.where(ok, vol[np.clip(cz, 0, D - 1), np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)], vol.dtype.type(0))


def near_half(s, band=HALF_BAND):
    """Voxels whose coordinate lies within `band` of a half-integer on any axis: there an fp32 coordinate may round the other way."""
    d = np.abs(s - np.floor(s) - 0.5)
    return (d < band).any(axis=0)


# ---------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the Box-Muller step
# ---------------------------------------------------------------------------------------------------------------------
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or ints) and key words -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def normal(seed, b, idx):
    """n(seed, b, linear voxel index): key = (seed low, seed high), counter = (idx low, idx high, b, 0); Box-Muller on the top
    24 bits of words 0 and 1: u1 = ((w0 >> 8) + 1) / 2^24 in (0, 1], u2 = (w1 >> 8) / 2^24."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & ((1 << 64) - 1)
    w = philox4x32_10(idx & _M32, idx >> np.uint64(32), b, 0, seed & 0xFFFFFFFF, seed >> 32)
    u1 = ((w[0] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (w[1] >> np.uint64(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def warp(mri, tau, roi, params, disp=None, seed=0):
    """The whole kernel in fp64.  -> dict(mri, tau, roi (B, D, H, W): mri / tau float64, roi float32; s: list of (3, D, H, W))."""
    B, D, H, W = mri.shape
    params = np.asarray(params, dtype=np.float64).reshape(B, NPARAM)      # (the fp32 table's values, exactly)
    om, ot, orr, ss = [], [], [], []
    for b in range(B):
        s = source_coords(params[b, :12], (D, H, W), None if disp is None else np.asarray(disp[b], dtype=np.float64))
        scale, shift, gamma, sigma = params[b, 12:]
        r = nearest(roi[b], s)
        m = trilinear(mri[b], s)
        if gamma != 1.0:
            m = np.maximum(m, 0.0) ** gamma
        m = scale * m + shift
        if sigma != 0.0:
            m = m + sigma * normal(seed, b, np.arange(D * H * W, dtype=np.uint64).reshape(D, H, W))
        m = np.where(r == 0, 0.0, m)
        om.append(m), ot.append(trilinear(tau[b], s)), orr.append(r), ss.append(s)
    return dict(mri=np.stack(om), tau=np.stack(ot), roi=np.stack(orr), s=ss)


def label_check(got, roi_b, s):
    """Case 3's label rule for one sample: exact outside the half-integer band, one of the two neighbouring candidates per axis
    inside it.  -> (mismatches outside the band, voxels inside the band that match no candidate, share of the band)."""
    want = nearest(roi_b, s)
    band = near_half(s)
    bad_out = int(np.count_nonzero((got != want) & ~band))
    ok = np.zeros(got.shape, dtype=bool)
    d = s - np.floor(s) - 0.5                                  # > 0: rounded up, the other candidate is one below
    for oz in (0, 1):
        for oy in (0, 1):
            for ox in (0, 1):
                off = [0, 0, 0]
                for a, o in enumerate((oz, oy, ox)):
                    if o:
                        off[a] = np.where(np.abs(d[a]) < HALF_BAND, np.where(d[a] >= 0, -1, 1), 0)
                ok |= got == nearest(roi_b, s, off)
    bad_in = int(np.count_nonzero(band & ~ok))
    return bad_out, bad_in, float(band.mean())
